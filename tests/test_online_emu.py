"""The host replays of tests/online_emu.py, checked from the references alone (no GPU).

tests/test_gpu_online_ranks.py compares every f32 online kernel instance bitwise with these replays,
so this file establishes what that comparison rests on:

  fma32        equals exact rational arithmetic, also where rounding a * b + c to f64 first and to f32
               afterwards (fma32_naive) gives another result;
  distance     tree_replay and fold_replay of the standard batch stay inside ONLINE_F32_TOL (1e-4 per
               factor row, tests/test_gpu_configs.py) of the f64 oracle's replay (coracle.online_apply)
               of the same batch from the same factors, with a stated margin;
  sensitivity  the replays tell the defects apart that the GPU comparison is there to catch.

Measured here (max over the user and the item side of max_row ||f32 - f64|| / ||f64||):

  tree  k =   1  1.08e-05        k = 100  4.49e-07        k = 192  4.95e-07
        k =   3  3.14e-07        k = 127  4.46e-07        k = 193  5.47e-07
        k =  63  4.67e-07        k = 128  4.48e-07        k = 200  5.69e-07
        k =  64  4.16e-07        k = 129  4.49e-07        k = 255  4.72e-07
        k =  65  4.24e-07        k = 160  4.64e-07        k = 256  5.09e-07
  fold  k =  40  4.43e-07   64  4.39e-07   128  4.71e-07   257  5.26e-07   300  5.36e-07   511  5.46e-07
        k = 512  5.54e-07

So the f32 references are at least 175x inside the tolerance at k >= 3 and 9x inside at k = 1 (one
product per dot, rows of one element: nothing averages the rounding errors out).  The asserted
margins are half of that: F32_MARGIN = 90 at k >= 3, F32_MARGIN_K1 = 4.

The two defects the tolerance must see, on the same batch: the last element of the user rows never
stored, 3.8e-2 .. 4.9e-1; one dropped update, 2.0e-3 (k = 256) .. 9.2e-2 (k = 3), 2.9e-4 in the fold
at k = 512 -- all outside 1e-4.  A wrong lane layout or the fold in place of the tree stays ~5e-7
from the oracle: only the bitwise comparison sees those.
"""
from fractions import Fraction

import numpy as np
import pytest

import coracle
import mf_oracle as O
import online_emu as E

ONLINE_F32_TOL = 1e-4  # tests/test_gpu_configs.py: the north star's row-relative factor tolerance
F32_MARGIN = 90.0      # distance * margin <= tolerance, k >= 3 (module docstring)
F32_MARGIN_K1 = 4.0    # k = 1

TREE_RANKS = (1, 3, 63, 64, 65, 100, 127, 128, 129, 160, 192, 193, 200, 255, 256)
FOLD_RANKS = (40, 64, 128, 257, 300, 511, 512)


# ---------------------------------------------------------------------------------------------
# fma32
def exact_fma32(a, b, c):
    """float32(a * b + c) through exact rationals and integer rounding (nearest, ties to even,
    subnormals below 2^-126, overflow to infinity)."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return np.float32(0.0)
    num, den = abs(x.numerator), x.denominator  # den is a power of two
    e = -(den.bit_length() - 1)  # x = +-num * 2^e
    q = max(e + num.bit_length() - 24, -149)  # exponent of the result's last bit
    if q <= e:
        mant = num << (e - q)
    else:
        sh = q - e
        mant, rem, half = num >> sh, num & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and (mant & 1)):
            mant += 1
    with np.errstate(over="ignore"):
        v = np.float32(float(mant) * 2.0 ** q) if q < 900 else np.float32(np.inf)
    return -v if x < 0 else v


def same_floats(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return np.array_equal(x, y)  # (no NaN in these checks; +0 == -0)


def test_exact_fma32_rounds_as_ieee():
    """The checker itself on cases with known answers."""
    f = np.float32
    assert exact_fma32(f(1), f(1), f(2.0 ** -24)) == f(1)                      # a tie, to even
    assert exact_fma32(f(1), f(1 + 2.0 ** -23), f(2.0 ** -24)) == f(1 + 2.0 ** -22)  # a tie, to even (up)
    assert exact_fma32(f(1), f(1), f(2.0 ** -24 + 2.0 ** -40)) == f(1 + 2.0 ** -23)
    assert exact_fma32(f(2.0 ** -100), f(2.0 ** -49), f(0)) == f(2.0 ** -149)  # the smallest subnormal
    assert exact_fma32(f(2.0 ** -100), f(2.0 ** -50), f(0)) == f(0)            # half of it: a tie, to even
    assert exact_fma32(f(2.0 ** 100), f(2.0 ** 100), f(0)) == f(np.inf)
    assert exact_fma32(f(3), f(-5), f(15)) == f(0)


def test_fma32_equals_exact_rationals_on_random_triples():
    rng = np.random.default_rng(3)
    n = 100000
    def rand(lo, hi):
        m = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        return (m * 2.0 ** rng.integers(lo, hi, n)).astype(np.float32)
    # wide exponents (subnormal results, results near overflow), and near-cancelling triples whose
    # sum's leading bits come from the product's low half
    a, b, c = rand(-60, 60), rand(-60, 60), rand(-130, 125)
    half = n // 2
    with np.errstate(over="ignore"):
        c[:half] = (-(a[:half].astype(np.float64) * b[:half]) * (1 + rng.uniform(-1, 1, half) * 2.0 ** -20)).astype(np.float32)
    got = E.fma32(a, b, c)
    want = np.array([exact_fma32(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.isfinite(want).mean() > 0.95
    bad = np.flatnonzero(~((got == want) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))))
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], c[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert same_floats(E.fma32(np.float32(3), np.float32(-5), np.float32(15)), 0.0)  # scalars broadcast


def test_fma32_on_double_rounding_ties():
    """c with an odd last bit, a * b = +-(half an ulp of c) (1 - x^2 2^-46): the exact sum lies just
    inside the tie towards c, the f64 sum (53 bits) lands on the tie itself and its conversion to
    f32 goes to the even neighbour.  fma32 must give c; fma32_naive must not."""
    rng = np.random.default_rng(4)
    n = 4000
    E_ = rng.integers(-40, 60, n)  # (a and b stay normal f32 numbers)
    x = rng.integers(1, 256, n)
    mant = (rng.integers(2 ** 22, 2 ** 23, n) * 2 + 1).astype(np.float64)  # 24 bits, odd
    sign_c = rng.choice([-1.0, 1.0], n)
    sign_p = rng.choice([-1.0, 1.0], n)
    c = (sign_c * mant * 2.0 ** (E_ - 23)).astype(np.float32)  # in [2^E, 2^(E+1)), ulp 2^(E-23)
    s1 = rng.integers(-30, 30, n)
    a = (sign_p * (2.0 ** 23 + x) * 2.0 ** s1).astype(np.float32)
    b = ((2.0 ** 23 - x) * 2.0 ** (E_ - 24 - 46 - s1)).astype(np.float32)  # a b = +-2^(E-24) (1 - x^2 2^-46)
    want = np.array([exact_fma32(p, q, z) for p, q, z in zip(a, b, c)], np.float32)
    assert same_floats(want, c)  # the construction: the exact result is c itself
    f64 = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert np.array_equal(f64, c.astype(np.float64) + sign_p * 2.0 ** (E_ - 24))  # the f64 sum is the tie
    assert same_floats(E.fma32(a, b, c), want)
    naive = E.fma32_naive(a, b, c)
    wrong = int((naive != want).sum())
    print(f"double-rounding ties: fma32 0 / {n} wrong, the naive f64 version {wrong} / {n}")
    assert wrong == n  # every one of them: the check sees double rounding


def test_fold_dot_is_the_left_fold_from_zero():
    rng = np.random.default_rng(5)
    for k in (1, 7, 300):
        p, q = rng.standard_normal(k).astype(np.float32), rng.standard_normal(k).astype(np.float32)
        acc = np.float32(0)
        for f in range(k):
            acc = np.float32(acc + np.float32(p[f] * q[f]))
        assert E.fold_dot(p, q) == acc


def test_lane_layouts():
    """online_f32.hpp f32_elem: contiguous at k = 64, 128, 256; strided elsewhere, 192 included; a
    lane's elements past k read as zero; every element of a row sits in exactly one lane slot."""
    for k in TREE_RANKS:
        idx = E.lane_elements(k)
        kpl = (k + 63) // 64
        assert idx.shape == (64, kpl)
        assert sorted(idx[idx < k].tolist()) == list(range(k)) and (idx[idx >= k] == k).all()
        if k in (64, 128, 256):
            assert np.array_equal(idx, np.arange(k).reshape(64, kpl))
        else:
            assert np.array_equal(idx, np.where(np.arange(64 * kpl).reshape(kpl, 64).T < k,
                                                np.arange(64 * kpl).reshape(kpl, 64).T, k))
    x = (np.arange(64) + 1).astype(np.float32)
    assert E.wave_sum(x) == np.float32(64 * 65 / 2)  # exact in f32 in any order
    # the order: ((x0 + x32) + (x16 + x48)) + ... -- lane 0's partner sums, in the documented order
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(64) * 2.0 ** rng.integers(-8, 8, 64)).astype(np.float32)
    s = x.copy()
    for m in (32, 16, 1, 2, 4, 8):  # after the l^1 and l^2 steps a quad is uniform: 7-l is l^4, 15-l is l^8
        s = s + s[np.arange(64) ^ m]
    assert (s == s[0]).all() and E.wave_sum(x) == s[0]


# ---------------------------------------------------------------------------------------------
# distance to the f64 oracle
_cache = {}


def standard(k):
    """The standard batch at rank k with its starting factors (new rows rounded to f32) and the f64
    oracle's replay of it."""
    if k not in _cache:
        b = E.standard_batch(k)
        U, I = b.start(O.pseudo_random_factor, True)
        U64, I64 = U.copy(), I.copy()
        coracle.online_apply(b.urow, b.irow, b.r, U64, I64, k, b.lr)
        for a in (U, I, U64, I64):
            a.setflags(write=False)
        _cache[k] = (b, U, I, U64, I64)
    return _cache[k]


def check_distance(name, k, got, ref):
    for a in (*got, *ref):
        assert np.isfinite(a).all() and 0 < np.abs(a).max() < 100.0  # no case degenerates
    dist = max(E.row_rel_err(got[0], ref[0]), E.row_rel_err(got[1], ref[1]))
    margin = F32_MARGIN_K1 if k == 1 else F32_MARGIN
    print(f"{name} k={k}: {dist:.3e} from the f64 oracle, {ONLINE_F32_TOL / dist:.0f}x inside the tolerance "
          f"(asserted: {margin:.0f}x)")
    assert dist * margin <= ONLINE_F32_TOL, dist
    assert dist > 0  # f32 is not f64: the two references are independent statements


def test_standard_batch_shape():
    b = E.standard_batch(64)
    assert len(b.r) == 3000 and b.split == 1500
    assert len(np.unique(b.uid)) <= 300 and len(np.unique(b.iid)) <= 100 and (np.bincount(b.irow).max() >= 600)
    assert (b.uid < 0).any() and (b.uid > 0).any() and set(np.unique(b.r)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    # the first call touches loaded ids only; the second brings about 5 % new ones, in first-touch order
    assert np.isin(b.uid[:b.split], b.known_u).all() and np.isin(b.iid[:b.split], b.known_i).all()
    assert 8 <= len(b.new_u) <= 15 and 2 <= len(b.new_i) <= 5
    assert b.urow.max() == len(b.known_u) + len(b.new_u) - 1 and b.irow.max() == len(b.known_i) + len(b.new_i) - 1
    first = [int(np.flatnonzero(b.uid == x)[0]) for x in b.new_u]
    assert first == sorted(first) and min(first) >= b.split
    # the dependency structure the sweeps are tested on: users and items that recur
    assert np.bincount(b.urow).max() >= 15


@pytest.mark.parametrize("k", TREE_RANKS)
def test_tree_replay_is_close_to_the_f64_oracle(k):
    b, U, I, U64, I64 = standard(k)
    check_distance("tree_replay", k, E.tree_replay(U, I, b.urow, b.irow, b.r, b.lr, k), (U64, I64))


@pytest.mark.parametrize("k", FOLD_RANKS)
def test_fold_replay_is_close_to_the_f64_oracle(k):
    b, U, I, U64, I64 = standard(k)
    check_distance("fold_replay", k, E.fold_replay(U, I, b.urow, b.irow, b.r, b.lr, k), (U64, I64))


@pytest.mark.parametrize("replay", [E.tree_replay, E.fold_replay])
def test_records_are_the_oracles_records(replay):
    """The per-rating records of both replays against mf_oracle.online_sequential's emitted list
    (f64), within the tolerance; the last "next" record of a row is its final value, bitwise."""
    k = 65
    b, U, I, _, _ = standard(k)
    Uf, If, rec = replay(U, I, b.urow, b.irow, b.r, b.lr, k, records="both")
    ratings = list(zip(b.urow.tolist(), b.irow.tolist(), b.r.tolist()))
    for name in ("next", "delta"):
        users = {j: v.tolist() for j, v in enumerate(U)}
        items = {j: v.tolist() for j, v in enumerate(I)}
        emitted = []
        O.online_sequential(ratings, users, items, k, b.lr, name, emitted=emitted)
        eu, ei = np.array([a for a, _ in emitted]), np.array([c for _, c in emitted])
        uo, io = rec[name]
        du = E.row_rel_err(uo, eu)
        # delta's item record is the small difference lr e u itself: relative to the row it updates
        di = E.row_rel_err(io, ei) if name == "next" else float(
            (np.linalg.norm(io - ei, axis=1) / np.linalg.norm(np.array([I[j] for j in b.irow]), axis=1)).max())
        print(f"{replay.__name__} {name} records: users {du:.3e} items {di:.3e}")
        assert du * F32_MARGIN <= ONLINE_F32_TOL and di * F32_MARGIN <= ONLINE_F32_TOL
    last_u = {int(u): j for j, u in enumerate(b.urow)}
    last_i = {int(i): j for j, i in enumerate(b.irow)}
    for row, j in last_u.items():
        assert np.array_equal(rec["next"][0][j], Uf[row])
    for row, j in last_i.items():
        assert np.array_equal(rec["next"][1][j], If[row])
    one = replay(U, I, b.urow, b.irow, b.r, b.lr, k, records="delta")
    assert np.array_equal(one[2], rec["delta"][0]) and np.array_equal(one[3], rec["delta"][1])
    assert np.array_equal(one[0], Uf) and np.array_equal(one[1], If)


# ---------------------------------------------------------------------------------------------
# defect sensitivity
def differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("k", [3, 64, 100, 128, 192, 256])
def test_tree_replay_sees_a_frozen_element_and_a_dropped_update(k):
    b, U, I, U64, I64 = standard(k)
    good = E.tree_replay(U, I, b.urow, b.irow, b.r, b.lr, k)
    frozen = E.tree_replay(U, I, b.urow, b.irow, b.r, b.lr, k, freeze_user_tail=True)
    keep = np.arange(len(b.r)) != 1234
    dropped = E.tree_replay(U, I, b.urow[keep], b.irow[keep], b.r[keep], b.lr, k)
    for name, bad in (("frozen last user element", frozen), ("one dropped update", dropped)):
        d64 = max(E.row_rel_err(bad[0], U64), E.row_rel_err(bad[1], I64))
        print(f"k={k} {name}: {d64:.3e} from the f64 oracle ({d64 / ONLINE_F32_TOL:.0f}x the tolerance)")
        assert differs(bad, good)
        assert d64 > ONLINE_F32_TOL  # leaves the band


@pytest.mark.parametrize("k", [257, 512])
def test_fold_replay_sees_a_frozen_element_and_a_dropped_update(k):
    b, U, I, U64, I64 = standard(k)
    good = E.fold_replay(U, I, b.urow, b.irow, b.r, b.lr, k)
    frozen = E.fold_replay(U, I, b.urow, b.irow, b.r, b.lr, k, freeze_user_tail=True)
    keep = np.arange(len(b.r)) != 1234
    dropped = E.fold_replay(U, I, b.urow[keep], b.irow[keep], b.r[keep], b.lr, k)
    for bad in (frozen, dropped):
        assert differs(bad, good)
        assert max(E.row_rel_err(bad[0], U64), E.row_rel_err(bad[1], I64)) > ONLINE_F32_TOL


def test_tree_replay_sees_the_lane_layout_and_the_fold():
    """Defects far inside the tolerance that only a bitwise comparison catches: the strided layout
    at k = 128, the contiguous one at k = 192 (deliberately not FULL), the fold in place of the tree."""
    assert np.array_equal(E.lane_elements(64, "strided"), E.lane_elements(64, "contiguous"))  # one layout at KPL = 1
    for k, layout in ((128, "strided"), (192, "contiguous"), (256, "strided")):
        b, U, I, U64, I64 = standard(k)
        good = E.tree_replay(U, I, b.urow, b.irow, b.r, b.lr, k)
        bad = E.tree_replay(U, I, b.urow, b.irow, b.r, b.lr, k, layout=layout)
        assert differs(bad, good), (k, layout)
        assert max(E.row_rel_err(bad[0], U64), E.row_rel_err(bad[1], I64)) < ONLINE_F32_TOL  # (invisible to it)
    for k in (40, 64, 100, 128, 200, 256):
        b, U, I, _, _ = standard(k)
        assert differs(E.fold_replay(U, I, b.urow, b.irow, b.r, b.lr, k),
                       E.tree_replay(U, I, b.urow, b.irow, b.r, b.lr, k)), k
