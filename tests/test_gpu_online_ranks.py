"""Every online kernel instance against a host replay of its arithmetic, bit for bit.

The references are independent of the library: tests/online_emu.py's tree_replay / fold_replay for
f32 (checked from the references alone by tests/test_online_emu.py) and coracle.online_apply /
mf_oracle.online_sequential for f64.  Each test loads the standard batch's model with set_factors
under shuffled signed ids and applies the batch as two online_update calls; the second brings ids
the model has not seen (rows appended in first-touch order, PseudoRandomFactorInitializer values
rounded to the mode's precision, the queued sweep skipped and run again on the device-lookup path).
Where a sweep is expected the test asserts one launch and no level per call (mf_get_stats), so a
silent fallback to the level replay cannot pass.  MFHIP_TEST online_waves=8 / 1 puts ~12 items and
~190 updates / everything on each wave: item switches, recurring items, prefetch across a switch,
many full 16-update chunks and a partial one; unset, a wave holds one or two items.

Which test drives which instance (k -> instance):

  k_online_f32<KPL, FULL> (kernels_online_sweep.hip), general and SINGLE wave bodies
    test_f32_tree[sweep-*]   <1,false> 1, 3, 63   <1,true> 64   <2,false> 65, 100, 127   <2,true> 128
                             <3,false> 129, 160, 192   <4,false> 193, 200, 255   <4,true> 256
                             waves unset: the hot and the sampled items on SINGLE waves, the others general;
                             waves 8: the hot item's SINGLE wave + 6 general waves; waves 1: one general wave
    test_f32_tree[multi-*]   the same instances with online_single=0: every wave on the general body
    test_edges               k = 100, 160, 256: one item with 15 / 16 / 17 / 33 ratings (SINGLE, and
                             general with online_single=0), one user across every wave, a batch of 1
    test_spark_sweep_order   k = 100, 256 in the Spark-sweep order (a permuted, staged sequence)
  k_level<float, KPL> / k_level_out<float, KPL, 1 | 2> (kernels_det.hip)
    test_f32_tree[level | out_next | out_delta]   KPL 1: 1, 3, 63, 64   KPL 2: 65..128   KPL 4: 129..256
    test_f32_fold[level | out_next | out_delta]   KPL 8 (the sequential fold): 257, 300, 511, 512
  k_online_sweep<float, KPL, FULL> (kernels_det.hip, the sequential fold)
    test_f32_fold[sweep-*]          <8,false> 257, 300, 511   <8,true> 512
    test_f32_fold_offset_fallback   offset_limit=1: <1,false> 40   <1,true> 64   <2,false> 100   <2,true> 128
                                    <4,false> 200   <4,true> 256
  k_online_sweep<double, KPL, FULL>
    test_f64[sweep-*]    <1,false> 1, 63   <2,false> 65, 127   <4,false> 129, 255   <8,false> 257, 300   <8,true> 512
    test_f64[ticket-*]   <1,true> 64   <2,true> 128   <4,true> 256
  the deterministic split sweep with nextFactors' update (kernels_detsweep.hip)
    test_f64[sweep-*]    64, 128, 256
  k_level<double, KPL> / k_level_out<double, KPL, 1 | 2>
    test_f64[level] and test_f64_records   KPL 1: 1   KPL 2: 65   KPL 4: 129   KPL 8: 300

All comparisons are bitwise (the factors' and records' bit patterns, signed zeros included).
"""
import functools

import numpy as np
import pytest

import coracle
import mf_oracle as O
import mfhip
import online_emu as E
from conftest import set_knob
from mfhip import _lib as L

pytestmark = pytest.mark.gpu

F32, F64 = L.MODE_FAST_F32, L.MODE_DETERMINISTIC_F64
TREE_RANKS = (1, 3, 63, 64, 65, 100, 127, 128, 129, 160, 192, 193, 200, 255, 256)
FOLD_RANKS = (257, 300, 511, 512)
OFFSET_RANKS = (40, 64, 100, 128, 200, 256)
F64_RANKS = (1, 63, 65, 127, 129, 255, 257, 300, 512)
F64_SPLIT_RANKS = (64, 128, 256)
F64_RECORD_RANKS = (1, 65, 129, 300)
WAVES = (None, 8, 1)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def reference(b, arith, seq=None):
    """The batch's factors after the updates in sequence seq (default: arrival order), and for f32
    both kinds of per-rating records: (U, I, records or None)."""
    U, I = b.start(O.pseudo_random_factor, arith != "f64")
    urow, irow, r = (b.urow, b.irow, b.r) if seq is None else b.reorder(seq)
    if arith == "f64":
        coracle.online_apply(urow, irow, r, U, I, b.k, b.lr)
        return (*frozen(U, I), None)
    replay = E.tree_replay if arith == "tree" else E.fold_replay
    Uf, If, rec = replay(U, I, urow, irow, r, b.lr, b.k, records="both")
    return (*frozen(Uf.astype(np.float64), If.astype(np.float64)), rec)


@functools.lru_cache(maxsize=None)
def standard(k, arith):
    """The standard batch at rank k and its reference, computed once per (k, arithmetic)."""
    b = E.standard_batch(k)
    return b, reference(b, arith)


def apply(monkeypatch, b, mode, knobs, call, expect):
    """The batch on the device as online calls [0, split) and [split, n): the model's (ids, factors)
    per side, and the concatenated records of the out calls.  expect: "sweep" (one launch, no level,
    per call) or "level"."""
    for key, value in knobs.items():
        if value is not None:
            set_knob(monkeypatch, key, value)
    p = L.default_params()
    p.num_factors, p.mode, p.online_learning_rate = b.k, mode, b.lr
    uos, ios = [], []
    with mfhip.Context(p) as ctx:
        ctx.set_factors(L.SIDE_USER, b.known_u, b.U0)
        ctx.set_factors(L.SIDE_ITEM, b.known_i, b.I0)
        for lo, hi in ((0, b.split), (b.split, len(b.r))):
            if lo == hi:
                continue
            u, i, r = b.uid[lo:hi], b.iid[lo:hi], b.r[lo:hi]
            ctx.reset_stats()
            if call == "update":
                touched = ctx.online_update(u, i, r, L.ONLINE_NEXT_FACTORS)
            elif call == "spark":
                touched = ctx.online_update(u, i, r, L.ONLINE_SPARK_SWEEP, num_partitions=4)
            else:
                uo, io = ctx.online_update_out(u, i, r, L.ONLINE_DELTA if call == "out_delta" else L.ONLINE_NEXT_FACTORS)
                uos.append(uo)
                ios.append(io)
                touched = None
            assert touched is None or touched == (len(np.unique(u)), len(np.unique(i)))
            st = ctx.stats()
            assert st["updates"] == hi - lo
            if expect == "sweep":
                assert (st["kernel_launches"], st["levels"]) == (1, 0), (lo, st)
            else:
                assert st["levels"] >= 1 and st["kernel_launches"] == st["levels"], (lo, st)
        res = ctx.factors(L.SIDE_USER), ctx.factors(L.SIDE_ITEM)
    return res, (np.concatenate(uos), np.concatenate(ios)) if uos else None


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def check_model(b, res, U, I, what):
    """ids sorted; every row bitwise the reference's row of that id."""
    for side, (ids, vecs), known, new, ref in ((0, res[0], b.known_u, b.new_u, U), (1, res[1], b.known_i, b.new_i, I)):
        allids = np.concatenate([known, new])
        order = np.argsort(allids)
        assert np.array_equal(ids, allids[order]), (what, side)  # loaded ids and first-touched ids, each once
        if not same_bits(vecs, ref[order]):
            bad = np.argwhere(vecs != ref[order])
            raise AssertionError(f"{what}, side {side}: {len(bad)} elements differ, first (row, element) {bad[:4].tolist()}, "
                                 f"max |diff| {np.abs(vecs - ref[order]).max():.3e}")


def check_records(got, want, what):
    for name, g, w in (("user", got[0], want[0]), ("item", got[1], want[1])):
        if not same_bits(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {len(bad)} {name} record elements differ, first (rating, element) "
                                 f"{bad[:4].tolist()}, max |diff| {np.abs(g - w).max():.3e}")


def variants(sweeps):
    """(id, knobs, call, expect): the sweep variants under every online_waves setting, the level
    replay and the two record modes under one."""
    out = []
    for name, knobs in sweeps:
        for w in WAVES:
            out.append(pytest.param({**knobs, "online_waves": w}, "update", "sweep", id=f"{name}-w{w or 'all'}"))
    out.append(pytest.param({"online_kernel": "level"}, "update", "level", id="level"))
    out.append(pytest.param({}, "out_next", "level", id="out_next"))
    out.append(pytest.param({}, "out_delta", "level", id="out_delta"))
    return out


def run_case(monkeypatch, k, mode, arith, knobs, call, expect):
    b, (U, I, rec) = standard(k, arith)
    what = f"k={k} {arith} {knobs} {call}"
    res, out = apply(monkeypatch, b, mode, knobs, call, expect)
    check_model(b, res, U, I, what)
    if out is not None and rec is not None:
        check_records(out, rec["delta" if call == "out_delta" else "next"], what)
    return b, out


@pytest.mark.parametrize("knobs,call,expect", variants([("sweep", {}), ("multi", {"online_single": "0"})]))
@pytest.mark.parametrize("k", TREE_RANKS)
def test_f32_tree(monkeypatch, k, knobs, call, expect):
    """f32 at k <= 256: k_online_f32 (default; every wave on the general body with online_single=0),
    k_level and k_level_out in both record modes, factors and records bitwise tree_replay."""
    run_case(monkeypatch, k, F32, "tree", knobs, call, expect)


@pytest.mark.parametrize("knobs,call,expect", variants([("sweep", {})]))
@pytest.mark.parametrize("k", FOLD_RANKS)
def test_f32_fold(monkeypatch, k, knobs, call, expect):
    """f32 past k = 256: k_online_sweep<float, 8, .>, k_level<float, 8> and k_level_out<float, 8, .>,
    bitwise fold_replay."""
    run_case(monkeypatch, k, F32, "fold", knobs, call, expect)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("k", OFFSET_RANKS)
def test_f32_fold_offset_fallback(monkeypatch, k, waves):
    """offset_limit=1 sends f32 at k <= 256 to k_online_sweep<float, 1 | 2 | 4, .>: bitwise fold_replay
    (and so not the tree: tests/test_online_emu.py shows the two differ at these ranks)."""
    run_case(monkeypatch, k, F32, "fold", {"offset_limit": "1", "online_waves": waves}, "update", "sweep")


def f64_variants():
    out = []
    for k in F64_RANKS + F64_SPLIT_RANKS:
        for w in (None, 8):
            out.append(pytest.param(k, {"online_waves": w}, "sweep", id=f"{k}-sweep-w{w or 'all'}"))
    for k in F64_SPLIT_RANKS:
        for w in (None, 8):
            out.append(pytest.param(k, {"online_kernel": "ticket", "online_waves": w}, "sweep", id=f"{k}-ticket-w{w or 'all'}"))
    for k in F64_RECORD_RANKS:
        out.append(pytest.param(k, {"online_kernel": "level"}, "level", id=f"{k}-level"))
    return out


@pytest.mark.parametrize("k,knobs,expect", f64_variants())
def test_f64(monkeypatch, k, knobs, expect):
    """f64: k_online_sweep<double, ., .> (every rank but 64 / 128 / 256 by default, those with
    online_kernel=ticket), the deterministic split sweep (64 / 128 / 256 by default) and k_level,
    bitwise coracle.online_apply."""
    run_case(monkeypatch, k, F64, "f64", knobs, "update", expect)


@functools.lru_cache(maxsize=None)
def f64_records(k, name):
    """mf_oracle.online_sequential on the standard batch: its emitted records and final factors."""
    b, (U, I, _) = standard(k, "f64")
    U0, I0 = b.start(O.pseudo_random_factor, False)
    users, items, emitted = {j: v.tolist() for j, v in enumerate(U0)}, {j: v.tolist() for j, v in enumerate(I0)}, []
    O.online_sequential(list(zip(b.urow.tolist(), b.irow.tolist(), b.r.tolist())), users, items, k, b.lr, name,
                        emitted=emitted)
    Uf, If = np.array([users[j] for j in range(len(U0))]), np.array([items[j] for j in range(len(I0))])
    if name == "next":  # the two oracles agree
        assert same_bits(Uf, U) and same_bits(If, I)
    return np.array([a for a, _ in emitted]), np.array([c for _, c in emitted]), Uf, If


@pytest.mark.parametrize("call", ["out_next", "out_delta"])
@pytest.mark.parametrize("k", F64_RECORD_RANKS)
def test_f64_records(monkeypatch, k, call):
    """k_level_out<double, 1 | 2 | 4 | 8, .>: records and factors bitwise mf_oracle.online_sequential's
    emitted list and result in the same flavour (NEXT: also coracle.online_apply's factors)."""
    b, _ = standard(k, "f64")
    eu, ei, Uf, If = f64_records(k, "delta" if call == "out_delta" else "next")
    res, out = apply(monkeypatch, b, F64, {}, call, "level")
    check_records(out, (eu, ei), f"k={k} f64 {call}")
    check_model(b, res, Uf, If, f"k={k} f64 {call}")


# ---------------------------------------------------------------------------------------------
# chunk and pipeline edges
def edge_batch(k, shape):
    rng = np.random.default_rng(k + 7)
    nu, ni = 40, 30
    if shape.startswith("item"):  # one item with exactly n ratings, users that recur
        n = int(shape[4:])
        uidx, iidx = rng.integers(0, 6, n), np.full(n, 3)
    elif shape == "one_user":  # a ticket chain through every wave
        n = 600
        uidx, iidx = np.full(n, 5), rng.integers(0, ni, n)
    else:
        n = 1
        uidx, iidx = np.array([2]), np.array([4])
    r = rng.integers(1, 6, n).astype(np.float64)
    return E.make_batch(k, uidx, iidx, r, nu, ni, rng, split=0, new_frac=0.0)


@functools.lru_cache(maxsize=None)
def edge(k, shape, arith):
    b = edge_batch(k, shape)
    return b, reference(b, arith)


def edge_cases():
    out = []
    for k in (100, 160, 256):
        for shape in ("item15", "item16", "item17", "item33", "one_user", "one"):
            out.append(pytest.param(k, F32, "tree", shape, {}, id=f"{k}-f32-{shape}"))
            out.append(pytest.param(k, F32, "tree", shape, {"online_single": "0"}, id=f"{k}-f32-{shape}-multi"))
            out.append(pytest.param(k, F64, "f64", shape, {}, id=f"{k}-f64-{shape}"))
        for mode, arith, name in ((F32, "tree", "f32"), (F64, "f64", "f64")):
            out.append(pytest.param(k, mode, arith, "one_user", {"online_waves": 8}, id=f"{k}-{name}-one_user-w8"))
    return out


@pytest.mark.parametrize("k,mode,arith,shape,knobs", edge_cases())
def test_edges(monkeypatch, k, mode, arith, shape, knobs):
    """One item with exactly 15, 16, 17 and 33 ratings (a partial chunk, a full one, a full one and
    one update, two and one: on a SINGLE wave by default, on the general body with online_single=0),
    one user across every wave, a batch of 1 -- against the replays, at k = 100 / 160 / 256
    (k_online_f32<2,false> / <3,false> / <4,true>; f64 k_online_sweep<double, 2 | 4, false> and the
    split sweep)."""
    b, (U, I, _) = edge(k, shape, arith)
    res, _ = apply(monkeypatch, b, mode, knobs, "update", "sweep")
    check_model(b, res, U, I, f"k={k} {arith} {shape} {knobs}")


@pytest.mark.parametrize("waves", [None, 8])
@pytest.mark.parametrize("mode,arith", [(F32, "tree"), (F64, "f64")], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [256, 100])  # one FULL and one masked rank
def test_spark_sweep_order(monkeypatch, k, mode, arith, waves):
    """ONLINE_SPARK_SWEEP with 4 partitions: each call's ratings in mf_oracle.spark_sweep_order's order
    (new ids still get their rows in arrival order), replayed on the host in that order."""
    b = spark_case(k, arith)
    res, _ = apply(monkeypatch, b[0], mode, {"online_waves": waves}, "spark", "sweep")
    check_model(b[0], res, b[1][0], b[1][1], f"k={k} {arith} spark w{waves}")


@functools.lru_cache(maxsize=None)
def spark_case(k, arith):
    b = E.standard_batch(k, signed=False)  # the Spark sweep partitions users by id % P: non-negative ids
    seq = []
    for lo, hi in ((0, b.split), (b.split, len(b.r))):
        rs = list(zip(b.uid[lo:hi].tolist(), b.iid[lo:hi].tolist(), b.r[lo:hi].tolist()))
        seq += [lo + j for j in O.spark_sweep_order(rs, 4)]
    assert sorted(seq) == list(range(len(b.r))) and seq != sorted(seq)
    return b, reference(b, arith, np.array(seq))
