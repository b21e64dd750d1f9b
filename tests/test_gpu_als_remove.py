"""Rating removal on the device: mf_als_remove, mf_als_remove_rows, mf_als_retract, StreamingALS.forget.

The yardstick throughout is exact.  The rule, in numpy: in ascending j, batch entry j removes the oldest
instance of its pair that is still alive in the history (arrival order).  The expected CSRs are numpy's stable
grouping of the surviving history on the row maps of the whole history, and a twin context that is given
als_prepare(whole history) and then als_prepare(surviving history): a second prepare keeps the rows, so row
numbering and initial factor bits match.  Everything is compared bit for bit.

The history (removal_problem): test_gpu_als_append's stream (parts A-D: the 700-rating hot item, users of 1 /
63 / 64 / 65 ratings, ratings <= 0 and the 1e-50 one, shuffled and partly negative ids) followed by 5,600
ratings of 200 more users over 30 more items -- 6.9k entries, four of the compaction kernel's 2048-entry
tiles on either side -- and three planted pairs of three instances with different values."""
import ctypes as C
import functools

import numpy as np
import pytest

from als_support import MODES, bits, dtype_of, frozen, make_ctx, shuffled_ids, small_problem
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context, als_solve
from test_gpu_als_append import (ALPHA, CG, F32, F64, HOT, HOWS, LAM, bad_hows, full_run, numpy_csr, same_csr,
                                 same_factors, same_state, state_of, stream_problem)

pytestmark = pytest.mark.gpu

TILE = 2048                       # entries per workgroup of the compaction kernels
NU_ALL, NI_ALL = 256, 64          # ids the tables hold; 252 .. 255 / 62, 63 are never rated (unknown to the model)
PLANT_ITEM = 60
U_ALL_GONE, I_ALL_GONE = 42, 31   # a 63-rating user and a filler item: every rating of theirs is removed


@functools.lru_cache(maxsize=None)
def removal_problem():
    d = stream_problem()
    rng = np.random.default_rng(2024)
    hu = np.concatenate([p[0] for p in d["parts"][:4]])
    hi = np.concatenate([p[1] for p in d["parts"][:4]])
    hr = np.concatenate([p[2] for p in d["parts"][:4]])
    fu, fi = rng.integers(50, 250, 5600), rng.integers(30, 60, 5600)
    fr = rng.integers(-2, 11, 5600) / 2.0                                   # some ratings <= 0
    plant = [(1, PLANT_ITEM, 1.0), (1, PLANT_ITEM, 2.0), (1, PLANT_ITEM, 3.0),
             (2, PLANT_ITEM, 4.0), (2, PLANT_ITEM, -1.0), (2, PLANT_ITEM, 0.5),
             (3, PLANT_ITEM, 2.5), (3, PLANT_ITEM, 1.5), (3, PLANT_ITEM, 5.0), (250, 61, 1.0), (251, 2, 2.0)]
    pu, pi, pr = (np.array(x) for x in zip(*plant))
    tu, ti, tr = np.concatenate([fu, pu]), np.concatenate([fi, pi]), np.concatenate([fr, pr])
    p = rng.permutation(len(tu))
    hu, hi, hr = np.concatenate([hu, tu[p]]), np.concatenate([hi, ti[p]]), np.concatenate([hr, tr[p]])
    uid, iid = shuffled_ids(rng, NU_ALL), shuffled_ids(rng, NI_ALL, 5)
    assert len(hu) >= 3 * TILE + 1
    assert (uid < 0).sum() > 50 and (iid < 0).sum() > 10
    return frozen(dict(hu=hu.astype(np.int64), hi=hi.astype(np.int64), hr=hr.astype(np.float64), uid=uid, iid=iid))


def row_maps(hu, hi):
    um, im = {}, {}
    for a in hu:
        um.setdefault(int(a), len(um))
    for a in hi:
        im.setdefault(int(a), len(im))
    return um, im


def numpy_rule(hu, hi, bu, bi):
    """(found per batch entry, alive per history entry)."""
    alive = np.ones(len(hu), bool)
    found = np.zeros(len(bu), bool)
    for j in range(len(bu)):
        c = np.flatnonzero((hu == bu[j]) & (hi == bi[j]) & alive)          # history in arrival order
        found[j] = len(c) > 0
        if found[j]:
            alive[c[0]] = False
    return found, alive


def expected_csrs(hu, hi, hr, alive, mode, um=None, im=None):
    if um is None:
        um, im = row_maps(hu, hi)
    ur = np.array([um[int(a)] for a in hu[alive]], np.int64)
    ir = np.array([im[int(a)] for a in hi[alive]], np.int64)
    r = hr[alive]
    return [numpy_csr(ur, ir, r, len(um), mode), numpy_csr(ir, ur, r, len(im), mode)]


@functools.lru_cache(maxsize=None)
def the_batch():
    """One batch with every case the removal has to get right, as index arrays, shuffled."""
    d = removal_problem()
    hu, hi, hr = d["hu"], d["hi"], d["hr"]
    um, im = row_maps(hu, hi)
    rng = np.random.default_rng(7)
    ur = np.array([um[int(a)] for a in hu])
    ir = np.array([im[int(a)] for a in hi])
    bu, bi = [], []

    def name(positions):
        bu.extend(hu[positions].tolist())
        bi.extend(hi[positions].tolist())

    def name_through(p):
        """The pair of history entry p as often as it occurs up to p: the rule then removes p itself."""
        c = int(((hu[:p + 1] == hu[p]) & (hi[:p + 1] == hi[p])).sum())
        bu.extend([int(hu[p])] * c)
        bi.extend([int(hi[p])] * c)

    # three-instance pairs: named once, twice, four times (one miss)
    bu += [1, 2, 2, 3, 3, 3, 3]
    bi += [PLANT_ITEM] * 7
    # an unknown user id, an unknown item id, known ids whose pair was never rated
    bu += [253, 5, 250, 41]
    bi += [3, 63, HOT, 61]
    # every rating of one user and of one non-hot item
    name(np.flatnonzero(hu == U_ALL_GONE))
    name(np.flatnonzero(hi == I_ALL_GONE))
    # 300 of the hot item's ratings, its first and its last entry among them
    hot = np.flatnonzero(hi == HOT)
    n0 = len(bu)
    name_through(hot[0])
    name_through(hot[-1])
    name(rng.choice(hot, 300 - (len(bu) - n0), replace=False))
    # two removed entries adjacent across a tile boundary, on both sides; the first and last entry of each CSR
    must_go = [hot[0], hot[-1]]
    for rows in (ur, ir):
        order = np.argsort(rows, kind="stable")                            # CSR position -> history position
        for p in order[[0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, len(order) - 1]]:
            name_through(p)
            must_go.append(p)
    # the 1e-50 rating
    tiny = np.flatnonzero(hr == 1e-50)
    assert len(tiny) == 1
    name_through(tiny[0])
    must_go.append(tiny[0])
    bu, bi = np.array(bu, np.int64), np.array(bi, np.int64)
    p = rng.permutation(len(bu))                                           # a row's entries interleave with other rows'
    bu, bi = bu[p], bi[p]
    found, alive = numpy_rule(hu, hi, bu, bi)
    assert not alive[must_go].any()
    assert not alive[hu == U_ALL_GONE].any() and not alive[hi == I_ALL_GONE].any()
    assert 300 <= (~alive[hot]).sum() < len(hot)
    assert found.sum() > 400 and (~found).sum() >= 5
    return frozen(dict(bu=bu, bi=bi, found=found, alive=alive))


def ids(d, u, i):
    return np.ascontiguousarray(d["uid"][u].astype(np.int32)), np.ascontiguousarray(d["iid"][i].astype(np.int32))


def prepared(mode, k, history=None):
    d = removal_problem()
    ctx = make_ctx(k, mode)
    hu, hi, hr = history if history is not None else (d["hu"], d["hi"], d["hr"])
    ctx.als_prepare(*ids(d, hu, hi), hr)
    return ctx


def twin_of(mode, k, alive):
    d = removal_problem()
    twin = prepared(mode, k)
    twin.als_prepare(*ids(d, d["hu"][alive], d["hi"][alive]), d["hr"][alive])
    return twin


def same_csrs(a, b_or_want, what):
    for side in (L.SIDE_USER, L.SIDE_ITEM):
        want = b_or_want[side] if isinstance(b_or_want, list) else b_or_want.als_csr(side)
        same_csr(a.als_csr(side), want, (what, side))


# ---------------------------------------------------------------------------------------------
# 1. the rule

@pytest.mark.parametrize("knobs", [dict(als_chunk=8, als_batch=4), dict(als_chunk=64)])
@pytest.mark.parametrize("mode", MODES)
def test_remove_follows_the_rule(monkeypatch, mode, knobs):
    for key, v in knobs.items():
        set_knob(monkeypatch, key, v)
    d, b = removal_problem(), the_batch()
    hu, hi, hr = d["hu"], d["hi"], d["hr"]
    want_found, alive = b["found"], b["alive"]
    with prepared(mode, 8) as sub, twin_of(mode, 8, alive) as twin:
        before = [sub.factors(s) for s in (0, 1)]
        found, removed = sub.als_remove(*ids(d, b["bu"], b["bi"]))
        assert np.array_equal(found, want_found), np.flatnonzero(found != want_found)[:8]
        assert removed == want_found.sum()
        want = expected_csrs(hu, hi, hr, alive, mode)
        same_csrs(sub, want, "numpy")
        same_csrs(sub, twin, "twin")
        um, im = row_maps(hu, hi)
        assert np.diff(want[0][0])[um[U_ALL_GONE]] == 0 and np.diff(want[1][0])[im[I_ALL_GONE]] == 0
        # 1e-50 is a positive rating in f64 and 0 in f32: the removed ratings > 0 differ by that one
        gone_pos = [(d["hr"][~alive].astype(dtype_of(m)) > 0).sum() for m in (F64, F32)]
        assert gone_pos[0] == gone_pos[1] + 1
        for side in (0, 1):
            f = sub.factors(side)
            assert np.array_equal(f[0], before[side][0]) and np.array_equal(bits(f[1]), bits(before[side][1]))
        assert sub.num_factors(L.SIDE_USER) == len(um) and sub.num_factors(L.SIDE_ITEM) == len(im)


# ---------------------------------------------------------------------------------------------
# 2. a sliding window

@pytest.mark.parametrize("mode", MODES)
def test_sliding_window(monkeypatch, mode):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    d = removal_problem()
    n = len(d["hu"])
    cuts = [0, int(0.4 * n), int(0.7 * n), n - 50, n]
    A, B, Cc, D = [(d["hu"][a:b], d["hi"][a:b], d["hr"][a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    both = set(zip(A[0].tolist(), A[1].tolist())) & set(zip(B[0].tolist(), B[1].tolist()))
    assert len(both) > 10                                                  # pairs rated in A and in B
    ABC = tuple(np.concatenate([A[c], B[c], Cc[c]]) for c in range(3))
    BC = tuple(np.concatenate([B[c], Cc[c]]) for c in range(3))
    with make_ctx(8, mode) as sub, make_ctx(8, mode) as twin:
        sub.als_prepare(*ids(d, A[0], A[1]), A[2])
        sub.als_append(*ids(d, B[0], B[1]), B[2])
        sub.als_append(*ids(d, Cc[0], Cc[1]), Cc[2])
        twin.als_prepare(*ids(d, ABC[0], ABC[1]), ABC[2])
        twin.als_prepare(*ids(d, BC[0], BC[1]), BC[2])
        found, removed = sub.als_remove(*ids(d, A[0], A[1]))
        assert found.all() and removed == len(A[0])
        same_csrs(sub, twin, "window")
        same_factors(sub, twin, "window")
        for part in (B, Cc):
            found, removed = sub.als_remove(*ids(d, part[0], part[1]))
            assert found.all() and removed == len(part[0])
        for side in (0, 1):
            off, cols, vals, npos = sub.als_csr(side)
            assert not off.any() and len(cols) == len(vals) == 0 and not npos.any()
            assert len(off) == sub.num_factors(side) + 1
        fac = [sub.factors(s) for s in (0, 1)]
        full_run(sub, 2, {})                                               # nothing to solve
        full_run(sub, 2, dict(implicit=True, alpha=ALPHA))
        for side in (0, 1):
            assert np.array_equal(bits(sub.factors(side)[1]), bits(fac[side][1]))
        sub.als_append(*ids(d, D[0], D[1]), D[2])
        twin.als_prepare(*ids(d, D[0], D[1]), D[2])
        same_csrs(sub, twin, "append after the window emptied")
        # a batch of misses: unknown ids, never-rated pairs, pairs that are gone
        before = state_of(sub)
        mu = np.concatenate([[253, 5, 250], A[0][:40]])
        mi = np.concatenate([[3, 63, HOT], A[1][:40]])
        gone = ~np.isin(mu * 1000 + mi, D[0] * 1000 + D[1])
        found, removed = sub.als_remove(*ids(d, mu[gone], mi[gone]))
        assert not found.any() and removed == 0 and gone.sum() > 30
        same_state(sub, before, "all misses")


# ---------------------------------------------------------------------------------------------
# 3. training afterwards is the twin's

@pytest.mark.parametrize("mode,k", [(F64, 8), (F32, 8), (F32, 130)])
def test_training_after_remove_is_the_twin_s(monkeypatch, mode, k):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    set_knob(monkeypatch, "als_slabs", 3)
    d, b = removal_problem(), the_batch()
    alive = b["alive"]
    with prepared(mode, k) as sub, twin_of(mode, k, alive) as twin:
        sub.als_remove(*ids(d, b["bu"], b["bi"]))
        for how in HOWS:
            for ctx in (sub, twin):
                full_run(ctx, 2, how)
            same_factors(sub, twin, (how, k))
        assert sub.als_nonneg_stats() == twin.als_nonneg_stats()


# ---------------------------------------------------------------------------------------------
# 4. whole rows

@pytest.mark.parametrize("side", [L.SIDE_USER, L.SIDE_ITEM])
@pytest.mark.parametrize("mode", MODES)
def test_remove_rows(monkeypatch, mode, side):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    d = removal_problem()
    hu, hi, hr = d["hu"], d["hi"], d["hr"]
    if side == L.SIDE_ITEM:
        named, table, hist = [HOT, 33, 33], d["iid"], hi                   # the hot item, another, a duplicate
    else:
        named, table, hist = [43, 77, 43], d["uid"], hu                    # a 64-rating user, another, a duplicate
    alive = ~np.isin(hist, named)
    with prepared(mode, 8) as sub, twin_of(mode, 8, alive) as twin:
        # a known id without ratings: one the model holds through set_factors alone
        lonely = int(table[255 if side == L.SIDE_USER else 63])
        for ctx in (sub, twin):
            ctx.set_factors(side, np.array([lonely], np.int32), np.full((1, 8), 0.25))
        unknown = int(table.max()) + 17
        arg = np.array([table[named[0]], unknown, table[named[1]], lonely, table[named[2]]], np.int32)
        assert sub.als_remove_rows(side, arg) == (~alive).sum()
        same_csrs(sub, expected_csrs(hu, hi, hr, alive, mode, *row_maps(hu, hi)), "numpy")
        same_csrs(sub, twin, "twin")
        assert sub.als_remove_rows(side, arg) == 0                         # nothing left to remove
        same_csrs(sub, twin, "again")
        same_factors(sub, twin, "rows stay")
        for how in (HOWS[0], HOWS[1]):
            for ctx in (sub, twin):
                full_run(ctx, 2, how)
            same_factors(sub, twin, how)


# ---------------------------------------------------------------------------------------------
# 5. retract is its definition

@pytest.mark.parametrize("rounds", [0, 1, 2])
@pytest.mark.parametrize("mode,how", [(F64, HOWS[0]), (F32, HOWS[3])])
def test_retract_is_remove_then_users_then_items(monkeypatch, mode, how, rounds):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    d, b = removal_problem(), the_batch()
    bu, bi = ids(d, b["bu"], b["bi"])
    solve = als_solve(LAM, **how)
    with prepared(mode, 8) as sub, prepared(mode, 8) as twin:
        for ctx in (sub, twin):
            full_run(ctx, 2, how)
        found, removed, su, si = sub.als_retract(bu, bi, solve, rounds)
        t_found, t_removed = twin.als_remove(bu, bi)
        tu = ti = 0
        for _ in range(rounds):
            tu = twin.als_run_rows(L.SIDE_USER, bu, solve)
            ti = twin.als_run_rows(L.SIDE_ITEM, bi, solve)
        assert np.array_equal(found, t_found) and removed == t_removed and (su, si) == (tu, ti)
        if rounds:
            assert 0 < su < len(np.unique(bu)) and 0 < si < len(np.unique(bi))     # emptied and unknown rows fall out
        same_csrs(sub, twin, "retract")
        same_factors(sub, twin, (how, rounds))
        assert sub.als_nonneg_stats() == twin.als_nonneg_stats()
        full_run(sub, 1, how)
        full_run(twin, 1, how)
        same_factors(sub, twin, "the next half-sweep")


# ---------------------------------------------------------------------------------------------
# 6. state and errors

def raw_remove(ctx, u, i, n):
    return L.lib().mf_als_remove(ctx._h, None if u is None else L.ptr(u, C.c_int32),
                                 None if i is None else L.ptr(i, C.c_int32), n, None, None)


def raw_remove_rows(ctx, side, ids_, n):
    return L.lib().mf_als_remove_rows(ctx._h, side, None if ids_ is None else L.ptr(ids_, C.c_int32), n, None)


def raw_retract(ctx, u, i, n, how, rounds):
    return L.lib().mf_als_retract(ctx._h, None if u is None else L.ptr(u, C.c_int32),
                                  None if i is None else L.ptr(i, C.c_int32), n,
                                  None if how is None else C.byref(how), rounds, None, None, None, None)


@pytest.mark.parametrize("mode", MODES)
def test_state_and_errors(monkeypatch, mode):
    set_knob(monkeypatch, "als_chunk", 8)
    rng = np.random.default_rng(5)
    u, i, r = small_problem(rng)
    u, i = np.ascontiguousarray(u), np.ascontiguousarray(i)
    bu, bi = u[:50].copy(), i[:50].copy()
    good = als_solve(LAM)

    def all_three(ctx, want):
        assert raw_remove(ctx, bu, bi, len(bu)) == want
        assert raw_remove_rows(ctx, L.SIDE_USER, bu, len(bu)) == want
        assert raw_retract(ctx, bu, bi, len(bu), good, 1) == want

    with make_ctx(8, mode) as ctx:
        all_three(ctx, L.MF_ERR_STATE)                                     # before mf_als_prepare
        ctx.als_prepare(u, i, r)
        ctx.als_run(2, LAM)
        before = state_of(ctx)
        assert raw_remove(ctx, bu, bi, -1) == L.MF_ERR_INVALID
        assert raw_remove(ctx, bu, bi, 2**31) == L.MF_ERR_INVALID
        assert raw_remove(ctx, None, bi, len(bu)) == L.MF_ERR_INVALID
        assert raw_remove(ctx, bu, None, len(bu)) == L.MF_ERR_INVALID
        assert raw_remove(ctx, None, None, 0) == L.MF_OK                   # n == 0: a no-op, NULL arrays allowed
        assert raw_remove_rows(ctx, 2, bu, len(bu)) == L.MF_ERR_INVALID
        assert raw_remove_rows(ctx, -1, bu, len(bu)) == L.MF_ERR_INVALID
        assert raw_remove_rows(ctx, L.SIDE_USER, bu, -1) == L.MF_ERR_INVALID
        assert raw_remove_rows(ctx, L.SIDE_USER, None, 3) == L.MF_ERR_INVALID
        assert raw_remove_rows(ctx, L.SIDE_USER, None, 0) == L.MF_OK
        for how in bad_hows() + [None]:
            assert raw_retract(ctx, bu, bi, len(bu), how, 1) == L.MF_ERR_INVALID
        assert raw_retract(ctx, bu, bi, len(bu), good, -1) == L.MF_ERR_INVALID
        assert raw_retract(ctx, bu, bi, -1, good, 1) == L.MF_ERR_INVALID
        assert raw_retract(ctx, bu, bi, 2**31, good, 1) == L.MF_ERR_INVALID
        assert raw_retract(ctx, None, bi, len(bu), good, 1) == L.MF_ERR_INVALID
        assert raw_retract(ctx, bu, None, len(bu), good, 1) == L.MF_ERR_INVALID
        assert raw_retract(ctx, None, None, 0, good, 1) == L.MF_OK
        same_state(ctx, before, "failing calls")
        # the counter and the NNLS statistics survive a remove
        ctx.als_run_nonneg(1, LAM)                                         # half-sweep 2: the item side
        stats = ctx.als_nonneg_stats()
        assert stats["rows"] > 0
        assert ctx.als_remove(bu, bi)[1] == 50
        assert ctx.als_nonneg_stats() == stats
        users = ctx.factors(L.SIDE_USER)[1]
        items = ctx.factors(L.SIDE_ITEM)[1]
        ctx.als_run(1, LAM)                                                # half-sweep 3: the user side
        assert not np.array_equal(bits(ctx.factors(L.SIDE_USER)[1]), bits(users))
        assert np.array_equal(bits(ctx.factors(L.SIDE_ITEM)[1]), bits(items))
        ctx.prepare(u, i, r)                                               # mf_dsgd_prepare
        all_three(ctx, L.MF_ERR_STATE)
        ctx.als_prepare(u, i, r)
        assert raw_remove(ctx, bu, bi, len(bu)) == L.MF_OK
        ctx.fit(u, i, r)                                                   # mf_dsgd_fit
        all_three(ctx, L.MF_ERR_STATE)
    with make_ctx(257, mode) as wide:                                      # a rank above 256
        all_three(wide, L.MF_ERR_INVALID)
    p = L.default_params()
    p.num_factors = 8
    p.mode = mode
    with Context(p, rank=(0, 1, 0, b"")) as ranked:                        # a rank-mode context (one rank)
        all_three(ranked, L.MF_ERR_STATE)


# ---------------------------------------------------------------------------------------------
# 7. StreamingALS.forget

def test_streaming_als_forgets():
    """fit, update, forget the same batch: the data is that of a twin that never trained on the batch, and a
    refit from the same factors equals the twin's.  The twin must hold the batch's new ids, so it appends the
    batch and removes it again."""
    import mfhip
    rng = np.random.default_rng(3)
    u, i, r = small_problem(rng)
    new = (np.concatenate([np.full(6, 900), u[:10]]).astype(np.int32),
           np.concatenate([np.arange(6), np.full(10, 77)]).astype(np.int32), rng.integers(1, 11, 16) / 2.0)
    s = mfhip.StreamingALS(rank=8, lambda_=LAM, seed=5)
    twin = mfhip.StreamingALS(rank=8, lambda_=LAM, seed=5)
    try:
        s.fit((u, i, r), iterations=2)
        twin.fit((u, i, r), iterations=2)
        s.update(new)
        # user 900 and item 77 are left without a rating: they are not solved
        assert s.forget((new[0], new[1])) == (16, len(np.unique(u[:10])), 6)
        twin._ctx.als_append(*new)
        assert twin._ctx.als_remove(new[0], new[1])[1] == 16
        same_csrs(s._ctx, twin._ctx, "forget")
        for side in (L.SIDE_USER, L.SIDE_ITEM):      # the rows update and forget solved, as the subject left them
            twin._ctx.set_factors(side, *s._ctx.factors(side))
        s.refit(2)
        twin.refit(2)
        same_factors(s._ctx, twin._ctx, "refit")
        # with rounds: the users and items that still have ratings are solved, user 900 and item 77 are not
        removed, su, si = s.forget((u[:5], i[:5]), rounds=1)
        assert removed == 5 and 0 < su <= 5 and 0 < si <= 5
        assert s.forget([(900, 0), (12345, 1)], rounds=1) == (0, 0, 2)
    finally:
        s.close()
        twin.close()
