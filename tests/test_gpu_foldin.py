"""Stateless ALS fold-in on the device: mf_als_foldin, mf_recommend_foldin.

Two yardsticks.  The twin: a context prepared on the same data that takes every session in as a new row
(zero factors through mf_set_factors, the kept entries through mf_als_append) and solves it with
mf_als_run_rows -- the fold-in vector must be that row bit for bit, for all six kinds of solve.  The planted
problems of als_support, whose solutions are integers known before the device is called: the independent
reference.  Beside them: nothing of the context changes, results do not depend on batching or order, a
context without prepared data folds in, and the fused call is the two-call route.

The data (fold_problem): als_support.small_problem (40 users, 25 items, 400 ratings) plus one hot item of 700
ratings; every user and every item is rated, so the twin's appends leave the row lists G is summed over alone.
Both sides' factors are set before the prepare, so that two contexts hold the same rows in the same order."""
import functools

import numpy as np
import pytest

from als_support import (MODES, N_ITEMS, REGS, TINY, bits, explicit_problem, first_difference, frozen,
                         implicit_problem, make_ctx, shuffled_ids, small_problem)
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context, als_solve

pytestmark = pytest.mark.gpu

F64, F32 = L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32
LAM, ALPHA, CG = 0.05, 0.7, 3
NU, NI = 40, 26
HOWS = [dict(), dict(implicit=True, alpha=ALPHA), dict(solver="cg", cg_steps=CG),
        dict(implicit=True, alpha=ALPHA, solver="cg", cg_steps=CG), dict(solver="nnls"),
        dict(implicit=True, alpha=ALPHA, solver="nnls")]
UNKNOWN = 10 ** 6            # ids from here on name nothing


def how_of(h, lam=LAM, reg=L.ALS_REG_WEIGHTED):
    return als_solve(lam, reg, h.get("implicit", False), h.get("alpha", 0.0), h.get("solver", "cholesky"),
                     h.get("cg_steps", CG))


@functools.lru_cache(maxsize=None)
def fold_problem():
    rng = np.random.default_rng(2024)
    u, i, r = small_problem(rng)
    u = np.concatenate([u, rng.integers(0, NU, 700)])
    i = np.concatenate([i, np.full(700, NI - 1)])
    r = np.concatenate([r, rng.integers(1, 11, 700) / 2.0])
    perm = rng.permutation(len(u))
    u, i, r = u[perm], i[perm], r[perm]
    assert len(np.unique(u)) == NU and len(np.unique(i)) == NI      # every row of both sides is rated
    return frozen(dict(u=u, i=i, r=r, uid=shuffled_ids(rng, NU), iid=shuffled_ids(rng, NI, 5),
                       vec=rng.uniform(-1.0, 1.0, (NU + NI, 256))))


def held(k, mode):
    """A context that holds both sides' rows (users first, in uid / iid order) and no prepared data."""
    d = fold_problem()
    ctx = make_ctx(k, mode)
    ctx.set_factors(L.SIDE_USER, d["uid"], d["vec"][:NU, :k])
    ctx.set_factors(L.SIDE_ITEM, d["iid"], d["vec"][NU:, :k])
    return ctx


def prepared(k, mode):
    d = fold_problem()
    ctx = held(k, mode)
    ctx.als_prepare(d["uid"][d["u"]], d["iid"][d["i"]], d["r"])
    return ctx


def sessions_of(side, lengths, seed=7, special=True):
    """Sessions as (ids, ratings, kept mask) naming the other side: one per kept length in `lengths` and, with
    `special`, one with a repeated id, one with unknown ids interleaved, one of unknown ids only and one with
    ratings 0, -1.5 and 1e-50 (n+ is 1 in f64 and 0 in f32)."""
    d = fold_problem()
    cid, n = (d["iid"], NI) if side == L.SIDE_USER else (d["uid"], NU)
    rng = np.random.default_rng(seed)
    out = []
    for c in lengths:
        out.append((cid[rng.integers(0, n, c)], rng.integers(1, 11, c) / 2.0))
    if special:
        out.append((cid[[3, 3, 7, 3]], np.array([4.0, 1.5, 2.0, 5.0])))
        mix = np.array([UNKNOWN, cid[1], UNKNOWN + 1, cid[5], cid[2], UNKNOWN + 2, cid[9], UNKNOWN, cid[4]])
        out.append((mix, rng.integers(1, 11, len(mix)) / 2.0))
        out.append((np.array([UNKNOWN + 3, UNKNOWN + 4, UNKNOWN + 3]), np.array([1.0, 2.0, 3.0])))
        out.append((cid[[0, 6, 8]], np.array([0.0, -1.5, 1e-50])))
    known = set(int(x) for x in cid)
    return [(np.asarray(a, np.int32), np.asarray(b, np.float64), np.array([int(x) in known for x in a], bool))
            for a, b in out]


def lists_of(sessions):
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in sessions])]).astype(np.int64)
    ids = np.concatenate([s[0] for s in sessions]) if sessions else np.zeros(0, np.int32)
    r = np.concatenate([s[1] for s in sessions]) if sessions else np.zeros(0)
    return off, ids.astype(np.int32), r.astype(np.float64)


def kept_counts(sessions):
    return np.array([int(s[2].sum()) for s in sessions], np.int32)


class Twin:
    """The twin context: every session with a kept entry is a fresh row of `side` holding exactly its kept
    entries in list order; solve(how) zeroes those rows and runs mf_als_run_rows over them."""

    def __init__(self, ctx, side, sessions, k):
        self.ctx, self.side, self.k = ctx, side, k
        self.kept = kept_counts(sessions)
        self.fresh = (2 * 10 ** 6 + np.arange(len(sessions))).astype(np.int32)
        self.live = self.fresh[self.kept > 0]
        ctx.set_factors(side, self.live, np.zeros((len(self.live), k)))
        me = np.concatenate([np.full(int(c), f) for c, f in zip(self.kept, self.fresh)]).astype(np.int32)
        other = np.concatenate([s[0][s[2]] for s in sessions]).astype(np.int32)
        r = np.concatenate([s[1][s[2]] for s in sessions])
        ctx.als_append(*((me, other, r) if side == L.SIDE_USER else (other, me, r)))

    def solve(self, how):
        self.ctx.set_factors(self.side, self.live, np.zeros((len(self.live), self.k)))
        assert self.ctx.als_run_rows(self.side, self.live, how) == len(self.live)
        want = np.zeros((len(self.fresh), self.k))
        want[self.kept > 0] = self.ctx.lookup(self.side, self.live)[0]
        return want


def check_against_twin(k, mode, side, sessions, hows):
    off, ids, r = lists_of(sessions)
    with prepared(k, mode) as sub, prepared(k, mode) as twin_ctx:
        twin = Twin(twin_ctx, side, sessions, k)
        for h in hows:
            how = how_of(h)
            vecs, used = sub.als_foldin(side, off, ids, r, how)
            want = twin.solve(how)
            assert np.array_equal(used, twin.kept), (h, used, twin.kept)
            assert np.array_equal(bits(vecs), bits(want)), (k, mode, side, h, first_difference(vecs, want))
            assert not bits(vecs[twin.kept == 0]).any()          # no kept entry: +0


# ---------------------------------------------------------------------------------------------
# 1. the twin, bit for bit

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [None, 16])
def test_foldin_is_the_twins_row_bit_for_bit(monkeypatch, mode, chunk):
    """Kept lengths 0, 1, 2, 3, 31, 32, 33 (the LDS tile is 32 ratings, one MFMA takes two) and, under
    als_chunk=16, 16, 17 and 40 (one, two and three chunks), a repeated item, unknown ids interleaved, only
    unknown ids, and ratings 0, -1.5, 1e-50: for all six kinds of solve the vector is the twin's row."""
    if chunk:
        set_knob(monkeypatch, "als_chunk", chunk)
    lengths = [0, 1, 2, 3, 31, 32, 33] + ([16, 17, 40] if chunk else [])
    sessions = sessions_of(L.SIDE_USER, lengths)
    assert kept_counts(sessions).tolist() == lengths + [4, 5, 0, 3]
    check_against_twin(8, mode, L.SIDE_USER, sessions, HOWS)


@pytest.mark.parametrize("mode", MODES)
def test_foldin_of_items_is_the_twins_row(monkeypatch, mode):
    """side = MF_SIDE_ITEM: the lists name users, the vectors are item vectors (a cold-start item)."""
    set_knob(monkeypatch, "als_chunk", 16)
    check_against_twin(8, mode, L.SIDE_ITEM, sessions_of(L.SIDE_ITEM, [0, 1, 33, 40], seed=8), HOWS)


# ---------------------------------------------------------------------------------------------
# 2. planted solutions: the independent reference

FOLD = [0, 2, 11]


def planted_lists(d):
    keep = ~np.isin(d["pi"], FOLD)
    pos = [np.flatnonzero(d["pi"] == t) for t in FOLD]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    at = np.concatenate(pos)
    return keep, off, d["uids"][d["pu"][at]].astype(np.int32), d["r"][at]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [None, 16])
def test_planted_explicit_rows_are_exact(monkeypatch, mode, chunk):
    """explicit_problem(8) prepared without the ratings of items 0, 2 and 11: folding those three lists in
    with lambda = 1e-300 gives the planted integer rows exactly, by whole rows and by chunks of 16."""
    if chunk:
        set_knob(monkeypatch, "als_chunk", chunk)
    k = 8
    d = explicit_problem(k)
    keep, off, ids, r = planted_lists(d)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
        ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
        ctx.als_prepare(d["uids"][d["pu"][keep]], d["iids"][d["pi"][keep]], d["r"][keep])
        for reg in REGS:
            vecs, used = ctx.als_foldin(L.SIDE_ITEM, off, ids, r, als_solve(TINY, reg))
            assert np.array_equal(used, np.diff(off))
            assert np.array_equal(vecs, d["X0"][FOLD]), (mode, chunk, reg, first_difference(vecs, d["X0"][FOLD]))
        assert np.array_equal(bits(ctx.lookup(L.SIDE_ITEM, d["iids"])[0]), bits(d["Q0"]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [None, 16])
def test_planted_implicit_rows_are_exact(monkeypatch, mode, chunk):
    """implicit_problem(8) likewise (alpha = 1): the rows are (I - N)^T [r > 0]; item 0 has no positive rating
    and is +0 bitwise, item 2 has a zero right-hand side that is still solved."""
    if chunk:
        set_knob(monkeypatch, "als_chunk", chunk)
    k = 8
    d = implicit_problem(k)
    keep, off, ids, r = planted_lists(d)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
        ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
        ctx.als_prepare(d["uids"][d["pu"][keep]], d["iids"][d["pi"][keep]], d["r"][keep])
        for reg in REGS:
            vecs, used = ctx.als_foldin(L.SIDE_ITEM, off, ids, r, als_solve(TINY, reg, True, 1.0))
            assert np.array_equal(used, np.diff(off))
            assert np.array_equal(vecs, d["X"][FOLD]), (mode, chunk, reg, first_difference(vecs, d["X"][FOLD]))
            assert not bits(vecs[0]).any()


# ---------------------------------------------------------------------------------------------
# 3. other ranks: the widest narrow instance and the wide kernels

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [128, 130])
def test_foldin_at_rank_128_and_130(monkeypatch, mode, k):
    set_knob(monkeypatch, "als_chunk", 16)
    check_against_twin(k, mode, L.SIDE_USER, sessions_of(L.SIDE_USER, [1, 33, 40], special=False), HOWS[:4])


# ---------------------------------------------------------------------------------------------
# 4. nothing changes

def state_of(ctx):
    return dict(fac=[ctx.factors(s) for s in (0, 1)], rows=[ctx.num_factors(s) for s in (0, 1)],
                csr=[ctx.als_csr(s) for s in (0, 1)], nnls=ctx.als_nonneg_stats(), seen=ctx.seen_count())


def same_state(ctx, before, what):
    now = state_of(ctx)
    assert now["rows"] == before["rows"] and now["nnls"] == before["nnls"] and now["seen"] == before["seen"], what
    for s in (0, 1):
        assert np.array_equal(now["fac"][s][0], before["fac"][s][0]), what
        assert np.array_equal(bits(now["fac"][s][1]), bits(before["fac"][s][1])), what
        for a, b in zip(now["csr"][s], before["csr"][s]):
            assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b), what


@pytest.mark.parametrize("mode", MODES)
def test_nothing_of_the_context_changes(monkeypatch, mode):
    """Factor bits, row counts, both CSRs, the NNLS counters and the seen set are the same after fold-ins of
    every kind, and one more half-sweep gives the bits of a context that never folded in."""
    set_knob(monkeypatch, "als_chunk", 16)
    k = 8
    off, ids, r = lists_of(sessions_of(L.SIDE_USER, [0, 1, 17, 33, 40]))
    ioff, iids, ir = lists_of(sessions_of(L.SIDE_ITEM, [2, 40], seed=9))
    with prepared(k, mode) as sub, prepared(k, mode) as ctl:
        for ctx in (sub, ctl):
            ctx.seen_from_als()
            ctx.als_run_nonneg(1, LAM)              # the counters are not zero
        before = state_of(sub)
        assert before["nnls"]["rows"] > 0 and before["seen"] > 0
        for h in HOWS:
            sub.als_foldin(L.SIDE_USER, off, ids, r, how_of(h))
            sub.als_foldin(L.SIDE_ITEM, ioff, iids, ir, how_of(h))
            for ex in (False, True):
                sub.recommend_foldin(L.SIDE_USER, off, ids, r, how_of(h), 5, exclude_rated=ex, vectors=ex)
            same_state(sub, before, h)
        for ctx in (sub, ctl):
            ctx.als_run(1, LAM)
        for s in (0, 1):
            assert np.array_equal(bits(sub.factors(s)[1]), bits(ctl.factors(s)[1]))


# ---------------------------------------------------------------------------------------------
# 5. batching and order

@pytest.mark.parametrize("mode", MODES)
def test_results_do_not_depend_on_batching_or_order(monkeypatch, mode):
    set_knob(monkeypatch, "als_chunk", 16)
    k = 8
    sessions = sessions_of(L.SIDE_USER, [0, 1, 2, 17, 33, 40])
    off, ids, r = lists_of(sessions)
    perm = np.random.default_rng(3).permutation(len(sessions))
    poff, pids, pr = lists_of([sessions[j] for j in perm])
    with prepared(k, mode) as ctx:
        for h in HOWS:
            how = how_of(h)
            base = ctx.als_foldin(L.SIDE_USER, off, ids, r, how)
            fused = ctx.recommend_foldin(L.SIDE_USER, off, ids, r, how, 7, vectors=True)
            for B in (1, 3):
                with monkeypatch.context() as mp:
                    set_knob(mp, "foldin_batch", B)
                    got = ctx.als_foldin(L.SIDE_USER, off, ids, r, how)
                    gotf = ctx.recommend_foldin(L.SIDE_USER, off, ids, r, how, 7, vectors=True)
                assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[1], base[1]), (h, B)
                for a, b in zip(gotf, fused):
                    assert np.array_equal(bits(a) if a.dtype == np.float64 else a,
                                          bits(b) if b.dtype == np.float64 else b), (h, B)
            got = ctx.als_foldin(L.SIDE_USER, poff, pids, pr, how)
            assert np.array_equal(bits(got[0]), bits(base[0][perm])) and np.array_equal(got[1], base[1][perm]), h


# ---------------------------------------------------------------------------------------------
# 6. no prepared data

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [None, 16])
def test_a_context_without_prepared_data_folds_in(monkeypatch, mode, chunk):
    """The same factors through mf_set_factors only: the explicit vectors are the prepared context's, and the
    implicit ones too, because in the prepared context every counterpart row is rated (G over all rows)."""
    if chunk:
        set_knob(monkeypatch, "als_chunk", chunk)
    k = 8
    off, ids, r = lists_of(sessions_of(L.SIDE_USER, [0, 1, 17, 33, 40]))
    with prepared(k, mode) as full, held(k, mode) as bare:
        for h in HOWS:
            want = full.als_foldin(L.SIDE_USER, off, ids, r, how_of(h))
            got = bare.als_foldin(L.SIDE_USER, off, ids, r, how_of(h))
            assert np.array_equal(got[1], want[1]), h
            assert np.array_equal(bits(got[0]), bits(want[0])), (mode, chunk, h, first_difference(got[0], want[0]))
        want = full.recommend_foldin(L.SIDE_USER, off, ids, r, how_of(HOWS[1]), 5)
        got = bare.recommend_foldin(L.SIDE_USER, off, ids, r, how_of(HOWS[1]), 5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        assert np.array_equal(got[2], want[2])


def test_a_prepare_of_nothing_is_prepared_and_its_gram_is_zero():
    """mf_als_prepare with n = 0 is "prepared": implicit G is summed over no row.  With G = 0 and one rating r
    on item q the system is (alpha r q q^T + lambda I) x = (1 + alpha r) q, so x = q (1 + alpha r) /
    (alpha r |q|^2 + lambda); a G over the held rows would give something else."""
    k = 8
    d = fold_problem()
    with held(k, F64) as ctx:
        e = np.zeros(0, np.int32)
        ctx.als_prepare(e, e, np.zeros(0))
        q = ctx.lookup(L.SIDE_ITEM, d["iid"][[4]])[0][0]
        vecs, used = ctx.als_foldin(L.SIDE_USER, np.array([0, 1]), d["iid"][[4]], np.array([2.0]),
                                    als_solve(LAM, L.ALS_REG_WEIGHTED, True, ALPHA))
        want = q * (1 + ALPHA * 2.0) / (ALPHA * 2.0 * (q @ q) + LAM)
        assert used.tolist() == [1]
        # one rank-1 system in f64: a few roundings in A, the factorisation and the substitutions
        assert np.allclose(vecs[0], want, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------
# 7. the fused call

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("knobs", [None, dict(rec_batch=2, rec_split=3)])
def test_fused_call_is_foldin_then_recommend_vectors(monkeypatch, mode, knobs):
    """ids, scores and counts of mf_recommend_foldin are those of mf_als_foldin followed by
    mf_recommend_vectors with the kept pairs as explicit exclusions (exclude_rated = 1) or none (0), at top_n
    1, 10 and 128 (more than the 26 candidates: the count clamps); a session without a kept entry has count 0
    and zeroed slots; vecs_out is mf_als_foldin's."""
    for a, b in (knobs or {}).items():
        set_knob(monkeypatch, a, b)
    k = 8
    sessions = sessions_of(L.SIDE_USER, [0, 1, 3, 33])
    off, ids, r = lists_of(sessions)
    kept = kept_counts(sessions)
    eq = np.concatenate([np.full(int(s[2].sum()), j) for j, s in enumerate(sessions)]).astype(np.int64)
    ec = np.concatenate([s[0][s[2]] for s in sessions]).astype(np.int32)
    with prepared(k, mode) as ctx:
        for h in (HOWS[0], HOWS[1], HOWS[3], HOWS[4]):
            how = how_of(h)
            vecs, used = ctx.als_foldin(L.SIDE_USER, off, ids, r, how)
            for top_n in (1, 10, 128):
                for ex in (0, 1):
                    wid, wsc, wcnt = ctx.recommend_vectors(vecs, top_n, side=L.SIDE_ITEM,
                                                           exclude=(eq, ec) if ex else None)
                    wid[kept == 0], wsc[kept == 0], wcnt[kept == 0] = 0, 0.0, 0
                    gid, gsc, gcnt, gvec, gused = ctx.recommend_foldin(L.SIDE_USER, off, ids, r, how, top_n,
                                                                       exclude_rated=bool(ex), vectors=True)
                    what = (mode, knobs, h, top_n, ex)
                    assert np.array_equal(gcnt, wcnt), (what, gcnt, wcnt)
                    assert np.array_equal(gid, wid), what
                    assert np.array_equal(bits(gsc), bits(wsc)), what
                    assert np.array_equal(bits(gvec), bits(vecs)) and np.array_equal(gused, used), what
                    if top_n == 128:
                        distinct = np.array([len(set(s[0][s[2]].tolist())) for s in sessions])
                        assert np.array_equal(gcnt[kept > 0], (NI - distinct * ex)[kept > 0]), what
                    gid2, gsc2, gcnt2, gvec2, _ = ctx.recommend_foldin(L.SIDE_USER, off, ids, r, how, top_n,
                                                                       exclude_rated=bool(ex), scores=False)
                    assert gsc2 is None and gvec2 is None
                    assert np.array_equal(gid2, gid) and np.array_equal(gcnt2, gcnt), what


def test_the_model_class_recommends_for_sessions():
    import mfhip
    d = fold_problem()
    model = mfhip.als.MatrixFactorizationModel(prepared(8, F64))
    try:
        basket = d["iid"][[1, 2, 3]]
        got = model.recommendProductsForSessions([(basket, [5.0, 4.0, 3.0]), ([UNKNOWN], [1.0])], 4, lambda_=LAM)
        assert len(got) == 2 and len(got[0]) == 4 and got[1] == []
        assert not set(p for p, _ in got[0]) & set(int(x) for x in basket)
        assert [s for _, s in got[0]] == sorted((s for _, s in got[0]), reverse=True)
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------
# 8. state and errors

def code(f, *a, **kw):
    try:
        f(*a, **kw)
    except L.MFError as e:
        return e.code
    return L.MF_OK


def test_state_errors_and_a_failing_call_changes_nothing():
    k = 8
    off, ids, r = lists_of(sessions_of(L.SIDE_USER, [1, 3]))
    how = how_of(HOWS[0])
    with make_ctx(k, F64) as empty:
        assert code(empty.als_foldin, L.SIDE_USER, off, ids, r, how) == L.MF_ERR_NOT_FITTED
        assert code(empty.recommend_foldin, L.SIDE_USER, off, ids, r, how, 5) == L.MF_ERR_NOT_FITTED
    p = L.default_params()
    p.num_factors = k
    with Context(p, rank=(0, 1, 0, b"")) as ctx:          # a rank-mode context
        assert code(ctx.als_foldin, L.SIDE_USER, off, ids, r, how) == L.MF_ERR_STATE
    if L.device_count() >= 2:
        p.num_blocks = 2
        with Context(p, n_devices=2) as ctx:
            assert code(ctx.als_foldin, L.SIDE_USER, off, ids, r, how) == L.MF_ERR_STATE
            assert code(ctx.recommend_foldin, L.SIDE_USER, off, ids, r, how, 5) == L.MF_ERR_STATE
    with prepared(k, F64) as ctx:
        ctx.seen_from_als()
        before = state_of(ctx)
        bad_off = off.copy()
        bad_off[1] = off[2] + 1
        assert code(ctx.als_foldin, 2, off, ids, r, how) == L.MF_ERR_INVALID
        assert code(ctx.als_foldin, L.SIDE_USER, off, ids, r, als_solve(-1.0)) == L.MF_ERR_INVALID
        assert code(ctx.als_foldin, L.SIDE_USER, off, ids, r, als_solve(LAM, solver="cg", cg_steps=0)) == L.MF_ERR_INVALID
        assert code(ctx.recommend_foldin, L.SIDE_USER, off, ids, r, how, 0) == L.MF_ERR_INVALID
        assert code(ctx.recommend_foldin, L.SIDE_USER, off, ids, r, how, L.RECOMMEND_MAX_TOP + 1) == L.MF_ERR_INVALID
        st = L.lib().mf_als_foldin(ctx._h, L.SIDE_USER, L.ptr(bad_off, L.C.c_int64), L.ptr(ids, L.C.c_int32),
                                   L.ptr(r, L.C.c_double), 2, L.C.byref(how), L.ptr(np.zeros((2, k)), L.C.c_double), None)
        assert st == L.MF_ERR_INVALID
        same_state(ctx, before, "failing calls")
        e = np.zeros(0, np.int32)
        vecs, used = ctx.als_foldin(L.SIDE_USER, np.zeros(1, np.int64), e, np.zeros(0), how)   # n_queries == 0
        assert vecs.shape == (0, k) and used.shape == (0,)
        # used_out may be NULL
        out = np.full((2, k), 7.0)
        assert L.lib().mf_als_foldin(ctx._h, L.SIDE_USER, L.ptr(off, L.C.c_int64), L.ptr(ids, L.C.c_int32),
                                     L.ptr(r, L.C.c_double), 2, L.C.byref(how), L.ptr(out, L.C.c_double), None) == L.MF_OK
        assert np.array_equal(bits(out), bits(ctx.als_foldin(L.SIDE_USER, off, ids, r, how)[0][:2]))
        same_state(ctx, before, "after valid calls")
