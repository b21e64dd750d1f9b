"""Incremental ALS on the device: mf_als_append, mf_als_run_rows, mf_als_update.

The yardstick throughout is a twin context that gets the same ratings through mf_als_prepare alone: append
must leave the CSR that prepare builds from the concatenation (checked against the twin and against numpy's
stable grouping), training afterwards must be the twin's bit for bit, a row solved by mf_als_run_rows must be
the row a full half-sweep of the twin stores, and mf_als_update must be its definition.

The stream (stream_problem): als_support.small_problem (40 users, 25 items, 400 ratings) plus one hot item of
700 ratings (three 256-thread workgroups' worth of entries for the move kernel's lanes, a split row at any
chunk length used here), users of exactly 0, 1, 63, 64 and 65 ratings, ids from shuffled_ids (half of them
negative), cut into a prepared part A and appended parts B, C, D (one rating) and E (none).  Most cases run
with als_chunk=8, als_batch=4: a handful of rows is then split rows and several launches.

Not covered: MF_ERR_INVALID for a row that would pass 2^31 - 1 ratings (it needs an 8 GB row)."""
import ctypes as C
import functools

import numpy as np
import pytest

from als_support import (MODES, N_ITEMS, TINY, bits, dtype_of, explicit_problem, first_difference, frozen,
                         implicit_problem, make_ctx, rows_of, shuffled_ids, small_problem)
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import als_solve

pytestmark = pytest.mark.gpu

F64, F32 = L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32
LAM, ALPHA, CG = 0.05, 0.7, 3
NU, NI, HOT = 40, 25, 25                 # small_problem's users and items; the hot item's index
U_NONE, U_LATE, U_NEVER = 40, 47, 49     # a held user rated from B on; one set between prepare and append; never rated
I_HELD, I_NEVER = 28, 29                 # a held item rated from B on; a held item never rated
N_USERS, N_ITEMS_ALL = 50, 30


@functools.lru_cache(maxsize=None)
def stream_problem():
    """Index arrays (ids are uid[...] / iid[...]) of the parts A, B, C, D, E and what the model holds beforehand."""
    rng = np.random.default_rng(4711)
    u, i, r = small_problem(rng)
    u = np.concatenate([u, rng.integers(0, NU, 700)])
    i = np.concatenate([i, np.full(700, HOT)])
    r = np.concatenate([r, rng.integers(1, 11, 700) / 2.0])
    for a, c in ((41, 1), (42, 63), (43, 64), (44, 65)):           # rows of exactly 1, 63, 64 and 65 ratings
        u = np.concatenate([u, np.full(c, a)])
        i = np.concatenate([i, rng.integers(0, NI + 1, c)])
        r = np.concatenate([r, rng.integers(1, 11, c) / 2.0])
    perm = rng.permutation(len(u))
    u, i, r = u[perm], i[perm], r[perm]
    # user 44 must cross 64 ratings through an append: its first 60 in A, the last 5 later
    late44 = np.flatnonzero(u == 44)[60:]
    na, nb = int(0.55 * len(u)), int(0.8 * len(u))
    part = np.where(np.arange(len(u)) < na, 0, np.where(np.arange(len(u)) < nb, 1, 2))
    part[np.flatnonzero(u == 44)[:60]] = 0
    part[late44] = 2
    A = [u[part == 0], i[part == 0], r[part == 0]]
    B = [u[part == 1], i[part == 1], r[part == 1]]
    Cc = [u[part == 2], i[part == 2], r[part == 2]]
    # user 48: 7 ratings in A, 2 in B -- crosses a chunk of 8 through the append
    A = [np.concatenate([A[0], np.full(7, 48)]), np.concatenate([A[1], rng.integers(0, NI, 7)]),
         np.concatenate([A[2], rng.integers(1, 11, 7) / 2.0])]
    extra_b = [
        (48, 3, 4.0), (48, 4, 1.5),
        (int(A[0][0]), int(A[1][0]), 2.5),        # a repeat of an existing pair
        (U_NONE, 2, 3.0), (3, I_HELD, 4.5),       # ids held through set_factors, no rating in A
        (45, 26, 5.0), (45, 5, -1.5), (2, 26, 0.0),   # unseen user 45 and item 26; ratings <= 0
        (7, 9, 1e-50),                            # 0 in f32: n+ differs by mode
        (U_NONE, I_HELD, -2.0),
    ]
    extra_c = [(46, 27, 2.0), (46, HOT, 3.5), (U_LATE, 27, 1.0), (U_LATE, 1, 4.0), (45, 27, 0.5), (9, 26, -0.5)]
    for part_, extra in ((B, extra_b), (Cc, extra_c)):
        eu, ei, er = (np.array(x) for x in zip(*extra))
        n = len(part_[0]) + len(eu)
        p = rng.permutation(n)                    # a row's new ratings interleaved with other rows'
        part_[0] = np.concatenate([part_[0], eu])[p]
        part_[1] = np.concatenate([part_[1], ei])[p]
        part_[2] = np.concatenate([part_[2], er])[p]
    D = [np.array([3]), np.array([HOT]), np.array([2.0])]         # an append of 1
    E = [np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)]
    parts = [(np.asarray(p[0], np.int64), np.asarray(p[1], np.int64), np.asarray(p[2], np.float64))
             for p in (A, B, Cc, D, E)]
    for p in parts:
        for x in p:
            x.setflags(write=False)
    uid, iid = shuffled_ids(rng, N_USERS), shuffled_ids(rng, N_ITEMS_ALL, 5)
    allu = np.concatenate([p[0] for p in parts])
    alli = np.concatenate([p[1] for p in parts])
    cnt = np.bincount(allu, minlength=N_USERS)
    assert (cnt[41], cnt[42], cnt[43], cnt[44], cnt[U_NEVER]) == (1, 63, 64, 65, 0)
    assert np.bincount(alli, minlength=N_ITEMS_ALL)[HOT] >= 700
    assert (parts[0][0] == 44).sum() == 60 and (parts[0][0] == 48).sum() == 7
    for held in (U_NONE, U_LATE, 45, 46):
        assert not (parts[0][0] == held).any()
    for held in (I_HELD, 26, 27):
        assert not (parts[0][1] == held).any()
    assert (uid < 0).sum() > 10 and (iid < 0).sum() > 5
    return frozen(dict(parts=parts, uid=uid, iid=iid,
                       held_u=np.array([U_NONE, U_NEVER]), held_i=np.array([I_HELD, I_NEVER]),
                       vec=np.random.default_rng(5).uniform(0.1, 1.0, (8, 256))))


def ids_of(d, part):
    return d["uid"][part[0]].astype(np.int32), d["iid"][part[1]].astype(np.int32), part[2]


def concat(d, parts):
    return tuple(np.concatenate([ids_of(d, p)[c] for p in parts]) for c in range(3))


def hold(ctx, d, k):
    ctx.set_factors(L.SIDE_USER, d["uid"][d["held_u"]], d["vec"][:2, :k])
    ctx.set_factors(L.SIDE_ITEM, d["iid"][d["held_i"]], d["vec"][2:4, :k])


def late(ctx, d, k):
    ctx.set_factors(L.SIDE_USER, d["uid"][[U_LATE]], d["vec"][4:5, :k])   # a row gained after the prepare


def subject_and_twin(mode, k):
    """(subject: prepare(A), a row gained, append B, C, D, E; twin: the same rows, prepare(A ++ B ++ C ++ D))."""
    d = stream_problem()
    P = d["parts"]
    sub, twin = make_ctx(k, mode), make_ctx(k, mode)
    for ctx in (sub, twin):
        hold(ctx, d, k)
        ctx.als_prepare(*ids_of(d, P[0]))
        late(ctx, d, k)
    for p in P[1:]:
        sub.als_append(*ids_of(d, p))
    twin.als_prepare(*concat(d, P))
    return d, sub, twin


def row_maps(d, parts, with_late=True):
    """id index -> factor row, first touch: the held ids, A's, the late user, then the rest."""
    um = {int(a): x for x, a in enumerate(d["held_u"])}
    im = {int(a): x for x, a in enumerate(d["held_i"])}
    for n, p in enumerate(parts):
        for a in p[0]:
            um.setdefault(int(a), len(um))
        for a in p[1]:
            im.setdefault(int(a), len(im))
        if n == 0 and with_late:
            um.setdefault(U_LATE, len(um))
    return um, im


def numpy_csr(rows, other, r, n_rows, mode):
    v = r.astype(dtype_of(mode)).astype(np.float64)
    groups = rows_of(rows, n_rows)
    order = np.concatenate(groups) if len(rows) else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    npos = np.array([(v[g] > 0).sum() for g in groups], np.int32)
    return off, other[order].astype(np.int32), v[order], npos


def same_csr(got, want, what):
    for name, g, w in zip(("off", "cols", "vals", "npos"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "vals":
            assert np.array_equal(bits(g), bits(w)), (what, name)
        else:
            assert np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:8])


def same_factors(a, b, what):
    for side in (L.SIDE_USER, L.SIDE_ITEM):
        ia, va = a.factors(side)
        ib, vb = b.factors(side)
        assert np.array_equal(ia, ib), (what, side)
        assert np.array_equal(bits(va), bits(vb)), (what, side, first_difference(va, vb))


def state_of(ctx):
    return [ctx.als_csr(s) for s in (0, 1)], [ctx.factors(s) for s in (0, 1)]


def same_state(ctx, before, what):
    csr, fac = state_of(ctx)
    for side in (0, 1):
        same_csr(csr[side], before[0][side], what)
        assert np.array_equal(fac[side][0], before[1][side][0]), what
        assert np.array_equal(bits(fac[side][1]), bits(before[1][side][1])), what


HOWS = [dict(), dict(implicit=True, alpha=ALPHA), dict(solver="cg", cg_steps=CG),
        dict(implicit=True, alpha=ALPHA, solver="cg", cg_steps=CG), dict(solver="nnls"),
        dict(implicit=True, alpha=ALPHA, solver="nnls")]


def full_run(ctx, half_sweeps, how):
    """The mf_als_run* call that `how` names."""
    imp, solver = how.get("implicit", False), how.get("solver", "cholesky")
    if solver == "cg":
        (ctx.als_run_implicit_cg(half_sweeps, LAM, ALPHA, cg_steps=CG) if imp
         else ctx.als_run_cg(half_sweeps, LAM, cg_steps=CG))
    elif solver == "nnls":
        ctx.als_run_implicit_nonneg(half_sweeps, LAM, ALPHA) if imp else ctx.als_run_nonneg(half_sweeps, LAM)
    else:
        ctx.als_run_implicit(half_sweeps, LAM, ALPHA) if imp else ctx.als_run(half_sweeps, LAM)


# ---------------------------------------------------------------------------------------------
# 1. the CSR is the concatenation's

@pytest.mark.parametrize("knobs", [dict(als_chunk=8, als_batch=4), dict(als_chunk=64)])
@pytest.mark.parametrize("mode", MODES)
def test_csr_is_the_concatenation_s(monkeypatch, mode, knobs):
    for key, v in knobs.items():
        set_knob(monkeypatch, key, v)
    d, sub, twin = subject_and_twin(mode, 8)
    with sub, twin:
        um, im = row_maps(d, d["parts"])
        allp = [np.concatenate([p[c] for p in d["parts"]]) for c in range(3)]
        ur = np.array([um[int(a)] for a in allp[0]])
        ir = np.array([im[int(a)] for a in allp[1]])
        want = [numpy_csr(ur, ir, allp[2], len(um), mode), numpy_csr(ir, ur, allp[2], len(im), mode)]
        for side in (L.SIDE_USER, L.SIDE_ITEM):
            got = sub.als_csr(side)
            same_csr(got, twin.als_csr(side), ("twin", side))
            same_csr(got, want[side], ("numpy", side))
        # 1e-50 is a positive rating in f64 and 0 in f32
        tiny_row = um[7]
        assert want[0][3][tiny_row] == (allp[2][ur == tiny_row].astype(dtype_of(mode)) > 0).sum()
        assert (numpy_csr(ur, ir, allp[2], len(um), F64)[3][tiny_row]
                == numpy_csr(ur, ir, allp[2], len(um), F32)[3][tiny_row] + 1)
        assert sub.num_factors(L.SIDE_USER) == len(um) == N_USERS and sub.num_factors(L.SIDE_ITEM) == len(im)
        same_factors(sub, twin, "after the appends")


@pytest.mark.parametrize("mode", MODES)
def test_csr_from_an_empty_start(monkeypatch, mode):
    """prepare(n = 0) is the valid empty start: append(A), append(B) is then prepare(A ++ B)."""
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    d = stream_problem()
    A, B = d["parts"][0], d["parts"][1]
    with make_ctx(8, mode) as sub, make_ctx(8, mode) as twin:
        sub.als_prepare(*ids_of(d, d["parts"][4]))
        for side in (0, 1):
            off, cols, vals, npos = sub.als_csr(side)
            assert off.tolist() == [0] and len(cols) == len(vals) == len(npos) == 0
        sub.als_append(*ids_of(d, A))
        sub.als_append(*ids_of(d, B))
        twin.als_prepare(*concat(d, [A, B]))
        for side in (0, 1):
            same_csr(sub.als_csr(side), twin.als_csr(side), side)
        same_factors(sub, twin, "empty start")
        full_run(sub, 2, {})
        full_run(twin, 2, {})
        same_factors(sub, twin, "empty start, trained")


# ---------------------------------------------------------------------------------------------
# 2. training afterwards is the twin's, bit for bit

@pytest.mark.parametrize("mode,k", [(F64, 8), (F32, 8), (F32, 130)])
def test_training_after_append_is_the_twin_s(monkeypatch, mode, k):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    set_knob(monkeypatch, "als_slabs", 3)
    d, sub, twin = subject_and_twin(mode, k)
    with sub, twin:
        for how in HOWS:
            for ctx in (sub, twin):
                full_run(ctx, 2, how)
            same_factors(sub, twin, (how, k))
        assert sub.als_nonneg_stats() == twin.als_nonneg_stats()


# ---------------------------------------------------------------------------------------------
# 3. row subsets

def subset_ids(d, side):
    """(ids, the id indices they name that have a rating): the hot split row in, another split row out;
    unknown ids, an id without a rating and duplicates among them."""
    if side == L.SIDE_ITEM:
        named, table, never = [HOT, 0, 3, 7, 26, I_HELD, 12], d["iid"], I_NEVER     # items 1, 2, 4 .. stay out
    else:
        named, table, never = [44, 42, 41, 0, 5, 45, U_LATE, 48], d["uid"], U_NEVER  # users 43 (64 ratings) .. stay out
    ids = [int(table[a]) for a in named]
    unknown = [int(table.max()) + 11, int(table.min()) - 7]
    return np.array(ids[:3] + unknown + [int(table[never])] + ids[3:] + ids[:2], np.int32), named


@pytest.mark.parametrize("how", HOWS, ids=lambda h: "-".join(f"{a}={b}" for a, b in h.items()) or "cholesky")
@pytest.mark.parametrize("mode", MODES)
def test_run_rows_is_the_half_sweep_s_rows(monkeypatch, mode, how):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    run_rows_case(mode, 8, how, (L.SIDE_ITEM, L.SIDE_USER))


def test_run_rows_wide_rank(monkeypatch):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    set_knob(monkeypatch, "als_slabs", 3)
    run_rows_case(F32, 130, {}, (L.SIDE_ITEM,))


def run_rows_case(mode, k, how, sides):
    d, sub, twin = subject_and_twin(mode, k)
    solve = als_solve(LAM, **how)
    nnls, cg = how.get("solver") == "nnls", how.get("solver") == "cg"
    with sub, twin:
        for side in sides:
            if side == L.SIDE_USER:          # the counter of both is odd here: the user side is next
                assert sides[0] == L.SIDE_ITEM
            table = d["iid"] if side == L.SIDE_ITEM else d["uid"]
            ids, named = subset_ids(d, side)
            before_ids, before = sub.factors(side)
            other_before = sub.factors(1 - side)
            stats0 = sub.als_nonneg_stats()["rows"]
            assert sub.als_run_rows(side, np.zeros(0, np.int32), solve) == 0
            assert sub.als_run_rows(side, ids[3:6], solve) == 0          # unknown ids and an id without a rating
            same_factors_side(sub, side, before_ids, before, "nothing to solve")
            solved = sub.als_run_rows(side, ids, solve)
            assert solved == len(named)
            assert sub.als_nonneg_stats()["rows"] - stats0 == (solved if nnls else 0)
            got_ids, got = sub.factors(side)
            if not cg:   # the same rows in another order: the same bits (a CG row would step on from its new value)
                assert sub.als_run_rows(side, ids[::-1].copy(), solve) == solved
                assert np.array_equal(bits(sub.factors(side)[1]), bits(got))
            full_run(twin, 1, how)           # the twin's full half-sweep of this side
            want_ids, want = twin.factors(side)
            assert np.array_equal(got_ids, want_ids)
            is_named = np.isin(got_ids, table[named])
            assert is_named.sum() == len(named)
            assert np.array_equal(bits(got[is_named]), bits(want[is_named])), (side, first_difference(got[is_named], want[is_named]))
            assert np.array_equal(bits(got[~is_named]), bits(before[~is_named])), side
            assert not np.array_equal(bits(got[is_named]), bits(before[is_named]))
            o_ids, o_vecs = sub.factors(1 - side)
            assert np.array_equal(bits(o_vecs), bits(other_before[1]))
            # the counter did not move: the subject's next half-sweep is still this side's, and ends as the twin's
            # did (a CG row steps on from the value run_rows left, so there only the other rows do)
            full_run(sub, 1, how)
            if cg:
                again = sub.factors(side)[1]
                assert np.array_equal(bits(again[~is_named]), bits(want[~is_named]))
                assert not np.array_equal(bits(again[is_named]), bits(got[is_named]))
                assert np.array_equal(bits(sub.factors(1 - side)[1]), bits(other_before[1]))
                sub.set_factors(side, want_ids, want)
            same_factors(sub, twin, ("after the subject's own half-sweep", side))


def same_factors_side(ctx, side, ids, vecs, what):
    i2, v2 = ctx.factors(side)
    assert np.array_equal(i2, ids) and np.array_equal(bits(v2), bits(vecs)), what


# ---------------------------------------------------------------------------------------------
# 4. update is its definition

@pytest.mark.parametrize("rounds", [0, 1, 2])
@pytest.mark.parametrize("mode,how", [(F64, HOWS[0]), (F32, HOWS[3]), (F64, HOWS[5]), (F32, HOWS[4])])
def test_update_is_append_then_users_then_items(monkeypatch, mode, how, rounds):
    set_knob(monkeypatch, "als_chunk", 8)
    set_knob(monkeypatch, "als_batch", 4)
    d = stream_problem()
    A, B = d["parts"][0], d["parts"][1]
    solve = als_solve(LAM, **how)
    with make_ctx(8, mode) as sub, make_ctx(8, mode) as twin:
        for ctx in (sub, twin):
            hold(ctx, d, 8)
            ctx.als_prepare(*ids_of(d, A))
            full_run(ctx, 2, how)
        bu, bi, br = ids_of(d, B)
        su, si = sub.als_update(bu, bi, br, solve, rounds)
        twin.als_append(bu, bi, br)
        tu = ti = 0
        for _ in range(rounds):
            tu = twin.als_run_rows(L.SIDE_USER, bu, solve)
            ti = twin.als_run_rows(L.SIDE_ITEM, bi, solve)
        assert (su, si) == (tu, ti)
        if rounds:
            assert su == len(np.unique(bu)) and si == len(np.unique(bi))
        for side in (0, 1):
            same_csr(sub.als_csr(side), twin.als_csr(side), side)
        same_factors(sub, twin, (how, rounds))
        assert sub.als_nonneg_stats() == twin.als_nonneg_stats()
        full_run(sub, 1, how)                # the counter: both are at 2, the item side is next on both
        full_run(twin, 1, how)
        same_factors(sub, twin, "the next half-sweep")


# ---------------------------------------------------------------------------------------------
# 5. fold-in is exact

FOLD = [0, 2, 11]        # item 2 has 200 fillers: a split row at als_chunk=16


@pytest.mark.parametrize("chunk", [None, 16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("implicit", [False, True])
def test_fold_in_is_exact(monkeypatch, mode, implicit, chunk):
    """The planted problems of the exact-solve tests, prepared without the ratings of three items; these are
    appended and the three rows solved with lambda = 1e-300: the planted integer solution, exactly."""
    if chunk:
        set_knob(monkeypatch, "als_chunk", chunk)
    k = 8
    d = implicit_problem(k) if implicit else explicit_problem(k)
    X = d["X"] if implicit else d["X0"]
    gone = np.isin(d["pi"], FOLD)
    u, i, r = d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"]
    solve = als_solve(TINY, implicit=implicit, alpha=1.0)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
        ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
        ctx.als_prepare(u[~gone], i[~gone], r[~gone])
        ctx.als_append(u[gone], i[gone], r[gone])
        assert ctx.als_run_rows(L.SIDE_ITEM, d["iids"][FOLD], solve) == len(FOLD)
        Q = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
        assert np.array_equal(Q[FOLD], X[FOLD]), (mode, implicit, chunk, first_difference(Q[FOLD], X[FOLD]))
        if implicit:
            assert np.array_equal(bits(Q[0]), bits(np.zeros(k)))       # no positive rating: +0
        rest = np.setdiff1d(np.arange(N_ITEMS + 2), FOLD)
        assert np.array_equal(bits(Q[rest]), bits(d["Q0"][rest]))
        assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, d["uids"])[0]), bits(d["P"]))


# ---------------------------------------------------------------------------------------------
# 6. a solved row's objective does not rise

def row_objective(x, Y, r, lam):
    e = r - Y @ x
    return e @ e + lam * len(r) * (x @ x)


def test_a_solved_row_s_objective_does_not_rise():
    """Cholesky, f64.  Every row an update solves is the minimiser of its regularised squared error over the
    row's whole rating list, taken against the counterpart as it stood when the row was solved (the users
    against the items before the update, the items against the users after it).  So the row's objective
    after <= before, up to rounding: the slack 1e-9 * max(1, before) is far above the k n 2^-53 < 1e-12
    relative rounding of these sums (k = 8, n <= 800) and is not a measurement."""
    rng = np.random.default_rng(77)
    u, i, r = small_problem(rng)
    uid, iid = shuffled_ids(rng, 46), shuffled_ids(rng, 28, 5)
    nu = np.concatenate([rng.integers(0, 30, 60), np.full(9, 44), np.full(5, 45), rng.integers(0, 30, 6)])
    ni = np.concatenate([rng.integers(0, 25, 60), rng.integers(0, 25, 9), np.full(5, 26), np.full(6, 27)])
    nr = rng.integers(1, 11, len(nu)) / 2.0
    solve = als_solve(LAM)
    with make_ctx(8, F64) as ctx:
        ctx.als_prepare(uid[u], iid[i], r)
        ctx.als_run(4, LAM)
        P0 = dict(zip(*ctx.factors(L.SIDE_USER)))
        Q0 = dict(zip(*ctx.factors(L.SIDE_ITEM)))
        su, si = ctx.als_update(uid[nu], iid[ni], nr, solve, 1)
        assert su == len(np.unique(nu)) and si == len(np.unique(ni))
        # rows of new ids exist only after the append: their "before" is the initial value the append gave them,
        # which a twin that only appends shows
        with make_ctx(8, F64) as twin:
            twin.als_prepare(uid[u], iid[i], r)
            twin.als_run(4, LAM)
            twin.als_append(uid[nu], iid[ni], nr)
            Pb = dict(zip(*twin.factors(L.SIDE_USER)))
            Qb = dict(zip(*twin.factors(L.SIDE_ITEM)))
        for key, v in P0.items():
            assert np.array_equal(bits(Pb[key]), bits(v))
        P1 = dict(zip(*ctx.factors(L.SIDE_USER)))
        Q1 = dict(zip(*ctx.factors(L.SIDE_ITEM)))
    au, ai, ar = np.concatenate([u, nu]), np.concatenate([i, ni]), np.concatenate([r, nr])
    checked = 0
    for a in np.unique(nu):
        pos = np.flatnonzero(au == a)
        Y = np.array([Qb[int(iid[b])] for b in ai[pos]])
        before = row_objective(Pb[int(uid[a])], Y, ar[pos], LAM)
        after = row_objective(P1[int(uid[a])], Y, ar[pos], LAM)
        print(f"user {a}: {before:.6g} -> {after:.6g}")
        assert after <= before + 1e-9 * max(1.0, before), (a, before, after)
        checked += 1
    for b in np.unique(ni):
        pos = np.flatnonzero(ai == b)
        Y = np.array([P1[int(uid[a])] for a in au[pos]])
        before = row_objective(Qb[int(iid[b])], Y, ar[pos], LAM)
        after = row_objective(Q1[int(iid[b])], Y, ar[pos], LAM)
        print(f"item {b}: {before:.6g} -> {after:.6g}")
        assert after <= before + 1e-9 * max(1.0, before), (b, before, after)
        checked += 1
    assert checked == su + si
    untouched = [key for key in P0 if key not in set(uid[nu].tolist())]
    assert untouched and all(np.array_equal(bits(P1[key]), bits(P0[key])) for key in untouched)


# ---------------------------------------------------------------------------------------------
# 7. state and errors

def raw_append(ctx, u, i, r, n):
    return L.lib().mf_als_append(ctx._h, None if u is None else L.ptr(u, C.c_int32),
                                 None if i is None else L.ptr(i, C.c_int32),
                                 None if r is None else L.ptr(r, C.c_double), n)


def raw_rows(ctx, side, ids, n, how):
    out = C.c_int64(-5)
    st = L.lib().mf_als_run_rows(ctx._h, side, None if ids is None else L.ptr(ids, C.c_int32), n,
                                 None if how is None else C.byref(how), C.byref(out))
    return st


def raw_update(ctx, u, i, r, n, how, rounds):
    return L.lib().mf_als_update(ctx._h, L.ptr(u, C.c_int32), L.ptr(i, C.c_int32), L.ptr(r, C.c_double), n,
                                 None if how is None else C.byref(how), rounds, None, None)


def bad_hows():
    out = [als_solve(0.0), als_solve(-1.0), als_solve(float("nan")), als_solve(LAM, reg=2),
           als_solve(LAM, implicit=True, alpha=-0.5), als_solve(LAM, implicit=True, alpha=float("nan")),
           als_solve(LAM, implicit=True, alpha=float("inf")), als_solve(LAM, solver="cg", cg_steps=0),
           als_solve(LAM, solver="cg", cg_steps=L.ALS_CG_MAX_STEPS + 1)]
    h = als_solve(LAM)
    h.solver = 3
    out.append(h)
    h = als_solve(LAM)
    h.solver = -1
    out.append(h)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_state_and_errors(monkeypatch, mode):
    set_knob(monkeypatch, "als_chunk", 8)
    d = stream_problem()
    A, B = d["parts"][0], d["parts"][1]
    bu, bi, br = ids_of(d, B)
    bu, bi, br = np.ascontiguousarray(bu), np.ascontiguousarray(bi), np.ascontiguousarray(br)
    good = als_solve(LAM)
    with make_ctx(8, mode) as ctx:
        # before mf_als_prepare
        assert raw_append(ctx, bu, bi, br, len(bu)) == L.MF_ERR_STATE
        assert raw_rows(ctx, L.SIDE_USER, bu, len(bu), good) == L.MF_ERR_STATE
        assert raw_update(ctx, bu, bi, br, len(bu), good, 1) == L.MF_ERR_STATE
        assert ctx.num_factors(L.SIDE_USER) == 0
        hold(ctx, d, 8)
        ctx.als_prepare(*ids_of(d, A))
        ctx.als_run(2, LAM)
        before = state_of(ctx)
        # mf_als_append
        assert raw_append(ctx, bu, bi, br, -1) == L.MF_ERR_INVALID
        assert raw_append(ctx, bu, bi, br, 2**31) == L.MF_ERR_INVALID
        for hole in range(3):
            cols = [bu, bi, br]
            cols[hole] = None
            assert raw_append(ctx, *cols, len(bu)) == L.MF_ERR_INVALID
        assert raw_append(ctx, None, None, None, 0) == L.MF_OK            # n == 0: a no-op, NULL arrays allowed
        same_state(ctx, before, "append errors")
        # mf_als_run_rows
        for how in bad_hows():
            assert raw_rows(ctx, L.SIDE_USER, bu, len(bu), how) == L.MF_ERR_INVALID, list(bytes(how))
        # (alpha and cg_steps are read only where they apply)
        for how in (als_solve(LAM, alpha=-1.0), als_solve(LAM, cg_steps=0), als_solve(LAM, solver="nnls", cg_steps=999)):
            assert raw_rows(ctx, L.SIDE_USER, bu, 0, how) == L.MF_OK
        assert raw_rows(ctx, 2, bu, len(bu), good) == L.MF_ERR_INVALID
        assert raw_rows(ctx, -1, bu, len(bu), good) == L.MF_ERR_INVALID
        assert raw_rows(ctx, L.SIDE_USER, bu, len(bu), None) == L.MF_ERR_INVALID
        assert raw_rows(ctx, L.SIDE_USER, bu, -1, good) == L.MF_ERR_INVALID
        assert raw_rows(ctx, L.SIDE_USER, None, 3, good) == L.MF_ERR_INVALID
        assert raw_rows(ctx, L.SIDE_USER, None, 0, good) == L.MF_OK
        same_state(ctx, before, "run_rows errors")
        # mf_als_update: everything is checked before the append
        for how in bad_hows() + [None]:
            assert raw_update(ctx, bu, bi, br, len(bu), how, 1) == L.MF_ERR_INVALID
        assert raw_update(ctx, bu, bi, br, len(bu), good, -1) == L.MF_ERR_INVALID
        assert raw_update(ctx, bu, bi, br, -1, good, 1) == L.MF_ERR_INVALID
        same_state(ctx, before, "update errors")
        assert ctx.num_factors(L.SIDE_USER) == len(before[1][0][0])       # no id was inserted on the way
        # the counter and the NNLS statistics survive an append
        ctx.als_run_nonneg(1, LAM)                                        # half-sweep 2: the item side
        stats = ctx.als_nonneg_stats()
        assert stats["rows"] > 0
        ctx.als_append(bu, bi, br)
        assert ctx.als_nonneg_stats() == stats
        users = ctx.factors(L.SIDE_USER)[1]
        ctx.als_run(1, LAM)                                               # half-sweep 3: the user side
        assert not np.array_equal(bits(ctx.factors(L.SIDE_USER)[1]), bits(users))
        # after a later mf_dsgd_prepare the CSR names rows that are gone
        ctx.prepare(bu, bi, br)
        assert raw_append(ctx, bu, bi, br, len(bu)) == L.MF_ERR_STATE
        assert raw_rows(ctx, L.SIDE_USER, bu, len(bu), good) == L.MF_ERR_STATE
        assert raw_update(ctx, bu, bi, br, len(bu), good, 1) == L.MF_ERR_STATE
        # a new mf_als_prepare makes them valid again; a later mf_dsgd_fit ends that as mf_dsgd_prepare does
        ctx.als_prepare(*ids_of(d, A))
        assert raw_append(ctx, bu, bi, br, len(bu)) == L.MF_OK
        assert raw_rows(ctx, L.SIDE_USER, bu, len(bu), good) == L.MF_OK
        ctx.fit(bu, bi, br)
        assert raw_append(ctx, bu, bi, br, len(bu)) == L.MF_ERR_STATE
        assert raw_rows(ctx, L.SIDE_USER, bu, len(bu), good) == L.MF_ERR_STATE
        assert raw_update(ctx, bu, bi, br, len(bu), good, 1) == L.MF_ERR_STATE
    with make_ctx(257, mode) as wide:                                    # a rank above 256
        assert raw_rows(wide, L.SIDE_USER, bu, len(bu), good) == L.MF_ERR_INVALID
        assert raw_append(wide, bu, bi, br, len(bu)) == L.MF_ERR_INVALID
        assert raw_update(wide, bu, bi, br, len(bu), good, 1) == L.MF_ERR_INVALID


def test_streaming_als_end_to_end():
    """fit, update (a new user folded in), refit: the model answers for the new user, and a refit on the
    resident data equals a cold fit's continuation on a twin that was prepared with everything."""
    import mfhip
    rng = np.random.default_rng(3)
    u, i, r = small_problem(rng)
    new = (np.full(6, 900, np.int32), np.arange(6, dtype=np.int32), np.array([5.0, 4.0, 1.0, 3.0, 5.0, 2.0]))
    s = mfhip.StreamingALS(rank=8, lambda_=LAM, seed=5)
    twin = mfhip.StreamingALS(rank=8, lambda_=LAM, seed=5)
    try:
        s.fit((u, i, r), iterations=3)
        twin.fit((u, i, r), iterations=3)
        with pytest.raises(KeyError):
            s.model.predict(900, 0)
        assert s.update(new) == (1, 6)
        assert np.isfinite(s.model.predict(900, 0))
        twin._ctx.als_append(*new)
        twin._ctx.als_run_rows(L.SIDE_USER, new[0], twin.how)
        twin._ctx.als_run_rows(L.SIDE_ITEM, new[1], twin.how)
        s.refit(2)
        twin.refit(2)
        same_factors(s._ctx, twin._ctx, "refit")
    finally:
        s.close()
        twin.close()
