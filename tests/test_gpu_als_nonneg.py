"""The non-negative ALS half-sweeps (mf_als_run_nonneg, mf_als_run_implicit_nonneg; nnls_row of
csrc/als_nnls_device.hpp inside the kernels of kernels_als.hip and kernels_als_wide.hip).

The yardstick is mf_nnls_solve, the host replay of the solve in the order mfhip.h states (checked on its
own in test_nnls_host.py).  A row's system is read with the existing hooks mf_debug_als_normal_eq[_implicit]
and fed to it; the row the device solves -- through the hook mf_debug_als_nnls_row and by a real half-sweep
-- must match in x, iteration count and reason code bit for bit.  A wrong lane layout, a dropped wall clamp
or a swapped sum order cannot pass that.

  test_bitwise_against_the_host_replay   k in RANKS (both sides of every bucket edge the two kernel files
        have, the narrow/wide threshold 128 | 129 included), f32 and f64, explicit and implicit, both regs,
        lambda 1e-300 and 0.25, whole rows and rows split by als_chunk; the rows of nnls_support.planted_als
        (k, k + 1, k + 200 and more ratings, one row with no positive rating)
  test_planted_solutions                 the explicit rows carry a planted integer x*: reason 0, x >= 0
        without -0, the zero set exactly, the error within the tolerance of nnls_support.  The implicit
        systems of the family cannot carry a free integer x* (their b is >= 0 entry by entry), so they take
        scipy's active-set solution of the f64 system as x*, with the same four assertions.
  test_interior_rows_agree_with_cholesky where x* > 0 everywhere the row of mf_als_run is the same
  test_kkt_on_a_random_problem           als_support.small_problem, all rows of a half-sweep
  test_training_*, test_reproducible_*, test_stats_*, test_arguments_*
"""
import numpy as np
import pytest

import mfhip
from als_support import MODES, REGS, TINY, bits, make_ctx, objective, rows_of, small_problem
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context, nnls_solve
from nnls_support import N_ROWS, assert_kkt, assert_planted, planted_als, planted_tolerance, scipy_nnls

pytestmark = pytest.mark.gpu

RANKS = [1, 31, 32, 33, 64, 96, 128, 129, 192, 256]
ALPHA = 1.0


def load(ctx, d):
    ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
    ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
    ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])


def system(ctx, item, lam, reg, alpha):
    if alpha is None:
        return ctx.als_normal_eq(L.SIDE_ITEM, int(item), lam, reg)
    return ctx.als_normal_eq_implicit(L.SIDE_ITEM, int(item), lam, alpha, reg)


def run_nonneg(ctx, n, lam, reg, alpha):
    if alpha is None:
        ctx.als_run_nonneg(n, lam, reg)
    else:
        ctx.als_run_implicit_nonneg(n, lam, alpha, reg)


def same(x, want):
    return np.array_equal(bits(x), bits(want))


# ---------------------------------------------------------------------------------------------
# 1. bit for bit against the host replay

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", RANKS)
def test_bitwise_against_the_host_replay(monkeypatch, mode, k):
    d = planted_als(k)
    f64 = mode == L.MODE_DETERMINISTIC_F64
    cases = [(None, alpha, reg, lam) for alpha in (None, ALPHA) for reg in REGS for lam in (TINY, 0.25)]
    # one long row (k + 200 ratings and more) through the split path, both kinds
    cases += [(("als_chunk", 64), alpha, L.ALS_REG_WEIGHTED, 0.25) for alpha in (None, ALPHA)]
    ctxs = {}
    try:
        for knob, alpha, reg, lam in cases:
            if knob not in ctxs:
                ctxs[knob] = make_ctx(k, mode)
            ctx = ctxs[knob]
            with monkeypatch.context() as mp:
                if knob:
                    set_knob(mp, *knob)
                load(ctx, d)                                               # the counter at 0: the item side is next
            want = []
            for t in range(N_ROWS):
                item = d["iids"][t]
                A, b = system(ctx, item, lam, reg, alpha)
                ref = nnls_solve(A, b, f64)
                got = ctx.als_nnls_row(L.SIDE_ITEM, int(item), lam, -1.0 if alpha is None else alpha, reg)
                what = (k, mode, knob, alpha, reg, lam, t, int(d["counts"][t]))
                assert got[1:] == ref[1:], (what, got[1:], ref[1:])
                assert same(got[0], ref[0]), (what, got[0], ref[0])
                assert ref[2] == 0
                want.append(ref[0])
            assert same(ctx.lookup(L.SIDE_ITEM, d["iids"])[0], d["Q0"])   # the hook stores nothing
            run_nonneg(ctx, 1, lam, reg, alpha)
            X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
            for t in range(N_ROWS):
                assert same(X[t], want[t]), ((k, mode, knob, alpha, reg, lam, t), X[t], want[t])
            assert same(X[0], np.zeros(k))                                 # no positive rating, b <= 0: +0
            assert same(X[N_ROWS:], d["Q0"][N_ROWS:])                      # rows without ratings
            assert same(ctx.lookup(L.SIDE_USER, d["uids"])[0], d["P"])
    finally:
        for ctx in ctxs.values():
            ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. planted solutions, and the interior rows against the Cholesky half-sweep

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", RANKS)
def test_planted_solutions(mode, k):
    d = planted_als(k)
    f64 = mode == L.MODE_DETERMINISTIC_F64
    with make_ctx(k, mode) as ctx:
        for alpha in (None, ALPHA):
            load(ctx, d)                                                   # the counter at 0: the item side is next
            systems = [system(ctx, d["iids"][t], TINY, L.ALS_REG_WEIGHTED, alpha) for t in range(N_ROWS)]
            rows = [ctx.als_nnls_row(L.SIDE_ITEM, int(d["iids"][t]), TINY, -1.0 if alpha is None else alpha)
                    for t in range(N_ROWS)]
            run_nonneg(ctx, 1, TINY, L.ALS_REG_WEIGHTED, alpha)
            X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
            for t in range(N_ROWS):
                A, b = systems[t]
                if alpha is None:
                    A0, b0, xs = d["systems"][t]
                    assert np.array_equal(A, A0) and np.array_equal(b, b0)  # the device formed the planted system
                else:
                    xs = scipy_nnls(A, b)
                    # an entry with b_i = 0 that no other entry is coupled to is exactly 0; scipy leaves rounding
                    # noise of the order of 1e-16 there
                    xs[xs < 1e-12 * xs.max(initial=0.0)] = 0.0
                assert rows[t][2] == 0, (k, mode, alpha, t, rows[t][1:])
                assert same(X[t], rows[t][0])
                if alpha is not None and not b.any():
                    assert same(X[t], np.zeros(k))
                    continue
                assert_planted(X[t], xs, A, b, f64, f"k {k} mode {mode} alpha {alpha} row {t} ({rows[t][1]} iterations)",
                               family=alpha is None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 33, 128, 129, 256])
def test_interior_rows_agree_with_cholesky(mode, k):
    """Items 1 and 2 have x* > 0 everywhere: the constraint is inactive and mf_als_run's row is the answer."""
    d = planted_als(k)
    f64 = mode == L.MODE_DETERMINISTIC_F64
    with make_ctx(k, mode) as ctx:
        load(ctx, d)
        ctx.als_run(1, TINY)
        chol = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
        load(ctx, d)                                                       # the item side again
        ctx.als_run_nonneg(1, TINY)
        X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
    for t in (1, 2):
        A, b, xs = d["systems"][t]
        assert (xs > 0).all() and (chol[t] > 0).all()
        tol = planted_tolerance(A, b, xs, f64)[0]
        assert np.linalg.norm(X[t] - chol[t]) <= tol, (k, mode, t, np.linalg.norm(X[t] - chol[t]), tol)


# ---------------------------------------------------------------------------------------------
# 3. KKT on a random problem

KKT_SEED = 20


def kkt_problem(k):
    rng = np.random.default_rng(KKT_SEED + k)
    u, i, r = small_problem(rng)
    nu, ni = int(u.max()) + 1, int(i.max()) + 1
    P = rng.random((nu, k)) - 0.3
    Q = rng.random((ni, k))
    return u, i, r, P, Q


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [8, 40, 160])
def test_kkt_on_a_random_problem(mode, k):
    """All rows of one half-sweep: x >= 0, reason 0, the KKT conditions against the f64 gradient, and every
    row within the planted tolerance of scipy's NNLS on the Cholesky-transformed system."""
    f64 = mode == L.MODE_DETERMINISTIC_F64
    u, i, r, P, Q = kkt_problem(k)
    lam = 0.05
    uid, iid = np.arange(len(P), dtype=np.int32), np.arange(len(Q), dtype=np.int32)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, uid, P)
        ctx.set_factors(L.SIDE_ITEM, iid, Q)
        ctx.als_prepare(u, i, r)
        rated = np.unique(i)
        systems = {int(t): ctx.als_normal_eq(L.SIDE_ITEM, int(t), lam) for t in rated}
        for t, (A, b) in systems.items():  # beforehand, on the CPU: the seed gives reason 0 on every row
            assert nnls_solve(A, b, f64)[2] == 0, t
        reasons = {t: ctx.als_nnls_row(L.SIDE_ITEM, t, lam)[2] for t in systems}
        ctx.als_run_nonneg(1, lam)
        X = ctx.lookup(L.SIDE_ITEM, iid)[0]
        st = ctx.als_nonneg_stats()
    assert not any(reasons.values()), reasons
    assert st["rows"] == len(rated) and st["capped"] == st["reason2"] == st["nan_rows"] == 0
    for t, (A, b) in systems.items():
        what = f"k {k} mode {mode} item {t}"
        assert_kkt(X[t], A, b, f64, what)
        ref = scipy_nnls(A, b)
        tol = planted_tolerance(A, b, ref, f64)[0]
        assert np.linalg.norm(X[t] - ref) <= tol, (what, np.linalg.norm(X[t] - ref), tol)


# ---------------------------------------------------------------------------------------------
# 4. training

def training_data():
    rng = np.random.default_rng(4)
    nu, ni, n = 60, 40, 1500
    Pt, Qt = rng.random((nu, 4)), rng.random((ni, 4))
    u = rng.integers(0, nu - 2, n).astype(np.int32)      # the last two users and items have no ratings
    i = rng.integers(0, ni - 2, n).astype(np.int32)
    return u, i, np.einsum("nk,nk->n", Pt[u], Qt[i]) * 4 + 0.5, nu, ni


@pytest.mark.parametrize("mode", MODES)
def test_training_keeps_factors_nonnegative_and_the_objective_falling(mode):
    k, lam = 8, 0.05
    u, i, r, nu, ni = training_data()
    rng = np.random.default_rng(5)
    P0, Q0 = rng.random((nu, k)), rng.random((ni, k))   # feasible, so no half-sweep can raise the objective
    P0[nu - 2:] = Q0[ni - 2:] = -1.0                     # the rows without ratings: untouched, sign and all
    uid, iid = np.arange(nu, dtype=np.int32), np.arange(ni, dtype=np.int32)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, uid, P0)
        ctx.set_factors(L.SIDE_ITEM, iid, Q0)
        ctx.als_prepare(u, i, r)
        obj = []
        for h in range(6):
            ctx.als_run_nonneg(1, lam)
            P, Q = ctx.lookup(L.SIDE_USER, uid)[0], ctx.lookup(L.SIDE_ITEM, iid)[0]
            obj.append(objective(P, Q, u, i, r, lam))
            solved = np.vstack([P[np.unique(u)], Q[np.unique(i)]])
            assert (solved >= 0).all() and not np.signbit(solved).any()
        st = ctx.als_nonneg_stats()
    print("objective per half-sweep:", obj)
    for a, b in zip(obj, obj[1:]):
        assert b <= a * (1 + 1e-6), obj
    # rows without ratings are untouched (also by sign)
    assert same(P[nu - 2:], P0[nu - 2:]) and same(Q[ni - 2:], Q0[ni - 2:])
    assert st["capped"] == 0 and st["nan_rows"] == 0
    assert st["rows"] == 3 * (len(np.unique(u)) + len(np.unique(i)))


@pytest.mark.parametrize("mode", MODES)
def test_training_implicit(mode):
    k, lam, alpha = 8, 0.05, 2.0
    u, i, r, nu, ni = training_data()
    r = np.round(r) - 1.0                                  # counts, some of them zero or negative
    assert (r > 0).any() and (r <= 0).any()
    with make_ctx(k, mode, has_seed=1, seed=3) as ctx:
        ctx.als_fit_implicit_nonneg(u, i, r, 3, lam, alpha)
        P, Q = ctx.lookup(L.SIDE_USER, np.unique(u))[0], ctx.lookup(L.SIDE_ITEM, np.unique(i))[0]
        st = ctx.als_nonneg_stats()
    for F in (P, Q):
        assert (F >= 0).all() and not np.signbit(F).any() and F.any()
    assert st["capped"] == 0 and st["nan_rows"] == 0
    model = mfhip.ALS.withSolver("nnls").trainImplicit((u, i, r), rank=k, iterations=3, lambda_=lam, alpha=alpha,
                                                       mode="fast" if mode == L.MODE_FAST_F32 else "deterministic",
                                                       seed=3)
    assert same(model.context.lookup(L.SIDE_USER, np.unique(u))[0], P)
    model.close()


# ---------------------------------------------------------------------------------------------
# 5. reproducibility, the shared counter, the stats

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [24, 136])
def test_reproducible_and_independent_of_the_launch_cut(monkeypatch, mode, k):
    u, i, r, P, Q = kkt_problem(k)
    uid, iid = np.arange(len(P), dtype=np.int32), np.arange(len(Q), dtype=np.int32)

    def fit(knob, calls):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, uid, P)
                ctx.set_factors(L.SIDE_ITEM, iid, Q)
                ctx.als_prepare(u, i, r)
                calls(ctx)
                return ctx.lookup(L.SIDE_USER, uid)[0], ctx.lookup(L.SIDE_ITEM, iid)[0], ctx.als_nonneg_stats()

    ref = fit(None, lambda c: c.als_run_nonneg(3, 0.1))
    for knob in (None, ("als_batch", 3)):
        got = fit(knob, lambda c: c.als_run_nonneg(3, 0.1))
        assert same(got[0], ref[0]) and same(got[1], ref[1]) and got[2] == ref[2], knob
    # one counter: item side (nonneg), user side (Cholesky), item side (nonneg) ...
    mixed = fit(None, lambda c: (c.als_run_nonneg(1, 0.1), c.als_run(1, 0.1), c.als_run_nonneg(1, 0.1)))
    chk = fit(None, lambda c: (c.als_run_nonneg(1, 0.1), c.als_run(1, 0.1)))
    assert same(mixed[0], chk[0])                          # the third half-sweep solved the item side again
    assert not same(mixed[1], chk[1])
    assert mixed[2]["rows"] == 2 * len(np.unique(i))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("implicit", [False, True])
def test_stats_sum_the_rows_of_a_half_sweep(mode, implicit):
    k = 16
    u, i, r, P, Q = kkt_problem(k)
    if implicit:
        r = r - 3.0
        r[i == i[0]] = -np.abs(r[i == i[0]])               # one item with no positive rating
    alpha = 1.5 if implicit else None
    uid, iid = np.arange(len(P), dtype=np.int32), np.arange(len(Q), dtype=np.int32)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, uid, P)
        ctx.set_factors(L.SIDE_ITEM, iid, Q)
        ctx.als_prepare(u, i, r)
        zero = {n: 0 for n in ("rows", "iterations", "max_iterations", "capped", "reason2", "nan_rows")}
        assert ctx.als_nonneg_stats() == zero
        rows = [ctx.als_nnls_row(L.SIDE_ITEM, int(t), 0.1, -1.0 if alpha is None else alpha) for t in np.unique(i)]
        assert ctx.als_nonneg_stats() == zero              # the hook counts nothing
        run_nonneg(ctx, 1, 0.1, L.ALS_REG_WEIGHTED, alpha)
        st = ctx.als_nonneg_stats()
        assert st["rows"] == len(rows)
        assert st["iterations"] == sum(x[1] for x in rows)
        assert st["max_iterations"] == max(x[1] for x in rows)
        assert st["capped"] == 0 and st["reason2"] == 0 and st["nan_rows"] == 0
        if implicit:
            assert rows[list(np.unique(i)).index(i[0])][1:] == (0, 0)
        ctx.als_prepare(u, i, r)                           # the counters start again
        assert ctx.als_nonneg_stats() == zero


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [33, 160])
def test_a_nan_reaches_exactly_the_rows_that_rate_it(mode, k):
    u, i, r, P, Q = kkt_problem(k)
    P = P.copy()
    P[7, 5] = np.nan
    hit = np.zeros(len(Q), bool)
    hit[np.unique(i[u == 7])] = True
    rated = np.zeros(len(Q), bool)
    rated[np.unique(i)] = True
    assert hit.any() and (rated & ~hit).any()
    uid, iid = np.arange(len(P), dtype=np.int32), np.arange(len(Q), dtype=np.int32)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, uid, P)
        ctx.set_factors(L.SIDE_ITEM, iid, Q)
        ctx.als_prepare(u, i, r)
        ctx.als_run_nonneg(1, 0.1)
        X = ctx.lookup(L.SIDE_ITEM, iid)[0]
        st = ctx.als_nonneg_stats()
    assert np.isnan(X[hit]).all() and np.isfinite(X[~hit]).all()
    assert st["nan_rows"] == hit.sum()


# ---------------------------------------------------------------------------------------------
# 6. errors

def test_arguments_are_validated():
    rng = np.random.default_rng(1)
    u, i, r = small_problem(rng)
    W = L.ALS_REG_WEIGHTED

    def code(fn, *a, **kw):
        with pytest.raises(mfhip.MFError) as e:
            fn(*a, **kw)
        return e.value.code

    with make_ctx(3, L.MODE_DETERMINISTIC_F64) as ctx:
        assert code(ctx.als_run_nonneg, 1, 0.1) == L.MF_ERR_STATE
        assert code(ctx.als_run_implicit_nonneg, 1, 0.1, 1.0) == L.MF_ERR_STATE
        assert code(ctx.als_nonneg_stats) == L.MF_ERR_STATE
        assert code(ctx.als_nnls_row, L.SIDE_ITEM, int(i[0]), 0.1) == L.MF_ERR_STATE
        assert code(ctx.als_fit_nonneg, u, i, r, 1, 0.0) == L.MF_ERR_INVALID
        assert code(ctx.als_fit_implicit_nonneg, u, i, r, 1, 0.1, -1.0) == L.MF_ERR_INVALID
        assert code(ctx.als_run_nonneg, 1, 0.1) == L.MF_ERR_STATE     # the rejected fits prepared nothing
        ctx.als_prepare(u, i, r)
        for lam in (0.0, -1.0, float("nan"), float("inf")):
            assert code(ctx.als_run_nonneg, 1, lam) == L.MF_ERR_INVALID
            assert code(ctx.als_run_implicit_nonneg, 1, lam, 1.0) == L.MF_ERR_INVALID
        for alpha in (-0.5, float("nan"), float("inf")):
            assert code(ctx.als_run_implicit_nonneg, 1, 0.1, alpha) == L.MF_ERR_INVALID
        assert code(ctx.als_run_nonneg, 1, 0.1, 7) == L.MF_ERR_INVALID
        assert code(ctx.als_run_implicit_nonneg, 1, 0.1, 1.0, 7) == L.MF_ERR_INVALID
        assert code(ctx.als_run_nonneg, -1, 0.1) == L.MF_ERR_INVALID
        assert code(ctx.als_nnls_row, L.SIDE_ITEM, 10 ** 6, 0.1) == L.MF_ERR_INVALID
        before = ctx.lookup(L.SIDE_ITEM, np.unique(i))[0]
        ctx.als_run_nonneg(0, 0.1)
        ctx.als_run_implicit_nonneg(0, 0.1, 0.0)
        assert same(ctx.lookup(L.SIDE_ITEM, np.unique(i))[0], before)
    p = L.default_params()
    p.num_factors = 4
    with Context(p, rank=(0, 1, 0, b"")) as ctx:          # a rank-mode context
        assert code(ctx.als_fit_nonneg, u, i, r, 1, 0.1) == L.MF_ERR_STATE
        assert code(ctx.als_fit_implicit_nonneg, u, i, r, 1, 0.1, 1.0) == L.MF_ERR_STATE
    if L.device_count() >= 2:
        p.num_blocks = 2
        with Context(p, n_devices=2) as ctx:
            assert code(ctx.als_fit_nonneg, u, i, r, 1, 0.1) == L.MF_ERR_STATE
    model = mfhip.ALS.withSolver("nnls").train((u, i, r), rank=3, iterations=2, lambda_=0.1)
    assert np.isfinite(model.predict(int(u[0]), int(i[0])))
    assert all((v >= 0).all() for _, v in model.productFeatures())
    model.close()
