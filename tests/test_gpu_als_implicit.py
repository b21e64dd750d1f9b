"""Implicit-feedback ALS on the device (mf_als_run_implicit / mf_als_fit_implicit, csrc/kernels_als.hip).

The reference is numpy f64 on the host.  Per row of the side being solved, over its ratings j,
    A = G + sum_j w_j q_j q_j^T + lambda' I,   b = sum_{r_j > 0} (1 + w_j) q_j,   w_j = alpha |r_j|,
G = Y^T Y over the counterpart's rated rows, lambda' = lambda * n+ (n+ = the row's ratings r > 0) or
lambda; a row with n+ = 0 is zero; half-sweeps alternate with the item side first."""
import numpy as np
import pytest

import mfhip
from als_support import MODES, REGS, bits, make_ctx, rows_of, shuffled_ids
from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth

pytestmark = pytest.mark.gpu



def as_stored(F, mode):
    return F.astype(np.float32).astype(np.float64) if mode == L.MODE_FAST_F32 else F


def implicit_system(F_other, G, other_index, r, pos, lam, reg, alpha, k):
    """(A, b, n+) of one row in numpy f64."""
    Qm = F_other[other_index[pos]]
    w = alpha * np.abs(r[pos])
    cf = np.where(r[pos] > 0, 1.0 + w, 0.0)
    npos = int((r[pos] > 0).sum())
    lam_row = lam * npos if reg == L.ALS_REG_WEIGHTED else lam
    return G + (Qm * w[:, None]).T @ Qm + lam_row * np.eye(k), Qm.T @ cf, npos


def gram(F, rows):
    rated = [a for a, pos in enumerate(rows) if len(pos)]
    return F[rated].T @ F[rated]


# ---------------------------------------------------------------------------------------------
# 1. the Gram matrix, exact

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 3, 10, 64, 100, 128])
def test_gram_exact(monkeypatch, mode, k):
    """Integer factors in {-3..3}: every product and sum is exact in f32, so G must equal numpy's
    Y^T Y over the rated rows exactly -- for 1, 31, 33 and 1002 rated rows (an odd count for the
    two-ratings-per-MFMA pairing, either side of the 32-row tile, many slices), with the default slice
    and with 64 rows per slice.  The last row of each side is in the model with non-zero factors but
    not in the data: it must not be counted."""
    rng = np.random.default_rng(300 + k)
    for m in (1, 31, 33, 1002):
        nu = 3
        pi = rng.permutation(m)
        pu = np.arange(m) % min(nu, m)          # users 0..2 (fewer when m < 3): user rows of many ratings
        r = rng.integers(-2, 6, m).astype(np.float64)
        uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, m + 1, 5)
        P = rng.integers(-3, 4, (nu + 1, k)).astype(np.float64)
        Q = rng.integers(-3, 4, (m + 1, k)).astype(np.float64)
        P[-1], Q[-1] = 3.0, -2.0                # the unrated rows: non-zero
        rated_u = np.unique(pu)
        want = {L.SIDE_ITEM: Q[:m].T @ Q[:m], L.SIDE_USER: P[rated_u].T @ P[rated_u]}
        for slice_ in (None, 64):
            with monkeypatch.context() as mp:
                if slice_:
                    set_knob(mp, "als_gram_slice", slice_)
                with make_ctx(k, mode) as ctx:
                    ctx.set_factors(L.SIDE_USER, uids, P)
                    ctx.set_factors(L.SIDE_ITEM, iids, Q)
                    ctx.als_prepare(uids[pu], iids[pi], r)
                    for side in (L.SIDE_ITEM, L.SIDE_USER):
                        G = ctx.als_gram(side)
                        assert np.array_equal(G, want[side]), (m, slice_, side)
                    # the hook changes nothing
                    assert np.array_equal(ctx.lookup(L.SIDE_ITEM, iids)[0], Q)


# ---------------------------------------------------------------------------------------------
# 2. exact normal equations through the hook

def int_problem(rng, k):
    """test_gpu_als.py's int_problem shape: item rows with 1000, 31, 33 and 2 ratings (one duplicated
    (user, item) pair), user rows with 33, 31 and 1..4, shuffled signed ids, one id per side that is in
    the model but not in the data.  Ratings in {-2..5}; item 3 (ratings -1 and 0) and user 999 (one
    rating, -2) have no positive rating."""
    nu, ni = 1002, 44
    pu, pi = [], []
    for item, users in ((0, range(1000)), (1, range(31)), (2, range(33)), (3, [5])):
        pu += list(users)
        pi += [item] * len(users)
    pu += [1000] * 33 + [1001] * 31
    pi += list(range(10, 43)) + list(range(10, 41))
    pu.append(5)                      # (5, 3) a second time
    pi.append(3)
    pu, pi = np.array(pu), np.array(pi)
    r = rng.integers(-2, 6, len(pu)).astype(np.float64)
    r[pi == 3] = [-1.0, 0.0]
    r[pu == 999] = -2.0
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, ni + 1, 5)
    P = rng.integers(-3, 4, (nu + 1, k)).astype(np.float64)
    Q = rng.integers(-3, 4, (ni + 1, k)).astype(np.float64)
    return pu, pi, r, uids, iids, P, Q


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 3, 10, 64, 100, 128])
def test_normal_equations_exact(monkeypatch, mode, k):
    """Entries in {-3..3}, ratings in {-2..5}, alpha 0.5 or 0 (weights exact halves), lambda 0.5: every
    product and sum is exact in f32, so A and b from the hook must equal numpy's exactly for every
    rated row of both sides and both regs -- whole rows and rows split over 16 chunks alike, under any
    batching.  Identical systems give identical solutions: the half-sweeps are bitwise the same under
    the three knobs; the rows with no positive rating come back exactly zero, the unrated ones
    unchanged."""
    rng = np.random.default_rng(500 + k)
    pu, pi, r, uids, iids, P, Q = int_problem(rng, k)
    urows, irows = rows_of(pu, len(uids)), rows_of(pi, len(iids))
    assert sorted({len(x) for x in irows} & {2, 31, 33, 1000}) == [2, 31, 33, 1000]
    assert len(urows[-1]) == 0 and len(irows[-1]) == 0  # in the model, not in the data
    assert (r[irows[3]] <= 0).all() and (r[urows[999]] <= 0).all()
    assert {-1.0, 0.0, 1.0} <= set(np.sign(r))
    lam = 0.5
    sides = ((L.SIDE_USER, uids, urows, Q, pi, gram(Q, irows)), (L.SIDE_ITEM, iids, irows, P, pu, gram(P, urows)))
    halves = []
    for knob in (None, ("als_chunk", 64), ("als_batch", 7)):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, uids, P)
                ctx.set_factors(L.SIDE_ITEM, iids, Q)
                ctx.als_prepare(uids[pu], iids[pi], r)
                for side, ids, rows, F_other, other_index, G in sides:
                    for a, pos in enumerate(rows):
                        if not len(pos):
                            continue
                        for alpha in (0.5, 0.0):
                            for reg in REGS:
                                A, b, npos = implicit_system(F_other, G, other_index, r, pos, lam, reg, alpha, k)
                                gA, gb = ctx.als_normal_eq_implicit(side, ids[a], lam, alpha, reg)
                                assert np.array_equal(gA, A), (knob, side, a, alpha, reg)
                                assert np.array_equal(gb, b), (knob, side, a, alpha, reg)
                                assert npos or not gb.any()
                # the hook changes nothing
                assert np.array_equal(ctx.lookup(L.SIDE_USER, uids)[0], P)
                assert np.array_equal(ctx.lookup(L.SIDE_ITEM, iids)[0], Q)
                with pytest.raises(mfhip.MFError):  # no rating in the data
                    ctx.als_normal_eq_implicit(L.SIDE_ITEM, iids[-1], lam, 0.5)
                ctx.als_run_implicit(1, lam, 0.5)
                X = ctx.lookup(L.SIDE_ITEM, iids)[0]
                assert np.array_equal(bits(X[-1]), bits(Q[-1]))   # unrated: untouched
                assert np.array_equal(bits(X[3]), bits(np.zeros(k)))  # no positive rating: +0 exactly
                assert np.isfinite(X).all() and X[0].any()
                assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, uids)[0]), bits(P))
                ctx.als_run_implicit(1, lam, 0.5)
                U = ctx.lookup(L.SIDE_USER, uids)[0]
                assert np.array_equal(bits(U[-1]), bits(P[-1]))
                assert np.array_equal(bits(U[999]), bits(np.zeros(k)))
                halves.append((X, U))
    for X, U in halves[1:]:
        assert np.array_equal(bits(X), bits(halves[0][0]))
        assert np.array_equal(bits(U), bits(halves[0][1]))


@pytest.mark.parametrize("mode", MODES)
def test_split_row_without_positive_rating(monkeypatch, mode):
    """A row cut into chunks whose ratings are all <= 0: its system is still reported exactly through
    the chunked path, the half-sweep sets it to zero, and its neighbour (split too, mixed signs) is
    solved as if whole."""
    rng = np.random.default_rng(77)
    k, n, lam, alpha = 10, 100, 0.5, 0.5
    pu = np.concatenate([np.arange(n), np.arange(n)])
    pi = np.repeat([0, 1], n)
    r = np.concatenate([rng.integers(-2, 1, n), rng.integers(-2, 6, n)]).astype(np.float64)
    uids, iids = shuffled_ids(rng, n), shuffled_ids(rng, 2, 5)
    P = rng.integers(-3, 4, (n, k)).astype(np.float64)
    Q = rng.integers(-3, 4, (2, k)).astype(np.float64)
    irows = rows_of(pi, 2)
    G = P.T @ P
    out = []
    for chunk in (None, 32):
        with monkeypatch.context() as mp:
            if chunk:
                set_knob(mp, "als_chunk", chunk)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, uids, P)
                ctx.set_factors(L.SIDE_ITEM, iids, Q)
                ctx.als_prepare(uids[pu], iids[pi], r)
                for a in (0, 1):
                    for reg in REGS:
                        A, b, npos = implicit_system(P, G, pu, r, irows[a], lam, reg, alpha, k)
                        gA, gb = ctx.als_normal_eq_implicit(L.SIDE_ITEM, iids[a], lam, alpha, reg)
                        assert np.array_equal(gA, A) and np.array_equal(gb, b), (chunk, a, reg)
                        assert (npos == 0) == (a == 0)
                ctx.als_run_implicit(1, lam, alpha)
                X = ctx.lookup(L.SIDE_ITEM, iids)[0]
                assert np.array_equal(bits(X[0]), bits(np.zeros(k)))
                assert np.isfinite(X[1]).all() and X[1].any()
                out.append(X)
    assert np.array_equal(bits(out[0]), bits(out[1]))


# ---------------------------------------------------------------------------------------------
# 3. the solve, within the backward-error bound of a Cholesky solve

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,lo,hi", [(3, 40, 33, 33), (10, 70, 5, 60), (64, 40, 100, 100), (128, 20, 200, 200),
                                          (33, 40, 40, 40), (80, 30, 120, 120), (100, 20, 150, 150)])
def test_solve_within_backward_error_bound(mode, k, rows, lo, hi):
    """One implicit half-sweep (items from users), test_gpu_als.py's method.  Per solved row with n
    ratings, m rated counterpart rows, A and b in numpy f64 (alpha and the stored factors as the mode
    rounds them):
        ||b - A x|| <= 2 u c (||A|| ||x|| + || |Q|^T cf ||),   cf = 1 + w for r > 0, else 0,
        c = k (n + 2) + k (m + 1) + 2 k + 4 k (3 k + 1) + 2.
    k (n + 2), 4 k (3 k + 1) and 2 are the explicit bound's terms: accumulation over n terms (k turns
    the entrywise bound on sum |.| into a 2-norm: || sum w |q||q|^T || <= trace <= k ||A||, A being the
    sum of positive semidefinite parts), Higham's bound for a Cholesky solve, the final rounding.
    Added here: k (m + 1) for G, a sum over m rows in any order plus its one addition into the matrix
    (|| |Y|^T |Y| || <= k ||G|| <= k ||A||), and 2 k for the weighted operand: the rounding of
    w = alpha |r| and the rounding of w q before the product, one more factor (1 + d) each on every
    term.  The right-hand side takes n + 2 <= c roundings (w, 1 + w, n FMAs).  The factor 2 covers
    second-order terms.  Measured on an MI355X, the largest residual / bound over the rows of a case:
    k = 3: 5.0e-4 (f64) / 6.8e-4 (f32), k = 10: 1.5e-4 / 3.4e-4, k = 64: 5.7e-6 / 6.3e-6, k = 128:
    1.6e-6 / 1.7e-6; at the other rank buckets k = 33: 2.2e-5 / 2.4e-5, k = 80: 4.1e-6 / 3.8e-6, k = 100:
    2.4e-6 / 2.4e-6."""
    rng = np.random.default_rng(11 * k + rows)
    f32 = mode == L.MODE_FAST_F32
    u_round = 2.0 ** -24 if f32 else 2.0 ** -53
    nu = 256
    counts = rng.integers(lo, hi + 1, rows)
    pu = np.concatenate([rng.choice(nu, c, replace=False) for c in counts])
    pi = np.repeat(np.arange(rows), counts)
    perm = rng.permutation(len(pu))
    pu, pi = pu[perm], pi[perm]
    r = rng.integers(-4, 11, len(pu)) / 2.0   # -2 .. 5 in halves: all three signs
    uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, rows + 2, 5)  # one user, two items unrated
    P = as_stored(rng.standard_normal((nu + 1, k)), mode)
    Q = as_stored(rng.standard_normal((rows + 2, k)), mode)
    urows, irows = rows_of(pu, len(uids)), rows_of(pi, len(iids))
    G = gram(P, urows)
    m = sum(1 for x in urows if len(x))
    lam, alpha = 0.1, 0.7
    alpha_ref = float(np.float32(alpha)) if f32 else alpha
    worst = 0.0
    for reg in REGS:
        with make_ctx(k, mode) as ctx:
            ctx.set_factors(L.SIDE_USER, uids, P)
            ctx.set_factors(L.SIDE_ITEM, iids, Q)
            ctx.als_prepare(uids[pu], iids[pi], r)
            ctx.als_run_implicit(1, lam, alpha, reg)
            X = ctx.lookup(L.SIDE_ITEM, iids)[0]
            assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, uids)[0]), bits(P))  # the side not solved
            assert np.array_equal(bits(X[rows:]), bits(Q[rows:]))                    # rows with no rating
        for a in range(rows):
            pos = irows[a]
            n = len(pos)
            A, b, npos = implicit_system(P, G, pu, r, pos, lam, reg, alpha_ref, k)
            x = X[a]
            assert np.isfinite(x).all()
            if npos == 0:
                assert not x.any()
                continue
            cf = np.where(r[pos] > 0, 1.0 + alpha_ref * np.abs(r[pos]), 0.0)
            c = k * (n + 2) + k * (m + 1) + 2 * k + 4 * k * (3 * k + 1) + 2
            bound = 2 * u_round * c * (np.linalg.norm(A, 2) * np.linalg.norm(x) +
                                       np.linalg.norm(np.abs(P[pu[pos]]).T @ cf))
            res = np.linalg.norm(b - A @ x)
            worst = max(worst, res / bound)
            assert res <= bound, (reg, a, res, bound)
    print(f"implicit als residual / bound: mode {mode} k {k}: {worst:.3e}")


# ---------------------------------------------------------------------------------------------
# 4. end to end against a numpy f64 implicit ALS

def numpy_half_sweep(X, Y, x_rows, y_rows, y_index, r, lam, alpha):
    G = gram(Y, y_rows)
    k = X.shape[1]
    for a, pos in enumerate(x_rows):
        if len(pos):
            A, b, npos = implicit_system(Y, G, y_index, r, pos, lam, L.ALS_REG_WEIGHTED, alpha, k)
            X[a] = np.linalg.solve(A, b) if npos else 0.0


def objective(P, Q, pu, pi, r, lam, alpha):
    """What both half-sweeps minimise (every row here is rated)."""
    s = np.einsum("nk,nk->n", P[pu], Q[pi])
    w = alpha * np.abs(r)
    pos = r > 0
    nu = np.bincount(pu[pos], minlength=len(P))
    ni = np.bincount(pi[pos], minlength=len(Q))
    return (np.sum((P.T @ P) * (Q.T @ Q)) + w @ (s * s) - 2 * ((1 + w[pos]) @ s[pos]) +
            lam * (nu @ (P * P).sum(1) + ni @ (Q * Q).sum(1)))


@pytest.fixture(scope="module")
def smoke_implicit():
    """The smoke data with its ratings shifted to r - 3, dense indices and the numpy result per mode
    (the start is rounded to f32 in fast mode, as the device stores it)."""
    d = synth.generate(300, 120, 6000, seed=3)
    r = d.r - 3.0
    assert {-1.0, 0.0, 1.0} <= set(np.sign(r))
    uids, pu = np.unique(d.u, return_inverse=True)
    iids, pi = np.unique(d.i, return_inverse=True)
    rng = np.random.default_rng(4)
    k, lam, alpha, T = 16, 0.1, 1.0, 5
    P0, Q0 = rng.random((len(uids), k)), rng.random((len(iids), k))
    urows, irows = rows_of(pu, len(uids)), rows_of(pi, len(iids))
    ref = {}
    for mode in MODES:
        P, Q = as_stored(P0.copy(), mode), as_stored(Q0.copy(), mode)
        for _ in range(T):
            numpy_half_sweep(Q, P, irows, urows, pu, r, lam, alpha)
            numpy_half_sweep(P, Q, urows, irows, pi, r, lam, alpha)
        ref[mode] = float(objective(P, Q, pu, pi, r, lam, alpha))
    return dict(u=d.u, i=d.i, r=r, uids=uids, iids=iids, pu=pu, pi=pi, k=k, lam=lam, alpha=alpha, T=T, P0=P0, Q0=Q0,
                ref=ref)


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_against_numpy_implicit_als(smoke_implicit, mode):
    """k = 16, lambda 0.1, alpha 1, 5 iterations, weighted reg: F decreases strictly at every
    half-sweep, the final F agrees with the numpy f64 implicit ALS within 0.5 % (the project's
    fast-mode band), and a twin context given the same calls is bitwise equal.  Measured on an
    MI355X: F falls 617992.4 -> -3067.96; the final F is -3067.962763134 on the device and in numpy in
    deterministic mode (relative difference 0) and -3067.962702759 in fast mode (2.0e-8)
    (DESIGN.md section 4.7.1)."""
    s = smoke_implicit
    k, lam, alpha, T = s["k"], s["lam"], s["alpha"], s["T"]

    def start():
        ctx = make_ctx(k, mode)
        ctx.set_factors(L.SIDE_USER, s["uids"], s["P0"])
        ctx.set_factors(L.SIDE_ITEM, s["iids"], s["Q0"])
        ctx.als_prepare(s["u"], s["i"], s["r"])
        return ctx

    def F(ctx):
        _, P = ctx.factors(L.SIDE_USER)
        _, Q = ctx.factors(L.SIDE_ITEM)
        return float(objective(P, Q, s["pu"], s["pi"], s["r"], lam, alpha))

    with start() as ctx, start() as twin:
        obj = [F(ctx)]
        for _ in range(2 * T):
            ctx.als_run_implicit(1, lam, alpha)
            obj.append(F(ctx))
        print("implicit als objective per half-sweep:", " ".join(f"{x:.6f}" for x in obj))
        assert all(b < a for a, b in zip(obj, obj[1:])), obj
        rel = abs(obj[-1] - s["ref"][mode]) / abs(s["ref"][mode])
        print(f"implicit als objective: mode {mode} device {obj[-1]:.9f} numpy {s['ref'][mode]:.9f} rel {rel:.3e}")
        assert rel < 0.005
        for _ in range(2 * T):
            twin.als_run_implicit(1, lam, alpha)
        for side in (L.SIDE_USER, L.SIDE_ITEM):
            assert np.array_equal(bits(twin.factors(side)[1]), bits(ctx.factors(side)[1]))


# ---------------------------------------------------------------------------------------------
# 5. the counter, the order, and mixing with explicit half-sweeps

def small_problem(rng, nu=40, ni=25, n=400):
    u = rng.integers(0, nu, n).astype(np.int32)
    i = rng.integers(0, ni, n).astype(np.int32)
    r = rng.integers(-4, 11, n) / 2.0
    return u, i, r


@pytest.mark.parametrize("mode", MODES)
def test_counter_order_and_mixing(mode):
    rng = np.random.default_rng(23)
    k, lam, alpha = 5, 0.1, 0.8
    u, i, r = small_problem(rng)
    uids, iids = np.unique(u), np.unique(i)
    P0, Q0 = rng.random((len(uids), k)), rng.random((len(iids), k))

    def start():
        ctx = make_ctx(k, mode)
        ctx.set_factors(L.SIDE_USER, uids, P0)
        ctx.set_factors(L.SIDE_ITEM, iids, Q0)
        return ctx

    def both(ctx):
        return bits(ctx.factors(L.SIDE_USER)[1]), bits(ctx.factors(L.SIDE_ITEM)[1])

    with start() as a, start() as b, start() as c, start() as d:
        a.als_prepare(u, i, r)
        a.als_run_implicit(2, lam, alpha)
        b.als_prepare(u, i, r)
        b.als_run_implicit(1, lam, alpha)
        assert np.array_equal(both(b)[0], bits(as_stored(P0, mode)))  # the item side came first
        assert not np.array_equal(both(b)[1], bits(as_stored(Q0, mode)))
        b.als_run_implicit(1, lam, alpha)
        for x, y in zip(both(a), both(b)):
            assert np.array_equal(x, y)
        T = 3
        c.als_fit_implicit(u, i, r, T, lam, alpha)
        d.als_prepare(u, i, r)
        d.als_run_implicit(2 * T, lam, alpha)
        for x, y in zip(both(c), both(d)):
            assert np.array_equal(x, y)
        # the counter is shared: after an odd number of implicit half-sweeps an explicit one solves the users
        d.als_run_implicit(1, lam, alpha)
        bu, bi = both(d)
        d.als_run(1, lam)
        au, ai = both(d)
        assert np.array_equal(ai, bi) and not np.array_equal(au, bu)
        # ... and the next implicit one the items
        d.als_run_implicit(1, lam, alpha)
        cu, ci = both(d)
        assert np.array_equal(cu, au) and not np.array_equal(ci, ai)


# ---------------------------------------------------------------------------------------------
# 6. errors

@pytest.mark.parametrize("mode", MODES)
def test_errors(mode):
    rng = np.random.default_rng(2)
    u, i, r = small_problem(rng)
    with make_ctx(4, mode) as ctx:
        for alpha in (-0.5, float("nan"), float("inf")):
            with pytest.raises(mfhip.MFError) as e:
                ctx.als_fit_implicit(u, i, r, 1, 0.1, alpha)
            assert e.value.code == L.MF_ERR_INVALID
            with pytest.raises(mfhip.MFError) as e:
                ctx.als_run_implicit(1, 0.1, alpha)
            assert e.value.code == L.MF_ERR_INVALID
        for lam in (0.0, -1.0, float("nan")):
            with pytest.raises(mfhip.MFError) as e:
                ctx.als_fit_implicit(u, i, r, 1, lam, 1.0)
            assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit_implicit(u, i, r, 1, 0.1, 1.0, 7)
        assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit_implicit(u, i, r, -1, 0.1, 1.0)
        assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_run_implicit(1, 0.1, 1.0)
        assert e.value.code == L.MF_ERR_STATE
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_gram(L.SIDE_USER)
        assert e.value.code == L.MF_ERR_STATE
        assert ctx.num_factors(L.SIDE_USER) == 0  # nothing above touched the context
        # n = 0: a no-op
        e0 = np.empty(0, np.int32)
        ctx.als_fit_implicit(e0, e0, np.empty(0), 3, 0.1, 1.0)
        assert ctx.num_factors(L.SIDE_USER) == 0 and ctx.num_factors(L.SIDE_ITEM) == 0
        ctx.als_prepare(u, i, r)
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_run_implicit(-1, 0.1, 1.0)
        assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_normal_eq_implicit(L.SIDE_USER, int(u[0]), 0.1, -1.0)
        assert e.value.code == L.MF_ERR_INVALID
        # alpha = 0 is valid: unit confidences on the positive ratings
        ctx.als_run_implicit(2, 0.1, 0.0)
        for side in (L.SIDE_USER, L.SIDE_ITEM):
            assert np.isfinite(ctx.factors(side)[1]).all()
    with make_ctx(L.ALS_MAX_RANK + 1, mode) as ctx:
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit_implicit(u, i, r, 1, 0.1, 1.0)
        assert e.value.code == L.MF_ERR_INVALID and str(L.ALS_MAX_RANK) in str(e.value)


# ---------------------------------------------------------------------------------------------
# 7. the mirror API

@pytest.mark.parametrize("mode", ["deterministic", "fast"])
def test_train_implicit_agrees_with_the_context(mode):
    d = synth.generate(300, 120, 6000, seed=3)
    r = d.r - 3.0
    model = mfhip.ALS.trainImplicit((d.u, d.i, r), rank=16, iterations=3, lambda_=0.1, alpha=2.0, mode=mode, seed=11)
    try:
        with make_ctx(16, L.MODE_FAST_F32 if mode == "fast" else L.MODE_DETERMINISTIC_F64, seed=11) as ctx:
            ctx.als_fit_implicit(d.u, d.i, r, 3, 0.1, 2.0)
            uf, pf = model.userFeatures(), model.productFeatures()
            ids, vecs = ctx.factors(L.SIDE_USER)
            assert [x for x, _ in uf] == ids.tolist()
            assert np.array_equal(bits(np.array([v for _, v in uf])), bits(vecs))
            pids, pvecs = ctx.factors(L.SIDE_ITEM)
            assert [x for x, _ in pf] == pids.tolist()
            assert np.array_equal(bits(np.array([v for _, v in pf])), bits(pvecs))
            user = int(d.u[0])
            rp = model.recommendProducts(user, 5)
            rid, rsc, rcnt = ctx.recommend([user], 5)
            assert len(rp) == 5
            assert [(a, b) for a, b, _ in rp] == [(user, int(x)) for x in rid[0, :rcnt[0]]]
            assert np.array_equal(bits([c for _, _, c in rp]), bits(rsc[0, :rcnt[0]]))
    finally:
        model.close()
