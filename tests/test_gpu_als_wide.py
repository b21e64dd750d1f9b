"""ALS at ranks 129..256 (csrc/kernels_als_wide.hip): rank buckets NB = 5..8, the normal matrix in
global memory, the blocked Cholesky of finish_wide with its 32-column panels.

The problems and the checks are those of tests/test_gpu_als_ranks.py and tests/test_gpu_als.py, which
are parametrised by k and verify their constructions in integers on the host; their test bodies are
called here at the wide ranks.  explicit_problem(k) and implicit_problem(k) hold for every k in WIDE
(the largest entry of A, b and r is 1,184, at k = 224), so the planted integer solutions are exact in
f32 and f64 under any summation order, any blocking of the factorisation and any contraction.

WIDE puts a rank on each side of every 32-bucket edge (= every panel edge of finish_wide) and of the
16-row edges of its thread grid, with the first and the last rank of the range:

  NB 5  129, 144, 145, 160      NB 6  161, 192      NB 7  193, 224      NB 8  225, 255, 256

Which test drives which instance (f32 and f64):
  test_explicit_solve_is_exact   k_als_wide whole rows (default; als_batch=5: three launches);
                                 als_chunk=16: chunks + k_als_reduce_wide
  test_implicit_solve_is_exact   k_als_wide<T, NB, true>, k_als_gram_wide (als_gram_slice=8: many slices);
                                 als_chunk=16: chunks + k_als_reduce_wide<T, NB, true>
  test_hooks_*                   the dump path of finish_wide and k_als_gram_wide, whole rows and rows
                                 split by als_chunk=64; the half-sweep bitwise the same either way
  test_solve_within_backward_error_bound, test_end_to_end_against_numpy_als   real-valued data
  test_strided_*                 the loop `for (wi = blockIdx.x; wi < n; wi += gridDim.x)` of k_als_wide
                                 and k_als_reduce_wide.  The grid is min(items, slabs) with 256 (f64) or 512
                                 (f32) slabs on an MI355X, so in every test above a workgroup meets one
                                 work item, als_batch=5 included; MFHIP_TEST als_slabs=N caps the grid
                                 at N workgroups, and with N = 1 and 3 each one meets several whole
                                 rows, chunks, split rows and rows without a positive rating in turn,
                                 reusing its slab and its LDS
"""
import os

import numpy as np
import pytest

import mfhip
import test_gpu_als_ranks as R
from als_support import (MODES, N_ITEMS, REGS, TINY, bits, explicit_problem, first_difference, implicit_problem,
                         make_ctx, normal_eq_reference, numpy_half_sweep, objective, rows_of, shuffled_ids,
                         small_problem)
from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth

pytestmark = pytest.mark.gpu

WIDE = [129, 144, 145, 160, 161, 192, 193, 224, 225, 255, 256]
HOOK_RANKS = [129, 160, 161, 192, 224, 225, 256]


# ---------------------------------------------------------------------------------------------
# 1, 2. the planted integer solutions come back exactly

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", WIDE)
def test_explicit_solve_is_exact(monkeypatch, mode, k):
    """als_run(1, 1e-300, reg) returns X0 exactly for both regs: whole rows, als_chunk=16 (every row
    through k_als_reduce_wide) and als_batch=5 (three launches); the unrated items and the whole user
    side stay bitwise as set."""
    R.test_explicit_solve_is_exact(monkeypatch, mode, k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", WIDE)
def test_implicit_solve_is_exact(monkeypatch, mode, k):
    """als_run_implicit(1, 1e-300, 1.0, reg) returns (I - N)^T [r > 0] exactly: whole rows, als_chunk=16
    and als_gram_slice=8; the item with no positive rating is +0 bitwise."""
    R.test_implicit_solve_is_exact(monkeypatch, mode, k)


# ---------------------------------------------------------------------------------------------
# 2b. several work items per workgroup (als_slabs caps the grid)

STRIDE_RANKS = [145, 192, 224, 256]   # one rank per bucket NB = 5..8


def run_exact(monkeypatch, d, k, mode, reg, knobs, implicit):
    with monkeypatch.context() as mp:
        for key, value in knobs.items():
            set_knob(mp, key, value)
        with make_ctx(k, mode) as ctx:
            ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
            ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
            ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
            if implicit:
                ctx.als_run_implicit(1, TINY, 1.0, reg)
            else:
                ctx.als_run(1, TINY, reg)
            assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, d["uids"])[0]), bits(d["P"]))
            return ctx.lookup(L.SIDE_ITEM, d["iids"])[0]


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", STRIDE_RANKS)
def test_strided_exact_solve(monkeypatch, mode, k, implicit):
    """The exact problems with the grid capped at 1 and at 3 workgroups, whole rows (12 items per
    launch: 12 or 4 per workgroup, the row without a positive rating among them in the implicit
    problem) and als_chunk=16 (every row through k_als_reduce_wide, 12 or 4 split rows and some
    hundred chunks per workgroup): the planted solution exactly, and every row bitwise as with the
    uncapped grid; the unrated items stay as set."""
    d = implicit_problem(k) if implicit else explicit_problem(k)
    want = d["X"] if implicit else d["X0"]
    for reg in REGS:
        for chunk in ({}, {"als_chunk": 16}):
            ref = run_exact(monkeypatch, d, k, mode, reg, chunk, implicit)
            assert np.array_equal(ref[:N_ITEMS], want), (reg, chunk, first_difference(ref, want))
            for slabs in (1, 3):
                X = run_exact(monkeypatch, d, k, mode, reg, dict(chunk, als_slabs=slabs), implicit)
                assert np.array_equal(X[:N_ITEMS], want), (reg, chunk, slabs, first_difference(X, want))
                assert np.array_equal(bits(X), bits(ref)), (reg, chunk, slabs)
                assert np.array_equal(bits(X[N_ITEMS:]), bits(d["Q0"][N_ITEMS:]))


@pytest.mark.parametrize("mode", MODES)
def test_strided_real_valued_iteration(monkeypatch, smoke_als_160, mode):
    """Real-valued data, where a slab or an LDS buffer left dirty by the previous item would show in
    the bits: one iteration on the smoke data at k = 160 (120 item rows, then 300 user rows), explicit
    and implicit, whole and als_chunk=16, is bitwise the same with 1, 3 and the default number of
    workgroups per launch."""
    s = smoke_als_160
    d, k, lam = s["d"], s["k"], s["lam"]

    def run(knobs, implicit):
        with monkeypatch.context() as mp:
            for key, value in knobs.items():
                set_knob(mp, key, value)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, s["uids"], s["P0"])
                ctx.set_factors(L.SIDE_ITEM, s["iids"], s["Q0"])
                ctx.als_prepare(d.u, d.i, d.r - 3.0 if implicit else d.r)
                if implicit:
                    ctx.als_run_implicit(2, lam, 1.0)
                else:
                    ctx.als_run(2, lam)
                return [bits(ctx.factors(side)[1]) for side in (L.SIDE_USER, L.SIDE_ITEM)]

    for implicit in (False, True):
        for chunk in ({}, {"als_chunk": 16}):
            ref = run(chunk, implicit)
            for slabs in (1, 3):
                got = run(dict(chunk, als_slabs=slabs), implicit)
                for x, y in zip(got, ref):
                    assert np.array_equal(x, y), (implicit, chunk, slabs)


# ---------------------------------------------------------------------------------------------
# 3. the normal equations and the Gram matrix through the hooks

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", HOOK_RANKS)
def test_hooks_normal_equations_exact(monkeypatch, mode, k):
    """edge_problem (1 to 200 ratings per row, a duplicate pair), lambda 0.5: A and b equal numpy's for
    every rated row of both sides and both regs, whole and als_chunk=64; the hook changes no factor; the
    half-sweep that follows is bitwise the same whole and split."""
    R.test_normal_equations_exact_at_bucket_edges(monkeypatch, mode, k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", HOOK_RANKS)
def test_hooks_implicit_normal_equations_exact(monkeypatch, mode, k):
    """The same for the implicit system, alpha 0.5 and 0."""
    R.test_implicit_normal_equations_exact_at_bucket_edges(monkeypatch, mode, k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", HOOK_RANKS)
def test_hooks_gram_exact(monkeypatch, mode, k):
    """als_gram for 1, 31, 33, 65 and 200 rated rows, default slice and als_gram_slice=64."""
    R.test_gram_exact_at_bucket_edges(monkeypatch, mode, k)


# ---------------------------------------------------------------------------------------------
# 4. backward error on real-valued data

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [129, 192, 256])
def test_solve_within_backward_error_bound(mode, k):
    """test_gpu_als.py's test of that name on 20 rows of 3 k / 2 ratings each, with its bound
    ||b - A x|| <= 2 u c (||A|| ||x|| + || |Q|^T |r| ||), c = k (n + 2) + 4 k (3 k + 1) + 2 (a blocked
    factorisation does the same number of operations per entry).  Measured on an MI355X, the largest
    residual / bound: see DESIGN.md section 4.7."""
    rows, n_row = 20, 3 * k // 2
    rng = np.random.default_rng(7 * k + rows)
    f32 = mode == L.MODE_FAST_F32
    u_round = 2.0 ** -24 if f32 else 2.0 ** -53
    nu = 512
    pu = np.concatenate([rng.choice(nu, n_row, replace=False) for _ in range(rows)])
    pi = np.repeat(np.arange(rows), n_row)
    perm = rng.permutation(len(pu))
    pu, pi = pu[perm], pi[perm]
    r = rng.integers(1, 11, len(pu)) / 2.0
    uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, rows + 2, 5)  # one user, two items unrated
    P, Q = rng.standard_normal((nu + 1, k)), rng.standard_normal((rows + 2, k))
    if f32:
        P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    irows = rows_of(pi, len(iids))
    lam = 0.1
    worst = 0.0
    for reg in REGS:
        with make_ctx(k, mode) as ctx:
            ctx.set_factors(L.SIDE_USER, uids, P)
            ctx.set_factors(L.SIDE_ITEM, iids, Q)
            ctx.als_prepare(uids[pu], iids[pi], r)
            ctx.als_run(1, lam, reg)
            X = ctx.lookup(L.SIDE_ITEM, iids)[0]
            assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, uids)[0]), bits(P))  # the side not solved
            assert np.array_equal(bits(X[rows:]), bits(Q[rows:]))                    # rows with no rating
        for a in range(rows):
            pos = irows[a]
            n = len(pos)
            M, b = normal_eq_reference(P, pu, r, pos, lam, reg, k)
            x = X[a]
            assert np.isfinite(x).all()
            c = k * (n + 2) + 4 * k * (3 * k + 1) + 2
            bound = 2 * u_round * c * (np.linalg.norm(M, 2) * np.linalg.norm(x) +
                                       np.linalg.norm(np.abs(P[pu[pos]]).T @ np.abs(r[pos])))
            res = np.linalg.norm(b - M @ x)
            worst = max(worst, res / bound)
            assert res <= bound, (reg, a, res, bound)
    print(f"als wide residual / bound: mode {mode} k {k}: {worst:.3e}")


# ---------------------------------------------------------------------------------------------
# 5. end to end at k = 160 against a numpy f64 ALS

@pytest.fixture(scope="module")
def smoke_als_160():
    d = synth.generate(300, 120, 6000, seed=3)
    uids, pu = np.unique(d.u, return_inverse=True)
    iids, pi = np.unique(d.i, return_inverse=True)
    rng = np.random.default_rng(4)
    k, lam, T = 160, 0.1, 2
    P0, Q0 = rng.random((len(uids), k)), rng.random((len(iids), k))
    urows, irows = rows_of(pu, len(uids)), rows_of(pi, len(iids))
    ref = {}
    for mode in MODES:
        P, Q = P0.copy(), Q0.copy()
        if mode == L.MODE_FAST_F32:
            P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
        for _ in range(T):
            numpy_half_sweep(Q, P, irows, pu, d.r, lam)
            numpy_half_sweep(P, Q, urows, pi, d.r, lam)
        err = d.r - np.einsum("nk,nk->n", P[pu], Q[pi])
        ref[mode] = float(np.sqrt(err @ err / len(err)))
    return dict(d=d, uids=uids, iids=iids, pu=pu, pi=pi, k=k, lam=lam, T=T, P0=P0, Q0=Q0, ref=ref)


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_against_numpy_als(smoke_als_160, mode):
    """The smoke data at k = 160, lambda 0.1 weighted, 2 iterations: the regularised objective falls at
    each of the 4 half-sweeps, the training RMSE is within the project's band (relative 0.005) of a
    numpy f64 ALS from the same start, and a twin context ends bitwise equal.  The measured relative
    difference: see DESIGN.md section 4.7."""
    s = smoke_als_160
    d, k, lam, T = s["d"], s["k"], s["lam"], s["T"]

    def start():
        ctx = make_ctx(k, mode)
        ctx.set_factors(L.SIDE_USER, s["uids"], s["P0"])
        ctx.set_factors(L.SIDE_ITEM, s["iids"], s["Q0"])
        ctx.als_prepare(d.u, d.i, d.r)
        return ctx

    with start() as ctx, start() as twin:
        _, P = ctx.factors(L.SIDE_USER)
        _, Q = ctx.factors(L.SIDE_ITEM)
        obj = [objective(P, Q, s["pu"], s["pi"], d.r, lam)]
        for _ in range(2 * T):
            ctx.als_run(1, lam)
            _, P = ctx.factors(L.SIDE_USER)
            _, Q = ctx.factors(L.SIDE_ITEM)
            obj.append(objective(P, Q, s["pu"], s["pi"], d.r, lam))
        print("als wide objective per half-sweep:", " ".join(f"{x:.6f}" for x in obj))
        assert all(b < a for a, b in zip(obj, obj[1:])), obj
        rmse, matched = ctx.rmse(d.u, d.i, d.r)
        rel = abs(rmse - s["ref"][mode]) / s["ref"][mode]
        print(f"als wide rmse: mode {mode} device {rmse:.9f} numpy {s['ref'][mode]:.9f} rel {rel:.3e}")
        assert matched == len(d.u)
        assert rel < 0.005
        for _ in range(2 * T):
            twin.als_run(1, lam)
        for side in (L.SIDE_USER, L.SIDE_ITEM):
            assert np.array_equal(bits(twin.factors(side)[1]), bits(ctx.factors(side)[1]))


# ---------------------------------------------------------------------------------------------
# 6. failure and bounds

@pytest.mark.parametrize("mode", MODES)
def test_singular_system_gives_nan_and_returns(mode):
    """test_gpu_als.py's singular system at k = 130: a pivot that is not a positive finite number makes
    the row NaN, and the kernel finishes."""
    k = 130
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, [1, 2], np.full((2, k), np.inf))
        ctx.set_factors(L.SIDE_ITEM, [5, 6], np.ones((2, k)))
        ctx.als_prepare([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
        ctx.als_run(1, 0.1)
        assert np.isnan(ctx.lookup(L.SIDE_ITEM, [5, 6])[0]).all()


@pytest.mark.parametrize("mode", MODES)
def test_k256_model_is_an_ordinary_one(mode, tmp_path):
    """als_fit at k = 256, then rmse, recommend and save / load on the fitted context."""
    d = synth.generate(300, 120, 6000, seed=3)
    k, lam = 256, 0.1
    uids = np.unique(d.u)
    with make_ctx(k, mode, seed=11) as ctx:
        ctx.als_fit(d.u, d.i, d.r, 1, lam)
        rmse, matched = ctx.rmse(d.u, d.i, d.r)
        # against numpy on the factors read back: a prediction is a k-term chain in another order than
        # numpy's, off by at most k u sum |p||q| (u = 2^-53, and 2^-24 allowed in fast mode)
        (iu, P), (ii, Q) = ctx.factors(L.SIDE_USER), ctx.factors(L.SIDE_ITEM)
        Pn, Qn = P[np.searchsorted(iu, d.u)], Q[np.searchsorted(ii, d.i)]
        err = d.r - np.einsum("nk,nk->n", Pn, Qn)
        want = float(np.sqrt(err @ err / len(err)))
        u_round = 2.0 ** -53 if mode == L.MODE_DETERMINISTIC_F64 else 2.0 ** -24
        eps = k * u_round * float((np.abs(Pn) * np.abs(Qn)).sum(1).max())
        assert matched == len(d.u) and abs(rmse - want) <= eps + 1e-12 * want, (rmse, want, eps)
        ids, sc, cnt = ctx.recommend(uids[:33], 10)
        assert (cnt == 10).all() and np.isfinite(sc).all()
        path = os.path.join(tmp_path, "als256.mfsnap")
        ctx.save(path)
        with make_ctx(k, mode, seed=11) as other:
            other.load(path)
            for side in (L.SIDE_USER, L.SIDE_ITEM):
                ia, va = ctx.factors(side)
                ib, vb = other.factors(side)
                assert np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))


@pytest.mark.parametrize("mode", MODES)
def test_rank_257_is_refused(mode):
    rng = np.random.default_rng(2)
    u, i, r = small_problem(rng)
    with make_ctx(257, mode) as ctx:
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit(u, i, r, 1, 0.1)
        assert e.value.code == L.MF_ERR_INVALID and "256" in str(e.value)
