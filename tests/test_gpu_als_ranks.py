"""ALS at every rank bucket, on systems whose solution is exact (csrc/kernels_als.hip).

kernels_als.hip is instantiated per rank bucket NB = ceil(k / 32), KP = 32 NB, and finish_row walks
the matrix in 16-column blocks (MB = 2 NB of them, the last one partial or empty unless 16 | k).
RANKS puts a rank on both sides of every bucket edge and of every 16-column block edge:

  NB 1 (MB 2)  1, 16, 17, 31, 32      NB 2 (MB 4)  33, 64
  NB 3 (MB 6)  65, 80, 96             NB 4 (MB 8)  97, 100, 127, 128

The solves are checked for equality, not against a bound.  The data are chosen so that every
intermediate of the accumulation, the Cholesky factorisation and both triangular solves is an
integer far below 2^24, so f32 and f64, any summation order and contracted multiply-adds all give
the same values, and the device must return a planted integer solution exactly:

  explicit  k counterpart rows carry the rows of L^T (L lower triangular, off the diagonal dense in
            {-1, 0, 1}, on it {1, 2, 3}); a solved row rates all of them with r = L^T x0, x0 in
            {-3..3}.  Then Q^T Q = L L^T, whose Cholesky factor is L itself (pivots perfect squares,
            quotients integers), Q^T r = L L^T x0 and x = x0.
  implicit  alpha = 1, one group of k counterpart rows with Q = L^T, L = I + N, N non-zero only in
            rows >= k // 2 and columns < k // 2 (so N^2 = 0 and L^-1 = I - N); ratings from
            {3, 8, 15, -3, -8, -15}, so 1 + |r| is a square.  G = L L^T, A = (L S)(L S)^T with
            S = diag sqrt(1 + |r|), b = L c with c = 1 + r where r > 0, else 0, and
            x = (I - N)^T [r > 0].
  lambda    the API wants lambda > 0: 1e-300 converts to 0 in f32 and is absorbed by the integer
            diagonal in f64 (times the row's count too), so A is L L^T exactly.  That lambda reaches
            the diagonal is pinned by the normal-equation tests, which read A after the addition.
  fillers   counterpart rows with all-zero factors and arbitrary ratings change neither A, b nor G;
            they set the rating count apart from k: k, k + 1 (the odd/even flip of the
            two-ratings-per-MFMA pairing, a row on either side of the 32-rating tile) and k + 200.

Every construction is verified in integers on the host before the device is called, with every
entry of A, b and r below 2^20.  A mismatch on the device therefore means a dropped or misplaced
update, an indexing error in some bucket, or a sqrt or division that is not correctly rounded.

Which test drives which instance (every rank in RANKS, f32 and f64):
  test_explicit_solve_is_exact   k_als<T, NB> whole rows (default, als_batch=5: three launches);
                                 als_chunk=16: k_als<T, NB> chunks + k_als_reduce<T, NB>
  test_implicit_solve_is_exact   k_als<T, NB, true>, k_als_gram<T, NB> (als_gram_slice=8: many
                                 slices); als_chunk=16: chunks + k_als_reduce<T, NB, true>
  test_normal_equations_exact_at_bucket_edges, test_implicit_normal_equations_exact_at_bucket_edges,
  test_gram_exact_at_bucket_edges   the hooks at k = 32, 33, 65, 80, 96, 97 (the ranks the tests of
                                 test_gpu_als.py and test_gpu_als_implicit.py do not run), whole
                                 rows and rows split by als_chunk=64
"""
import numpy as np
import pytest

import mfhip
from als_support import (MODES, N_ITEMS, REGS, TINY, bits, explicit_problem, first_difference, implicit_problem,
                         make_ctx, rows_of, shuffled_ids)
from conftest import set_knob
from mfhip import _lib as L

pytestmark = pytest.mark.gpu

RANKS = [1, 16, 17, 31, 32, 33, 64, 65, 80, 96, 97, 100, 127, 128]
EDGE_RANKS = [32, 33, 65, 80, 96, 97]


# ---------------------------------------------------------------------------------------------
# 1. the explicit half-sweep returns the planted solution exactly

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", RANKS)
def test_explicit_solve_is_exact(monkeypatch, mode, k):
    """als_run(1, 1e-300) must return x0 for every item, with both regs, by whole rows in one launch,
    in three launches (als_batch=5) and by split rows (als_chunk=16: every row of more than 16 ratings
    goes through k_als_reduce; at k <= 16 a row of exactly k ratings stays whole).  The user side
    and the items without ratings stay bitwise as they were."""
    d = explicit_problem(k)
    for knob in (None, ("als_chunk", 16), ("als_batch", 5)):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
                for reg in REGS:
                    ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
                    ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
                    ctx.als_run(1, TINY, reg)
                    X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
                    assert np.array_equal(X[:N_ITEMS], d["X0"]), (k, mode, knob, reg, first_difference(X, d["X0"]))
                    assert np.array_equal(bits(X[N_ITEMS:]), bits(d["Q0"][N_ITEMS:]))
                    assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, d["uids"])[0]), bits(d["P"]))


# ---------------------------------------------------------------------------------------------
# 2. the implicit half-sweep returns the planted solution exactly

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", RANKS)
def test_implicit_solve_is_exact(monkeypatch, mode, k):
    """als_run_implicit(1, 1e-300, 1.0) must return (I - N)^T [r > 0] for every item, with both regs,
    by whole rows, by split rows (als_chunk=16) and with G summed over many slices (als_gram_slice=8).
    The item without a positive rating is +0 bitwise; the user side and the items without ratings
    stay bitwise as they were."""
    d = implicit_problem(k)
    for knob in (None, ("als_chunk", 16), ("als_gram_slice", 8)):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
                for reg in REGS:
                    ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
                    ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
                    ctx.als_run_implicit(1, TINY, 1.0, reg)
                    X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
                    assert np.array_equal(X[:N_ITEMS], d["X"]), (k, mode, knob, reg, first_difference(X, d["X"]))
                    assert np.array_equal(bits(X[0]), bits(np.zeros(k)))
                    assert np.array_equal(bits(X[N_ITEMS:]), bits(d["Q0"][N_ITEMS:]))
                    assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, d["uids"])[0]), bits(d["P"]))


# ---------------------------------------------------------------------------------------------
# 3. the normal equations and the Gram matrix at the ranks the other two files leave out

EDGE_COUNTS = (1, 31, 32, 33, 64, 65, 200)


def edge_problem(rng, k, lo):
    """A reduced int_problem (test_gpu_als.py): items 0..6 with 1, 31, 32, 33, 64, 65 and 200 ratings,
    item 7 with three, two of them the same (user, item) pair; 200 users; one id per side that is in the
    model but not in the data; factors in {-3..3}, ratings in {lo..5}.  Under als_chunk=64 the
    200-rating row is 4 chunks with a last chunk of 8 and the 65-rating row has a last chunk of 1."""
    nu, ni = 200, len(EDGE_COUNTS) + 1
    pu, pi = [], []
    for item, c in enumerate(EDGE_COUNTS):
        pu += rng.choice(nu, c, replace=False).tolist()
        pi += [item] * c
    pu += [5, 5, 9]
    pi += [ni - 1] * 3
    pu, pi = np.array(pu), np.array(pi)
    r = rng.integers(lo, 6, len(pu)).astype(np.float64)
    if lo < 0:
        r[pi == ni - 1] = [-1.0, 0.0, -2.0]            # no positive rating
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, ni + 1, 5)
    P = rng.integers(-3, 4, (nu + 1, k)).astype(np.float64)
    Q = rng.integers(-3, 4, (ni + 1, k)).astype(np.float64)
    urows, irows = rows_of(pu, nu + 1), rows_of(pi, ni + 1)
    assert [len(x) for x in irows] == list(EDGE_COUNTS) + [3, 0] and len(urows[-1]) == 0
    return pu, pi, r, uids, iids, P, Q, urows, irows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", EDGE_RANKS)
def test_normal_equations_exact_at_bucket_edges(monkeypatch, mode, k):
    """test_gpu_als.py's test_normal_equations_exact at the ranks it leaves out: A and b through the
    hook equal numpy's exactly for every rated row of both sides and both regs, whole and split
    (als_chunk=64), and the half-sweep is bitwise the same either way."""
    rng = np.random.default_rng(100 + k)
    pu, pi, r, uids, iids, P, Q, urows, irows = edge_problem(rng, k, 1)
    lam = 0.5
    sides = ((L.SIDE_USER, uids, urows, Q, pi), (L.SIDE_ITEM, iids, irows, P, pu))
    first_half = []
    for knob in (None, ("als_chunk", 64)):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, uids, P)
                ctx.set_factors(L.SIDE_ITEM, iids, Q)
                ctx.als_prepare(uids[pu], iids[pi], r)
                for side, ids, rows, F_other, other_index in sides:
                    for a, pos in enumerate(rows):
                        if not len(pos):
                            continue
                        Qm = F_other[other_index[pos]]
                        for reg in REGS:
                            lam_row = lam * len(pos) if reg == L.ALS_REG_WEIGHTED else lam
                            gA, gb = ctx.als_normal_eq(side, ids[a], lam, reg)
                            assert np.array_equal(gA, Qm.T @ Qm + lam_row * np.eye(k)), (knob, reg, side, a)
                            assert np.array_equal(gb, Qm.T @ r[pos]), (knob, reg, side, a)
                assert np.array_equal(ctx.lookup(L.SIDE_USER, uids)[0], P)  # the hook changes nothing
                assert np.array_equal(ctx.lookup(L.SIDE_ITEM, iids)[0], Q)
                with pytest.raises(mfhip.MFError):  # no rating in the data
                    ctx.als_normal_eq(L.SIDE_ITEM, iids[-1], lam)
                ctx.als_run(1, lam)
                first_half.append(ctx.lookup(L.SIDE_ITEM, iids)[0])
                assert np.array_equal(first_half[-1][-1], Q[-1])
                assert np.isfinite(first_half[-1]).all()
    assert np.array_equal(bits(first_half[1]), bits(first_half[0]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", EDGE_RANKS)
def test_implicit_normal_equations_exact_at_bucket_edges(monkeypatch, mode, k):
    """test_gpu_als_implicit.py's test_normal_equations_exact at the ranks it leaves out: ratings in
    {-2..5}, alpha 0.5 (both sides) and 0 (the item side), lambda 0.5; A and b through the hook equal
    numpy's exactly, whole and split (als_chunk=64); the half-sweep is bitwise the same either way and
    sets the item without a positive rating to +0."""
    rng = np.random.default_rng(500 + k)
    pu, pi, r, uids, iids, P, Q, urows, irows = edge_problem(rng, k, -2)
    assert {-1.0, 0.0, 1.0} <= set(np.sign(r)) and not (r[irows[-2]] > 0).any()
    lam = 0.5
    rated_u, rated_i = np.unique(pu), np.unique(pi)
    sides = ((L.SIDE_USER, uids, urows, Q, pi, Q[rated_i].T @ Q[rated_i], (0.5,)),
             (L.SIDE_ITEM, iids, irows, P, pu, P[rated_u].T @ P[rated_u], (0.5, 0.0)))
    halves = []
    for knob in (None, ("als_chunk", 64)):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, uids, P)
                ctx.set_factors(L.SIDE_ITEM, iids, Q)
                ctx.als_prepare(uids[pu], iids[pi], r)
                for side, ids, rows, F_other, other_index, G, alphas in sides:
                    for a, pos in enumerate(rows):
                        if not len(pos):
                            continue
                        Qm = F_other[other_index[pos]]
                        npos = int((r[pos] > 0).sum())
                        for alpha in alphas:
                            w = alpha * np.abs(r[pos])
                            b = Qm.T @ np.where(r[pos] > 0, 1.0 + w, 0.0)
                            for reg in REGS:
                                lam_row = lam * npos if reg == L.ALS_REG_WEIGHTED else lam
                                A = G + (Qm * w[:, None]).T @ Qm + lam_row * np.eye(k)
                                gA, gb = ctx.als_normal_eq_implicit(side, ids[a], lam, alpha, reg)
                                assert np.array_equal(gA, A), (knob, side, a, alpha, reg)
                                assert np.array_equal(gb, b), (knob, side, a, alpha, reg)
                assert np.array_equal(ctx.lookup(L.SIDE_USER, uids)[0], P)  # the hook changes nothing
                assert np.array_equal(ctx.lookup(L.SIDE_ITEM, iids)[0], Q)
                ctx.als_run_implicit(1, lam, 0.5)
                X = ctx.lookup(L.SIDE_ITEM, iids)[0]
                assert np.array_equal(bits(X[-1]), bits(Q[-1]))           # unrated: untouched
                assert np.array_equal(bits(X[-2]), bits(np.zeros(k)))     # no positive rating: +0 exactly
                assert np.isfinite(X).all() and X[len(EDGE_COUNTS) - 1].any()
                ctx.als_run_implicit(1, lam, 0.5)
                U = ctx.lookup(L.SIDE_USER, uids)[0]
                assert np.array_equal(bits(U[-1]), bits(P[-1])) and np.isfinite(U).all()
                halves.append((X, U))
    assert np.array_equal(bits(halves[1][0]), bits(halves[0][0]))
    assert np.array_equal(bits(halves[1][1]), bits(halves[0][1]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", EDGE_RANKS)
def test_gram_exact_at_bucket_edges(monkeypatch, mode, k):
    """test_gpu_als_implicit.py's test_gram_exact at the ranks it leaves out, for 1, 31, 33, 65 and 200
    rated rows, with the default slice and with 64 rows per slice (65 rows: a last slice of 1; 200:
    four slices, the last of 8)."""
    rng = np.random.default_rng(300 + k)
    for m in (1, 31, 33, 65, 200):
        nu = 3
        pi = rng.permutation(m)
        pu = np.arange(m) % min(nu, m)
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
                        assert np.array_equal(ctx.als_gram(side), want[side]), (m, slice_, side)
                    assert np.array_equal(ctx.lookup(L.SIDE_ITEM, iids)[0], Q)  # the hook changes nothing
