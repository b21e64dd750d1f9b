"""mf_nnls_solve: the non-negative solve of the ALS half-sweeps on the host (csrc/nnls.cpp), in f32 and f64.

It is the replay the kernels are checked against bit for bit (test_gpu_als_nonneg.py); here it is checked
on its own, without a GPU: planted systems with a unique known solution at every rank bucket edge
(nnls_support.planted), the special cases of the rule set in mfhip.h, the scale-freeness of the stopping
rule, and the KKT conditions on systems shaped like an ALS row's.
"""
import numpy as np
import pytest

from mfhip import _lib as L
from mfhip.context import nnls_solve
from nnls_support import RANKS_HOST, als_shaped, assert_kkt, assert_planted, planted, scipy_nnls

PRECISIONS = [True, False]  # f64, f32


@pytest.mark.parametrize("f64", PRECISIONS)
@pytest.mark.parametrize("k", RANKS_HOST)
def test_planted_solution_is_found(k, f64):
    """Reason 0, x >= 0 without -0, the zero set of x* exactly, and |x - x*| within the tolerance."""
    for seed in (k, 1000 + k):
        A, b, xs, mu = planted(k, seed)
        assert (mu[xs == 0] >= 1).all() and not mu[xs > 0].any()
        x, it, why = nnls_solve(A, b, f64)
        assert why == 0, (k, f64, why)
        assert 0 <= it <= max(400, 20 * k)
        assert_planted(x, xs, A, b, f64, f"k {k} {'f64' if f64 else 'f32'} seed {seed} ({it} iterations)")


def test_rank_one_takes_one_iteration():
    for f64 in PRECISIONS:
        x, it, why = nnls_solve([[4.0]], [8.0], f64)
        assert (x[0], it, why) == (2.0, 1, 0)


@pytest.mark.parametrize("f64", PRECISIONS)
def test_nonpositive_right_hand_side_is_zero_at_once(f64):
    for k in (1, 33, 200):
        A, b, _, _ = planted(k, 5)
        for rhs in (-np.abs(b) - 1.0, np.zeros(k), np.where(np.arange(k) % 2, -1.0, 0.0)):
            x, it, why = nnls_solve(A, rhs, f64)
            assert (it, why) == (0, 0)
            assert not x.any() and not np.signbit(x).any()


@pytest.mark.parametrize("f64", PRECISIONS)
def test_nan_in_b_makes_the_row_nan(f64):
    A, b, _, _ = planted(40, 6)
    for bad in (np.nan, np.inf):
        rhs = b.copy()
        rhs[17] = bad
        x, it, why = nnls_solve(A, rhs, f64)
        assert why == 3 and it == 0 and np.isnan(x).all()
    A2 = A.copy()
    A2[3, 3] = np.nan
    x, it, why = nnls_solve(A2, b, f64)
    assert why == 3 and np.isnan(x).all()


@pytest.mark.parametrize("f64", PRECISIONS)
@pytest.mark.parametrize("k", [7, 64, 129])
def test_scaling_the_system_changes_nothing(k, f64):
    """(A, b) * 2^10: the same x and the same iteration count bit for bit, on a planted system and on an
    ALS-shaped one (whose entries are not integers)."""
    for A, b in (planted(k, 77)[:2], als_shaped(k, 3 * k + 50, 78)):
        if not f64:  # the scaled system must be the f32 system scaled: round first
            A, b = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        x, it, why = nnls_solve(A, b, f64)
        for s in (1024.0, 1.0 / 1024.0):
            x2, it2, why2 = nnls_solve(A * s, b * s, f64)
            assert (it2, why2) == (it, why)
            assert np.array_equal(x2.view(np.uint64), x.view(np.uint64))


@pytest.mark.parametrize("f64", PRECISIONS)
@pytest.mark.parametrize("k", [1, 8, 32, 100, 128, 160, 256])
def test_kkt_on_als_shaped_systems(k, f64):
    """Q^T Q + 0.05 n I for n in {5, 3 k + 50}: reason 0, the KKT conditions against the f64 gradient, and
    agreement with scipy's active-set solution where both have the same support."""
    for n in (5, 3 * k + 50):
        A, b = als_shaped(k, n, 31 * k + n)
        x, it, why = nnls_solve(A, b, f64)
        what = f"k {k} n {n} {'f64' if f64 else 'f32'} ({it} iterations)"
        assert why == 0, (what, why)
        assert it < max(400, 20 * k)
        assert_kkt(x, A, b, f64, what)
        ref = scipy_nnls(A, b)
        ev = np.linalg.eigvalsh(A)
        eps = np.finfo(np.float64 if f64 else np.float32).eps
        tol = 1e-6 * np.linalg.norm(b) / ev[0] + 64 * eps * (ev[-1] / ev[0]) * np.linalg.norm(ref)
        assert np.linalg.norm(x - ref) <= tol, (what, np.linalg.norm(x - ref), tol)


def test_arguments_are_checked():
    lib = L.lib()
    import ctypes as C
    g = (C.c_double * 4)(1.0, 0.0, 0.0, 1.0)
    for st in (lib.mf_nnls_solve(0, g, g, 1, g, None, None), lib.mf_nnls_solve(257, g, g, 1, g, None, None),
               lib.mf_nnls_solve(2, None, g, 1, g, None, None), lib.mf_nnls_solve(2, g, None, 1, g, None, None),
               lib.mf_nnls_solve(2, g, g, 1, None, None, None)):
        assert st == L.MF_ERR_INVALID and lib.mf_last_error().decode()
    x = (C.c_double * 2)()
    assert lib.mf_nnls_solve(2, g, (C.c_double * 2)(2.0, 3.0), 0, x, None, None) == L.MF_OK
    assert list(x) == [2.0, 3.0]
