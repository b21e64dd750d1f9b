"""mf_als_objective / mf_als_run_until without a device: the numpy replay of the objective's arithmetic
(mfhip.als.replay_objective) against integer values and the dense formula, the bindings, and the argument checks that
need no context."""
import ctypes as C

import numpy as np
import pytest

import mfhip
from als_objective_support import (COUNTS, FIELDS, RANKS, csr_of, dense_objective, field_error, how_of,
                                   integer_objective, planted)
from als_support import REGS, bits
from mfhip import _lib as L
from mfhip.als import ALS, StreamingALS, _sum64, replay_objective


def gram(F, rated):
    return F[rated].T @ F[rated]


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("k", RANKS)
def test_replay_is_exact_on_the_planted_problems(k, implicit):
    """Every intermediate is an integer below 2^24 (asserted by integer_objective), so the replay must return the
    integer value of every field in f32 and in f64, at the start factors and at the planted solution, in either
    orientation, whole rows and rows cut by chunk = 5."""
    for exchanged in (False, True):
        d = planted(implicit, k, exchanged)
        off, cols, vals = csr_of(d["pu"], d["pi"], d["r"], len(d["P"]))
        for at in ("start", "sol"):
            P, Q = (d["sol"] if exchanged and at == "sol" else d["P"]), (d["sol"] if not exchanged and at == "sol" else d["Q"])
            GU, GI = gram(P, np.unique(d["pu"])), gram(Q, np.unique(d["pi"]))
            for reg in REGS:
                want = integer_objective(P, Q, d["pu"], d["pi"], d["r"], implicit, reg)
                for dtype in (np.float32, np.float64):
                    for chunk in (16384, 5):
                        got = replay_objective(P, Q, off, cols, vals, GU, GI, how_of(1.0, reg, implicit, 1.0), chunk, dtype)
                        assert {f: got[f] for f in FIELDS + COUNTS} == {f: want[f] for f in FIELDS + COUNTS}, \
                            (k, implicit, exchanged, at, reg, dtype, chunk)


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_replay_lies_within_the_forward_bound(dtype, implicit):
    """Random data, k = 3, 64 and 160: every field of the replay within dense_objective's bound of the dense
    value; a chunk of 7 cuts most rows."""
    rng = np.random.default_rng(5)
    for k in (3, 64, 160):
        nu, ni, n = 60, 25, 900
        P, Q = rng.normal(0, 0.4, (nu, k)).astype(dtype), rng.normal(0, 0.4, (ni, k)).astype(dtype)
        pu, pi = rng.integers(0, nu - 2, n), rng.integers(0, ni - 1, n)   # two users and an item without ratings
        r = rng.integers(1, 11, n) / 2.0 - (3.0 if implicit else 0.0)
        off, cols, vals = csr_of(pu, pi, r, nu)
        GU = gram(P, np.unique(pu)).astype(dtype)
        GI = gram(Q, np.unique(pi)).astype(dtype)
        for reg in REGS:
            how = how_of(0.1, reg, implicit, 0.7)
            got = replay_objective(P, Q, off, cols, vals, GU, GI, how, 7, dtype)
            val, bound = dense_objective(P, Q, off, cols, vals, how, dtype)
            for f in FIELDS:
                assert field_error(got[f], val[f]) <= bound[f], (k, reg, f, got[f], float(val[f]), bound[f])
            assert (got["ratings"], got["user_rows"], got["item_rows"]) == (n, len(np.unique(pu)), len(np.unique(pi)))
            assert implicit or got["unobserved"] == 0.0


def test_sum64_order():
    """Lane l chains v[l], v[l + 64], ...; then the xor butterfly 32 .. 1: checked against a scalar restatement
    on values whose sum depends on the order."""
    rng = np.random.default_rng(1)
    for n in (0, 1, 63, 64, 65, 200, 1000):
        v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        lanes = [0.0] * 64
        for j in range(n):
            lanes[j % 64] = lanes[j % 64] + v[j]
        for b in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ b] for l in range(64)]
        assert bits(np.array([_sum64(v)])) == bits(np.array([lanes[0]]))


def test_replay_of_no_ratings_is_zero():
    out = replay_objective(np.ones((3, 4)), np.ones((2, 4)), np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0),
                           None, None, how_of(0.5, L.ALS_REG_WEIGHTED), 16384, np.float32)
    assert all(out[f] == 0 for f in FIELDS + COUNTS)


def test_bindings_and_struct_layout():
    """mf_als_loss is 5 doubles, 3 int64 and 4 reserved doubles; both symbols are bound with their signatures."""
    assert C.sizeof(L.mf_als_loss) == 12 * 8
    assert [n for n, _ in L.mf_als_loss._fields_][:8] == list(FIELDS + COUNTS)
    lib = L.lib()
    assert lib.mf_als_objective.argtypes[1:] == [C.POINTER(L.mf_als_solve), C.POINTER(L.mf_als_loss)]
    assert len(lib.mf_als_run_until.argtypes) == 6
    assert {"mf_als_objective", "mf_als_run_until"} <= set(L.EXPORTS)


def test_null_arguments_are_refused_without_a_context():
    lib = L.lib()
    how, out = how_of(0.1, L.ALS_REG_WEIGHTED), L.mf_als_loss()
    assert lib.mf_als_objective(None, C.byref(how), C.byref(out)) == L.MF_ERR_INVALID
    assert lib.mf_als_run_until(None, C.byref(how), 1, 0.0, None, None) == L.MF_ERR_INVALID


def test_python_argument_checks():
    """tol= belongs to ALS.withSolver (ALS.train's own parameter list is pinned by test_als_api.py) and is checked
    before a context is made; the trainers keep ALS.train's parameters; StreamingALS.objective needs a fit."""
    import inspect
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ALS.withSolver("cg", tol=bad)
    s = ALS.withSolver("cholesky", tol=1e-3)
    assert s.tol == 1e-3 and ALS.withSolver("cg").tol is None
    assert list(inspect.signature(s.train).parameters) == list(inspect.signature(ALS.train).parameters)
    with pytest.raises(ValueError):
        s.train(([1], [1], [1.0]), 4, iterations=-1)
    with pytest.raises(RuntimeError):
        StreamingALS(rank=4).objective()
