"""The non-negative ALS surface that needs no GPU: header, exports, bindings, the rule set the header
states, the checks made before a context is needed, the mirror API, the JNI declarations and the bench
tool's option.  (The argument checks that need a context are in test_gpu_als_nonneg.py.)"""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT
from mfhip import _lib as L

FUNCS = ["mf_als_run_nonneg", "mf_als_run_implicit_nonneg", "mf_als_fit_nonneg", "mf_als_fit_implicit_nonneg",
         "mf_als_nonneg_stats", "mf_nnls_solve"]
HOOKS = ["mf_debug_als_nnls_row"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_and_exports_list_the_nonneg_functions():
    pub, tst = header("mfhip.h"), header("mfhip_testing.h")
    for f in FUNCS:
        assert re.search(r"^int\s+%s\s*\(" % f, pub, flags=re.M), f
        assert f in L.EXPORTS
        assert hasattr(L.lib(), f)
    for f in HOOKS:
        assert re.search(r"^int\s+%s\s*\(" % f, tst, flags=re.M), f
        assert f not in pub
        assert f in L.TESTING_EXPORTS and f not in L.EXPORTS
        assert hasattr(L.lib(), f)


def test_stats_struct_matches_the_header():
    m = re.search(r"struct\s+mf_als_nonneg_stats\s*\{([^}]*)\}", header("mfhip.h"))
    assert m
    names = re.findall(r"\b([a-z_0-9]+)\s*[,;]", m.group(1))
    assert names == [n for n, _ in L.mf_als_nonneg_stats._fields_]
    assert names == ["rows", "iterations", "max_iterations", "capped", "reason2", "nan_rows"]
    assert C.sizeof(L.mf_als_nonneg_stats) == 48


def test_header_states_the_rule_set():
    txt = header("mfhip.h")
    for phrase in ("nd <= tol2 * bb", "slack = 1 - 64 eps", "max(400, 20 k)", "tol2 = 1e-12",
                   "if it > lastWall + 1", "do not cross a wall", "x_i = +0, lastWall = it",
                   "0  converged", "1  hit the iteration cap", "2  step <= 0", "3  a non-finite step or bb",
                   "the whole row is NaN", "never -0", "set to +0 without", "l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1",
                   "over j = 0 .. k-1 of A[j][i] v[j]", "over i ascending", "No floating-point atomics",
                   "may be mixed", "scale-free", "a function of k alone"):
        assert phrase in txt, phrase


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    u = (C.c_int32 * 1)(1)
    r = (C.c_double * 1)(1.0)
    n = C.c_int32(0)
    st = L.mf_als_nonneg_stats()
    W = L.ALS_REG_WEIGHTED
    for code in (lib.mf_als_run_nonneg(None, 1, 0.1, W), lib.mf_als_run_implicit_nonneg(None, 1, 0.1, W, 1.0),
                 lib.mf_als_fit_nonneg(None, u, u, r, 1, 1, 0.1, W),
                 lib.mf_als_fit_implicit_nonneg(None, u, u, r, 1, 1, 0.1, W, 1.0),
                 lib.mf_als_nonneg_stats(None, C.byref(st)),
                 lib.mf_debug_als_nnls_row(None, L.SIDE_USER, 1, 0.1, W, -1.0, r, C.byref(n), C.byref(n))):
        assert code == L.MF_ERR_INVALID
        assert lib.mf_last_error().decode()


def test_context_has_the_nonneg_methods():
    from mfhip.context import Context
    for m in ("als_run_nonneg", "als_run_implicit_nonneg", "als_fit_nonneg", "als_fit_implicit_nonneg",
              "als_nnls_row", "nnls_solve", "als_nonneg_stats"):
        assert callable(getattr(Context, m)), m
    for m in ("als_run_nonneg", "als_run_implicit_nonneg", "als_fit_nonneg", "als_fit_implicit_nonneg", "als_nnls_row"):
        assert inspect.signature(getattr(Context, m)).parameters["reg"].default == L.ALS_REG_WEIGHTED, m
    x, it, why = Context.nnls_solve([[4.0, 0.0], [0.0, 9.0]], [8.0, -1.0], f64=False)
    assert (x.tolist(), why) == ([2.0, 0.0], 0)


def test_solver_argument_offers_nnls():
    import mfhip
    from mfhip import als
    assert "nnls" in als.SOLVERS
    s = mfhip.ALS.withSolver("nnls")
    assert s.solver == "nnls"
    assert mfhip.ALS.withSolver("nnls", cg_steps=7).solver == "nnls"
    with pytest.raises(ValueError):
        mfhip.ALS.withSolver("NNLS")
    assert list(inspect.signature(s.train).parameters) == list(inspect.signature(mfhip.ALS.train).parameters)
    assert (list(inspect.signature(s.trainImplicit).parameters) ==
            list(inspect.signature(mfhip.ALS.trainImplicit).parameters))


def test_jni_declares_the_nonneg_calls():
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    for native, cfn in (("alsRunNonneg", "mf_als_run_nonneg("), ("alsRunImplicitNonneg", "mf_als_run_implicit_nonneg("),
                        ("alsFitNonneg", "mf_als_fit_nonneg("), ("alsFitImplicitNonneg", "mf_als_fit_implicit_nonneg(")):
        assert re.search(r"native\s+void\s+%s\s*\(" % native, java), native
        assert "JFN(%s)" % native in shim and cfn in shim, native


def test_als_bench_offers_the_solver():
    txt = open(os.path.join(ROOT, "tools", "als_bench.py")).read()
    assert re.search(r'choices=\("cholesky", "cg", "nnls"\)', txt)
    assert "als_run_nonneg" in txt and "als_nonneg_stats" in txt


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        assert "mf_als_run_nonneg" in txt, doc
