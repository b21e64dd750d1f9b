"""The conjugate-gradient ALS surface that needs no GPU: header, bindings, constants, the checks made
before a context is needed, the mirror API and the JNI declarations.  (The argument checks that need
a context -- cg_steps, lambda, alpha, reg, a run before prepare -- are in test_gpu_als_cg.py: a
context cannot be created without a device.)"""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT
from mfhip import _lib as L

FUNCS = ["mf_als_run_cg", "mf_als_run_implicit_cg", "mf_als_fit_cg", "mf_als_fit_implicit_cg"]
HOOKS = ["mf_debug_als_cg_matvec", "mf_debug_als_cg_capacity"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_and_exports_list_the_cg_functions():
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


def test_constant_matches_the_header():
    m = re.search(r"^#define\s+MF_ALS_CG_MAX_STEPS\s+(\d+)", header("mfhip.h"), flags=re.M)
    assert m and int(m.group(1)) == L.ALS_CG_MAX_STEPS == 256


def test_header_states_the_arithmetic_and_the_order():
    txt = header("mfhip.h")
    for phrase in ("a = rs / (p.Ap)", "x = fma(a, p, x)", "r = fma(-a, Ap, r)", "p = fma(rs'/rs, p, r)",
                   "rs == 0 ends the", "p.Ap == 0", "not finite makes the row NaN", "set to +0 without iterating",
                   "l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1", "ratings in CSR order", "in ascending order",
                   "((g0 + g1) + g2) + g3", "No floating-point atomics", "may be mixed",
                   "cg_steps outside 1 .. MF_ALS_CG_MAX_STEPS"):
        assert phrase in txt, phrase


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    u = (C.c_int32 * 1)(1)
    r = (C.c_double * 1)(1.0)
    g = (C.c_double * 1)(0.0)
    n = C.c_int32(0)
    W = L.ALS_REG_WEIGHTED
    for st in (lib.mf_als_run_cg(None, 1, 0.1, W, 3), lib.mf_als_run_implicit_cg(None, 1, 0.1, W, 1.0, 3),
               lib.mf_als_fit_cg(None, u, u, r, 1, 1, 0.1, W, 3),
               lib.mf_als_fit_implicit_cg(None, u, u, r, 1, 1, 0.1, W, 1.0, 3),
               lib.mf_debug_als_cg_matvec(None, L.SIDE_USER, 1, 0.1, W, -1.0, g, g, g),
               lib.mf_debug_als_cg_capacity(None, C.byref(n))):
        assert st == L.MF_ERR_INVALID
        assert lib.mf_last_error().decode()


def test_context_has_the_cg_methods():
    from mfhip.context import Context
    for m in ("als_run_cg", "als_run_implicit_cg", "als_fit_cg", "als_fit_implicit_cg", "als_cg_matvec"):
        assert callable(getattr(Context, m)), m
    for m in ("als_run_cg", "als_run_implicit_cg", "als_fit_cg", "als_fit_implicit_cg"):
        p = inspect.signature(getattr(Context, m)).parameters
        assert p["reg"].default == L.ALS_REG_WEIGHTED and p["cg_steps"].default == 3, m


def test_solver_argument_rejects_unknown_names_and_step_counts():
    import mfhip
    for name in ("lu", "CG", "", "conjugate"):
        with pytest.raises(ValueError):
            mfhip.ALS.withSolver(name)
    for steps in (0, -1, 257):
        with pytest.raises(ValueError):
            mfhip.ALS.withSolver("cg", cg_steps=steps)
    s = mfhip.ALS.withSolver("cg", cg_steps=256)
    assert (s.solver, s.cg_steps) == ("cg", 256)
    d = mfhip.ALS.withSolver()
    assert (d.solver, d.cg_steps) == ("cholesky", 3)
    # the chosen solver offers ALS.train's and ALS.trainImplicit's own parameters
    assert list(inspect.signature(s.train).parameters) == list(inspect.signature(mfhip.ALS.train).parameters)
    assert (list(inspect.signature(s.trainImplicit).parameters) ==
            list(inspect.signature(mfhip.ALS.trainImplicit).parameters))


def test_jni_declares_the_cg_calls():
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    for native, cfn in (("alsRunCg", "mf_als_run_cg("), ("alsRunImplicitCg", "mf_als_run_implicit_cg("),
                        ("alsFitCg", "mf_als_fit_cg("), ("alsFitImplicitCg", "mf_als_fit_implicit_cg(")):
        assert re.search(r"native\s+void\s+%s\s*\(" % native, java), native
        assert "JFN(%s)" % native in shim and cfn in shim, native


def test_als_bench_offers_the_solver():
    txt = open(os.path.join(ROOT, "tools", "als_bench.py")).read()
    assert "--solver" in txt and "--cg-steps" in txt
