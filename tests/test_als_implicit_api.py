"""The implicit-feedback ALS surface that needs no GPU: header, bindings, argument checks, the mirror
API and the JNI declaration."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT
from mfhip import _lib as L

FUNCS = ["mf_als_run_implicit", "mf_als_fit_implicit"]
HOOKS = ["mf_debug_als_gram", "mf_debug_als_normal_eq_implicit"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_and_exports_list_the_implicit_functions():
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


def test_header_states_the_contract():
    txt = header("mfhip.h")
    for phrase in ("w_j = alpha * |r_j|", "numExplicits", "then + G; then + lambda'", "share the counter",
                   "alpha = 0 is valid"):
        assert phrase in txt, phrase


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    u = (C.c_int32 * 1)(1)
    r = (C.c_double * 1)(1.0)
    g = (C.c_double * 1)(0.0)
    for st in (lib.mf_als_fit_implicit(None, u, u, r, 1, 1, 0.1, L.ALS_REG_WEIGHTED, 1.0),
               lib.mf_als_run_implicit(None, 1, 0.1, L.ALS_REG_WEIGHTED, 1.0),
               lib.mf_debug_als_gram(None, L.SIDE_USER, g),
               lib.mf_debug_als_normal_eq_implicit(None, L.SIDE_USER, 1, 0.1, L.ALS_REG_WEIGHTED, 1.0, g, g)):
        assert st == L.MF_ERR_INVALID
        assert lib.mf_last_error().decode()


def test_train_implicit_signature_and_defaults():
    import mfhip
    sig = inspect.signature(mfhip.ALS.trainImplicit)
    assert list(sig.parameters) == ["ratings", "rank", "iterations", "lambda_", "alpha", "mode", "seed"]
    p = sig.parameters
    assert p["iterations"].default == 10 and p["lambda_"].default == 0.01 and p["alpha"].default == 0.01
    assert p["mode"].default == "deterministic" and p["seed"].default == 0


def test_context_has_the_implicit_methods():
    from mfhip.context import Context
    for m in ("als_run_implicit", "als_fit_implicit", "als_gram", "als_normal_eq_implicit"):
        assert callable(getattr(Context, m)), m
    assert inspect.signature(Context.als_run_implicit).parameters["reg"].default == L.ALS_REG_WEIGHTED
    assert inspect.signature(Context.als_fit_implicit).parameters["reg"].default == L.ALS_REG_WEIGHTED


def test_jni_declares_als_fit_implicit():
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    assert re.search(r"native\s+void\s+alsFitImplicit\s*\(", java)
    assert "JFN(alsFitImplicit)" in shim and "mf_als_fit_implicit(" in shim
