"""The ALS surface that needs no GPU: header, bindings, constants, argument checks and the mirror API."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT
from mfhip import _lib as L

ALS_FUNCS = ["mf_als_fit", "mf_als_prepare", "mf_als_run"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_and_exports_list_the_als_functions():
    pub, tst = header("mfhip.h"), header("mfhip_testing.h")
    for f in ALS_FUNCS:
        assert re.search(r"^int\s+%s\s*\(" % f, pub, flags=re.M), f
        assert f in L.EXPORTS
        assert hasattr(L.lib(), f)
    assert re.search(r"^int\s+mf_debug_als_normal_eq\s*\(", tst, flags=re.M)
    assert "mf_debug_als_normal_eq" not in pub
    assert "mf_debug_als_normal_eq" in L.TESTING_EXPORTS
    assert hasattr(L.lib(), "mf_debug_als_normal_eq")


def test_constants_match_the_header():
    txt = header("mfhip.h")
    for name, val in (("MF_ALS_REG_WEIGHTED", L.ALS_REG_WEIGHTED), ("MF_ALS_REG_PLAIN", L.ALS_REG_PLAIN)):
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, txt, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert L.ALS_REG_WEIGHTED != L.ALS_REG_PLAIN


def test_header_documents_order_and_initial_factors():
    txt = header("mfhip.h")
    assert "Half-sweep 0 solves the item side" in txt
    assert "MLlib's own initial factors" in txt


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    u = (C.c_int32 * 1)(1)
    r = (C.c_double * 1)(1.0)
    for st in (lib.mf_als_fit(None, u, u, r, 1, 1, 0.1, L.ALS_REG_WEIGHTED), lib.mf_als_prepare(None, u, u, r, 1),
               lib.mf_als_run(None, 1, 0.1, L.ALS_REG_WEIGHTED)):
        assert st == L.MF_ERR_INVALID
        assert lib.mf_last_error().decode()


def test_als_is_importable_with_the_model_methods():
    import mfhip
    from mfhip.als import ALS, MatrixFactorizationModel
    assert mfhip.ALS is ALS
    sig = inspect.signature(ALS.train)
    assert list(sig.parameters) == ["ratings", "rank", "iterations", "lambda_", "mode", "seed"]
    assert sig.parameters["iterations"].default == 10 and sig.parameters["lambda_"].default == 0.01
    for m in ("userFeatures", "productFeatures", "predict", "recommendProducts", "recommendUsers",
              "recommendProductsForUsers"):
        assert callable(getattr(MatrixFactorizationModel, m)), m


def test_context_has_the_als_methods():
    from mfhip.context import Context
    for m in ("als_prepare", "als_run", "als_fit"):
        assert callable(getattr(Context, m)), m
    assert inspect.signature(Context.als_run).parameters["reg"].default == L.ALS_REG_WEIGHTED


def test_online_offline_spark_accepts_offline_algorithm():
    from mfhip.combined import OnlineOfflineSpark
    p = inspect.signature(OnlineOfflineSpark.__init__).parameters
    assert p["offline_algorithm"].default == "DSGD"


def test_jni_declares_als_fit():
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    assert re.search(r"native\s+void\s+alsFit\s*\(", java)
    assert "JFN(alsFit)" in shim and "mf_als_fit(" in shim
