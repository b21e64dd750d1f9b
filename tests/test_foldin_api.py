"""mf_als_foldin / mf_recommend_foldin: the surface that needs no GPU -- exports, declarations, wrappers, the
JNI natives, and the argument checks, which read nothing of the context."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from mfhip import _lib as L
from mfhip.context import als_solve

HEADER = os.path.join(ROOT, "include", "mfhip.h")
NEW = ("mf_als_foldin", "mf_recommend_foldin")


def test_symbols_are_exported_declared_and_wrapped():
    lib = L.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    import mfhip
    assert hasattr(mfhip.Context, "als_foldin") and hasattr(mfhip.Context, "recommend_foldin")
    assert hasattr(mfhip.als.MatrixFactorizationModel, "recommendProductsForSessions")


def test_java_natives_present():
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    for native, call in (("alsFoldin", "mf_als_foldin"), ("recommendFoldin", "mf_recommend_foldin")):
        assert re.search(r"public static native \w+(\[\])* " + native + r"\(", java), native
        assert re.search(r"JFN\(" + native + r"\)\(", shim) and re.search(r"\b" + call + r"\b", shim), native


OFF = np.array([0, 2, 3], np.int64)
I32 = np.zeros(8, np.int32)
F64 = np.zeros(64, np.float64)
FAKE = C.c_void_p(8)   # never dereferenced: each call below fails an argument check first


def _foldin(ctx=FAKE, side=L.SIDE_USER, off=OFF, ids=I32, r=F64, n=2, how=als_solve(0.1), vecs=F64, used=I32):
    p = lambda a, t: None if a is None else L.ptr(a, t)
    return L.lib().mf_als_foldin(ctx, side, p(off, C.c_int64), p(ids, C.c_int32), p(r, C.c_double), n,
                                 None if how is None else C.byref(how), p(vecs, C.c_double), p(used, C.c_int32))


def _fused(ctx=FAKE, side=L.SIDE_USER, off=OFF, ids=I32, r=F64, n=2, how=als_solve(0.1), top_n=5, exclude=1,
           out=I32, scores=F64, counts=I32, vecs=None, used=None):
    p = lambda a, t: None if a is None else L.ptr(a, t)
    return L.lib().mf_recommend_foldin(ctx, side, p(off, C.c_int64), p(ids, C.c_int32), p(r, C.c_double), n,
                                       None if how is None else C.byref(how), top_n, exclude, p(out, C.c_int32),
                                       p(scores, C.c_double), p(counts, C.c_int32), p(vecs, C.c_double),
                                       p(used, C.c_int32))


def test_null_context_is_invalid_with_a_message():
    for st in (_foldin(ctx=None), _fused(ctx=None)):
        assert st == L.MF_ERR_INVALID
        assert b"null context" in L.lib().mf_last_error()


def test_argument_checks_come_before_the_context_is_used():
    """Every MF_ERR_INVALID case that can be told from the arguments alone is refused on an opaque non-null
    handle, with a message that names the argument."""
    lib = L.lib()
    nan, inf = float("nan"), float("inf")
    big = np.array([0, 2 ** 31], np.int64)         # 2^31 entries: never read, the total is refused first
    for call in (_foldin, _fused):
        cases = [
            (dict(side=2), "side"), (dict(side=-1), "side"),
            (dict(n=-1), "n_queries"),
            (dict(how=None), "mf_als_solve"),
            (dict(off=None), "offsets"),
            (dict(off=np.array([1, 2, 3], np.int64)), "offsets[0]"),
            (dict(off=np.array([0, 3, 2], np.int64)), "offsets"),
            (dict(off=big, n=1), "2^31"),
            (dict(ids=None), "cand_ids"), (dict(r=None), "ratings"),
            (dict(how=als_solve(0.0)), "lambda"), (dict(how=als_solve(-1.0)), "lambda"),
            (dict(how=als_solve(nan)), "lambda"), (dict(how=als_solve(inf)), "lambda"),
            (dict(how=als_solve(0.1, reg=7)), "reg"),
            (dict(how=als_solve(0.1, implicit=True, alpha=-1.0)), "alpha"),
            (dict(how=als_solve(0.1, implicit=True, alpha=inf)), "alpha"),
            (dict(how=als_solve(0.1, solver="cg", cg_steps=0)), "cg_steps"),
            (dict(how=als_solve(0.1, solver="cg", cg_steps=L.ALS_CG_MAX_STEPS + 1)), "cg_steps"),
        ]
        bad_solver = als_solve(0.1)
        bad_solver.solver = 9
        cases.append((dict(how=bad_solver), "solver"))
        for kw, word in cases:
            assert call(**kw) == L.MF_ERR_INVALID, (call.__name__, kw)
            assert word in lib.mf_last_error().decode(), (call.__name__, kw, lib.mf_last_error())
    for kw, word in ((dict(vecs=None), "vecs_out"),):
        assert _foldin(**kw) == L.MF_ERR_INVALID, kw
        assert word in lib.mf_last_error().decode(), kw
    for kw, word in ((dict(out=None), "ids_out"), (dict(counts=None), "counts_out"),
                     (dict(exclude=2), "exclude_rated"), (dict(exclude=-1), "exclude_rated"),
                     (dict(top_n=0), "top_n"), (dict(top_n=L.RECOMMEND_MAX_TOP + 1), "top_n")):
        assert _fused(**kw) == L.MF_ERR_INVALID, kw
        assert word in lib.mf_last_error().decode(), kw


def test_python_wrappers_check_their_lists():
    import mfhip
    import pytest
    ctx = mfhip.Context.__new__(mfhip.Context)      # no handle: the checks below come before any call
    ctx._h, ctx.k = C.c_void_p(None), 4
    how = als_solve(0.1)
    with pytest.raises(ValueError):
        ctx.als_foldin(L.SIDE_USER, [0, 2], [1, 2, 3], [1.0, 2.0, 3.0], how)      # offsets end short of the lists
    with pytest.raises(ValueError):
        ctx.als_foldin(L.SIDE_USER, [0, 2], [1, 2], [1.0], how)                   # columns differ in length
    with pytest.raises(ValueError):
        ctx.recommend_foldin(L.SIDE_USER, [], [], [], how, 5)                     # no offsets at all
    model = mfhip.als.MatrixFactorizationModel.__new__(mfhip.als.MatrixFactorizationModel)
    model._ctx = ctx
    with pytest.raises(ValueError):
        model.recommendProductsForSessions([([1, 2], [1.0])], 5)
