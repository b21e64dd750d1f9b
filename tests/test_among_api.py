"""mf_recommend_among: the surface that needs no GPU -- the export, the header, the bindings, and the argument
checks, every one of which is raised before the context is read."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from mfhip import _lib as L

HEADER = os.path.join(ROOT, "include", "mfhip.h")
FAKE = C.c_void_p(8)  # an opaque non-null handle, never dereferenced: each call below fails an argument check first


def test_symbol_is_exported_declared_and_wrapped():
    lib = L.lib()
    assert "mf_recommend_among" in L.EXPORTS and hasattr(lib, "mf_recommend_among")
    assert re.search(r"^int\s+mf_recommend_among\s*\(", open(HEADER).read(), flags=re.M)
    import mfhip
    assert hasattr(mfhip.Context, "recommend_among")
    for cls in (mfhip.DSGDforMF, mfhip.als.MatrixFactorizationModel):
        assert hasattr(cls, "recommendProductsAmong")
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    assert re.search(r"public static native void recommendAmong\(", java)
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    assert "JFN(recommendAmong)" in shim and "mf_recommend_among(" in shim


def among(ctx=FAKE, side=L.SIDE_USER, n=2, top_n=5, offsets=(0, 2, 3), n_cand=3, seen=0, ne=0, queries=True,
          cand=True, ids=True, counts=True, excl=True):
    """One call with small valid arrays; every keyword breaks one argument."""
    a = (C.c_int32 * 16)()
    d = (C.c_double * 16)()
    off = None if offsets is None else (C.c_int64 * len(offsets))(*offsets)
    return L.lib().mf_recommend_among(ctx, side, a if queries else None, n, top_n, off, a if cand else None, n_cand,
                                      seen, a if excl else None, a if excl else None, ne, a if ids else None, d,
                                      a if counts else None)


def test_null_context_is_invalid_with_a_message():
    assert among(ctx=None) == L.MF_ERR_INVALID
    assert "context" in L.lib().mf_last_error().decode()


CASES = [
    (dict(side=2), "side"), (dict(side=-1), "side"),
    (dict(top_n=0), "top_n"), (dict(top_n=L.RECOMMEND_MAX_TOP + 1), "top_n"),
    (dict(n=-1), "count"), (dict(n_cand=-1), "count"), (dict(ne=-1), "count"),
    (dict(n=2 ** 31, offsets=None), "n_queries"), (dict(n_cand=2 ** 31, offsets=None), "n_cand"),
    (dict(queries=False), "queries"), (dict(ids=False), "ids_out"), (dict(counts=False), "counts_out"),
    (dict(cand=False), "cand_ids"), (dict(cand=False, offsets=None), "cand_ids"),
    (dict(ne=1, excl=False), "exclusion"),
    (dict(offsets=(1, 2, 3)), "offsets[0]"), (dict(offsets=(0, 2, 1), n_cand=1), "offsets"),
    (dict(offsets=(0, 2, 2)), "n_cand"), (dict(offsets=(0, 2, 4)), "n_cand"),
    (dict(seen=2), "exclude_seen"), (dict(seen=-1), "exclude_seen"),
    (dict(seen=1, ne=1), "n_excl"),
]


@pytest.mark.parametrize("kw,word", CASES)
def test_argument_checks_come_before_the_context_is_read(kw, word):
    """Each MF_ERR_INVALID case of the header, with a message that names the argument; the opaque handle shows
    that nothing of the context was read."""
    assert among(**kw) == L.MF_ERR_INVALID
    assert word in L.lib().mf_last_error().decode()
