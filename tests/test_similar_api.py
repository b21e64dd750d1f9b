"""mf_similar / mf_recommend_vectors: the surface that needs no GPU -- exports, the header's metric constants
against the binding's, and the argument checks, which read nothing of the context."""
import ctypes as C
import os
import re

from conftest import ROOT
from mfhip import _lib as L

HEADER = os.path.join(ROOT, "include", "mfhip.h")


def test_symbols_are_exported_declared_and_wrapped():
    lib = L.lib()
    text = open(HEADER).read()
    for name in ("mf_similar", "mf_recommend_vectors"):
        assert name in L.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    import mfhip
    assert hasattr(mfhip.Context, "similar") and hasattr(mfhip.Context, "recommend_vectors")
    for cls in (mfhip.DSGDforMF, mfhip.als.MatrixFactorizationModel):
        assert hasattr(cls, "similarProducts") and hasattr(cls, "similarUsers")


def test_metric_values_match_the_header():
    text = open(HEADER).read()
    for name, val in (("MF_METRIC_DOT", L.METRIC_DOT), ("MF_METRIC_COSINE", L.METRIC_COSINE)):
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)\s*$", text, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert (L.METRIC_DOT, L.METRIC_COSINE) == (0, 1)
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    assert re.search(r"METRIC_DOT = 0, METRIC_COSINE = 1;", java)


def _similar(ctx, side=L.SIDE_ITEM, n=1, top_n=5, metric=L.METRIC_COSINE, include_self=0, ne=0):
    q = (C.c_int32 * 8)()
    d = (C.c_double * 8)()
    return L.lib().mf_similar(ctx, side, q, n, top_n, metric, include_self, q, q, ne, q, d, q)


def _vectors(ctx, side=L.SIDE_ITEM, n=1, top_n=5, metric=L.METRIC_DOT, ne=0):
    q = (C.c_int32 * 8)()
    x = (C.c_int64 * 8)()
    d = (C.c_double * 8)()
    return L.lib().mf_recommend_vectors(ctx, side, d, n, top_n, metric, x, q, ne, q, d, q)


def test_null_context_is_invalid_with_a_message():
    for st in (_similar(None), _vectors(None)):
        assert st == L.MF_ERR_INVALID
        assert L.lib().mf_last_error().decode()


def test_argument_checks_come_before_the_context_is_used():
    """A bad side, an unknown metric, an include_self other than 0 or 1, top_n 0 and 129 and negative counts are
    refused with MF_ERR_INVALID and a message that names the argument; an opaque non-null handle shows that
    the checks read nothing of the context."""
    lib = L.lib()
    fake = C.c_void_p(8)  # never dereferenced: each call below fails an argument check first
    cases = [
        (_similar(fake, side=2), "side"), (_similar(fake, side=-1), "side"),
        (_similar(fake, metric=2), "metric"), (_similar(fake, metric=-1), "metric"),
        (_similar(fake, include_self=2), "include_self"), (_similar(fake, include_self=-1), "include_self"),
        (_similar(fake, top_n=0), "top_n"), (_similar(fake, top_n=L.RECOMMEND_MAX_TOP + 1), "top_n"),
        (_similar(fake, n=-1), "count"), (_similar(fake, ne=-1), "count"),
        (_vectors(fake, side=2), "side"), (_vectors(fake, metric=7), "metric"),
        (_vectors(fake, top_n=0), "top_n"), (_vectors(fake, top_n=L.RECOMMEND_MAX_TOP + 1), "top_n"),
        (_vectors(fake, n=-1), "count"), (_vectors(fake, ne=-1), "count"),
    ]
    # each status was taken in turn, so only the last message is left to read: check the statuses here ...
    for n, (st, _) in enumerate(cases):
        assert st == L.MF_ERR_INVALID, n
    # ... and every message right after its own call
    for call, word in ((lambda: _similar(fake, side=2), "side"), (lambda: _similar(fake, metric=2), "metric"),
                       (lambda: _similar(fake, include_self=2), "include_self"),
                       (lambda: _similar(fake, top_n=0), "top_n"), (lambda: _similar(fake, top_n=129), "top_n"),
                       (lambda: _vectors(fake, metric=2), "metric"), (lambda: _vectors(fake, top_n=129), "top_n")):
        assert call() == L.MF_ERR_INVALID
        assert word in lib.mf_last_error().decode()
