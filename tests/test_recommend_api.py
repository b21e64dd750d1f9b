"""mf_recommend's surface that needs no GPU: argument checks and the header / binding constants."""
import ctypes as C
import os
import re

from conftest import ROOT
from mfhip import _lib as L


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    q = (C.c_int32 * 1)(1)
    ids = (C.c_int32 * 4)()
    cnt = (C.c_int32 * 1)()
    st = lib.mf_recommend(None, L.SIDE_USER, q, 1, 4, None, None, 0, ids, None, cnt)
    assert st == L.MF_ERR_INVALID
    assert lib.mf_last_error().decode()


def test_max_top_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "mfhip.h")).read()
    m = re.search(r"^#define\s+MF_RECOMMEND_MAX_TOP\s+(\d+)", txt, flags=re.M)
    assert m and int(m.group(1)) == L.RECOMMEND_MAX_TOP
