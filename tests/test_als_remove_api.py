"""Rating removal, the parts that need no GPU: the exports and their bindings, the header's contract, the
NULL-context errors, StreamingALS.forget's argument checks, and mf_debug_als_remove_select -- the selection
rule in plain C++ -- against the numpy statement of the same rule."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import mfhip
from mfhip import _lib as L
from mfhip.context import Context

ROOT = pathlib.Path(__file__).resolve().parents[1]
API = ["mf_als_remove", "mf_als_remove_rows", "mf_als_retract", "mf_seen_remove"]
HOOK = "mf_debug_als_remove_select"


def test_exports_headers_and_bindings():
    lib = L.lib()
    header = (ROOT / "include" / "mfhip.h").read_text()
    testing = (ROOT / "include" / "mfhip_testing.h").read_text()
    for name in API:
        assert hasattr(lib, name) and name in L.EXPORTS
        assert re.search(rf"\bint {name}\(", header), name
    assert hasattr(lib, HOOK) and HOOK in L.TESTING_EXPORTS
    assert re.search(rf"\bint {HOOK}\(", testing)
    for name in ("als_remove", "als_remove_rows", "als_retract", "seen_remove"):
        assert callable(getattr(Context, name))
    assert callable(mfhip.StreamingALS.forget)
    java = (ROOT / "jni" / "MfHip.java").read_text()
    shim = (ROOT / "jni" / "mfhip_jni.c").read_text()
    for native, c_name in zip(("alsRemove", "alsRemoveRows", "alsRetract", "seenRemove"), API):
        assert re.search(rf"native \w[\w\[\]]* {native}\(", java), native
        assert f"JFN({native})(" in shim and f"{c_name}(CTX(h)" in shim, native


def test_the_header_states_the_contract():
    header = (ROOT / "include" / "mfhip.h").read_text()
    text = " ".join(header.split())
    assert "OLDEST remaining rating" in text or "oldest remaining rating" in text
    assert "The factor row stays" in text
    assert "mf_seen_from_als again" in text


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    u = np.zeros(1, np.int32)
    p = L.ptr(u, C.c_int32)
    how = mfhip.context.als_solve(0.05)
    calls = [lambda: lib.mf_als_remove(None, p, p, 1, None, None),
             lambda: lib.mf_als_remove_rows(None, L.SIDE_USER, p, 1, None),
             lambda: lib.mf_als_retract(None, p, p, 1, C.byref(how), 1, None, None, None, None),
             lambda: lib.mf_seen_remove(None, p, p, 1, None, None)]
    for call in calls:
        assert call() == L.MF_ERR_INVALID
        assert lib.mf_last_error()


def test_forget_checks_its_arguments():
    s = mfhip.StreamingALS(rank=4)
    with pytest.raises(RuntimeError):
        s.forget([(1, 2)])
    with pytest.raises(ValueError):
        s.forget([(1, 2)], rounds=-1)


# ---------------------------------------------------------------------------------------------
# the selection rule

def numpy_select(off, cols, brow, bcol):
    """The rule: in ascending j, entry j takes the oldest remaining instance of its pair."""
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    alive = np.ones(len(cols), bool)
    pos = np.full(len(brow), -1, np.int64)
    for j in range(len(brow)):
        c = np.flatnonzero((rows == brow[j]) & (cols == bcol[j]) & alive)
        if len(c):
            pos[j] = c[0]
            alive[c[0]] = False
    return pos


def raw_select(off, rows, cols, brow, bcol, n, pos):
    def p(a, t):
        return None if a is None else L.ptr(a, t)
    return L.lib().mf_debug_als_remove_select(p(off, C.c_int64), rows, p(cols, C.c_int32), p(brow, C.c_int32),
                                              p(bcol, C.c_int32), n, p(pos, C.c_int64))


def random_case(rng, rows):
    """About half the rows empty; pairs with 1 .. 4 instances, interleaved inside their row."""
    r_list, c_list = [], []
    for x in range(rows):
        if rng.random() < 0.5:
            continue
        for col in rng.choice(12, rng.integers(1, 6), replace=False):
            m = int(rng.integers(1, 5))
            r_list += [x] * m
            c_list += [int(col)] * m
    r_arr, c_arr = np.array(r_list, np.int64), np.array(c_list, np.int32)
    p = rng.permutation(len(r_arr))
    r_arr, c_arr = r_arr[p], c_arr[p]
    order = np.argsort(r_arr, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(r_arr, minlength=rows))]).astype(np.int64)
    return off, np.ascontiguousarray(c_arr[order])


@pytest.mark.parametrize("rows", [0, 1, 7, 300])
def test_select_matches_the_numpy_rule(rows):
    rng = np.random.default_rng(100 + rows)
    for trial in range(4):
        off, cols = random_case(rng, rows)
        if rows == 0:
            brow, bcol = np.zeros(0, np.int32), np.zeros(0, np.int32)
        else:
            # stored pairs named up to twice as often as they exist, never-rated pairs, rows without entries
            stored_rows = np.repeat(np.arange(rows), np.diff(off))
            take = rng.integers(0, max(len(cols), 1), 2 * len(cols)) if len(cols) else np.zeros(0, np.int64)
            brow = np.concatenate([stored_rows[take], rng.integers(0, rows, 20)]).astype(np.int32)
            bcol = np.concatenate([cols[take], rng.integers(0, 14, 20)]).astype(np.int32)
            p = rng.permutation(len(brow))
            brow, bcol = np.ascontiguousarray(brow[p]), np.ascontiguousarray(bcol[p])
        want = numpy_select(off, cols, brow, bcol)
        pos = np.full(max(len(brow), 1), -7, np.int64)
        cols_arg = cols if len(cols) else None
        assert raw_select(off, rows, cols_arg, brow if len(brow) else None, bcol if len(brow) else None, len(brow),
                          pos) == L.MF_OK
        assert np.array_equal(pos[:len(brow)], want), (rows, trial)
        if len(brow):
            hit = want >= 0
            assert len(np.unique(want[hit])) == hit.sum()                 # no entry is taken twice
            if rows > 1:
                assert hit.any() and (~hit).any()
        # n == 0
        assert raw_select(off, rows, cols_arg, None, None, 0, None) == L.MF_OK


def test_select_rejects_bad_input():
    off = np.array([0, 2, 2, 3], np.int64)
    cols = np.array([5, 5, 1], np.int32)
    brow, bcol = np.array([0, 2], np.int32), np.array([5, 1], np.int32)
    pos = np.zeros(2, np.int64)
    assert raw_select(off, 3, cols, brow, bcol, 2, pos) == L.MF_OK and pos.tolist() == [0, 2]
    assert raw_select(np.array([0, 2, 1, 3], np.int64), 3, cols, brow, bcol, 2, pos) == L.MF_ERR_INVALID   # descending
    assert raw_select(np.array([1, 2, 2, 3], np.int64), 3, cols, brow, bcol, 2, pos) == L.MF_ERR_INVALID
    assert raw_select(off, 3, cols, np.array([0, 3], np.int32), bcol, 2, pos) == L.MF_ERR_INVALID           # row >= rows
    assert raw_select(off, 3, cols, np.array([0, -1], np.int32), bcol, 2, pos) == L.MF_ERR_INVALID
    assert raw_select(off, 3, cols, brow, bcol, -1, pos) == L.MF_ERR_INVALID
    assert raw_select(off, -1, cols, brow, bcol, 2, pos) == L.MF_ERR_INVALID
    assert raw_select(None, 3, cols, brow, bcol, 2, pos) == L.MF_ERR_INVALID
    assert raw_select(off, 3, None, brow, bcol, 2, pos) == L.MF_ERR_INVALID
    assert raw_select(off, 3, cols, brow, bcol, 2, None) == L.MF_ERR_INVALID
    assert L.lib().mf_last_error()
