"""Incremental ALS without a GPU: the exports and the struct of the binding, the argument checks that need
no device, StreamingALS's argument checks, the Java natives, and the placement rule of mf_als_append (where
every old and every new entry of a side lands) against numpy's stable argsort.  The GPU tests
(test_gpu_als_append.py) check the kernels against the same rule through the CSR they leave."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mfhip
from mfhip import _lib as L
from mfhip.context import als_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mf_als_append", "mf_als_run_rows", "mf_als_update")


def test_exports_and_header():
    lib = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mfhip.h")).read()
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
    for name in ("mf_debug_als_csr", "mf_debug_als_append_placement"):
        assert name in L.TESTING_EXPORTS and hasattr(lib, name)
    for name, value in (("MF_ALS_SOLVER_CHOLESKY", 0), ("MF_ALS_SOLVER_CG", 1), ("MF_ALS_SOLVER_NNLS", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", header), name
    assert (L.ALS_SOLVER_CHOLESKY, L.ALS_SOLVER_CG, L.ALS_SOLVER_NNLS) == (0, 1, 2)
    assert "users go first" in header.lower().replace("\n", " ")  # the contract names its departure from MLlib
    for name in ("StreamingALS",):
        assert hasattr(mfhip, name) and name in mfhip.__all__
    for name in ("als_append", "als_run_rows", "als_update", "als_csr"):
        assert hasattr(mfhip.Context, name)


def test_struct_layout_is_the_header_s():
    """typedef struct mf_als_solve { double; int32; int32; double; int32; int32; int32[4] }: 48 bytes."""
    S = L.mf_als_solve
    assert [n for n, _ in S._fields_] == ["lambda_", "reg", "implicit", "alpha", "solver", "cg_steps", "reserved"]
    offs = {n: getattr(S, n).offset for n, _ in S._fields_}
    assert offs == {"lambda_": 0, "reg": 8, "implicit": 12, "alpha": 16, "solver": 24, "cg_steps": 28, "reserved": 32}
    assert C.sizeof(S) == 48
    header = open(os.path.join(ROOT, "include", "mfhip.h")).read()
    body = re.search(r"typedef struct mf_als_solve \{(.*?)\} mf_als_solve;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+)(\[\d+\])?;", body)
    assert [(t, n.rstrip("_")) for t, n, _ in fields] == [
        ("double", "lambda"), ("int32_t", "reg"), ("int32_t", "implicit"), ("double", "alpha"),
        ("int32_t", "solver"), ("int32_t", "cg_steps"), ("int32_t", "reserved")]
    how = als_solve(0.1, L.ALS_REG_PLAIN, True, 0.5, "cg", 7)
    assert (how.lambda_, how.reg, how.implicit, how.alpha, how.solver, how.cg_steps) == (0.1, 1, 1, 0.5, 1, 7)
    assert list(how.reserved) == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        als_solve(0.1, solver="lu")


def test_null_context_and_null_arguments():
    lib = L.lib()
    how = als_solve(0.1)
    one = np.zeros(1, np.int32)
    r = np.zeros(1, np.float64)
    p32, pf = L.ptr(one, C.c_int32), L.ptr(r, C.c_double)
    assert lib.mf_als_append(None, p32, p32, pf, 1) == L.MF_ERR_INVALID
    assert b"null context" in lib.mf_last_error()
    assert lib.mf_als_run_rows(None, L.SIDE_USER, p32, 1, C.byref(how), None) == L.MF_ERR_INVALID
    assert lib.mf_als_update(None, p32, p32, pf, 1, C.byref(how), 1, None, None) == L.MF_ERR_INVALID
    n = C.c_int64(0)
    o64 = np.zeros(2, np.int64)
    assert lib.mf_debug_als_csr(None, 0, L.ptr(o64, C.c_int64), p32, pf, p32, 0, 0, C.byref(n),
                                C.byref(n)) == L.MF_ERR_INVALID


def test_streaming_als_argument_checks():
    S = mfhip.StreamingALS
    for bad in (dict(rank=0), dict(rank=257), dict(rank=8, lambda_=0.0), dict(rank=8, lambda_=float("nan")),
                dict(rank=8, solver="lu"), dict(rank=8, cg_steps=0), dict(rank=8, cg_steps=257),
                dict(rank=8, implicit=True, alpha=-1.0), dict(rank=8, implicit=True, alpha=float("inf")),
                dict(rank=8, mode="quick")):
        with pytest.raises(ValueError):
            S(**bad)
    s = S(rank=8, lambda_=0.05, implicit=True, alpha=2.0, solver="nnls", mode="fast", seed=3)
    assert (s.how.lambda_, s.how.implicit, s.how.alpha, s.how.solver) == (0.05, 1, 2.0, L.ALS_SOLVER_NNLS)
    assert s.how.reg == L.ALS_REG_WEIGHTED
    for call in (lambda: s.update(([1], [2], [3.0])), lambda: s.refit(2), lambda: s.model):
        with pytest.raises(RuntimeError):
            call()                                      # before fit(): no context yet
    with pytest.raises(ValueError):
        s.update(([1], [2], [3.0]), rounds=-1)
    with pytest.raises(ValueError):
        s.refit(-1)
    with pytest.raises(ValueError):
        s.fit(([1], [2], [3.0]), iterations=-1)
    s.close()


def test_java_natives_present():
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    for native, call in (("alsAppend", "mf_als_append"), ("alsRunRows", "mf_als_run_rows"),
                         ("alsUpdate", "mf_als_update")):
        assert re.search(r"public static native \w+ " + native + r"\(", java), native
        assert re.search(r"JFN\(" + native + r"\)\(", shim) and re.search(r"\b" + call + r"\b", shim), native


# ---------------------------------------------------------------------------------------------
# the placement rule

def placement(old_off, batch_row, new_rows):
    old_off = np.ascontiguousarray(old_off, np.int64)
    batch_row = np.ascontiguousarray(batch_row, np.int32)
    new_off = np.full(new_rows + 1, -1, np.int64)
    pos = np.full(max(len(batch_row), 1), -1, np.int64)
    L.check(L.lib().mf_debug_als_append_placement(L.ptr(old_off, C.c_int64), len(old_off) - 1,
                                                  L.ptr(batch_row, C.c_int32), len(batch_row), new_rows,
                                                  L.ptr(new_off, C.c_int64), L.ptr(pos, C.c_int64)))
    return new_off, pos[:len(batch_row)]


@pytest.mark.parametrize("old_rows,new_rows,n,seed", [(0, 0, 0, 0), (0, 5, 9, 1), (7, 7, 0, 2), (7, 7, 1, 3),
                                                       (7, 12, 40, 4), (300, 310, 5000, 5), (3, 3, 700, 6)])
def test_placement_is_numpy_s_stable_grouping(old_rows, new_rows, n, seed):
    """Tag every old entry with (row, its position) and every batch entry with (row, old nnz + j): a stable
    argsort of the rows of old ++ batch is the layout mf_als_prepare builds from the concatenated arrays.  The
    rule must send old entry p of row x to p + new_off[x] - old_off[x] and batch entry j to batch_pos[j]."""
    rng = np.random.default_rng(100 + seed)
    counts = rng.integers(0, 6, old_rows) * rng.integers(0, 2, old_rows)       # about half the rows are empty
    old_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    old_row = np.repeat(np.arange(old_rows), counts)
    batch_row = rng.integers(0, new_rows, n) if new_rows else np.zeros(0, np.int64)
    new_off, pos = placement(old_off, batch_row, new_rows)
    every = np.concatenate([old_row, batch_row]).astype(np.int64)
    order = np.argsort(every, kind="stable")                                   # order[d] = the entry that lands at d
    want_off = np.searchsorted(every[order], np.arange(new_rows + 1))
    assert np.array_equal(new_off, want_off)
    landing = np.empty(len(every), np.int64)
    landing[order] = np.arange(len(every))
    p = np.arange(len(old_row))
    assert np.array_equal(p + new_off[old_row] - old_off[old_row], landing[:len(old_row)])
    assert np.array_equal(pos, landing[len(old_row):])


def test_placement_rejects_bad_input():
    lib = L.lib()
    off = np.array([0, 2, 1], np.int64)
    row = np.array([0, 5], np.int32)
    out = np.zeros(8, np.int64)
    po, pr, pout = L.ptr(off, C.c_int64), L.ptr(row, C.c_int32), L.ptr(out, C.c_int64)
    assert lib.mf_debug_als_append_placement(po, 2, pr, 1, 2, pout, pout) == L.MF_ERR_INVALID      # descending
    ok = np.array([0, 1, 2], np.int64)
    pok = L.ptr(ok, C.c_int64)
    assert lib.mf_debug_als_append_placement(pok, 2, pr, 2, 3, pout, pout) == L.MF_ERR_INVALID     # row 5 >= 3
    assert lib.mf_debug_als_append_placement(pok, 2, pr, 1, 1, pout, pout) == L.MF_ERR_INVALID     # new < old rows
    assert lib.mf_debug_als_append_placement(pok, 2, pr, -1, 3, pout, pout) == L.MF_ERR_INVALID
    assert lib.mf_debug_als_append_placement(None, 2, pr, 1, 3, pout, pout) == L.MF_ERR_INVALID
