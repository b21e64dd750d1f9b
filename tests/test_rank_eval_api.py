"""mf_rank_eval's surface that needs no GPU: argument checks, the header / binding constants and struct,
and the host statement of the metrics (mfhip/ranking.py host_metrics) on MLlib's RankingMetricsSuite
example."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mfhip import _lib as L
from mfhip.ranking import host_metrics

HEADER = os.path.join(ROOT, "include", "mfhip.h")


def test_null_context_is_invalid_with_a_message():
    lib = L.lib()
    q = (C.c_int32 * 1)(1)
    out = L.mf_rank_metrics()
    st = lib.mf_rank_eval(None, L.SIDE_USER, q, q, 1, 4, None, None, 0, C.byref(out), None, None, None, 0)
    assert st == L.MF_ERR_INVALID
    assert lib.mf_last_error().decode()
    nq, ne = C.c_int64(0), C.c_int64(0)
    off = (C.c_int64 * 2)()
    st = lib.mf_debug_rank_csr(None, L.SIDE_USER, 1, q, q, 1, q, off, q, 1, 1, C.byref(nq), C.byref(ne))
    assert st == L.MF_ERR_INVALID


def test_nmetrics_matches_the_header():
    m = re.search(r"^#define\s+MF_RANK_NMETRICS\s+(\d+)", open(HEADER).read(), flags=re.M)
    assert m and int(m.group(1)) == L.RANK_NMETRICS == 6


def test_struct_sizes_agree():
    """sizeof(mf_rank_metrics) as the C compiler lays it out equals the ctypes structure's, and so do
    the offsets of the first and last named fields."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    T = L.mf_rank_metrics
    src = (f'#include <stddef.h>\n#include "mfhip.h"\n'
           f"_Static_assert(sizeof(mf_rank_metrics) == {C.sizeof(T)}, \"size\");\n"
           f"_Static_assert(offsetof(mf_rank_metrics, hits) == {T.hits.offset}, \"hits\");\n"
           f"_Static_assert(offsetof(mf_rank_metrics, precision) == {T.precision.offset}, \"precision\");\n"
           f"_Static_assert(offsetof(mf_rank_metrics, hit_rate) == {T.hit_rate.offset}, \"hit_rate\");\n"
           f"_Static_assert(offsetof(mf_rank_metrics, reserved) == {T.reserved.offset}, \"reserved\");\n")
    r = subprocess.run([gcc, "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(T) == 4 * 8 + 6 * 8 + 6 * 8


# MLlib RankingMetricsSuite: two labelled queries and a third without labels (which adds 0 to every sum)
LISTS = [[1, 6, 2, 7, 8, 3, 9, 10, 4, 5], [4, 1, 5, 6, 2, 7, 3, 8, 9, 10]]
TRUTH = [{1, 2, 3, 4, 5}, {1, 2, 3}]


def mllib(top_n):
    ids = np.array(LISTS, np.int32)
    counts, values = host_metrics(ids, np.array([10, 10], np.int32), TRUTH, top_n)
    return counts, values, values.sum(axis=0) / 3.0


def test_host_metrics_on_the_mllib_example():
    want_p = {1: 1 / 3, 2: 1 / 3, 3: 1 / 3, 4: 0.25, 5: 0.8 / 3, 10: 0.8 / 3, 15: 8 / 45}
    for n, p in want_p.items():
        assert abs(mllib(n)[2][0] - p) < 1e-12, n
    assert abs(mllib(10)[2][2] - 0.355026) < 1e-6  # MAP
    for n, v in {3: 1 / 3, 5: 0.328788, 10: 0.487913, 15: 0.487913}.items():
        assert abs(mllib(n)[2][3] - v) < 1e-6, n
    counts, values, _ = mllib(10)
    assert counts.tolist() == [[5, 5], [3, 3]]
    assert abs(values[0, 2] - 28 / 45) < 1e-15 and abs(values[1, 2] - 0.44285714285714284) < 1e-15  # ap
    assert values[:, 4].tolist() == [1.0, 0.5]  # rr
    assert values[:, 1].tolist() == [1.0, 1.0]  # recall
    assert values[:, 5].tolist() == [1.0, 1.0]  # hit


def test_host_metrics_reads_only_the_valid_part_of_a_row():
    """Slots past the count hold id 0, which may be a real id in the ground truth."""
    ids = np.array([[7, 0, 0, 0]], np.int32)
    counts, values = host_metrics(ids, [1], [{0, 7}], 4)
    assert counts.tolist() == [[1, 2]]
    g0, g1 = 1.0 / math.log(2), 1.0 / math.log(3)
    assert values[0].tolist() == [0.25, 0.5, 0.5, g0 / (g0 + g1), 1.0, 1.0]
    with pytest.raises(ValueError):
        host_metrics(ids, [1], [set()], 4)
    with pytest.raises(ValueError):
        host_metrics(ids, [1], [{1}], 129)
