"""mf_pair_ranks / mf_online_prequential: the surface that needs no GPU -- exports, argument checks, the
header / binding constants and struct, and the host statement of the metrics and of the sum order
(mfhip/prequential.py host_prequential) on hand-worked cases."""
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
from mfhip.prequential import host_prequential, slice_tree_sum
from mfhip.ranking import GAIN, IDCG

HEADER = os.path.join(ROOT, "include", "mfhip.h")


def test_symbols_are_exported_and_declared():
    lib = L.lib()
    text = open(HEADER).read()
    for name in ("mf_pair_ranks", "mf_online_prequential"):
        assert name in L.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    import mfhip
    for name in ("Prequential", "PrequentialEvaluator", "host_prequential"):
        assert hasattr(mfhip, name) and name in mfhip.__all__
    assert hasattr(mfhip.Context, "pair_ranks") and hasattr(mfhip.Context, "online_prequential")


def test_codes_match_the_header():
    text = open(HEADER).read()
    for name, val in (("MF_PAIR_RANK_COLD", L.PAIR_RANK_COLD), ("MF_PAIR_RANK_EXCLUDED", L.PAIR_RANK_EXCLUDED)):
        m = re.search(r"^#define\s+" + name + r"\s+\((-?\d+)\)", text, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert (L.PAIR_RANK_COLD, L.PAIR_RANK_EXCLUDED) == (-1, -2)


def _pair_ranks(ctx, side, n, ne):
    q = (C.c_int32 * 1)(1)
    d = (C.c_double * 1)()
    return L.lib().mf_pair_ranks(ctx, side, q, q, n, q, q, ne, q, q, d)


def _prequential(ctx, n, top_n, ne, out=True):
    q = (C.c_int32 * 1)(1)
    d = (C.c_double * 1)(1.0)
    o = L.mf_prequential()
    return L.lib().mf_online_prequential(ctx, q, q, d, n, L.ONLINE_NEXT_FACTORS, 0, top_n, q, q, ne,
                                         C.byref(o) if out else None, None, None, None)


def test_null_context_is_invalid_with_a_message():
    for st in (_pair_ranks(None, L.SIDE_USER, 1, 0), _prequential(None, 1, 10, 0)):
        assert st == L.MF_ERR_INVALID
        assert L.lib().mf_last_error().decode()


def test_argument_checks_come_before_the_context_is_used():
    """A bad side, a bad top_n, negative counts and a NULL out are refused with MF_ERR_INVALID and a message;
    the checks read nothing of the context, so an opaque non-null handle shows their order."""
    lib = L.lib()
    fake = C.c_void_p(8)  # never dereferenced: each call below fails an argument check first
    cases = [
        _pair_ranks(fake, 2, 1, 0), _pair_ranks(fake, -1, 1, 0), _pair_ranks(fake, L.SIDE_USER, -1, 0),
        _pair_ranks(fake, L.SIDE_USER, 1, -1),
        _prequential(fake, 1, 0, 0), _prequential(fake, 1, L.RECOMMEND_MAX_TOP + 1, 0), _prequential(fake, -1, 10, 0),
        _prequential(fake, 1, 10, -1), _prequential(fake, 1, 10, 0, out=False),
    ]
    for n, st in enumerate(cases):
        assert st == L.MF_ERR_INVALID, n
        assert lib.mf_last_error().decode()
    q = (C.c_int32 * 1)(1)
    assert lib.mf_pair_ranks(fake, L.SIDE_USER, None, q, 1, None, None, 0, q, None, None) == L.MF_ERR_INVALID
    assert lib.mf_pair_ranks(fake, L.SIDE_USER, q, q, 1, None, None, 0, None, None, None) == L.MF_ERR_INVALID
    assert lib.mf_pair_ranks(fake, L.SIDE_USER, q, q, 1, None, q, 1, q, None, None) == L.MF_ERR_INVALID
    o = L.mf_prequential()
    assert lib.mf_online_prequential(fake, q, q, None, 1, 0, 0, 10, None, None, 0, C.byref(o), None, None,
                                     None) == L.MF_ERR_INVALID
    assert lib.mf_online_prequential(fake, q, q, (C.c_double * 1)(), 1, 0, 0, 10, q, None, 1, C.byref(o), None, None,
                                     None) == L.MF_ERR_INVALID


def test_struct_sizes_agree():
    """sizeof(mf_prequential) and every named field's offset as the C compiler lays them out equal the
    ctypes structure's."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    T = L.mf_prequential
    src = f'#include <stddef.h>\n#include "mfhip.h"\n_Static_assert(sizeof(mf_prequential) == {C.sizeof(T)}, "size");\n'
    for name, _ in T._fields_:
        src += f'_Static_assert(offsetof(mf_prequential, {name}) == {getattr(T, name).offset}, "{name}");\n'
    r = subprocess.run([gcc, "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(T) == 5 * 8 + 3 * 8 + 4 * 8 + 6 * 8


def test_host_prequential_hand_worked():
    N = 10
    # r = 0; r = N - 1 (a hit); r = N (not a hit); V = 1; cold; excluded
    ranks = [0, N - 1, N, 0, L.PAIR_RANK_COLD, L.PAIR_RANK_EXCLUDED]
    valid = [7, 21, 21, 1, 0, 0]
    vals, sums = host_prequential(ranks, valid, N)
    assert vals[0].tolist() == [1.0, 1.0, 1.0, 0.0]
    assert vals[1].tolist() == [GAIN[N - 1] / IDCG[1], 1.0 / N, 1.0, (N - 1) / 20]
    assert abs(vals[1, 0] - 1.0 / math.log2(N + 1)) < 1e-15
    assert vals[2].tolist() == [0.0, 0.0, 0.0, N / 20]
    assert vals[3].tolist() == [1.0, 1.0, 1.0, 0.0]
    assert vals[4].tolist() == [0.0] * 4 and vals[5].tolist() == [0.0] * 4
    assert sums[1] == 1.0 + 1.0 / N + 1.0
    # cold and excluded events add nothing, wherever they stand
    _, sums2 = host_prequential(ranks[:4], valid[:4], N)
    assert sums2 == sums
    with pytest.raises(ValueError):
        host_prequential(ranks, valid, 0)
    with pytest.raises(ValueError):
        host_prequential(ranks, valid, 129)


def test_sum_order_is_slices_of_1024_with_a_pairwise_tree():
    """1025 events: the first 1024 make one slice, reduced by the tree t += t + d for d = 512 .. 1, and
    the last event is a slice of its own, added after it.  Stated a second time here as a recursion on
    the stride: slice[t] for t < d takes slice[t + d], i.e. the tree sums elements t, t + d, t + 2d, ...
    of the stride-d comb."""
    rng = np.random.default_rng(5)
    V = 5000
    ranks = rng.integers(0, V, 1025).astype(np.int32)
    ranks[::97] = L.PAIR_RANK_COLD
    valid = np.where(ranks >= 0, V, 0).astype(np.int32)
    vals, sums = host_prequential(ranks, valid, 128)

    def comb(v, t, d):  # the value thread t holds once strides >= d are folded: v is 1024 long
        if d == 1024:
            return v[t]
        return comb(v, t, 2 * d) + comb(v, t + d, 2 * d)

    for col, got in ((0, sums[0]), (1, sums[1]), (3, sums[2])):
        v = vals[:, col].tolist()
        want = (0.0 + comb(v[:1024], 0, 1)) + (v[1024] + 0.0)
        assert got == want
        assert got == slice_tree_sum(v)
        assert abs(got - math.fsum(v)) <= 1025 * 2.0 ** -53 * math.fsum(v)
    # the order matters: a plain left-to-right sum differs in the last bits for at least one column
    assert any(float(np.cumsum(vals[:, c])[-1]) != s for c, s in ((0, sums[0]), (1, sums[1]), (3, sums[2])))
