"""The resident seen set (mf_seen_* and the four *_seen readers): the surface that needs no GPU -- exports,
argument checks, and the host statement of the merge rule (mf_debug_seen_merge_placement), which the merge
kernels of csrc/kernels_seen.hip follow, against numpy's union."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mfhip import _lib as L

HEADER = os.path.join(ROOT, "include", "mfhip.h")
TESTING = os.path.join(ROOT, "include", "mfhip_testing.h")
PUBLIC = ("mf_seen_set", "mf_seen_add", "mf_seen_from_als", "mf_seen_clear", "mf_seen_count", "mf_recommend_seen",
          "mf_rank_eval_seen", "mf_pair_ranks_seen", "mf_online_prequential_seen")
HOOKS = ("mf_debug_seen_csr", "mf_debug_seen_merge_placement")


def test_symbols_are_exported_and_declared():
    lib = L.lib()
    for names, listed, path in ((PUBLIC, L.EXPORTS, HEADER), (HOOKS, L.TESTING_EXPORTS, TESTING)):
        text = open(path).read()
        for name in names:
            assert name in listed
            assert hasattr(lib, name)
            assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    import mfhip
    assert mfhip.SEEN is L.SEEN and "SEEN" in mfhip.__all__
    for name in ("seen_set", "seen_add", "seen_from_als", "seen_clear", "seen_count", "debug_seen_csr"):
        assert hasattr(mfhip.Context, name)


# ---- the merge rule ------------------------------------------------------------------------------------
def placement(old, batch):
    old = np.ascontiguousarray(old, np.uint64)
    batch = np.ascontiguousarray(batch, np.uint64)
    old_pos = np.full(max(len(old), 1), -1, np.int64)
    nov_pos = np.full(max(len(batch), 1), -1, np.int64)
    m = C.c_int64(-1)
    u64p = C.POINTER(C.c_uint64)
    st = L.lib().mf_debug_seen_merge_placement(old.ctypes.data_as(u64p), len(old), batch.ctypes.data_as(u64p),
                                               len(batch), L.ptr(old_pos, C.c_int64), L.ptr(nov_pos, C.c_int64),
                                               C.byref(m))
    assert st == L.MF_OK, L.lib().mf_last_error().decode()
    return old_pos[:len(old)], nov_pos[:m.value]


def check_merge(old, batch):
    old = np.asarray(old, np.uint64)
    batch = np.asarray(batch, np.uint64)
    old_pos, nov_pos = placement(old, batch)
    novel = np.setdiff1d(batch, old)  # sorted, distinct
    union = np.union1d(old, batch)
    assert len(nov_pos) == len(novel)
    merged = np.zeros(len(union), np.uint64)
    filled = np.zeros(len(union), np.int32)
    for pos, keys in ((old_pos, old), (nov_pos, novel)):
        np.add.at(filled, pos, 1)
        merged[pos] = keys
    assert np.array_equal(filled, np.ones(len(union), np.int32))  # every slot written exactly once
    assert np.array_equal(merged, union)
    # the rule itself
    assert np.array_equal(old_pos, np.arange(len(old)) + np.searchsorted(novel, old, side="left"))
    assert np.array_equal(nov_pos, np.arange(len(novel)) + np.searchsorted(old, novel, side="left"))


def key(r, c):
    return (np.asarray(r, np.uint64) << np.uint64(32)) | np.asarray(c, np.uint64)


OLD = key([0, 0, 3, 3, 3, 7], [1, 5, 0, 2, 9, 4])


@pytest.mark.parametrize("name, old, batch", [
    ("empty old", [], key([2, 1, 2], [3, 1, 3])),
    ("empty batch", OLD, []),
    ("both empty", [], []),
    ("batch inside old", OLD, OLD[[4, 0, 2, 2]]),
    ("novel before", OLD, key([0, 0], [0, 0])),
    ("novel after", OLD, key([7, 9, 8], [5, 0, 2])),
    ("novel interleaved", OLD, key([0, 3, 3, 5, 7], [3, 1, 5, 5, 0])),
    ("duplicates", OLD, key([3, 3, 3, 0, 0, 3], [1, 1, 2, 1, 7, 1])),
    ("top bits", key([2**31 - 2], [2**31 - 1]), key([2**31 - 2, 2**31 - 2, 0], [2**31 - 2, 0, 2**31 - 1])),
])
def test_merge_placement_small(name, old, batch):
    check_merge(old, batch)


@pytest.mark.parametrize("novel", [1, 2047, 2048, 2049])
def test_merge_placement_tile_counts(novel):
    """5,000 old keys (more than two 2,048-entry tiles) with novel counts around a tile, plus keys the table holds."""
    rng = np.random.default_rng(novel)
    pool = key(rng.integers(0, 300, 40000), rng.integers(0, 4000, 40000))
    pool = rng.permutation(np.unique(pool))
    old = np.sort(pool[:5000])
    batch = np.concatenate([pool[5000:5000 + novel], old[rng.integers(0, 5000, 700)], pool[5000:5000 + min(novel, 50)]])
    assert len(np.setdiff1d(batch, old)) == novel
    check_merge(old, rng.permutation(batch))


def test_merge_placement_refuses_unsorted_old_keys():
    old = np.array([5, 5], np.uint64)
    pos = np.zeros(2, np.int64)
    m = C.c_int64(0)
    u64p = C.POINTER(C.c_uint64)
    st = L.lib().mf_debug_seen_merge_placement(old.ctypes.data_as(u64p), 2, old.ctypes.data_as(u64p), 0,
                                               L.ptr(pos, C.c_int64), L.ptr(pos, C.c_int64), C.byref(m))
    assert st == L.MF_ERR_INVALID


# ---- argument checks -----------------------------------------------------------------------------------
def _calls(ctx, n, top_n=10, side=L.SIDE_USER, arrays=True, out=True):
    """The seven calls that take arguments, with count n, as thunks (a caller runs only those whose arguments
    fail a check); arrays=False passes NULL arrays."""
    lib = L.lib()
    q = (C.c_int32 * 1)(1) if arrays else None
    d = (C.c_double * 1)(1.0) if arrays else None
    buf = (C.c_int32 * 128)()
    cnt = C.c_int64(0)
    m = L.mf_rank_metrics()
    p = L.mf_prequential()
    return {
        "mf_seen_set": lambda: lib.mf_seen_set(ctx, q, q, n, None),
        "mf_seen_add": lambda: lib.mf_seen_add(ctx, q, q, n, None),
        "mf_recommend_seen": lambda: lib.mf_recommend_seen(ctx, side, q, n, top_n, buf, None, buf),
        "mf_rank_eval_seen": lambda: lib.mf_rank_eval_seen(ctx, side, q, q, n, top_n, C.byref(m) if out else None,
                                                           None, None, None, 0),
        "mf_pair_ranks_seen": lambda: lib.mf_pair_ranks_seen(ctx, side, q, q, n, buf, None, None),
        "mf_online_prequential_seen": lambda: lib.mf_online_prequential_seen(
            ctx, q, q, d, n, L.ONLINE_NEXT_FACTORS, top_n, C.byref(p) if out else None, None, None, None, 0, 0.0, 0, 0,
            None, 0),
        "mf_seen_count": lambda: lib.mf_seen_count(ctx, C.byref(cnt) if out else None),
    }


def test_null_context_is_invalid_with_a_message():
    for name, call in _calls(None, 1).items():
        assert call() == L.MF_ERR_INVALID, name
        assert L.lib().mf_last_error().decode()
    for fn in (L.lib().mf_seen_from_als, L.lib().mf_seen_clear):
        assert fn(None) == L.MF_ERR_INVALID


def test_argument_checks_come_before_the_context_is_used():
    """Negative counts, NULL arrays with a positive count, a bad side, a bad top_n and a NULL out are refused
    with MF_ERR_INVALID; the checks read nothing of the context, so an opaque non-null handle shows their order."""
    fake = C.c_void_p(8)  # never dereferenced: each call below fails an argument check first
    takes_count = ("mf_seen_set", "mf_seen_add", "mf_recommend_seen", "mf_rank_eval_seen", "mf_pair_ranks_seen",
                   "mf_online_prequential_seen")
    res = _calls(fake, -1)
    for name in takes_count:
        assert res[name]() == L.MF_ERR_INVALID, name
    res = _calls(fake, 1, arrays=False)
    for name in takes_count:
        assert res[name]() == L.MF_ERR_INVALID, name
    for side in (-1, 2):
        res = _calls(fake, 1, side=side)
        for name in ("mf_recommend_seen", "mf_rank_eval_seen", "mf_pair_ranks_seen"):
            assert res[name]() == L.MF_ERR_INVALID, name
    for top_n in (0, L.RECOMMEND_MAX_TOP + 1):
        res = _calls(fake, 1, top_n=top_n)
        for name in ("mf_recommend_seen", "mf_rank_eval_seen", "mf_online_prequential_seen"):
            assert res[name]() == L.MF_ERR_INVALID, name
    res = _calls(fake, 1, out=False)
    for name in ("mf_rank_eval_seen", "mf_online_prequential_seen", "mf_seen_count"):
        assert res[name]() == L.MF_ERR_INVALID, name
    # 2^31 - 1 pairs or more in one call
    q = (C.c_int32 * 1)(1)
    for fn in (L.lib().mf_seen_set, L.lib().mf_seen_add):
        assert fn(fake, q, q, 2**31, None) == L.MF_ERR_INVALID
        assert fn(fake, q, q, 2**31 - 1, None) == L.MF_ERR_INVALID
    # the sampled call's refusals carry over
    d = (C.c_double * 1)(1.0)
    p = L.mf_prequential()
    pre = L.lib().mf_online_prequential_seen
    assert pre(fake, q, q, d, 1, L.ONLINE_NEXT_FACTORS, 10, C.byref(p), None, None, None, L.NEG_MAX + 1, 0.0, 0, 0,
               None, 0) == L.MF_ERR_INVALID
    assert pre(fake, q, q, d, 1, L.ONLINE_NEXT_FACTORS, 10, C.byref(p), None, None, None, 1, 0.0, 0, -1, None,
               0) == L.MF_ERR_INVALID
