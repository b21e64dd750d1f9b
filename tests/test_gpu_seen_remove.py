"""mf_seen_remove: set difference on the resident seen set.

The yardstick is a twin context given mf_seen_set of the pairs that remain (both tables bit for bit, through
mf_debug_seen_csr) and the readers' namesakes given the remaining pairs as arrays.  The model is the small
integer-factor one of test_gpu_seen (exact scores, many ties); the set holds a few thousand pairs -- two of the
compaction kernel's 2048-entry tiles -- with a user of more than 700 seen items and a user of exactly one."""
import ctypes as C

import numpy as np
import pytest

from mfhip import SEEN
from mfhip import _lib as L
from mfhip.context import Context
from test_gpu_seen import ITEM, MODES, USER, int_model, make_ctx, same_tables, set_pairs

pytestmark = pytest.mark.gpu

NU, NI, K = 60, 900, 8
BIG, ONE, U_CLEARED, I_CLEARED = 3, 7, 11, 5          # indices into uid / iid


def problem(rng, ctx):
    """(uid, iid, set users, set items) as index arrays: about 3,400 distinct pairs."""
    uid, iid = int_model(rng, ctx, NU, NI, K)
    su = [np.full(760, BIG), np.full(1, ONE)]
    si = [rng.choice(NI, 760, replace=False), np.array([17])]
    for a in range(NU):
        if a in (BIG, ONE):
            continue
        c = int(rng.integers(20, 70))
        su.append(np.full(c, a))
        si.append(rng.choice(NI, c, replace=False))
    su.append(np.arange(10, 40))                                           # item I_CLEARED is seen by 30 users
    si.append(np.full(30, I_CLEARED))
    su, si = np.concatenate(su), np.concatenate(si)
    p = rng.permutation(len(su))
    return uid, iid, su[p], si[p]


def removal_batch(rng, uid, iid, su, si):
    """Held pairs (some twice), pairs not held, unknown ids, every pair of one user and of one item, as ids."""
    held = rng.choice(len(su), 600, replace=False)
    bu = [uid[su[held]], uid[su[held[:50]]], uid[su[su == U_CLEARED]], uid[su[si == I_CLEARED]],
          uid[rng.integers(0, NU, 200)], np.array([uid.max() + 9, uid[0], uid.min() - 4], np.int32)]
    bi = [iid[si[held]], iid[si[held[:50]]], iid[si[su == U_CLEARED]], iid[si[si == I_CLEARED]],
          iid[rng.integers(0, NI, 200)], np.array([iid[0], iid.max() + 6, iid.min() - 11], np.int32)]
    bu, bi = np.concatenate(bu).astype(np.int32), np.concatenate(bi).astype(np.int32)
    p = rng.permutation(len(bu))
    return np.ascontiguousarray(bu[p]), np.ascontiguousarray(bi[p])


def pair_set(u, i):
    return set(zip(np.asarray(u).tolist(), np.asarray(i).tolist()))


@pytest.mark.parametrize("mode", MODES)
def test_remove_is_the_set_difference(mode):
    rng = np.random.default_rng(31)
    with make_ctx(K, mode) as ctx, make_ctx(K, mode) as twin:
        uid, iid, su, si = problem(rng, ctx)
        twin.set_factors(USER, uid, ctx.lookup(USER, uid)[0])              # the same rows in the same order
        twin.set_factors(ITEM, iid, ctx.lookup(ITEM, iid)[0])
        assert ctx.seen_set(uid[su], iid[si]) == 0
        n0 = ctx.seen_count()
        assert n0 > 2048 and n0 == len(pair_set(su, si))
        rid, off, _, _ = ctx.debug_seen_csr(ITEM)                          # the item-major table exists before the removal
        assert off[-1] == n0
        assert ctx.recommend(iid[:4], 5, side=ITEM, exclude=SEEN)[0].shape == (4, 5)
        bu, bi = removal_batch(rng, uid, iid, su, si)
        held = pair_set(uid[su], iid[si])
        batch = pair_set(bu, bi)
        known_u, known_i = set(uid.tolist()), set(iid.tolist())
        want_ignored = sum(1 for a, b in zip(bu.tolist(), bi.tolist()) if a not in known_u or b not in known_i)
        want_removed = len(held & batch)
        assert want_ignored == 3 and want_removed > 600 and len(batch - held) > 100
        assert ctx.seen_remove(bu, bi) == (want_removed, want_ignored)
        left = sorted(held - batch)
        lu, li = np.array([a for a, _ in left], np.int32), np.array([b for _, b in left], np.int32)
        assert ctx.seen_count() == len(left) == n0 - want_removed
        assert twin.seen_set(lu, li) == 0
        same_tables(ctx, twin)
        assert pair_set(*set_pairs(ctx)) == set(left)
        assert not (lu == uid[U_CLEARED]).any() and not (li == iid[I_CLEARED]).any()
        # the readers, both query sides: the remaining pairs as arrays
        for side, queries in ((USER, uid[[BIG, ONE, U_CLEARED, 20, 21]]), (ITEM, iid[[I_CLEARED, 17, 100, 101]])):
            excl = (lu, li) if side == USER else (li, lu)
            got = ctx.recommend(queries, 12, side=side, exclude=SEEN)
            want = ctx.recommend(queries, 12, side=side, exclude=excl)
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and np.array_equal(x, y), side
        eq, ec = np.ascontiguousarray(bu[:300]), np.ascontiguousarray(bi[:300])
        for side in (USER, ITEM):
            q, c = (eq, ec) if side == USER else (ec, eq)
            excl = (lu, li) if side == USER else (li, lu)
            got = ctx.pair_ranks(q, c, side=side, exclude=SEEN, scores=True)
            want = ctx.pair_ranks(q, c, side=side, exclude=excl, scores=True)
            for x, y in zip(got, want):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), side
        # the same batch again: nothing is held any more
        assert ctx.seen_remove(bu, bi) == (0, want_ignored)
        same_tables(ctx, twin)
        # everything goes
        assert ctx.seen_remove(lu, li) == (len(left), 0)
        assert ctx.seen_count() == 0
        for side in (USER, ITEM):
            q = uid[:6] if side == USER else iid[:6]
            for x, y in zip(ctx.recommend(q, 10, side=side, exclude=SEEN), ctx.recommend(q, 10, side=side)):
                assert np.array_equal(x, y)
        for x, y in zip(ctx.pair_ranks(eq, ec, exclude=SEEN), ctx.pair_ranks(eq, ec)):
            assert np.array_equal(x, y)
        # and the set takes pairs again
        assert ctx.seen_add(lu[:40], li[:40]) == 0 and ctx.seen_count() == 40


def raw(ctx, u, i, n, removed=None, ignored=None):
    return L.lib().mf_seen_remove(ctx._h if isinstance(ctx, Context) else ctx,
                                  None if u is None else L.ptr(u, C.c_int32),
                                  None if i is None else L.ptr(i, C.c_int32), n,
                                  None if removed is None else C.byref(removed),
                                  None if ignored is None else C.byref(ignored))


@pytest.mark.parametrize("mode", MODES)
def test_no_set_and_errors(mode):
    rng = np.random.default_rng(32)
    with make_ctx(K, mode) as ctx:
        uid, iid = int_model(rng, ctx, 20, 30, K)
        bu = np.array([uid[0], uid.max() + 5, uid[1], uid[2]], np.int32)
        bi = np.array([iid[0], iid[1], iid.min() - 3, iid[2]], np.int32)
        removed, ignored = C.c_int64(-5), C.c_int64(-5)
        assert raw(ctx, bu, bi, 4, removed, ignored) == L.MF_OK             # no set: a no-op, both outputs written
        assert (removed.value, ignored.value) == (0, 2)
        assert ctx.seen_count() == 0
        assert ctx.debug_seen_csr(USER)[1][-1] == 0
        assert raw(ctx, None, None, 0, removed, ignored) == L.MF_OK and (removed.value, ignored.value) == (0, 0)
        ctx.seen_set(uid[:5], iid[:5])
        assert raw(ctx, bu, bi, -1) == L.MF_ERR_INVALID
        assert raw(ctx, None, bi, 4) == L.MF_ERR_INVALID
        assert raw(ctx, bu, None, 4) == L.MF_ERR_INVALID
        assert raw(ctx, bu, bi, 2**31 - 1) == L.MF_ERR_INVALID
        assert raw(None, bu, bi, 4) == L.MF_ERR_INVALID
        assert ctx.seen_count() == 5
        assert raw(ctx, bu, bi, 4, None, None) == L.MF_OK                  # NULL outputs
        assert ctx.seen_count() == 3                                       # (uid[0], iid[0]) and (uid[2], iid[2]) went
    p = L.default_params()
    p.num_factors = K
    p.mode = mode
    with Context(p, rank=(0, 1, 0, b"")) as ranked:                        # a rank-mode context (one rank)
        with pytest.raises(L.MFError) as err:
            ranked.seen_remove(bu, bi)
        assert err.value.code == L.MF_ERR_STATE
