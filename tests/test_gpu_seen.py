"""The resident seen set on the device (csrc/seen.cpp, csrc/kernels_seen.hip): mf_seen_set / mf_seen_add /
mf_seen_from_als and the four readers that take it (exclude=SEEN).

The table is read back with mf_debug_seen_csr and compared with numpy's grouping of the distinct known pairs;
an add must leave, bit for bit, the table a set of the union builds; and every reader must return, bit for
bit, what its namesake returns when given the set's pairs as arrays -- on integer-valued models (factor
entries in {-2 .. 2}: small integer scores, plenty of ties) in both precisions.

Not verified here: the MF_ERR_STATE refusal on a rank-mode context (it needs the multi-process rehearsal of
tests/test_gpu_rank.py, a fixture this module does not have)."""
import dataclasses

import numpy as np
import pytest

from mfhip import SEEN
from mfhip import _lib as L
from mfhip.context import Context

pytestmark = pytest.mark.gpu

F64, F32 = L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32
MODES = [F64, F32]
USER, ITEM = L.SIDE_USER, L.SIDE_ITEM


def make_ctx(k, mode, **kw):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    for a, b in kw.items():
        setattr(p, a, b)
    return Context(p)


def shuffled_ids(rng, n, scale=3):
    """n distinct ids, about half of them negative, in random order (row order is call order)."""
    return (rng.permutation(n).astype(np.int32) - n // 2) * scale + 1


def int_model(rng, ctx, nu, ni, k):
    """Users and items with factor entries in {-2 .. 2}: exact small integer scores in f32 and f64, many ties."""
    uid, iid = shuffled_ids(rng, nu), shuffled_ids(rng, ni, 5)
    ctx.set_factors(USER, uid, rng.integers(-2, 3, (nu, k)).astype(np.float64))
    ctx.set_factors(ITEM, iid, rng.integers(-2, 3, (ni, k)).astype(np.float64))
    return uid, iid


def tables(ctx):
    """Both orientations as the readers see them: per side (row ids, offsets, counterpart rows, counterpart ids)."""
    return [ctx.debug_seen_csr(side) for side in (USER, ITEM)]


def same_tables(a, b):
    for ta, tb in zip(tables(a), tables(b)):
        for x, y in zip(ta, tb):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def check_table(ctx, u, i):
    """Both tables against numpy's grouping of the distinct pairs of (u, i) whose ids the model holds."""
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    known = [set(ctx.factors(side)[0].tolist()) for side in (USER, ITEM)]
    keep = np.array([a in known[0] and b in known[1] for a, b in zip(u.tolist(), i.tolist())], bool)
    pairs = np.unique(np.stack([u[keep], i[keep]], 1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    assert ctx.seen_count() == len(pairs)
    for side in (USER, ITEM):
        rid, off, ent, eid = ctx.debug_seen_csr(side)
        assert len(rid) == ctx.num_factors(side) and len(off) == len(rid) + 1
        assert off[0] == 0 and off[-1] == len(pairs) == len(ent) and np.all(np.diff(off) >= 0)
        mine, other = pairs[:, side], pairs[:, 1 - side]
        order = np.argsort(mine, kind="stable")
        grouped = dict(zip(*[x.tolist() for x in np.unique(mine, return_counts=True)]))
        for row, q in enumerate(rid.tolist()):
            b, e = int(off[row]), int(off[row + 1])
            assert e - b == grouped.get(q, 0), (side, q)
            assert np.all(np.diff(ent[b:e]) > 0), (side, q)  # distinct counterpart rows, ascending
            if e > b:
                assert sorted(eid[b:e].tolist()) == sorted(other[order][mine[order] == q].tolist()), (side, q)
    return int(keep.size - keep.sum())


def set_pairs(ctx):
    """The set as id arrays (users, items), from the user-major table."""
    rid, off, _, eid = ctx.debug_seen_csr(USER)
    return np.repeat(rid, np.diff(off)).astype(np.int32), eid.astype(np.int32)


# ---- the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_table_is_numpys_grouping_of_the_distinct_known_pairs(mode):
    rng = np.random.default_rng(17)
    nu, ni = 5100, 80
    with make_ctx(5, mode) as ctx:
        uid, iid = int_model(rng, ctx, nu, ni, 5)
        assert (uid < 0).any() and (iid < 0).any()
        u, i = [], []
        # rows of 1, 63, 64 and 65 entries, one that holds every item; user 0 and the last fifty: no entry
        for a, c in ((1, 1), (2, 63), (3, 64), (4, 65), (5, ni)):
            u += [uid[a]] * c
            i += rng.permutation(iid)[:c].tolist()
        hot = iid[7]                                            # an item seen by 5,000 users: three 2,048-entry tiles
        u += uid[50:5050].tolist()
        i += [hot] * 5000
        m = rng.integers(100, 3000, 4000)
        u += uid[m].tolist()                                    # scattered pairs
        i += iid[rng.integers(0, ni, 4000)].tolist()
        u += u[:300]                                            # duplicates
        i += i[:300]
        unknown = [(99_000_001, int(iid[0])), (int(uid[0]), 99_000_003), (99_000_001, 99_000_003)] * 2
        u += [a for a, _ in unknown]
        i += [b for _, b in unknown]
        p = rng.permutation(len(u))
        u, i = np.array(u, np.int32)[p], np.array(i, np.int32)[p]
        assert ctx.seen_set(u, i) == len(unknown)
        assert check_table(ctx, u, i) == len(unknown)
        _, off, _, _ = ctx.debug_seen_csr(ITEM)
        assert np.diff(off).max() >= 5000
        # n == 0 leaves an empty set; so does a list of unknown ids
        assert ctx.seen_set([], []) == 0
        assert ctx.seen_count() == 0 and check_table(ctx, [], []) == 0
        assert ctx.seen_set([99_000_001], [int(iid[0])]) == 1 and ctx.seen_count() == 0
        ctx.seen_set(u[:10], i[:10])
        ctx.seen_clear()
        assert ctx.seen_count() == 0


# ---- add = set of the union --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_adds_leave_the_table_a_set_of_the_union_builds(mode):
    rng = np.random.default_rng(23)
    nu, ni, k = 300, 3000, 4
    with make_ctx(k, mode) as a, make_ctx(k, mode) as b, make_ctx(k, mode) as c:
        for ctx in (a, b, c):
            uid, iid = int_model(np.random.default_rng(5), ctx, nu, ni, k)
        long_user = uid[11]
        held = rng.permutation(iid)
        A = [np.concatenate([np.full(2500, long_user), uid[rng.integers(0, nu, 3000)]]),
             np.concatenate([held[:2500], iid[rng.integers(0, ni, 3000)]])]
        A = [x.astype(np.int32) for x in A]
        new_u = np.array([7_000_001, 7_000_002], np.int32)
        new_i = np.array([8_000_001], np.int32)
        B1 = [np.concatenate([uid[rng.integers(0, nu, 900)], A[0][:200], [99_000_001]]).astype(np.int32),
              np.concatenate([iid[rng.integers(0, ni, 900)], A[1][:200], [int(iid[0])]]).astype(np.int32)]
        B2 = [A[0][100:400], A[1][100:400]]                     # no novel pair
        B3 = [np.zeros(0, np.int32), np.zeros(0, np.int32)]     # empty
        B4 = [np.array([new_u[0], new_u[1], new_u[0], uid[3]], np.int32),
              np.array([iid[5], new_i[0], new_i[0], new_i[0]], np.int32)]  # rows gained after the set, and one old
        B5 = [np.full(300, long_user, np.int32), held[2500:2800].astype(np.int32)]  # wholly inside one long row
        gain = (np.concatenate([new_u, [uid[0]]]), np.concatenate([[iid[0], iid[1]], new_i]), np.ones(3))

        assert a.seen_set(*A) == 0
        a.debug_seen_csr(ITEM)                                  # the item-major table exists before the adds
        a.online_update(*gain)                                  # rows gained after the set was built
        check_table(a, *A)                                      # (read through the padded offsets)
        assert a.seen_add(*B1) == 1
        a.debug_seen_csr(ITEM)
        before = a.seen_count()
        for B in (B2, B3):
            assert a.seen_add(*B) == 0 and a.seen_count() == before
        assert a.seen_add(*B4) == 0 and a.seen_count() == before + 4
        assert a.seen_add(*B5) == 0 and a.seen_count() > before + 4 + 250

        b.online_update(*gain)
        union = [np.concatenate([A[s], B1[s], B2[s], B3[s], B4[s], B5[s]]) for s in (0, 1)]
        assert b.seen_set(*union) == 1
        check_table(b, *union)
        same_tables(a, b)
        # on a context with no set, add is set
        c.online_update(*gain)
        assert c.seen_add(*union) == 1
        same_tables(c, b)


# ---- from the ALS data -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_from_als_is_a_set_of_the_prepared_pairs(mode):
    rng = np.random.default_rng(29)
    nu, ni, k, n = 60, 2300, 4, 6000
    uid, iid = shuffled_ids(rng, nu + 4), shuffled_ids(rng, ni + 4, 5)
    u = uid[rng.integers(0, nu, n)]
    i = iid[rng.integers(0, ni, n)]
    u[:2200], i[:2200] = uid[3], rng.permutation(iid[:ni])[:2200]  # one user row longer than a 2,048-entry tile
    u[-200:], i[-200:] = u[:200], i[:200]                         # duplicate pairs, in the batch and
    u[4000:4200], i[4000:4200] = u[100:300], i[100:300]           # in the prepared part
    r = rng.integers(-4, 11, n) / 2.0                             # ratings <= 0 among them
    cut = 4500
    # the batch: the rest, and two pairs of ids nobody holds yet
    bu, bi, br = (np.concatenate([x[cut:], y]) for x, y in ((u, uid[nu:nu + 2]), (i, iid[ni:ni + 2]), (r, np.ones(2))))
    with make_ctx(k, mode) as a, make_ctx(k, mode) as twin, make_ctx(k, mode) as whole:
        with pytest.raises(L.MFError) as err:
            a.seen_from_als()
        assert err.value.code == L.MF_ERR_STATE
        for ctx in (a, twin, whole):                              # rows that have no rating in the data
            ctx.set_factors(USER, uid[nu + 2:], np.ones((2, k)))
            ctx.set_factors(ITEM, iid[ni + 2:], np.ones((2, k)))
        a.als_prepare(u[:cut], i[:cut], r[:cut])
        twin.als_prepare(u[:cut], i[:cut], r[:cut])
        a.seen_from_als()
        assert twin.seen_set(u[:cut], i[:cut]) == 0
        check_table(a, u[:cut], i[:cut])
        same_tables(a, twin)
        # a snapshot: an append does not change it
        a.als_append(bu, bi, br)
        twin.als_append(bu, bi, br)
        check_table(a, u[:cut], i[:cut])
        same_tables(a, twin)
        # ... the caller adds the batch; that is from_als of the concatenation
        assert a.seen_add(bu, bi) == 0
        whole.als_prepare(np.concatenate([u[:cut], bu]), np.concatenate([i[:cut], bi]), np.concatenate([r[:cut], br]))
        whole.seen_from_als()
        same_tables(a, whole)


# ---- the readers against their definition ------------------------------------------------------------
def reader_case(rng, ctx, k, side):
    """An integer model, a set over it, rows gained afterwards; returns what the comparisons need."""
    nq, nc = 150, 200
    ids = [None, None]
    ids[side], ids[1 - side] = shuffled_ids(rng, nq), shuffled_ids(rng, nc, 5)
    ctx.set_factors(side, ids[side], rng.integers(-2, 3, (nq, k)).astype(np.float64))
    ctx.set_factors(1 - side, ids[1 - side], rng.integers(-2, 3, (nc, k)).astype(np.float64))
    qids, cids = ids[side], ids[1 - side]
    m = rng.random((nq, nc)) < 0.3
    m[4] = True                                                 # a query with everything seen
    m[5] = False
    qa, cb = np.nonzero(m)
    sq = np.concatenate([qids[qa], qids[qa][:40], [99_000_001, qids[0]]]).astype(np.int32)  # duplicates, unknown ids
    sc = np.concatenate([cids[cb], cids[cb][:40], [cids[0], 99_000_003]]).astype(np.int32)
    pair = [None, None]
    pair[side], pair[1 - side] = sq, sc
    assert ctx.seen_set(pair[USER], pair[ITEM]) == 2
    # rows gained after the set was built, on both sides
    late_q, late_c = np.array([5_000_001], np.int32), np.array([6_000_001, 6_000_002], np.int32)
    ctx.set_factors(side, late_q, rng.integers(-2, 3, (1, k)).astype(np.float64))
    ctx.set_factors(1 - side, late_c, rng.integers(-2, 3, (2, k)).astype(np.float64))
    pair[side], pair[1 - side] = np.full(2, qids[4], np.int32), late_c   # query 4 has seen those too
    assert ctx.seen_add(pair[USER], pair[ITEM]) == 0
    su, si = set_pairs(ctx)
    excl = (su, si) if side == USER else (si, su)
    queries = np.concatenate([qids, late_q, [99_000_001], qids[:3]]).astype(np.int32)
    cands = np.concatenate([cids, late_c])
    return qids, cands, m, excl, queries, late_q


@pytest.mark.parametrize("top_n", [1, 10, 128])
@pytest.mark.parametrize("k", [5, 64, 130])
@pytest.mark.parametrize("side", [USER, ITEM])
@pytest.mark.parametrize("mode", MODES)
def test_readers_equal_their_namesakes_given_the_sets_pairs(mode, side, k, top_n):
    rng = np.random.default_rng(1000 * k + top_n)
    with make_ctx(k, mode) as ctx:
        qids, cands, m, excl, queries, late_q = reader_case(rng, ctx, k, side)
        assert len(excl[0]) == ctx.seen_count() == int(m.sum()) + 2

        got = ctx.recommend(queries, top_n, side=side, exclude=SEEN)
        want = ctx.recommend(queries, top_n, side=side, exclude=excl)
        for x, y in zip(got, want):
            assert np.array_equal(x, y) and x.dtype == y.dtype
        assert got[2][4] == 0 and got[2][len(qids)] == top_n and got[2][len(qids) + 1] == 0
        plain = ctx.recommend(queries, top_n, side=side)
        assert not np.array_equal(plain[0], got[0])               # the set does exclude

        # ground truth: random pairs, some of them seen, an unknown query, the late query
        qa, cb = np.nonzero(m)
        pick = rng.integers(0, len(qa), 60)
        gq = np.concatenate([qids[rng.integers(0, len(qids), 400)], qids[qa[pick]], [99_000_001], late_q])
        gc = np.concatenate([cands[rng.integers(0, len(cands), 400)], cands[cb[pick]], [cands[0], cands[1]]])
        a = ctx.rank_eval(gq, gc, top_n, side=side, exclude=SEEN, per_query=True)
        b = ctx.rank_eval(gq, gc, top_n, side=side, exclude=excl, per_query=True)
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, np.ndarray):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f.name
            else:
                assert x == y and np.float64(x).tobytes() == np.float64(y).tobytes(), f.name
        assert a.unknown_queries == 1 and a.queries > 100

        eq = np.concatenate([qids[rng.integers(0, len(qids), 300)], qids[qa[pick]], [99_000_001], late_q, qids[:1]])
        ec = np.concatenate([cands[rng.integers(0, len(cands), 300)], cands[cb[pick]], cands[:2], [99_000_003]])
        eq, ec = eq.astype(np.int32), ec.astype(np.int32)
        got = ctx.pair_ranks(eq, ec, side=side, exclude=SEEN, scores=True)
        want = ctx.pair_ranks(eq, ec, side=side, exclude=excl, scores=True)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert (got[0] == L.PAIR_RANK_EXCLUDED).sum() >= 60 and (got[0] == L.PAIR_RANK_COLD).sum() == 2


@pytest.mark.parametrize("mode", MODES)
def test_an_absent_or_empty_set_excludes_nothing(mode):
    rng = np.random.default_rng(31)
    with make_ctx(6, mode) as ctx:
        uid, iid = int_model(rng, ctx, 40, 70, 6)
        for prepare in (lambda: None, lambda: ctx.seen_set([], []), ctx.seen_clear):
            prepare()
            for side, q in ((USER, uid), (ITEM, iid)):
                for x, y in zip(ctx.recommend(q, 10, side=side, exclude=SEEN), ctx.recommend(q, 10, side=side)):
                    assert np.array_equal(x, y)
            for x, y in zip(ctx.pair_ranks(uid[:20], iid[:20], exclude=SEEN), ctx.pair_ranks(uid[:20], iid[:20])):
                assert np.array_equal(x, y)
            assert ctx.rank_eval(uid[:20], iid[:20], 10, exclude=SEEN) == ctx.rank_eval(uid[:20], iid[:20], 10)


# ---- the prequential loop ----------------------------------------------------------------------------
def same_record(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), f.name
        else:
            assert x == y and np.float64(x).tobytes() == np.float64(y).tobytes(), f.name


def same_model(a, b):
    for side in (USER, ITEM):
        (ia, va), (ib, vb) = a.factors(side), b.factors(side)
        assert np.array_equal(ia, ib) and np.array_equal(va.view(np.uint64), vb.view(np.uint64))


@pytest.mark.parametrize("negatives", [0, 2])
@pytest.mark.parametrize("flavour", [L.ONLINE_NEXT_FACTORS, L.ONLINE_DELTA])
@pytest.mark.parametrize("mode", MODES)
def test_prequential_loop_equals_the_hand_written_one(mode, flavour, negatives):
    rng = np.random.default_rng(37)
    k, nu, ni = 8, 60, 90
    with make_ctx(k, mode) as a, make_ctx(k, mode) as b:
        for ctx in (a, b):
            uid, iid = int_model(np.random.default_rng(3), ctx, nu, ni, k)
        start = [uid[rng.integers(0, nu, 800)], iid[rng.integers(0, ni, 800)]]
        a.seen_set(*start)
        cum = [start[0].copy(), start[1].copy()]
        first = 0
        for step in range(3):
            n = 200
            # ... with a new user and a new item in every batch
            u = np.concatenate([uid[rng.integers(0, nu, n)], [9_000_000 + step, uid[1]]]).astype(np.int32)
            i = np.concatenate([iid[rng.integers(0, ni, n)], [iid[2], 9_500_000 + step]]).astype(np.int32)
            u[:20], i[:20] = cum[0][-20:], cum[1][-20:]         # events that are seen by now
            r = rng.integers(1, 11, len(u)) / 2.0
            if negatives:
                kw = dict(seed=5, first_event=first, flavour=flavour, ranks=True)
                ra = a.online_prequential_sampled(u, i, r, 10, negatives, 0.5, exclude=SEEN, add_events=True, **kw)
                rb = b.online_prequential_sampled(u, i, r, 10, negatives, 0.5, exclude=tuple(cum), **kw)
            else:
                ra = a.online_prequential(u, i, r, 10, flavour=flavour, exclude=SEEN, ranks=True, add_events=True)
                rb = b.online_prequential(u, i, r, 10, flavour=flavour, exclude=tuple(cum), ranks=True)
            same_record(ra, rb)
            assert ra.excluded >= 20 and ra.cold == 2
            first += len(u)
            cum = [np.concatenate([cum[0], u]), np.concatenate([cum[1], i])]
            assert a.seen_count() == len(np.unique(np.stack(cum, 1), axis=0))
        same_model(a, b)
        check_table(a, *cum)


def test_prequential_seen_refuses_the_spark_sweep():
    with make_ctx(4, F64) as ctx:
        int_model(np.random.default_rng(1), ctx, 5, 5, 4)
        with pytest.raises(L.MFError) as err:
            ctx.online_prequential([1], [1], [1.0], 10, flavour=L.ONLINE_SPARK_SWEEP, num_partitions=1, exclude=SEEN)
        assert err.value.code == L.MF_ERR_INVALID


# ---- lifecycle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_set_factors_and_load_keep_the_set_and_dsgd_prepare_empties_it(mode, tmp_path):
    from mfhip import synth
    d = synth.generate(300, 120, 6000, seed=3)
    with make_ctx(16, mode, iterations=1, num_blocks=3, seed=11, has_seed=1) as ctx:
        ctx.fit(d.u, d.i, d.r)
        ctx.seen_set(d.u, d.i)
        held = ctx.seen_count()
        assert held == len(np.unique(np.stack([d.u, d.i], 1), axis=0))
        before = tables(ctx)
        queries = np.unique(d.u)[:50]
        want = ctx.recommend(queries, 10, exclude=(d.u, d.i))
        path = str(tmp_path / "model.mfsnap")
        ctx.save(path)
        ctx.set_factors(USER, np.array([77_000_001], np.int32), np.ones((1, 16)))
        ctx.load(path)
        assert ctx.seen_count() == held
        for (rid, off, ent, eid), (rid0, off0, ent0, eid0) in zip(tables(ctx), before):
            assert np.array_equal(ent, ent0) and np.array_equal(eid, eid0)
            assert np.array_equal(off[:len(off0)], off0) and np.all(off[len(off0):] == off0[-1])
        for x, y in zip(ctx.recommend(queries, 10, exclude=SEEN), want):
            assert np.array_equal(x, y)
        # the rows are rebuilt: no set is left
        ctx.prepare(d.u, d.i, d.r)
        assert ctx.seen_count() == 0
        ctx.run(3)
        for x, y in zip(ctx.recommend(queries, 10, exclude=SEEN), ctx.recommend(queries, 10)):
            assert np.array_equal(x, y)
