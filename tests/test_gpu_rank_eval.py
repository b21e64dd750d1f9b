"""mf_rank_eval on the device (csrc/kernels_rank.hip, csrc/rank_eval.cpp): ranking metrics of held-out
pairs against the model's top-N lists.

The reference is the definition of record, mfhip.ranking.host_metrics, over Context.recommend's output
for the same ids, top_n and exclusions: ids, (hits, g) and the six per-query values must be bitwise
equal, and an aggregate within (n + 1) 2^-53 relative of the math.fsum mean (n non-negative terms summed
in any order and one division on either side: an a-priori bound, nothing measured)."""
import ctypes as C
import math

import numpy as np
import pytest

import mfhip
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context
from mfhip.ranking import ground_truth_sets, host_metrics

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
FIELDS = ["precision", "recall", "map", "ndcg", "mrr", "hit_rate"]


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


def fill(ctx, rng, nq, nc, k, side=L.SIDE_USER):
    qids, cids = shuffled_ids(rng, nq), shuffled_ids(rng, nc, 5)
    ctx.set_factors(side, qids, rng.standard_normal((nq, k)))
    ctx.set_factors(1 - side, cids, rng.standard_normal((nc, k)))
    return qids, cids


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_against_definition(ctx, qids, gq, gc, top_n, exclude, side=L.SIDE_USER):
    m = ctx.rank_eval(gq, gc, top_n, side=side, exclude=exclude, per_query=True)
    known = np.unique(gq[np.isin(gq, qids)]).astype(np.int32)
    ids, _, cnt = ctx.recommend(known, top_n, side=side, exclude=exclude, scores=False)
    sets = ground_truth_sets(gq, gc)
    hc, hv = host_metrics(ids, cnt, [sets[int(q)] for q in known], top_n)
    n = len(known)
    assert m.queries == n and np.array_equal(m.ids, known)
    assert m.unknown_queries == len(np.unique(gq[~np.isin(gq, qids)]))
    assert np.array_equal(m.counts, hc)
    assert np.array_equal(bits(m.values), bits(hv)), np.argwhere(bits(m.values) != bits(hv))[:5]
    assert m.hits == int(hc[:, 0].sum()) and m.gt_pairs == int(hc[:, 1].sum())
    for c, f in enumerate(FIELDS):
        ref = math.fsum(hv[:, c]) / n if n else 0.0
        assert abs(getattr(m, f) - ref) <= (n + 1) * 2.0 ** -53 * ref, (f, getattr(m, f), ref)
    return m, cnt


def pairs_for(rng, qids, cids, top_n):
    """Ground truth and exclusions with every corner: per query a ground truth of 1, 2, top_n + 3 or 200
    candidates (unknown candidate ids fill up what the catalogue cannot give), duplicated pairs, unknown
    query ids, 30% of the grid excluded; with three or more queries, query 0 has its whole ground truth
    excluded and query 1 every candidate."""
    nq, nc = len(qids), len(cids)
    gq, gc = [], []
    for j, q in enumerate(qids):
        g = (1, 2, top_n + 3, 200)[j % 4]
        known = rng.choice(cids, min(g, nc), replace=False)
        unknown = 10_000_000 + 7 * np.arange(g - len(known)) - (j % 2) * 20_000_000  # of either sign
        cand = np.concatenate([known, unknown]).astype(np.int32)
        gq += [q] * len(cand)
        gc += cand.tolist()
    gq, gc = np.array(gq, np.int32), np.array(gc, np.int32)
    dup = rng.integers(0, len(gq), max(3, len(gq) // 5))
    gq = np.concatenate([gq, gq[dup], [77_000_001, 77_000_001, -77_000_002]]).astype(np.int32)
    gc = np.concatenate([gc, gc[dup], [cids[0], cids[0], 12345]]).astype(np.int32)
    order = rng.permutation(len(gq))
    gq, gc = gq[order], gc[order]
    excl = rng.random((nq, nc)) < 0.3
    if nq >= 3:
        excl[0] = np.isin(cids, gc[gq == qids[0]])
        excl[1] = True
    qq, cc = np.nonzero(excl)
    eq = np.concatenate([qids[qq], qids[qq][:5], [99_000_000, qids[0]]]).astype(np.int32)
    ec = np.concatenate([cids[cc], cids[cc][:5], [cids[0], 88_000_000]]).astype(np.int32)
    return gq, gc, (eq, ec)


# (queries, candidates, k, top_n): the 64-lane and second-slot edges of the metrics kernel, top_n above
# the candidate count, one query / one candidate
SHAPES = [(1, 1, 1, 1), (33, 31, 3, 10), (70, 1000, 64, 64), (70, 1000, 10, 65), (33, 40, 100, 128), (1, 33, 130, 10)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq,nc,k,top_n", SHAPES)
def test_equals_the_definition(mode, nq, nc, k, top_n):
    rng = np.random.default_rng(100 * nq + nc + k + top_n)
    with make_ctx(k, mode) as ctx:
        qids, cids = fill(ctx, rng, nq, nc, k)
        gq, gc, excl = pairs_for(rng, qids, cids, top_n)
        m, cnt = check_against_definition(ctx, qids, gq, gc, top_n, excl)
        if nq >= 3:
            known = np.unique(gq[np.isin(gq, qids)])
            j0, j1 = int(np.searchsorted(known, qids[0])), int(np.searchsorted(known, qids[1]))
            assert m.counts[j0, 0] == 0 and m.counts[j0, 1] >= 1 and not m.values[j0].any()
            assert cnt[j1] == 0 and m.counts[j1, 0] == 0
        check_against_definition(ctx, qids, gq, gc, top_n, None)


@pytest.mark.parametrize("mode", MODES)
def test_a_single_query_with_nothing_left_to_recommend(mode):
    rng = np.random.default_rng(4)
    with make_ctx(5, mode) as ctx:
        qids, cids = fill(ctx, rng, 1, 33, 5)
        gq, gc = np.repeat(qids, 4), cids[:4].copy()
        m, cnt = check_against_definition(ctx, qids, gq, gc, 10, (np.repeat(qids, 33), cids))
        assert cnt[0] == 0 and m.hits == 0 and m.gt_pairs == 4 and m.ndcg == 0.0
        m, _ = check_against_definition(ctx, qids, gq, gc, 10, (gq, gc))  # the whole ground truth excluded
        assert m.hits == 0 and m.recall == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_item_side_queries(mode):
    rng = np.random.default_rng(21)
    nq, nc, k, top_n = 33, 150, 12, 20
    with make_ctx(k, mode) as ctx:
        qids, cids = fill(ctx, rng, nq, nc, k, side=L.SIDE_ITEM)
        gq, gc, excl = pairs_for(rng, qids, cids, top_n)
        m, _ = check_against_definition(ctx, qids, gq, gc, top_n, excl, side=L.SIDE_ITEM)
        assert m.hits > 0


def snapshot(m):
    return ([m.queries, m.unknown_queries, m.gt_pairs, m.hits], bits([getattr(m, f) for f in FIELDS]).tolist(),
            m.ids.tolist(), m.counts.tolist(), bits(m.values).tolist())


@pytest.mark.parametrize("mode", MODES)
def test_geometry_independence(monkeypatch, mode):
    """2,500 queries cross two edges of the 1,024-query reduction slices; batches of 1, 3, 1,000 and 8,192
    queries, 1 and 4 candidate splits, and a repeat of every call give the same bits."""
    rng = np.random.default_rng(13)
    nq, nc, k, top_n = 2500, 40, 4, 10
    with make_ctx(k, mode) as ctx:
        qids, cids = fill(ctx, rng, nq, nc, k)
        n = 5 * nq
        gq, gc = rng.choice(qids, n), rng.choice(cids, n)
        excl = (rng.choice(qids, n), rng.choice(cids, n))
        base = None
        for batch in (1, 3, 1000, 8192):
            for split in (1, 4):
                set_knob(monkeypatch, "rec_batch", batch)
                set_knob(monkeypatch, "rec_split", split)
                for _ in range(2):
                    got = snapshot(ctx.rank_eval(gq, gc, top_n, exclude=excl, per_query=True))
                    base = base or got
                    assert got == base, (batch, split)
        assert base[0][0] > 2048 and base[0][3] > 0


def table_reference(qids, cids, q, c, ground_truth):
    """(query ids, offsets, entries) from numpy.unique on the packed pairs; a row is an id's position in
    the set_factors call (qids / cids)."""
    qrow = {int(x): r for r, x in enumerate(qids)}
    crow = {int(x): r for r, x in enumerate(cids)}
    rq = np.array([qrow.get(int(x), -1) for x in q], np.int64)
    rows = np.unique(rq[rq >= 0])
    keep = rq >= 0
    if ground_truth:
        low = (np.asarray(c, np.int64) & 0xFFFFFFFF) ^ 0x80000000
    else:
        low = np.array([crow.get(int(x), -1) for x in c], np.int64)
        keep &= low >= 0
    packed = np.unique((np.searchsorted(rows, rq[keep]).astype(np.uint64) << np.uint64(32)) | low[keep].astype(np.uint64))
    ent = (packed & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if ground_truth:
        ent = ((ent ^ 0x80000000) + 2 ** 31) % 2 ** 32 - 2 ** 31
    off = np.searchsorted((packed >> np.uint64(32)).astype(np.int64), np.arange(len(rows) + 1))
    return np.asarray(qids)[rows].astype(np.int32), off.astype(np.int64), ent.astype(np.int32)


@pytest.mark.parametrize("ground_truth", [True, False])
def test_device_tables(ground_truth):
    """mf_debug_rank_csr: 0, 1 and 100,000 pairs (several sort blocks) with heavy duplication, negative
    ids, unknown queries and unknown candidates (dropped for exclusions, kept for ground truth)."""
    rng = np.random.default_rng(17)
    with make_ctx(2, L.MODE_DETERMINISTIC_F64) as ctx:
        qids, cids = fill(ctx, rng, 300, 500, 2)
        qpool = np.concatenate([qids[:120], [50_000_001, -50_000_002, 50_000_003]]).astype(np.int32)
        cpool = np.concatenate([cids[:90], np.arange(40, dtype=np.int32) * 11 - 60_000_000, [2 ** 31 - 1, -2 ** 31]])
        cpool = cpool.astype(np.int32)
        cases = [(np.empty(0, np.int32), np.empty(0, np.int32)),
                 (qids[5:6], cids[7:8]),
                 (qids[5:6], np.array([60_000_000], np.int32)),
                 (rng.choice(qpool, 100_000), rng.choice(cpool, 100_000)),
                 (rng.choice(qpool[-3:], 50), rng.choice(cpool, 50))]  # only unknown queries
        for q, c in cases:
            got = ctx.rank_csr(q, c, ground_truth=ground_truth)
            want = table_reference(qids, cids, q, c, ground_truth)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and np.array_equal(a, b), (len(q), a[:8], b[:8])
        got = ctx.rank_csr(*cases[3], ground_truth=ground_truth)
        # 100,000 draws from the 123 x 132 pool: nearly every kept combination occurs, most of them repeatedly
        full = (132 if ground_truth else 90) * 120
        assert len(got[0]) == 120 and 0.95 * full < len(got[2]) <= full


def raw_eval(ctx, gq, gc, ng, top_n, out, side=L.SIDE_USER, eq=None, ec=None, ne=0, per=(None, None, None), cap=0):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_int32))
    return L.lib().mf_rank_eval(ctx._h, side, p(gq), p(gc), ng, top_n, p(eq), p(ec), ne,
                                None if out is None else C.byref(out), p(per[0]), p(per[1]), p(per[2]), cap)


@pytest.mark.parametrize("mode", MODES)
def test_errors_and_edges(monkeypatch, mode):
    rng = np.random.default_rng(3)
    one = np.array([1], np.int32)
    out = L.mf_rank_metrics()
    with make_ctx(6, mode) as ctx:
        with pytest.raises(L.MFError, match="has not been fitted") as e:
            ctx.rank_eval([1], [2], 5)
        assert e.value.code == L.MF_ERR_NOT_FITTED
        qids, cids = fill(ctx, rng, 3, 40, 6)
        for bad in (0, L.RECOMMEND_MAX_TOP + 1):
            with pytest.raises(L.MFError) as e:
                ctx.rank_eval(qids, cids[:3], bad)
            assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(L.MFError) as e:
            ctx.rank_eval(qids, cids[:3], 5, side=2)
        assert e.value.code == L.MF_ERR_INVALID
        assert raw_eval(ctx, one, one, 1, 5, None) == L.MF_ERR_INVALID            # NULL out
        assert raw_eval(ctx, one, one, -1, 5, out) == L.MF_ERR_INVALID            # negative counts
        assert raw_eval(ctx, one, one, 1, 5, out, ne=-1) == L.MF_ERR_INVALID
        assert raw_eval(ctx, None, one, 1, 5, out) == L.MF_ERR_INVALID            # NULL arrays, positive count
        assert raw_eval(ctx, one, None, 1, 5, out) == L.MF_ERR_INVALID
        assert raw_eval(ctx, one, one, 1, 5, out, eq=one, ec=None, ne=1) == L.MF_ERR_INVALID
        ids, cnt, val = np.zeros(8, np.int32), np.zeros((8, 2), np.int32), np.zeros((8, 6))
        assert raw_eval(ctx, one, one, 1, 5, out, per=(ids, None, val), cap=8) == L.MF_ERR_INVALID  # not all three
        assert L.lib().mf_last_error().decode()
        # capacity: three evaluated queries, room for two
        st = raw_eval(ctx, qids, cids[:3].copy(), 3, 5, out, per=(ids, cnt, val), cap=2)
        assert st == L.MF_ERR_CAPACITY and out.queries == 3 and "3" in L.lib().mf_last_error().decode()
        assert raw_eval(ctx, qids, cids[:3].copy(), 3, 5, out, per=(ids, cnt, val), cap=3) == L.MF_OK
        assert sorted(ids[:3].tolist()) == sorted(qids.tolist()) and out.queries == 3
        # n_gt == 0 and only-unknown queries: all zeros, not NaN
        for m in (ctx.rank_eval([], [], 5, per_query=True), ctx.rank_eval([123456, 123456, 7], cids[:3], 5, per_query=True)):
            assert (m.queries, m.gt_pairs, m.hits) == (0, 0, 0) and len(m.ids) == 0
            assert [getattr(m, f) for f in FIELDS] == [0.0] * 6
        assert m.unknown_queries == 2
    # the candidate side holds no row: every list is empty, so counts and metrics are 0 while the queries and
    # their ground truth are still counted -- in one batch and in batches of two (SHAPES holds the catalogue
    # smaller than top_n)
    with make_ctx(3, mode) as ctx:
        qids = shuffled_ids(rng, 5)
        ctx.set_factors(L.SIDE_USER, qids, rng.standard_normal((5, 3)))
        gq, gc = np.repeat(qids, 2)[:9], np.arange(9, dtype=np.int32)
        for batch in (8192, 2):
            set_knob(monkeypatch, "rec_batch", batch)
            for excl in (None, (gq, gc)):
                m, cnt = check_against_definition(ctx, qids, gq, gc, 10, excl)
                assert (m.queries, m.gt_pairs, m.hits) == (5, 9, 0) and not cnt.any()
                assert not m.counts[:, 0].any() and m.counts[:, 1].sum() == 9 and not m.values.any()
                assert [getattr(m, f) for f in FIELDS] == [0.0] * 6
    p = L.default_params()
    p.num_factors, p.mode = 6, mode
    with Context(p, rank=(0, 1, 0, b"")) as ctx:  # a rank-mode context (one rank: no communicator)
        with pytest.raises(L.MFError) as e:
            ctx.rank_eval([1], [2], 5)
        assert e.value.code == L.MF_ERR_STATE


@pytest.mark.parametrize("mode", ["deterministic", "fast"])
def test_after_training_the_mirror_api_agrees_with_the_definition(mode):
    """ALS.trainImplicit on a planted set, 10% of the pairs held out, the train pairs excluded:
    rankingMetrics(...).ndcgAt(10) equals host_metrics over recommendProductsForUsers (consistency, not
    a quality threshold)."""
    rng = np.random.default_rng(8)
    nu, ni, k = 300, 200, 8
    P, Q = rng.standard_normal((nu, k)), rng.standard_normal((ni, k))
    uu, ii = np.nonzero(P @ Q.T > 1.5 * np.sqrt(k) * 0.8)
    order = rng.permutation(len(uu))
    uu, ii = uu[order].astype(np.int32), ii[order].astype(np.int32)
    cut = len(uu) // 10
    test, train = (uu[:cut], ii[:cut]), (uu[cut:], ii[cut:])
    model = mfhip.ALS.trainImplicit((train[0], train[1], np.ones(len(train[0]))), rank=k, iterations=3, lambda_=0.1,
                                    alpha=2.0, mode=mode, seed=11)
    try:
        metrics = model.rankingMetrics(test, exclude=train)
        users = np.unique(test[0][np.isin(test[0], train[0])]).astype(np.int32)
        lists = model.recommendProductsForUsers(10, users=users, exclude=train)
        ids = np.zeros((len(users), 10), np.int32)
        cnt = np.zeros(len(users), np.int32)
        for j, u in enumerate(users):
            got = [t[1] for t in lists[int(u)]]
            ids[j, :len(got)], cnt[j] = got, len(got)
        sets = ground_truth_sets(*test)
        hc, hv = host_metrics(ids, cnt, [sets[int(u)] for u in users], 10)
        n = len(users)
        at = metrics.at(10)
        assert at.queries == n and at.hits == int(hc[:, 0].sum())
        for f, c in (("precisionAt", 0), ("recallAt", 1), ("meanAveragePrecisionAt", 2), ("ndcgAt", 3)):
            ref = math.fsum(hv[:, c]) / n
            assert abs(getattr(metrics, f)(10) - ref) <= (n + 1) * 2.0 ** -53 * ref, f
        assert metrics.at(10) is at  # cached
    finally:
        model.close()
