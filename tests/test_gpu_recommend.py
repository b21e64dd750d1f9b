"""mf_recommend on the device: top-N by p.q, fused score + select (csrc/kernels_recommend.hip).

The reference is numpy on the host: Context.predict over the full query x candidate grid, ordered
with np.lexsort((candidate ids, -scores)) -- score descending, ties by id ascending, NaN last."""
import numpy as np
import pytest

import mfhip
from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth
from mfhip.context import Context

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]


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


def grid_scores(ctx, qids, cids, side=L.SIDE_USER):
    q = np.repeat(qids, len(cids))
    c = np.tile(cids, len(qids))
    pred, found = ctx.predict(q, c) if side == L.SIDE_USER else ctx.predict(c, q)
    assert found.all()
    return pred.reshape(len(qids), len(cids))


def reference(scores, cids, top_n, excluded=None):
    """(ids, scores, counts) as mf_recommend lays them out; excluded: per query row a bool mask over cids."""
    nq = scores.shape[0]
    ids = np.zeros((nq, top_n), np.int32)
    sc = np.zeros((nq, top_n), np.float64)
    cnt = np.zeros(nq, np.int32)
    for j in range(nq):
        keep = np.ones(len(cids), bool) if excluded is None else ~excluded[j]
        cj, sj = cids[keep], scores[j][keep]
        order = np.lexsort((cj, -sj))[:top_n]
        cnt[j] = len(order)
        ids[j, :len(order)] = cj[order]
        sc[j, :len(order)] = sj[order]
    return ids, sc, cnt


def assert_same(got, want, bitwise=True):
    ids, sc, cnt = got
    rids, rsc, rcnt = want
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(ids, rids)
    if bitwise:
        assert np.array_equal(sc.view(np.uint64), rsc.view(np.uint64))
    else:
        assert np.array_equal(sc, rsc, equal_nan=True)


def fill(ctx, rng, nq, nc, k, draw):
    qids, cids = shuffled_ids(rng, nq), shuffled_ids(rng, nc, 5)
    P, Q = draw((nq, k)), draw((nc, k))
    ctx.set_factors(L.SIDE_USER, qids, P)
    ctx.set_factors(L.SIDE_ITEM, cids, Q)
    return qids, cids, P, Q


# every value of each axis: k {1,3,10,64,100,130,256}, candidates {1,31,33,1000}, queries {1,33,70},
# top_n {1,10,128} (top_n above the candidate count included); then k_rec_f32<2, false> (top_n in
# 17..48, k no multiple of 4) with 70 queries over its 64-query tile, and the NW = 4 instance with 130
# queries, a second query block
INT_CASES = [(1, 1, 1, 1), (3, 31, 33, 10), (10, 33, 70, 128), (64, 1000, 70, 10), (100, 1000, 33, 128),
             (130, 33, 1, 10), (256, 1000, 70, 1), (64, 31, 1, 128), (10, 200, 70, 32), (3, 40, 130, 10)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,nc,nq,top_n", INT_CASES)
def test_integer_data_exact(mode, k, nc, nq, top_n):
    """Entries in {-3..3}: every product and sum is exact in f32, so both modes must equal the numpy
    reference exactly, tie-breaks among the many equal scores included."""
    rng = np.random.default_rng(1000 * k + nc + nq + top_n)
    with make_ctx(k, mode) as ctx:
        qids, cids, _, _ = fill(ctx, rng, nq, nc, k, lambda s: rng.integers(-3, 4, s).astype(np.float64))
        want = reference(grid_scores(ctx, qids, cids), cids, top_n)
        assert_same(ctx.recommend(qids, top_n), want, bitwise=False)


def check_f64_bitwise(ctx, qids, cids, top_n):
    ids, sc, cnt = ctx.recommend(qids, top_n)
    assert_same((ids, sc, cnt), reference(grid_scores(ctx, qids, cids), cids, top_n))
    for j, q in enumerate(qids):
        n = cnt[j]
        pred, found = ctx.predict(np.full(n, q, np.int32), ids[j, :n])
        assert found.all() and np.array_equal(pred.view(np.uint64), sc[j, :n].view(np.uint64))


def test_f64_scores_are_bitwise_predict():
    rng = np.random.default_rng(7)
    with make_ctx(37, L.MODE_DETERMINISTIC_F64) as ctx:
        qids, cids, _, _ = fill(ctx, rng, 70, 500, 37, lambda s: rng.standard_normal(s))
        check_f64_bitwise(ctx, qids, cids, 10)


def test_f64_after_a_blocked_fit():
    """Rows grouped by factor block (nb = 3), not by id, after a real fit of the smoke shape."""
    d = synth.generate(300, 120, 6000, seed=3)
    with make_ctx(16, L.MODE_DETERMINISTIC_F64, iterations=2, num_blocks=3, seed=11, has_seed=1) as ctx:
        ctx.fit(d.u, d.i, d.r)
        uids, _ = ctx.factors(L.SIDE_USER)
        iids, _ = ctx.factors(L.SIDE_ITEM)
        check_f64_bitwise(ctx, uids[::2][:200].copy(), iids, 10)


@pytest.mark.parametrize("k,nc,nq,top_n", [(100, 1000, 70, 10), (7, 300, 33, 128), (256, 1000, 20, 40)])
def test_f32_scores_within_the_fma_chain_bound(k, nc, nq, top_n):
    rng = np.random.default_rng(k)
    with make_ctx(k, L.MODE_FAST_F32) as ctx:
        qids, cids, P, Q = fill(ctx, rng, nq, nc, k, lambda s: rng.standard_normal(s))
        P32, Q32 = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
        ref = P32 @ Q32.T
        eps = k * 2.0 ** -24 * (np.abs(P32) @ np.abs(Q32).T)  # bound of a k-term f32 fma chain
        ids, sc, cnt = ctx.recommend(qids, top_n)
        col = {int(c): x for x, c in enumerate(cids)}
        assert np.array_equal(cnt, np.full(nq, min(top_n, nc)))
        for j in range(nq):
            n = cnt[j]
            cols = np.array([col[int(c)] for c in ids[j, :n]])
            assert len(set(cols)) == n
            assert (np.abs(sc[j, :n] - ref[j, cols]) <= eps[j, cols]).all()
            # sorted by the returned scores, ties by id
            assert np.array_equal(np.lexsort((ids[j, :n], -sc[j, :n])), np.arange(n))
            rest = np.ones(nc, bool)
            rest[cols] = False
            assert (ref[j, rest] <= ref[j, cols[-1]] + 2 * eps[j].max()).all()
            assert not ids[j, n:].any() and not sc[j, n:].any()


def test_geometry_independence(monkeypatch):
    """A score is one fmaf chain over f, so splits, batches, query order and repeats change nothing."""
    rng = np.random.default_rng(11)
    k, nq, nc, top_n = 100, 70, 1000, 10
    with make_ctx(k, L.MODE_FAST_F32) as ctx:
        qids, cids, _, _ = fill(ctx, rng, nq, nc, k, lambda s: rng.standard_normal(s))
        base = ctx.recommend(qids, top_n)
        by_id = {int(q): (base[0][j].copy(), base[1][j].view(np.uint64).copy(), int(base[2][j]))
                 for j, q in enumerate(qids)}
        lists = [qids, qids[::-1].copy(), np.concatenate([qids[:5], qids[:5], qids[40:], qids[3:4]])]
        for split in (1, 2, 7):
            for batch in (16, 64):
                set_knob(monkeypatch, "rec_split", split)
                set_knob(monkeypatch, "rec_batch", batch)
                for ql in lists:
                    ids, sc, cnt = ctx.recommend(ql, top_n)
                    for j, q in enumerate(ql):
                        want = by_id[int(q)]
                        assert np.array_equal(ids[j], want[0]) and cnt[j] == want[2]
                        assert np.array_equal(sc[j].view(np.uint64), want[1])


@pytest.mark.parametrize("mode", MODES)
def test_exclusion(mode):
    rng = np.random.default_rng(5)
    k, nq, nc, top_n = 10, 33, 40, 16
    with make_ctx(k, mode) as ctx:
        qids, cids, _, _ = fill(ctx, rng, nq, nc, k, lambda s: rng.integers(-3, 4, s).astype(np.float64))
        scores = grid_scores(ctx, qids, cids)
        plain = reference(scores, cids, top_n)
        excl = rng.random((nq, nc)) < 0.3
        excl[0, :] = True            # the whole catalogue excluded: count 0
        excl[1, :] = True
        excl[1, :5] = False          # 5 candidates left: count 5, zero tail
        excl[2, :] = False           # nothing excluded
        qq, cc = np.nonzero(excl)
        eq, ec = qids[qq], cids[cc]
        # duplicates, unknown ids on either side, and a pair for a query that is not asked
        asked = qids[:-1]
        eq = np.concatenate([eq, eq[:7], [999999, qids[2], qids[-1]]]).astype(np.int32)
        ec = np.concatenate([ec, ec[:7], [cids[0], 888888, cids[0]]]).astype(np.int32)
        got = ctx.recommend(asked, top_n, exclude=(eq, ec))
        want = reference(scores[:-1], cids, top_n, excluded=excl[:-1])
        assert_same(got, want, bitwise=False)
        assert got[2][0] == 0 and got[2][1] == 5
        assert not got[0][1, 5:].any() and not got[1][1, 5:].any()
        assert np.array_equal(got[0][2], plain[0][2])
        for j in range(len(asked)):
            assert not set(got[0][j, :got[2][j]].tolist()) & set(cids[excl[j]].tolist())
        # the last query was asked without its pair list: unchanged by pairs naming other queries
        alone = ctx.recommend(qids[-1:], top_n, exclude=(eq[:5], ec[:5]))
        assert np.array_equal(alone[0][0], plain[0][-1])


@pytest.mark.parametrize("mode", MODES)
def test_item_side_is_the_transpose(mode):
    rng = np.random.default_rng(9)
    k, nu, ni, top_n = 12, 150, 33, 20
    with make_ctx(k, mode) as ctx:
        uids, iids, _, _ = fill(ctx, rng, nu, ni, k, lambda s: rng.integers(-3, 4, s).astype(np.float64))
        scores = grid_scores(ctx, uids, iids)  # [user][item]
        want = reference(np.ascontiguousarray(scores.T), uids, top_n)
        assert_same(ctx.recommend(iids, top_n, side=L.SIDE_ITEM), want, bitwise=False)


@pytest.mark.parametrize("mode", MODES)
def test_edges_and_errors(mode):
    rng = np.random.default_rng(3)
    k, nc = 6, 40
    with make_ctx(k, mode) as ctx:
        with pytest.raises(L.MFError, match="has not been fitted") as e:
            ctx.recommend([1], 5)
        assert e.value.code == L.MF_ERR_NOT_FITTED
        cids = shuffled_ids(rng, nc)
        Q = rng.integers(4, 13, (nc, k)) / 8.0  # positive eighths: sums exact in f32 too
        Q[7, 2] = np.nan
        Q[11, :] = -np.inf
        ctx.set_factors(L.SIDE_USER, [5, -6], rng.integers(4, 13, (2, k)) / 8.0)  # positive: -inf stays -inf
        ctx.set_factors(L.SIDE_ITEM, cids, Q)
        ids, sc, cnt = ctx.recommend([5, 123456, -6], nc)
        assert cnt.tolist() == [nc, 0, nc]
        assert not ids[1].any() and not sc[1].any()
        for j in (0, 2):
            assert ids[j, -1] == cids[7] and np.isnan(sc[j, -1])
            assert ids[j, -2] == cids[11] and sc[j, -2] == -np.inf
            assert np.isfinite(sc[j, :-2]).all()
        want = reference(grid_scores(ctx, np.array([5, -6], np.int32), cids), cids, nc)
        assert np.array_equal(ids[[0, 2]], want[0])
        assert np.array_equal(sc[[0, 2]], want[1], equal_nan=True)
        ids, sc, cnt = ctx.recommend([], 5)
        assert ids.shape == (0, 5) and sc.shape == (0, 5) and cnt.shape == (0,)
        for bad in (0, L.RECOMMEND_MAX_TOP + 1):
            with pytest.raises(L.MFError) as e:
                ctx.recommend([5], bad)
            assert e.value.code == L.MF_ERR_INVALID
        ids, sc, cnt = ctx.recommend([5], 3, scores=False)
        assert sc is None and np.array_equal(ids, want[0][:1, :3])


def test_mirror_api_agrees_with_the_context():
    d = synth.generate(300, 120, 6000, seed=3)
    sgd = mfhip.DSGDforMF().setNumFactors(16).setIterations(2).setBlocks(3).setSeed(11)
    sgd.fit((d.u, d.i, d.r))
    ctx = sgd.context
    users = np.unique(d.u)[:50].astype(np.int32)
    ids, sc, cnt = ctx.recommend(users, 7)
    one = sgd.recommendProducts(int(users[3]), 7)
    assert one == [(int(users[3]), int(ids[3, x]), float(sc[3, x])) for x in range(cnt[3])]
    many = sgd.recommendProductsForUsers(7, users=users)
    assert many[int(users[3])] == one and len(many) == len(users)
    for j, u in enumerate(users):
        assert [t[1] for t in many[int(u)]] == ids[j, :cnt[j]].tolist()
    excl = (np.array([users[3]] * 2, np.int32), np.array([one[0][1], one[1][1]], np.int32))
    assert [t[1] for t in sgd.recommendProductsForUsers(5, users=users[3:4], exclude=excl)[int(users[3])]] == \
        [t[1] for t in one[2:7]]
    everyone = sgd.recommendProductsForUsers(3)
    assert len(everyone) == ctx.num_factors(L.SIDE_USER)
    item = int(ids[3, 0])
    ru = sgd.recommendUsers(item, 4)
    iu, isc, icnt = ctx.recommend([item], 4, side=L.SIDE_ITEM)
    assert ru == [(int(iu[0, x]), item, float(isc[0, x])) for x in range(icnt[0])]


def test_two_device_context():
    if L.device_count() < 2:
        pytest.skip("needs two GPUs")
    d = synth.generate(300, 120, 6000, seed=3)
    out = []
    for devices in ([0], [0, 1]):
        p = L.default_params()
        p.num_factors, p.iterations, p.num_blocks, p.seed, p.has_seed = 16, 2, 4, 11, 1
        with Context(p, devices=devices) as ctx:
            ctx.fit(d.u, d.i, d.r)
            users = np.unique(d.u)[:200].astype(np.int32)
            out.append(ctx.recommend(users, 10))
    assert_same(out[1], out[0])
