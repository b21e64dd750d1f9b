"""mf_online_prequential on the device (csrc/pair_rank.cpp): test-then-train on a micro-batch.

The ranking step is mf_pair_ranks' (tests/test_gpu_pair_ranks.py checks it against numpy and
mf_recommend); here: the update is bitwise mf_online_update's, the ranks are those of the model on
entry, the counts and the three sums equal the host statement (mfhip.prequential.host_prequential) bit for
bit, and the per-event values equal mf_rank_eval's per-query rows for one-item ground truths."""
import numpy as np
import pytest

from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth
from mfhip.combined import OnlineOfflineSpark, PSOfflineOnlineMF
from mfhip.context import Context
from mfhip.prequential import PrequentialEvaluator, host_prequential

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
COLD, EXCLUDED = L.PAIR_RANK_COLD, L.PAIR_RANK_EXCLUDED


def make_ctx(k, mode, **kw):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    for a, b in kw.items():
        setattr(p, a, b)
    return Context(p)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_model(a, b):
    for side in (L.SIDE_USER, L.SIDE_ITEM):
        ia, va = a.factors(side)
        ib, vb = b.factors(side)
        assert np.array_equal(ia, ib)
        assert np.array_equal(bits(va), bits(vb)), side


def check_record(rec, ranks, valid, top_n):
    """Counts and sums of a record against the definition, bit for bit."""
    n = len(ranks)
    vals, sums = host_prequential(ranks, valid, top_n)
    assert rec.events == n
    assert rec.evaluated == int((ranks >= 0).sum())
    assert rec.cold == int((ranks == COLD).sum()) and rec.excluded == int((ranks == EXCLUDED).sum())
    assert rec.hits == int(vals[:, 2].sum())
    got = (rec.sum_ndcg, rec.sum_rr, rec.sum_pr)
    assert bits(got).tolist() == bits(sums).tolist(), (got, sums)
    ev = rec.evaluated
    means = (rec.ndcg, rec.mrr, rec.hit_rate, rec.mpr)
    want = (sums[0] / ev, sums[1] / ev, rec.hits / ev, sums[2] / ev) if ev else (0.0,) * 4
    assert bits(means).tolist() == bits(want).tolist()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("flavour,parts", [(L.ONLINE_NEXT_FACTORS, 0), (L.ONLINE_DELTA, 0), (L.ONLINE_SPARK_SWEEP, 2)])
def test_update_is_bitwise_online_update_and_ranks_are_those_on_entry(mode, flavour, parts):
    rng = np.random.default_rng(3 + flavour)
    k, n = 8, 600
    u1, i1 = rng.integers(0, 40, n).astype(np.int32), rng.integers(0, 90, n).astype(np.int32)
    u2, i2 = rng.integers(20, 70, n).astype(np.int32), rng.integers(50, 130, n).astype(np.int32)  # new ids too
    r1, r2 = rng.integers(1, 6, n).astype(np.float64), rng.integers(1, 6, n).astype(np.float64)
    excl = (u1[:200], i1[:200])
    u2[:5], i2[:5] = u1[:5], i1[:5]  # events that are themselves excluded
    with make_ctx(k, mode) as a, make_ctx(k, mode) as b:
        for ctx in (a, b):
            ctx.online_update(u1, i1, r1, flavour, parts)
        ranks, valid, _ = a.pair_ranks(u2, i2, exclude=excl)
        assert (ranks == COLD).any() and (ranks >= 0).any() and (ranks == EXCLUDED).any()
        rec = a.online_prequential(u2, i2, r2, 10, flavour, parts, exclude=excl, ranks=True)
        tu, ti = b.online_update(u2, i2, r2, flavour, parts)
        assert np.array_equal(rec.ranks, ranks)
        check_record(rec, ranks, valid, 10)
        assert (rec.touched_users, rec.touched_items) == (tu, ti)
        same_model(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_counts_and_sums_equal_the_host_statement(monkeypatch, mode):
    rng = np.random.default_rng(17)
    k, nc, nu = 8, 64, 50
    with make_ctx(k, mode) as ctx:
        uids = (rng.permutation(nu).astype(np.int32) - 20) * 3
        iids = (rng.permutation(nc).astype(np.int32) - 30) * 5
        ctx.set_factors(L.SIDE_USER, uids, 0.3 * rng.standard_normal((nu, k)))
        ctx.set_factors(L.SIDE_ITEM, iids, 0.3 * rng.standard_normal((nc, k)))
        m = rng.random((nu, nc)) < 0.2
        a, b = np.nonzero(m)
        excl = (uids[a], iids[b])
        for n, batch in ((1, None), (1023, None), (1025, None), (2049, None), (1025, 7)):
            u = rng.choice(uids, n).astype(np.int32)
            i = rng.choice(iids, n).astype(np.int32)  # only known ids: the model keeps its 64 items
            if n > 1:
                u[::50] = 77_000_000  # cold, every call the same new user
            r = rng.integers(1, 6, n).astype(np.float64)
            if batch is not None:
                set_knob(monkeypatch, "pr_batch", batch)
            ranks, valid, _ = ctx.pair_ranks(u, i, exclude=excl)
            rec = ctx.online_prequential(u, i, r, 10, exclude=excl, ranks=True)
            monkeypatch.delenv("MFHIP_TEST", raising=False)
            assert np.array_equal(rec.ranks, ranks)
            assert valid[ranks >= 0].max() <= nc
            check_record(rec, ranks, valid, 10)


@pytest.mark.parametrize("mode", MODES)
def test_per_event_values_equal_rank_eval_per_query_rows(mode):
    """Each user once: the event's ndcg / rr / hit are mf_rank_eval's row of the query whose ground truth
    is that one item, with the same exclusions -- an excluded or unknown item scores 0 on both sides."""
    rng = np.random.default_rng(23)
    k, nc, nu, top_n = 12, 200, 150, 20
    with make_ctx(k, mode) as ctx:
        uids = (rng.permutation(nu).astype(np.int32) - 70) * 3
        iids = (rng.permutation(nc).astype(np.int32) - 90) * 5
        ctx.set_factors(L.SIDE_USER, uids, rng.standard_normal((nu, k)))
        ctx.set_factors(L.SIDE_ITEM, iids, rng.standard_normal((nc, k)))
        u = np.sort(uids)
        i = rng.choice(iids, nu).astype(np.int32)
        i[5] = 66_000_000  # an item the model does not hold
        m = rng.random((nu, nc)) < 0.5
        row = {int(x): a for a, x in enumerate(uids)}
        col = {int(x): b for b, x in enumerate(iids)}
        for x, y in zip(u.tolist(), i.tolist()):  # half of every user's items, but not the event's own
            if y in col:
                m[row[x], col[y]] = False
        a, b = np.nonzero(m)
        excl = (np.concatenate([uids[a], u[:3]]).astype(np.int32), np.concatenate([iids[b], i[:3]]).astype(np.int32))
        ranks, valid, _ = ctx.pair_ranks(u, i, exclude=excl)
        assert (ranks[:3] == EXCLUDED).all() and ranks[5] == COLD and (ranks >= 0).sum() > 100
        assert ((ranks >= 0) & (ranks < top_n)).sum() >= 10
        vals, _ = host_prequential(ranks, valid, top_n)
        ref = ctx.rank_eval(u, i, top_n, exclude=excl, per_query=True)
        assert np.array_equal(ref.ids, u)
        assert np.array_equal(bits(ref.values[:, 3]), bits(vals[:, 0]))  # ndcg
        assert np.array_equal(bits(ref.values[:, 4]), bits(vals[:, 1]))  # rr
        assert np.array_equal(bits(ref.values[:, 5]), bits(vals[:, 2]))  # hit
        rec = ctx.online_prequential(u, i, np.ones(nu), top_n, exclude=excl)
        assert rec.hits == ref.hits
        check_record(rec, ranks, valid, top_n)


@pytest.mark.parametrize("mode", MODES)
def test_fresh_context_is_all_cold_and_learns(mode):
    rng = np.random.default_rng(29)
    n = 100
    u, i = rng.integers(0, 30, n).astype(np.int32), rng.integers(0, 20, n).astype(np.int32)
    r = rng.integers(1, 6, n).astype(np.float64)
    with make_ctx(6, mode) as a, make_ctx(6, mode) as b:
        rec = a.online_prequential(u, i, r, 5, ranks=True)
        assert (rec.events, rec.evaluated, rec.cold, rec.excluded, rec.hits) == (n, 0, n, 0, 0)
        assert (rec.ranks == COLD).all()
        assert (rec.sum_ndcg, rec.sum_rr, rec.sum_pr, rec.ndcg, rec.mrr, rec.hit_rate, rec.mpr) == (0.0,) * 7
        b.online_update(u, i, r)
        same_model(a, b)
        rec0 = a.online_prequential(u[:0], i[:0], r[:0], 5)  # n == 0
        assert rec0.events == 0 and rec0.evaluated == 0
        same_model(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_a_refused_call_leaves_the_model_untouched(mode):
    rng = np.random.default_rng(31)
    with make_ctx(6, mode) as ctx:
        ctx.online_update([1, 2, 3], [1, 2, 3], [1.0, 2.0, 3.0])
        before = [ctx.factors(s) for s in (0, 1)]
        u, i, r = np.array([1, 9, -4], np.int32), np.array([2, 8, 7], np.int32), np.ones(3)
        for top_n, flavour, parts in ((0, L.ONLINE_NEXT_FACTORS, 0), (129, L.ONLINE_NEXT_FACTORS, 0),
                                      (10, 7, 0), (10, L.ONLINE_SPARK_SWEEP, 0), (10, L.ONLINE_SPARK_SWEEP, 2)):
            with pytest.raises(L.MFError) as e:  # the last: the Spark sweep refuses the negative user id
                ctx.online_prequential(u, i, r, top_n, flavour, parts)
            assert e.value.code == L.MF_ERR_INVALID
            for s in (0, 1):
                ids, vecs = ctx.factors(s)
                assert np.array_equal(ids, before[s][0]) and np.array_equal(bits(vecs), bits(before[s][1]))


def smoke_batches(nb=5):
    d = synth.generate(300, 120, 6000, seed=3)
    return d, np.array_split(np.arange(len(d.u)), nb)


def test_evaluator_cumulative_values_add_the_batches():
    d, parts = smoke_batches()
    with make_ctx(8, L.MODE_FAST_F32) as ctx:
        ev = PrequentialEvaluator(ctx, 10)
        seen_u, seen_i = np.zeros(0, np.int32), np.zeros(0, np.int32)
        for p in parts:
            ev.process(d.u[p], d.i[p], d.r[p], exclude=(seen_u, seen_i))
            seen_u, seen_i = np.concatenate([seen_u, d.u[p]]), np.concatenate([seen_i, d.i[p]])
        assert len(ev.batches) == 5 and ev.events == 6000
        assert ev.batches[0].evaluated == 0 and ev.batches[-1].evaluated > 0
        for name in ("events", "evaluated", "cold", "excluded", "hits"):
            assert getattr(ev, name) == sum(getattr(b, name) for b in ev.batches)
        assert ev.events == ev.evaluated + ev.cold + ev.excluded
        for name in ("sum_ndcg", "sum_rr", "sum_pr"):
            total = 0.0
            for b in ev.batches:
                total = total + getattr(b, name)
            assert getattr(ev, name) == total
        assert ev.ndcg == ev.sum_ndcg / ev.evaluated and ev.mpr == ev.sum_pr / ev.evaluated
        assert ev.hit_rate == ev.hits / ev.evaluated and ev.mrr == ev.sum_rr / ev.evaluated
        assert ev.curve("mpr").tolist() == [b.mpr for b in ev.batches]
        assert 0.0 < ev.mpr < 1.0 and 0.0 <= ev.ndcg <= 1.0


def same_vectors(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(bits(a[key]), bits(b[key])), key


def test_combined_models_return_the_same_vectors_with_evaluation():
    d, parts = smoke_batches()
    kw = dict(num_factors=8, num_partitions=2, offline_every=3, iterations=2)
    plain, judged = OnlineOfflineSpark(**kw), OnlineOfflineSpark(eval_top_n=10, **kw)
    try:
        assert plain.metrics is None
        for p in parts:
            ua, ia, oa = plain.process(d.u[p], d.i[p], d.r[p])
            ub, ib, ob = judged.process(d.u[p], d.i[p], d.r[p])
            assert oa == ob
            same_vectors(ua, ub)
            same_vectors(ia, ib)
        assert len(judged.metrics.batches) == 5 and judged.metrics.events == 6000
        assert judged.metrics.evaluated > 0
    finally:
        plain.close()
        judged.close()
    plain, judged = PSOfflineOnlineMF(8), PSOfflineOnlineMF(8, eval_top_n=10)
    try:
        for p in parts[:2]:
            ua, ia = plain.process(d.u[p], d.i[p], d.r[p])
            ub, ib = judged.process(d.u[p], d.i[p], d.r[p])
            same_vectors(ua, ub)
            same_vectors(ia, ib)
        assert len(judged.metrics.batches) == 2 and judged.metrics.evaluated > 0
    finally:
        plain.close()
        judged.close()


def test_planted_stream_ranks_its_best_rated_items_better_over_time():
    """Sanity, not a gate on quality: four passes over the planted stream in five batches each, learning
    every rating and judging the 5-star events; their mean percentile rank in the last batch is below
    that of the first batch with evaluated events (a numpy replay of the same schedule goes 0.51 -> 0.33)."""
    d, parts = smoke_batches()
    with make_ctx(8, L.MODE_FAST_F32, online_learning_rate=0.05) as ctx:
        ev = PrequentialEvaluator(ctx, 10)
        for _ in range(4):
            for p in parts:
                top = d.r[p] >= 5
                ev.process(d.u[p][top], d.i[p][top], d.r[p][top])
                ctx.online_update(d.u[p][~top], d.i[p][~top], d.r[p][~top])
        judged = [b for b in ev.batches if b.evaluated > 0]
        print("mpr first / last:", judged[0].mpr, judged[-1].mpr)
        assert judged[-1].mpr < judged[0].mpr
