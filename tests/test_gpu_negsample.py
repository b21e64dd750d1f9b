"""mf_online_update_sampled / mf_online_prequential_sampled on the device: the expansion, not the update.

The update arithmetic of every online kernel instance is pinned by test_gpu_online_ranks.py.  What can go
wrong here is the expansion in front of it -- its layout on each path, the rows after a miss, the pool,
the stream counter -- so the shapes are small and every comparison is bitwise against a twin context that
received online_update(negsample.expand(...)): the batch a caller would have expanded on the host, with
the ids negsample.draws (plain Python integers) gives for the rows the test computes itself.

The model: 40 users and 23 items under shuffled signed ids, loaded by set_factors, so rows are in
insertion order.  300 events, the hottest item in about a third of them, applied as calls [0, 200) and
[200, 300) with first_event 0 and 200; the second call brings 5 new users and 3 new items (the miss path:
the queued expansion is void, the pool grows to 26, the expansion runs again with the final rows).
"""
import copy
import functools

import numpy as np
import pytest

import mfhip
from conftest import set_knob
from mfhip import _lib as L
from mfhip import negsample as NS
from mfhip.prequential import PrequentialEvaluator

pytestmark = pytest.mark.gpu

F32, F64 = L.MODE_FAST_F32, L.MODE_DETERMINISTIC_F64
NU, NI, N, SPLIT = 40, 23, 300, 200
SEED = 7
NEG_RATING = 0.125
# mode, k, whether one sweep launch per call is expected
PATHS = [(F32, 8, "f32 sweep"), (F32, 300, "ticket sweep"), (F64, 8, "ticket sweep"), (F64, 64, "split sweep")]


class Stream:
    """The model's ids and factors and the 300 events; the same for every test (k only sizes the factors)."""

    def __init__(self, k):
        rng = np.random.default_rng(20 + k)
        ids = rng.permutation(np.arange(-60, 60, dtype=np.int32))
        self.known_u, self.new_u = ids[:NU].copy(), ids[NU:NU + 5].copy()
        ids = rng.permutation(np.arange(-50, 50, dtype=np.int32))
        self.known_i, self.new_i = ids[:NI].copy(), ids[NI:NI + 3].copy()
        self.U0 = rng.random((NU, k))
        self.I0 = rng.random((NI, k))
        hot = self.known_i[4]
        u = rng.choice(self.known_u, N)
        i = np.where(rng.random(N) < 1 / 3, hot, rng.choice(self.known_i, N))
        # the second call's new ids, each more than once, new users also on known items
        for x, pos in enumerate(range(SPLIT + 3, N, 9)):
            u[pos] = self.new_u[x % 5]
        for x, pos in enumerate(range(SPLIT + 5, N, 12)):
            i[pos] = self.new_i[x % 3]
        self.u, self.i = u.astype(np.int32), i.astype(np.int32)
        self.r = np.round(rng.uniform(0.5, 1.5, N), 3)
        assert set(self.new_u) <= set(u[SPLIT:]) and set(self.new_i) <= set(i[SPLIT:])
        for a in (self.u, self.i, self.r, self.U0, self.I0):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def stream(k):
    return Stream(k)


def expected_ids(row_id, i, first_event, negatives, seed=SEED):
    """The drawn ids of one call.  row_id: the model's item ids by row before the call (a list, extended
    in place by the call's new ids in first-touch order, as the library gives them rows)."""
    row_of = {int(x): r for r, x in enumerate(row_id)}
    for x in i:
        if int(x) not in row_of:
            row_of[int(x)] = len(row_id)
            row_id.append(int(x))
    rows = NS.draws(seed, first_event, [row_of[int(x)] for x in i], len(row_id), negatives)
    return np.asarray(row_id, np.int32)[rows]


def context(s, mode, k, lr=None):
    p = L.default_params()
    p.num_factors, p.mode = k, mode
    if lr is not None:
        p.online_learning_rate = lr
    ctx = mfhip.Context(p)
    if s is not None:
        ctx.set_factors(L.SIDE_USER, s.known_u, s.U0)
        ctx.set_factors(L.SIDE_ITEM, s.known_i, s.I0)
    return ctx


def model(ctx):
    return ctx.factors(L.SIDE_USER), ctx.factors(L.SIDE_ITEM)


def same_model(a, b):
    for (ida, va), (idb, vb) in zip(a, b):
        if not (np.array_equal(ida, idb) and va.shape == vb.shape
                and np.array_equal(np.ascontiguousarray(va).view(np.int64), np.ascontiguousarray(vb).view(np.int64))):
            return False
    return True


def run_sampled(s, mode, k, negatives, calls=((0, SPLIT), (SPLIT, N)), expect_sweep=True, loaded=True):
    """The stream through online_update_sampled in `calls`: (ids per call, touched per call, model)."""
    ids, touched = [], []
    with context(s if loaded else None, mode, k) as ctx:
        for lo, hi in calls:
            ctx.reset_stats()
            tu, ti, got = ctx.online_update_sampled(s.u[lo:hi], s.i[lo:hi], s.r[lo:hi], negatives, NEG_RATING, SEED,
                                                    first_event=lo, sampled=True)
            st = ctx.stats()
            assert st["updates"] == (hi - lo) * (1 + negatives)
            if expect_sweep:
                assert (st["kernel_launches"], st["levels"]) == (1, 0), (lo, st)
            else:
                assert st["levels"] >= 1 and st["kernel_launches"] == st["levels"], (lo, st)
            ids.append(got)
            touched.append((tu, ti))
        return ids, touched, model(ctx)


def run_twin(s, mode, k, ids, calls=((0, SPLIT), (SPLIT, N)), loaded=True):
    """online_update on the host-expanded batches: (touched per call, model)."""
    touched = []
    with context(s if loaded else None, mode, k) as ctx:
        for (lo, hi), got in zip(calls, ids):
            U, I, R = NS.expand(s.u[lo:hi], s.i[lo:hi], s.r[lo:hi], got, NEG_RATING)
            touched.append(ctx.online_update(U, I, R))
        return touched, model(ctx)


def want_ids(s, negatives, calls=((0, SPLIT), (SPLIT, N)), loaded=True):
    row_id = [int(x) for x in s.known_i] if loaded else []
    return [expected_ids(row_id, s.i[lo:hi], lo, negatives) for lo, hi in calls]


@pytest.mark.parametrize("negatives", [1, 5, 64])
@pytest.mark.parametrize("mode, k, path", PATHS, ids=[f"{'f32' if m == F32 else 'f64'}-k{k}" for m, k, _ in PATHS])
def test_every_path_equals_the_host_expanded_batch(mode, k, path, negatives):
    s = stream(k)
    ids, touched, got = run_sampled(s, mode, k, negatives)
    want = want_ids(s, negatives)
    for a, b in zip(ids, want):
        assert a.shape == b.shape and np.array_equal(a, b), path
    twin_touched, twin = run_twin(s, mode, k, want)
    assert touched == twin_touched
    assert same_model(got, twin), path
    assert len(got[0][0]) == NU + 5 and len(got[1][0]) == NI + 3


@pytest.mark.parametrize("knob, value, sweep", [("online_lookup", "host", True), ("online_kernel", "level", False),
                                               ("online_waves", "1", True)])
@pytest.mark.parametrize("mode, k", [(F32, 8), (F64, 64)], ids=["f32-k8", "f64-k64"])
def test_knobs_give_the_default_result(monkeypatch, mode, k, knob, value, sweep):
    s = stream(k)
    ids, touched, got = run_sampled(s, mode, k, 5)
    set_knob(monkeypatch, knob, value)
    kids, ktouched, kgot = run_sampled(s, mode, k, 5, expect_sweep=sweep)
    for a, b in zip(ids, kids):
        assert np.array_equal(a, b)
    assert touched == ktouched
    assert same_model(got, kgot)


@pytest.mark.parametrize("mode, k", [(F32, 8), (F64, 8)], ids=["f32", "f64"])
def test_split_invariance_without_new_items(mode, k):
    """No new item id (the new users stay: the miss path with the pool unchanged): the pool is 23
    throughout, so the draws depend on the event's number alone."""
    s = copy.copy(stream(k))
    s.i = np.where(np.isin(s.i, s.new_i), s.known_i[0], s.i).astype(np.int32)
    ids1, _, m1 = run_sampled(s, mode, k, 5, calls=((0, N),))
    ids2, _, m2 = run_sampled(s, mode, k, 5, calls=((0, 120), (120, N)))
    assert np.array_equal(ids1[0], np.concatenate(ids2))
    assert np.array_equal(ids1[0], want_ids(s, 5, calls=((0, N),))[0])
    assert same_model(m1, m2)
    assert len(m1[0][0]) == NU + 5 and len(m1[1][0]) == NI


@pytest.mark.parametrize("mode, k", [(F32, 8), (F64, 64)], ids=["f32", "f64"])
def test_empty_context_first_batch_brings_every_id(mode, k):
    s = stream(k)
    calls = ((0, N),)
    ids, touched, got = run_sampled(s, mode, k, 5, calls=calls, loaded=False)
    want = want_ids(s, 5, calls=calls, loaded=False)
    assert np.array_equal(ids[0], want[0])
    twin_touched, twin = run_twin(s, mode, k, want, calls=calls, loaded=False)
    assert touched == twin_touched and same_model(got, twin)


@pytest.mark.parametrize("mode", [F32, F64], ids=["f32", "f64"])
def test_small_pools_and_small_batches(mode):
    k = 8
    s = stream(k)
    u, r = s.u[:50], s.r[:50]

    def both(known_items, items, n=50):
        out = []
        for sampled in (True, False):
            with context(None, mode, k) as ctx:
                ctx.set_factors(L.SIDE_USER, s.known_u, s.U0)
                if len(known_items):
                    ctx.set_factors(L.SIDE_ITEM, known_items, s.I0[:len(known_items)])
                if sampled:
                    tu, ti, ids = ctx.online_update_sampled(u[:n], items[:n], r[:n], 5, NEG_RATING, SEED, 3, sampled=True)
                    out.append(((tu, ti), ids, model(ctx), ctx.stats()["updates"]))
                else:
                    U, I, R = NS.expand(u[:n], items[:n], r[:n], out[0][1], NEG_RATING)
                    out.append((ctx.online_update(U, I, R), None, model(ctx), ctx.stats()["updates"]))
        return out

    one = s.known_i[:1]
    # a model with one item (known, or brought by the batch): no negatives, the plain batch
    for known in (one, one[:0]):
        a, b = both(known, np.repeat(one, 50))
        assert a[1].shape == (50, 0) and a[3] == b[3] == 50
        assert a[0] == b[0] and same_model(a[2], b[2])
    # two items (both known; one of them new): every negative is the other item
    two = s.known_i[:2]
    items = np.where(np.arange(50) % 3 == 0, two[0], two[1]).astype(np.int32)
    for known in (two, two[:1], two[:0]):
        a, b = both(known, items)
        assert np.array_equal(a[1], np.repeat(np.where(items == two[0], two[1], two[0])[:, None], 5, axis=1))
        assert a[3] == b[3] == 300 and a[0] == b[0] and same_model(a[2], b[2])
    # n = 1, and n = 0
    a, b = both(s.known_i, s.i, n=1)
    assert np.array_equal(a[1], expected_ids([int(x) for x in s.known_i], s.i[:1], 3, 5))
    assert a[3] == b[3] == 6 and a[0] == b[0] and same_model(a[2], b[2])
    a, b = both(s.known_i, s.i, n=0)
    assert a[1].shape == (0, 0) and a[3] == 0 and a[0] == (0, 0) and same_model(a[2], b[2])


@pytest.mark.parametrize("mode", [F32, F64], ids=["f32", "f64"])
def test_no_negatives_is_online_update(mode):
    k = 8
    s = stream(k)
    with context(s, mode, k) as a, context(s, mode, k) as b:
        ta = a.online_update_sampled(s.u, s.i, s.r, 0, NEG_RATING, SEED, 5)
        tb = b.online_update(s.u, s.i, s.r)
        assert ta == tb and same_model(model(a), model(b))
        assert a.stats()["updates"] == b.stats()["updates"] == N


def test_refusals_leave_the_model_untouched():
    k = 8
    s = stream(k)
    with context(s, F64, k) as ctx:
        before = model(ctx)
        new = s.new_i[:1].repeat(4)
        for kw in (dict(flavour=L.ONLINE_SPARK_SWEEP), dict(negatives=65), dict(negatives=-1), dict(first_event=-1),
                   dict(negative_rating=float("nan")), dict(flavour=7)):
            args = dict(negatives=5, negative_rating=0.0, seed=1, first_event=0)
            args.update(kw)
            with pytest.raises(L.MFError) as e:
                ctx.online_update_sampled(s.u[:4], new, s.r[:4], **args)
            assert e.value.code == L.MF_ERR_INVALID, kw
            with pytest.raises(L.MFError) as e:
                ctx.online_prequential_sampled(s.u[:4], new, s.r[:4], 10, **args)
            assert e.value.code == L.MF_ERR_INVALID, kw
        assert ctx.stats()["updates"] == 0
        assert same_model(model(ctx), before)         # (the new item id was not inserted either)
    p = L.default_params()
    p.num_factors = k
    contexts = [dict(rank=(0, 1, 0, b""))]
    if mfhip.device_count() >= 2:
        contexts.append(dict(n_devices=2))
    for kw in contexts:
        with mfhip.Context(p, **kw) as ctx:
            with pytest.raises(L.MFError) as plain:
                ctx.online_update(s.u[:4], s.i[:4], s.r[:4])
            with pytest.raises(L.MFError) as sampled:
                ctx.online_update_sampled(s.u[:4], s.i[:4], s.r[:4], 5)
            assert sampled.value.code == plain.value.code
            assert str(sampled.value) == str(plain.value)


@pytest.mark.parametrize("mode, k", [(F32, 8), (F64, 64)], ids=["f32", "f64"])
def test_prequential_sampled(mode, k):
    s = stream(k)
    lo, hi = SPLIT, N     # the call with new ids: cold events in step 1
    excl = (s.u[:40], s.i[:40])
    with context(s, mode, k) as a, context(s, mode, k) as b, context(s, mode, k) as c:
        rec, ids = a.online_prequential_sampled(s.u[lo:hi], s.i[lo:hi], s.r[lo:hi], 10, 5, NEG_RATING, SEED, lo,
                                                exclude=excl, ranks=True, sampled=True)
        ref = b.online_prequential(s.u[lo:hi], s.i[lo:hi], s.r[lo:hi], 10, exclude=excl, ranks=True)
        tu, ti, cids = c.online_update_sampled(s.u[lo:hi], s.i[lo:hi], s.r[lo:hi], 5, NEG_RATING, SEED, lo, sampled=True)
        assert np.array_equal(rec.ranks, ref.ranks) and rec.cold == ref.cold > 0
        for f in ("events", "evaluated", "cold", "excluded", "hits", "sum_ndcg", "sum_rr", "sum_pr", "ndcg", "mrr",
                  "hit_rate", "mpr"):
            assert getattr(rec, f) == getattr(ref, f), f
        assert np.array_equal(ids, cids) and (rec.touched_users, rec.touched_items) == (tu, ti)
        assert same_model(model(a), model(c))
    # the evaluator advances first_event: two process calls = one sampled call when the pool is unchanged
    with context(s, mode, k) as a, context(s, mode, k) as b:
        ev = PrequentialEvaluator(a, 10, negatives=5, negative_rating=NEG_RATING, seed=SEED)
        ev.process(s.u[:120], s.i[:120], s.r[:120])
        assert ev.first_event == 120
        ev.process(s.u[120:SPLIT], s.i[120:SPLIT], s.r[120:SPLIT])
        assert ev.first_event == SPLIT and ev.events == SPLIT
        b.online_update_sampled(s.u[:SPLIT], s.i[:SPLIT], s.r[:SPLIT], 5, NEG_RATING, SEED, 0)
        assert same_model(model(a), model(b))


@functools.lru_cache(maxsize=None)
def grouped_stream():
    """200 users and 100 items in 4 groups (user u in group u % 4, items 25 g .. 25 g + 24); 20,000 events,
    the user uniform, the item uniform over the items of the user's group."""
    rng = np.random.default_rng(3)
    u = rng.integers(0, 200, 20000).astype(np.int32)
    i = ((u % 4) * 25 + rng.integers(0, 25, 20000)).astype(np.int32)
    return u, i, np.ones(20000)


@pytest.mark.parametrize("mode", [F32, F64], ids=["f32", "f64"])
def test_it_learns_from_implicit_feedback(mode):
    """Every target is 1: without negatives the updates push every p.q towards 1 and the ranking stays at
    chance (hit rate at 10 of 100 items: 0.1; the ceiling is 10 / 25 = 0.4).  With 5 sampled negatives
    per event the hit rate over the second half of the stream must be at least twice that and at least 0.2
    (a numpy f64 replay of this rule gave 0.379 against 0.066)."""
    u, i, r = grouped_stream()
    rates = []
    for negatives in (0, 5):
        with context(None, mode, 8, lr=0.05) as ctx:
            hits = evaluated = 0
            for b in range(40):
                sl = slice(500 * b, 500 * b + 500)
                if negatives:
                    rec = ctx.online_prequential_sampled(u[sl], i[sl], r[sl], 10, negatives, 0.0, SEED, 500 * b)
                else:
                    rec = ctx.online_prequential(u[sl], i[sl], r[sl], 10)
                if b >= 20:
                    hits += rec.hits
                    evaluated += rec.evaluated
            rates.append(hits / evaluated)
    print("hit rate at 10, batches 20..39: without negatives", rates[0], "with 5 negatives", rates[1])
    assert rates[1] >= 2 * rates[0] and rates[1] >= 0.2
