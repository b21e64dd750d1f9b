"""mf_recommend_among on the device: the top N within caller-given candidate lists (csrc/kernels_among.hip for
per-query lists, the MAP instances of csrc/kernels_recommend.hip over a gathered slab for one shared list).

The oracle is the header's definition, run through existing, tested code: position j must hold what
mf_recommend on the same context returns for queries[j] alone when given the complement of list j as
exclusion pairs, plus the call's own exclusions or the seen pairs.  Every comparison is of ids, counts and the
scores' 64-bit patterns.  Rows <= 1000 and queries <= 70 keep a complement under ~70k pairs."""
import numpy as np
import pytest

import mfhip
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
ITEM, USER = L.SIDE_ITEM, L.SIDE_USER
SIDES = [USER, ITEM]

# (k, rows, queries, top_n): k = 1, 3, 64, 100, 130, 256 (one chunk of a cache line, a partial one, several, a
# partial last one; both VEC instances of the shared path), top_n = 1, 10, 48, 128 (the three NW instances),
# top_n above the list length (lists are at most `rows` long, often far shorter), 70 queries = a second
# query tile of the shared path and 18 workgroups of the per-query one
SHAPES = [(1, 5, 4, 1), (3, 33, 33, 10), (64, 1000, 70, 10), (100, 300, 33, 48), (130, 257, 5, 128),
          (256, 300, 40, 17)]


def make_ctx(k, mode):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    return Context(p)


def shuffled_ids(rng, n, scale=3):
    """n distinct ids, about half of them negative, in random order (row order is call order)."""
    return (rng.permutation(n).astype(np.int32) - n // 2) * scale + 1


class Model:
    """A context with `rows` rows on both sides, so either side can ask."""

    def __init__(self, k, rows, mode, rng, X=None, Y=None):
        self.uid, self.iid = shuffled_ids(rng, rows), shuffled_ids(rng, rows, scale=5)
        self.ctx = make_ctx(k, mode)
        self.ctx.set_factors(USER, self.uid, rng.standard_normal((rows, k)) if X is None else X)
        self.ctx.set_factors(ITEM, self.iid, rng.standard_normal((rows, k)) if Y is None else Y)

    def ids(self, side):
        return self.uid if side == USER else self.iid

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()


def oracle(m, side, queries, top_n, lists, exclude=None, seen_pairs=None):
    """mf_recommend per position with the complement of its list as exclusion pairs (plus `exclude`, plus the
    seen pairs given as (query-side ids, candidate-side ids))."""
    cids = m.ids(1 - side)
    ids = np.zeros((len(queries), top_n), np.int32)
    sc = np.zeros((len(queries), top_n), np.float64)
    cnt = np.zeros(len(queries), np.int32)
    for j, q in enumerate(queries):
        comp = np.setdiff1d(cids, np.asarray(lists[j], np.int32)).astype(np.int32)
        eq = [np.full(len(comp), q, np.int32)]
        ec = [comp]
        for extra in (exclude, seen_pairs):
            if extra is not None:
                eq.append(np.asarray(extra[0], np.int32))
                ec.append(np.asarray(extra[1], np.int32))
        a, b, c = m.ctx.recommend([q], top_n, side=side, exclude=(np.concatenate(eq), np.concatenate(ec)))
        ids[j], sc[j], cnt[j] = a[0], b[0], c[0]
    return ids, sc, cnt


def pack(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    cand = np.concatenate([np.asarray(x, np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return cand.astype(np.int32), off


def among(m, side, queries, top_n, lists, **kw):
    cand, off = pack(lists)
    return m.ctx.recommend_among(queries, top_n, cand, offsets=off, side=side, **kw)


def assert_same(got, want):
    ids, sc, cnt = got
    rids, rsc, rcnt = want
    print("counts", cnt.tolist(), "want", rcnt.tolist())
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(ids, rids)
    assert np.array_equal(sc.view(np.uint64), rsc.view(np.uint64))


def random_lists(rng, cids, nq, max_len):
    """Lists of random lengths 0 .. max_len drawn with replacement (so ids repeat), every fifth entry or so an id
    the model does not hold."""
    out = []
    for _ in range(nq):
        x = rng.choice(cids, int(rng.integers(0, max_len + 1)), replace=True).astype(np.int32)
        x[rng.random(len(x)) < 0.2] += 1  # ids are 1 mod the scale: these are unknown
        out.append(x)
    return out


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,nq,top_n", SHAPES)
def test_per_query_lists_equal_recommend_with_the_complement_excluded(mode, side, k, rows, nq, top_n):
    rng = np.random.default_rng(1000 * k + rows + side)
    with Model(k, rows, mode, rng) as m:
        q = rng.choice(m.ids(side), nq, replace=False)
        lists = random_lists(rng, m.ids(1 - side), nq, min(rows, 200))
        assert_same(among(m, side, q, top_n, lists), oracle(m, side, q, top_n, lists))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,nq,top_n", SHAPES)
def test_shared_list_equals_recommend_with_the_complement_excluded(mode, side, k, rows, nq, top_n):
    rng = np.random.default_rng(2000 * k + rows + side)
    with Model(k, rows, mode, rng) as m:
        q = rng.choice(m.ids(side), nq, replace=False)
        shared = random_lists(rng, m.ids(1 - side), 1, rows)[0]
        got = m.ctx.recommend_among(q, top_n, shared, side=side)
        assert_same(got, oracle(m, side, q, top_n, [shared] * nq))


@pytest.mark.parametrize("mode", MODES)
def test_list_lengths_repeats_unknowns_and_parts(mode, monkeypatch):
    """One call: empty, one entry, 63 / 64 / 65 entries, every id, ids repeated inside a part and across parts,
    unknown ids, an unknown query, the same query twice with different lists, a list longer than 64 * 64
    entries built from repeats -- with among_chunk = 64 that list caps the parts at 64 and lengthens them -- and
    one of exactly 64 * 64 entries, 64 parts of 64.  The
    results under among_chunk = 64, under the default and in batches of 3 positions are identical, and equal
    the oracle."""
    rng = np.random.default_rng(7)
    k, rows, top_n = 20, 700, 10
    with Model(k, rows, mode, rng) as m:
        cids = m.iid
        inside = np.concatenate([cids[:20], cids[:20], cids[5:9]])                # repeated inside one 64-part
        across = np.concatenate([cids[100:190], cids[100:190], cids[150:160]])    # ... and across parts
        long_list = np.tile(cids[:600], 7)[:64 * 64 + 37]                         # 4133 entries, 600 distinct
        exact = np.tile(cids[50:690], 7)[:64 * 64]                                # 64 parts of 64 at among_chunk = 64
        lists = [np.zeros(0, np.int32), cids[3:4], cids[:63], cids[10:74], cids[20:85], cids, inside, across,
                 np.array([cids[0] + 1, cids[1] + 1], np.int32), np.concatenate([[cids[2] + 1], cids[:5]]),
                 cids[:50], cids[40:45], cids[300:420], long_list, exact]
        q = np.concatenate([m.uid[:10], [m.uid[0] + 1], m.uid[4:5], m.uid[4:5], m.uid[11:13]]).astype(np.int32)
        assert len(q) == len(lists) and q[11] == q[12] == q[4]
        want = oracle(m, USER, q, top_n, lists)
        assert want[2].tolist() == [0, 1, 10, 10, 10, 10, 10, 10, 0, 5, 0, 5, 10, 10, 10]
        default = among(m, USER, q, top_n, lists)
        assert_same(default, want)
        set_knob(monkeypatch, "among_chunk", 64)
        assert_same(among(m, USER, q, top_n, lists), want)
        set_knob(monkeypatch, "among_batch", 3)
        assert_same(among(m, USER, q, top_n, lists), want)
        # top_n above every list's distinct count but the longest ones'
        assert_same(among(m, USER, q, 128, lists), oracle(m, USER, q, 128, lists))


@pytest.mark.parametrize("mode", MODES)
def test_ties_and_specials(mode, monkeypatch):
    """Duplicated factor rows (equal scores fall back to the id), rows holding NaN, +-inf and -0, and a duplicated
    id whose score is NaN -- per-query lists (cut into parts of 64) and the shared list."""
    rng = np.random.default_rng(11)
    k, rows, top_n = 8, 200, 128
    Y = rng.standard_normal((rows, k))
    Y[10:60] = Y[5]               # fifty ties
    Y[70] = np.nan
    Y[71, 3] = np.nan
    Y[72, 0], Y[73, 0] = np.inf, -np.inf
    Y[74] = -0.0
    Y[75] = 0.0
    X = rng.standard_normal((rows, k))
    X[1] = 0.0                    # every score +-0 (or NaN against inf)
    X[2] = -X[0]
    with Model(k, rows, mode, rng, X=X, Y=Y) as m:
        q = m.uid[:6]
        cids = m.iid
        special = np.concatenate([cids[70:76], cids[70:72], cids[5:60], cids[70:71], cids[100:130], cids[72:74]])
        lists = [special, special[::-1].copy(), cids, np.tile(cids[70:72], 40), special, cids[60:80]]
        want = oracle(m, USER, q, top_n, lists)
        assert_same(among(m, USER, q, top_n, lists), want)
        set_knob(monkeypatch, "among_chunk", 64)
        assert_same(among(m, USER, q, top_n, lists), want)
        assert_same(among(m, USER, q, 10, lists), oracle(m, USER, q, 10, lists))
        assert_same(m.ctx.recommend_among(q, top_n, special, side=USER), oracle(m, USER, q, top_n, [special] * 6))
        assert_same(m.ctx.recommend_among(q, 7, special, side=USER), oracle(m, USER, q, 7, [special] * 6))


def test_f32_subnormal_products_follow_recommend():
    """Fast mode: the per-query kernel's fmaf chain against the f32-input MFMA of mf_recommend where products
    and sums are f32 subnormals (factors around 2^-70, so a product is around 2^-140) and where one factor is
    itself subnormal."""
    rng = np.random.default_rng(13)
    k, rows, top_n = 12, 150, 20
    X = rng.standard_normal((rows, k)) * 2.0 ** -70
    Y = rng.standard_normal((rows, k)) * 2.0 ** -70
    Y[:30] *= 2.0 ** -60          # subnormal inputs (2^-130)
    X[:5] *= 2.0 ** 60            # ... against normal ones: products near 2^-140 again
    with Model(k, rows, L.MODE_FAST_F32, rng, X=X, Y=Y) as m:
        q = m.uid[:12]
        lists = [m.iid[rng.permutation(rows)[:100]] for _ in q]
        want = oracle(m, USER, q, top_n, lists)
        assert np.unique(want[1]).size > 20, "the scores must not all have collapsed to zero"
        assert_same(among(m, USER, q, top_n, lists), want)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_exclusions(mode, side):
    """The call's arrays (naming listed and unlisted candidates, unknown ids, and queries not asked), the
    resident seen set, and exclude_seen with no set -- per-query lists and the shared list."""
    rng = np.random.default_rng(17 + side)
    k, rows, nq, top_n = 16, 120, 9, 10
    with Model(k, rows, mode, rng) as m:
        qids, cids = m.ids(side), m.ids(1 - side)
        q = np.concatenate([qids[:nq - 1], qids[:1]]).astype(np.int32)  # the first query twice
        lists = [cids[rng.permutation(rows)[:30]] for _ in q]
        shared = cids[rng.permutation(rows)[:40]]
        # pairs: half of every list, twenty unlisted candidates per query, unknown ids, a query not asked
        eq = np.concatenate([np.repeat(q, 15), np.repeat(q, 20), [q[0], q[0] + 1, qids[50]]]).astype(np.int32)
        ec = np.concatenate([np.concatenate([x[:15] for x in lists]), np.tile(cids[:20], len(q)),
                             [cids[0] + 1, cids[1], lists[0][20]]]).astype(np.int32)
        excl = (eq, ec)
        got = among(m, side, q, top_n, lists, exclude=excl)
        assert_same(got, oracle(m, side, q, top_n, lists, exclude=excl))
        assert not np.array_equal(got[0], among(m, side, q, top_n, lists)[0])
        assert_same(m.ctx.recommend_among(q, top_n, shared, side=side, exclude=excl),
                    oracle(m, side, q, top_n, [shared] * len(q), exclude=excl))
        # exclude_seen with no set: no exclusions
        assert m.ctx.seen_count() == 0
        assert_same(among(m, side, q, top_n, lists, seen=True), oracle(m, side, q, top_n, lists))
        assert_same(m.ctx.recommend_among(q, top_n, shared, side=side, seen=True),
                    oracle(m, side, q, top_n, [shared] * len(q)))
        # the seen set is (user, item) pairs whichever side asks
        su, si = (eq, ec) if side == USER else (ec, eq)
        m.ctx.seen_set(su, si)
        assert m.ctx.seen_count() > 0
        want = oracle(m, side, q, top_n, lists, seen_pairs=excl)
        assert_same(among(m, side, q, top_n, lists, seen=True), want)
        assert_same(among(m, side, q, top_n, lists, exclude=L.SEEN), want)
        assert_same(m.ctx.recommend_among(q, top_n, shared, side=side, seen=True),
                    oracle(m, side, q, top_n, [shared] * len(q), seen_pairs=excl))


@pytest.mark.parametrize("split", [1, 3, None])
@pytest.mark.parametrize("mode", MODES)
def test_shared_list_under_batches_and_splits(mode, split, monkeypatch):
    """The shared list given shuffled and with repeats, in batches of 7 queries, with the gathered slab walked in
    1 split, in 3, and in the default number."""
    rng = np.random.default_rng(19)
    k, rows, nq, top_n = 24, 500, 30, 10
    with Model(k, rows, mode, rng) as m:
        q = np.concatenate([m.uid[:nq - 2], [m.uid[0] + 1], m.uid[3:4]]).astype(np.int32)  # an unknown, a repeat
        shared = rng.permutation(np.concatenate([m.iid[:300], m.iid[100:200], m.iid[:3] + 1])).astype(np.int32)
        want = oracle(m, USER, q, top_n, [shared] * nq)
        assert want[2][nq - 2] == 0
        set_knob(monkeypatch, "rec_batch", 7)
        if split is not None:
            set_knob(monkeypatch, "rec_split", split)
        assert_same(m.ctx.recommend_among(q, top_n, shared, side=USER), want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,nq,top_n", [(3, 33, 33, 10), (64, 1000, 70, 48), (130, 257, 5, 128)])
def test_shared_and_per_query_paths_agree(mode, k, rows, nq, top_n):
    """A shared list and that same list repeated per query return identical bytes (fast mode: the f32-input MFMA
    against the fmaf chain)."""
    rng = np.random.default_rng(23 + k)
    with Model(k, rows, mode, rng) as m:
        q = rng.choice(m.uid, nq, replace=True).astype(np.int32)
        shared = random_lists(rng, m.iid, 1, rows)[0]
        a = m.ctx.recommend_among(q, top_n, shared, side=USER)
        b = among(m, USER, q, top_n, [shared] * nq)
        assert_same(a, b)
        assert a[2].max() > 0


@pytest.mark.parametrize("mode", MODES)
def test_nothing_in_the_context_changes(mode):
    rng = np.random.default_rng(29)
    k, rows = 10, 90
    with Model(k, rows, mode, rng) as m:
        m.ctx.seen_set(m.uid[:40], m.iid[:40])
        before = (m.ctx.factors(USER), m.ctx.factors(ITEM), m.ctx.seen_count(), m.ctx.recommend(m.uid[:20], 10))
        lists = random_lists(rng, m.iid, 20, 60)
        among(m, USER, m.uid[:20], 10, lists)
        among(m, USER, m.uid[:20], 10, lists, seen=True)
        m.ctx.recommend_among(m.iid[:20], 10, m.uid[:50], side=ITEM, seen=True)
        after = (m.ctx.factors(USER), m.ctx.factors(ITEM), m.ctx.seen_count(), m.ctx.recommend(m.uid[:20], 10))
        for (bi, bv), (ai, av) in zip(before[:2], after[:2]):
            assert np.array_equal(bi, ai) and np.array_equal(bv.view(np.uint64), av.view(np.uint64))
        assert before[2] == after[2] == 40
        assert_same(after[3], before[3])


def test_empty_calls_and_the_model_wrapper():
    d = mfhip.synth.generate(300, 120, 6000, seed=3)
    sgd = mfhip.DSGDforMF().setNumFactors(16).setIterations(2).setBlocks(3).setSeed(11)
    sgd.fit((d.u, d.i, d.r))
    ctx = sgd.context
    users, items = np.unique(d.u)[:4].astype(np.int32), np.unique(d.i).astype(np.int32)
    # no query; no candidate at all (shared and per query)
    ids, sc, cnt = ctx.recommend_among(np.zeros(0, np.int32), 5, items[:10])
    assert ids.shape == (0, 5) and len(cnt) == 0
    for off in (None, np.zeros(5, np.int64)):
        ids, sc, cnt = ctx.recommend_among(users, 5, np.zeros(0, np.int32), offsets=off)
        assert not cnt.any() and not ids.any() and not sc.any()
    off = np.array([0, 10, 10, 30, 40], np.int64)
    ids, sc, cnt = ctx.recommend_among(users, 7, items[:40], offsets=off)
    got = sgd.recommendProductsAmong(users, 7, items[:40], offsets=off)
    assert got == {j: [(int(u), int(ids[j, x]), float(sc[j, x])) for x in range(cnt[j])] for j, u in enumerate(users)}
    assert [len(got[j]) for j in range(4)] == [7, 0, 7, 7]
    ids, sc, cnt = ctx.recommend_among(users, 7, items[:40])
    assert sgd.recommendProductsAmong(users, 7, items[:40]) == {
        j: [(int(u), int(ids[j, x]), float(sc[j, x])) for x in range(cnt[j])] for j, u in enumerate(users)}


@pytest.mark.parametrize("mode", MODES)
def test_lists_past_2_pow_24_entries_are_resolved_to_their_end(mode):
    """One list of more than 2^24 entries (the reach of one launch of the online id lookup), built from repeats of
    1,000 shuffled ids, about half negative, none equal to its row, with unknown ids among them; a short list
    before it and one behind it, whose entries lie past 2^24 in the upload; and the long list as a shared one.
    An entry left unresolved would be scored as the row that carries its id's number."""
    rng = np.random.default_rng(37)
    k, rows, top_n = 8, 1000, 10
    with Model(k, rows, mode, rng) as m:
        assert not np.array_equal(m.iid, np.arange(rows)) and (m.iid < 0).sum() > rows // 3
        base = np.concatenate([m.iid[100:900], m.iid[:50] + 1]).astype(np.int32)
        n = (1 << 24) + 1000
        long_list = np.tile(rng.permutation(base), n // len(base) + 1)[:n]
        long_list[-3:] = m.iid[950:953]  # three candidates named only at the very end
        lists = [m.iid[:30], long_list, m.iid[900:1000]]
        q = m.uid[:3]
        want = oracle(m, USER, q, top_n, lists)
        assert_same(among(m, USER, q, top_n, lists), want)
        assert_same(m.ctx.recommend_among(q, top_n, long_list, side=USER), oracle(m, USER, q, top_n, [long_list] * 3))
