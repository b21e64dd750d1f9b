"""mf_similar / mf_recommend_vectors on the device: nearest rows of the same side, and top-N for vectors
the model does not hold, by dot product or cosine (csrc/kernels_recommend.hip, COS instances).

The oracle is existing, tested code plus numpy: a *twin* context holds the same ids and the same vectors on
both sides, so mf_recommend (user queries) and mf_pair_ranks(..., scores) give the DOT value of any (a, b)
pair of rows bit for bit.  The cosine is replayed on the host from those dots exactly as include/mfhip.h
defines it: nn by the sequential chain (online_emu.fma32 in fast mode, nn + x*x in numpy f64 in
deterministic mode), inv = 1 / sqrt((double)nn) in f64 (rounded once to f32 in fast mode), score =
dot * (inv(q) * inv(c)) with each multiply rounded in the context's precision.  Every comparison is of
ids, counts and the scores' 64-bit patterns."""
import numpy as np
import pytest

import mfhip
from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context
from online_emu import fma32

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
METRICS = [L.METRIC_DOT, L.METRIC_COSINE]
ITEM, USER = L.SIDE_ITEM, L.SIDE_USER

# (k, rows, queries, top_n): both VEC instances (k % 4), the three NW instances (top_n <= 16, <= 48, above), a
# second query block (70 queries over the 64- and 32-query tiles), top_n above the row count, k = 1 and 256
SHAPES = [(1, 2, 2, 1), (3, 33, 33, 10), (10, 129, 70, 128), (64, 1000, 70, 10), (100, 1000, 33, 48),
          (130, 257, 5, 17), (256, 300, 40, 1)]


def make_ctx(k, mode):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    return Context(p)


def shuffled_ids(rng, n, scale=3):
    """n distinct ids, about half of them negative, in random order (row order is call order)."""
    return (rng.permutation(n).astype(np.int32) - n // 2) * scale + 1


def held(X, mode):
    """The rows as a context of this mode holds them, widened back to f64."""
    X = np.ascontiguousarray(X, np.float64)
    return X.astype(np.float32).astype(np.float64) if mode == L.MODE_FAST_F32 else X


def twin(k, mode, ids, X):
    ctx = make_ctx(k, mode)
    ctx.set_factors(USER, ids, X)
    ctx.set_factors(ITEM, ids, X)
    return ctx


def dot_grid(tw, qids, ids):
    """DOT of every (query, row) pair as mf_recommend reports it: the twin's mf_pair_ranks scores."""
    q = np.repeat(qids, len(ids)).astype(np.int32)
    c = np.tile(ids, len(qids)).astype(np.int32)
    ranks, _, sc = tw.pair_ranks(q, c, side=USER, scores=True)
    assert (ranks >= 0).all()
    return sc.reshape(len(qids), len(ids))


def inv_norms(X, mode):
    """inv(x) per row as the header defines it; X as held().  f32 values come back widened."""
    n, k = X.shape
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if mode == L.MODE_FAST_F32:
            x = X.astype(np.float32)
            nn = np.zeros(n, np.float32)
            for f in range(k):
                nn = fma32(x[:, f], x[:, f], nn)
            return (1.0 / np.sqrt(nn.astype(np.float64))).astype(np.float32)
        nn = np.zeros(n, np.float64)
        for f in range(k):
            nn = nn + X[:, f] * X[:, f]
        return 1.0 / np.sqrt(nn)


def as_reported(s):
    """A score as the merge writes it: f64, NaN canonical, -0 as +0."""
    s = np.asarray(s).astype(np.float64)
    s[s == 0] = 0.0
    s[np.isnan(s)] = np.nan
    return s


def scale(dots, inv_q, inv_c, mode):
    """score = dot * (inv(q) * inv(c)), each multiply rounded in the context's precision."""
    T = np.float32 if mode == L.MODE_FAST_F32 else np.float64
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return as_reported(dots.astype(T) * (inv_q.astype(T)[:, None] * inv_c.astype(T)[None, :]))


def lists(scores, cids, top_n, excluded=None):
    """(ids, scores, counts) as the calls lay them out; excluded: per query a bool mask over cids."""
    nq = scores.shape[0]
    ids = np.zeros((nq, top_n), np.int32)
    sc = np.zeros((nq, top_n), np.float64)
    cnt = np.zeros(nq, np.int32)
    for j in range(nq):
        keep = np.ones(len(cids), bool) if excluded is None else ~excluded[j]
        cj, sj = cids[keep], scores[j][keep]
        order = np.lexsort((cj, -sj))[:top_n]  # score descending, ties by id ascending, NaN last
        cnt[j] = len(order)
        ids[j, :len(order)] = cj[order]
        sc[j, :len(order)] = sj[order]
    return ids, sc, cnt


def replay_scores(k, mode, ids, X, qids, metric):
    """The full [query][row] score grid of `metric` for the rows (ids, X), through a twin of its own."""
    Xh = held(X, mode)
    with twin(k, mode, ids, Xh) as tw:
        dots = dot_grid(tw, qids, ids)
    if metric == L.METRIC_DOT:
        return dots
    inv = inv_norms(Xh, mode)
    row = {int(v): x for x, v in enumerate(ids)}
    return scale(dots, inv[[row[int(q)] for q in qids]], inv, mode)


def self_mask(ids, qids):
    return ids[None, :] == np.asarray(qids)[:, None]


def assert_same(got, want):
    ids, sc, cnt = got
    rids, rsc, rcnt = want
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(ids, rids)
    assert np.array_equal(sc.view(np.uint64), rsc.view(np.uint64))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,nq,top_n", SHAPES)
def test_dot_equals_recommend_on_the_twin(mode, k, rows, nq, top_n):
    rng = np.random.default_rng(100 * k + rows)
    ids = shuffled_ids(rng, rows)
    with twin(k, mode, ids, rng.standard_normal((rows, k))) as tw:
        q = rng.choice(ids, nq, replace=False)
        assert_same(tw.similar(q, top_n, side=ITEM, metric=L.METRIC_DOT, include_self=True),
                    tw.recommend(q, top_n, side=USER))
        assert_same(tw.similar(q, top_n, side=USER, metric=L.METRIC_DOT, include_self=True),
                    tw.recommend(q, top_n, side=ITEM))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,nq,top_n", SHAPES)
def test_cosine_equals_the_host_replay(mode, k, rows, nq, top_n):
    rng = np.random.default_rng(200 * k + rows)
    ids = shuffled_ids(rng, rows)
    X = rng.standard_normal((rows, k))
    q = rng.choice(ids, nq, replace=False)
    want = replay_scores(k, mode, ids, X, q, L.METRIC_COSINE)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(ITEM, ids, X)
        ctx.set_factors(USER, ids[:1], X[:1])
        assert_same(ctx.similar(q, top_n, side=ITEM, include_self=True), lists(want, ids, top_n))
        assert_same(ctx.similar(q, top_n, side=ITEM), lists(want, ids, top_n, self_mask(ids, q)))
        if k > 1:  # at k = 1 every cosine is +-1: nothing to bound
            sc = ctx.similar(q, top_n, side=ITEM)[1]
            assert (np.abs(sc) <= 1.0 + k * 2.0 ** (-23 if mode == L.MODE_FAST_F32 else -52)).all()


@pytest.mark.parametrize("mode", MODES)
def test_specials(mode):
    """Zero rows (NaN, last, id ascending among them), a row with its copies scaled by 2^40 and 2^-40 (powers of
    two go through the square root and the division exactly, so all three tie and the id decides; no f32
    denormal is involved), and two identical rows."""
    rng = np.random.default_rng(31)
    k, n = 8, 40
    ids = shuffled_ids(rng, n)
    X = rng.standard_normal((n, k))
    z1, z2, a, big, small, b1, b2 = 3, 17, 5, 22, 30, 9, 35
    X[z1] = X[z2] = 0.0
    X[big], X[small] = X[a] * 2.0 ** 40, X[a] * 2.0 ** -40
    X[b2] = X[b1]
    want = replay_scores(k, mode, ids, X, ids, L.METRIC_COSINE)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(USER, ids, X)
        got = ctx.similar(ids, n, side=USER, include_self=True)
        assert_same(got, lists(want, ids, n))
        gi, gs, gc = got
        assert (gc == n).all()
        zeros = sorted([int(ids[z1]), int(ids[z2])])
        for j in range(n):
            if j in (z1, z2):  # a zero query: every score NaN, so the list is the ids ascending
                assert np.isnan(gs[j]).all() and gi[j].tolist() == sorted(ids.tolist())
                continue
            assert gi[j, -2:].tolist() == zeros and np.isnan(gs[j, -2:]).all()
            assert not np.isnan(gs[j, :-2]).any()
            at = {int(c): x for x, c in enumerate(gi[j])}
            trio = sorted(int(ids[r]) for r in (a, big, small))
            pos = [at[c] for c in trio]
            assert pos == list(range(pos[0], pos[0] + 3))  # adjacent, in id order
            assert len({gs[j, p].tobytes() for p in pos}) == 1
            pair = sorted(int(ids[r]) for r in (b1, b2))
            assert at[pair[1]] == at[pair[0]] + 1 and gs[j, at[pair[0]]] == gs[j, at[pair[1]]]


@pytest.mark.parametrize("mode", MODES)
def test_self(mode, monkeypatch):
    rng = np.random.default_rng(41)
    k, rows = 16, 257
    ids = shuffled_ids(rng, rows)
    X = rng.standard_normal((rows, k))
    q = ids[[0, 127, 128, 256]]
    want = {m: replay_scores(k, mode, ids, X, q, m) for m in METRICS}
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(ITEM, ids, X)
        for split in (1, 3):
            set_knob(monkeypatch, "rec_split", split)
            for metric in METRICS:
                for top_n in (10, 128):
                    out = ctx.similar(q, top_n, side=ITEM, metric=metric)
                    assert_same(out, lists(want[metric], ids, top_n, self_mask(ids, q)))
                    assert (out[2] == min(top_n, rows - 1)).all()
                    for j in range(len(q)):
                        assert int(q[j]) not in out[0][j].tolist()
                    assert_same(ctx.similar(q, top_n, side=ITEM, metric=metric, include_self=True),
                                lists(want[metric], ids, top_n))
            first = ctx.similar(q, 3, side=ITEM, include_self=True)
            assert np.array_equal(first[0][:, 0], q)
    # rows - 1 - exclusions below top_n, and a side of one row
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(USER, ids[:20], X[:20])
        ex = (np.array([ids[0]] * 3, np.int32), ids[[4, 5, 6]])
        out = ctx.similar(ids[:2], 128, side=USER, exclude=ex)
        assert out[2].tolist() == [20 - 1 - 3, 20 - 1]
        assert not out[0][0, 16:].any() and not out[1][0, 16:].any()
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(USER, ids[:1], X[:1])
        ctx.set_factors(ITEM, ids[:3], X[:3])
        for metric in METRICS:
            i1, s1, c1 = ctx.similar([ids[0], 424242], 5, side=USER, metric=metric)
            assert c1.tolist() == [0, 0] and not i1.any() and not s1.any()
        i1, _, c1 = ctx.similar(ids[:1], 5, side=USER, include_self=True)
        assert c1.tolist() == [1] and i1[0, 0] == ids[0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("metric", METRICS)
def test_exclusions(mode, metric):
    rng = np.random.default_rng(51)
    k, rows, nq, top_n = 10, 60, 33, 16
    ids = shuffled_ids(rng, rows)
    X = rng.standard_normal((rows, k))
    q = ids[:nq].copy()
    want = replay_scores(k, mode, ids, X, q, metric)
    excl = rng.random((nq, rows)) < 0.3
    excl[0, :] = True    # every candidate excluded: count 0
    excl[1, :] = True
    excl[1, 40:45] = False  # five left
    excl[2, :] = False
    excl[3, 3] = True    # the self pair, given explicitly
    qq, cc = np.nonzero(excl)
    eq, ec = q[qq], ids[cc]
    # duplicates, unknown ids on either side, and a pair of a query that is not asked
    eq = np.concatenate([eq, eq[:9], [999999, q[2], ids[-1]]]).astype(np.int32)
    ec = np.concatenate([ec, ec[:9], [ids[0], 888888, ids[0]]]).astype(np.int32)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(ITEM, ids, X)
        got = ctx.similar(q, top_n, side=ITEM, metric=metric, exclude=(eq, ec))
        mask = excl | self_mask(ids, q)
        assert_same(got, lists(want, ids, top_n, mask))
        assert got[2][0] == 0 and got[2][1] == 5 and got[2][2] == top_n
        assert np.array_equal(got[2], np.minimum(top_n, rows - mask.sum(1)))
        # include_self = 1 with the self pair excluded all the same: query 3 still does not see itself
        got = ctx.similar(q, top_n, side=ITEM, metric=metric, include_self=True, exclude=(eq, ec))
        assert_same(got, lists(want, ids, top_n, excl))
        assert int(q[3]) not in got[0][3].tolist()


@pytest.mark.parametrize("mode", MODES)
def test_geometry_independence(mode, monkeypatch):
    rng = np.random.default_rng(61)
    k, rows, nq, top_n = 20, 300, 130, 10
    ids = shuffled_ids(rng, rows)
    X = rng.standard_normal((rows, k))
    q = rng.choice(ids, nq, replace=False)
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(ITEM, ids, X)
        base = {m: ctx.similar(q, top_n, side=ITEM, metric=m) for m in METRICS}
        vbase = {m: ctx.recommend_vectors(held(X[:nq], mode), top_n, side=ITEM, metric=m) for m in METRICS}
        for batch in (1, 7):
            for split in (1, 3, 64):
                set_knob(monkeypatch, "rec_batch", batch)
                set_knob(monkeypatch, "rec_split", split)
                for m in METRICS:
                    assert_same(ctx.similar(q, top_n, side=ITEM, metric=m), base[m])
        set_knob(monkeypatch, "rec_batch", 7)
        set_knob(monkeypatch, "rec_split", 3)
        for m in METRICS:
            assert_same(ctx.recommend_vectors(held(X[:nq], mode), top_n, side=ITEM, metric=m), vbase[m])
        # duplicate query ids each take their row's result
        dup = np.concatenate([q[:5], q[:5], q[3:4]])
        out = ctx.similar(dup, top_n, side=ITEM)
        for j, src in enumerate([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 3]):
            assert np.array_equal(out[0][j], base[L.METRIC_COSINE][0][src])
            assert np.array_equal(out[1][j].view(np.uint64), base[L.METRIC_COSINE][1][src].view(np.uint64))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [1, 33, 130])
def test_vectors(mode, nq):
    rng = np.random.default_rng(70 + nq)
    k, ni, top_n = 12, 150, 20
    uids, iids = shuffled_ids(rng, 130), shuffled_ids(rng, ni, 5)
    P, Q = rng.standard_normal((130, k)), rng.standard_normal((ni, k))
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(USER, uids, P)
        ctx.set_factors(ITEM, iids, Q)
        users = uids[:nq]
        vecs, found = ctx.lookup(USER, users)
        assert found.all()
        assert_same(ctx.recommend_vectors(vecs, top_n, side=ITEM, metric=L.METRIC_DOT), ctx.recommend(users, top_n))
        # the unrounded f64 vectors convert as set_factors converted them
        assert_same(ctx.recommend_vectors(P[:nq], top_n, side=ITEM), ctx.recommend(users, top_n))
        # exclusions by position; positions outside [0, nq) are ignored
        pos = rng.integers(0, nq, 40)
        cand = rng.choice(iids, 40)
        xq = np.concatenate([pos, [-1, nq, 2 ** 40]]).astype(np.int64)
        xc = np.concatenate([cand, iids[:3]]).astype(np.int32)
        assert_same(ctx.recommend_vectors(vecs, top_n, side=ITEM, exclude=(xq, xc)),
                    ctx.recommend(users, top_n, exclude=(users[pos], cand)))
    # cosine on a twin: a row's vector as a query is the row as a query, itself included
    ids = iids
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(ITEM, ids, Q)
        q = ids[:nq]
        vecs, _ = ctx.lookup(ITEM, q)
        for m in METRICS:
            assert_same(ctx.recommend_vectors(vecs, top_n, side=ITEM, metric=m),
                        ctx.similar(q, top_n, side=ITEM, metric=m, include_self=True))
        # a NaN entry: every score of that query is NaN, so the ids come back ascending
        vecs = vecs.copy()
        vecs[0, k // 2] = np.nan
        for m in METRICS:
            gi, gs, gc = ctx.recommend_vectors(vecs, top_n, side=ITEM, metric=m)
            assert gc[0] == top_n and np.isnan(gs[0]).all()
            assert gi[0].tolist() == sorted(ids.tolist())[:top_n]
        empty = ctx.recommend_vectors(np.zeros((0, k)), 5, side=ITEM)
        assert empty[0].shape == (0, 5) and empty[2].shape == (0,)


@pytest.mark.parametrize("mode", MODES)
def test_symmetry(mode):
    rng = np.random.default_rng(81)
    k, n = 37, 40
    ids = np.sort(shuffled_ids(rng, n))
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(USER, ids, rng.standard_normal((n, k)) * np.exp(rng.standard_normal((n, 1)) * 3))
        gi, gs, gc = ctx.similar(ids, n, side=USER, include_self=True)
        assert (gc == n).all()
        S = np.zeros((n, n), np.uint64)
        for j in range(n):
            S[j, np.searchsorted(ids, gi[j])] = gs[j].view(np.uint64)
        assert np.array_equal(S, S.T)


@pytest.mark.parametrize("mode", MODES)
def test_freshness(mode):
    """Norms are taken per call: a changed row, new rows and an online batch show in the next call."""
    rng = np.random.default_rng(91)
    k, rows, top_n = 10, 50, 12
    ids = shuffled_ids(rng, rows)
    X = rng.standard_normal((rows, k))

    def check(ctx):
        cur, vecs = ctx.factors(ITEM)
        want = replay_scores(k, mode, cur, vecs, cur, L.METRIC_COSINE)
        assert_same(ctx.similar(cur, top_n, side=ITEM), lists(want, cur, top_n, self_mask(cur, cur)))
        return cur, vecs

    with make_ctx(k, mode) as ctx:
        ctx.set_factors(ITEM, ids, X)
        ctx.set_factors(USER, ids[:5], X[:5])
        check(ctx)
        new_ids = np.array([ids[7], 70001, -70002], np.int32)
        ctx.set_factors(ITEM, new_ids, rng.standard_normal((3, k)) * 5)
        cur, _ = check(ctx)
        assert len(cur) == rows + 2
        before = ctx.lookup(ITEM, ids[:3])[0].copy()
        ctx.online_update(np.array([ids[0], ids[1], ids[2]], np.int32), np.array([ids[0], ids[1], 80003], np.int32),
                          np.array([4.0, 1.0, 5.0]))
        cur, _ = check(ctx)
        assert len(cur) == rows + 3 and 80003 in cur.tolist()
        assert not np.array_equal(ctx.lookup(ITEM, ids[:3])[0], before)


def test_mirror_api():
    d = mfhip.synth.generate(300, 120, 6000, seed=3)
    sgd = mfhip.DSGDforMF().setNumFactors(16).setIterations(2).setBlocks(3).setSeed(11)
    sgd.fit((d.u, d.i, d.r))
    ctx = sgd.context
    item, user = int(d.i[0]), int(d.u[0])
    ids, sc, cnt = ctx.similar([item], 7, side=ITEM)
    assert sgd.similarProducts(item, 7) == [(int(ids[0, x]), float(sc[0, x])) for x in range(cnt[0])]
    ids, sc, cnt = ctx.similar([user], 7, side=USER, metric=L.METRIC_DOT)
    assert sgd.similarUsers(user, 7, metric=L.METRIC_DOT) == [(int(ids[0, x]), float(sc[0, x])) for x in range(cnt[0])]
    assert item not in [t[0] for t in sgd.similarProducts(item, 7)]
