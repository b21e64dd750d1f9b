"""mf_pair_ranks on the device (csrc/kernels_pairrank.hip, csrc/pair_rank.cpp): the position of given
(query, candidate) pairs in the query's complete ranked list.

Exact ranks.  Models with factor entries in {-2 .. 2} (set with mf_set_factors) give small integer scores
in f32 and f64 alike, with plenty of ties; the expected rank is counted with numpy,
#(s' > s) + #(s' == s and id' < id) over the non-excluded others, NaN below every number.  Against
mf_recommend.  Random factors: an event of rank r < 128 must be entry r of the query's 128-list with
the same score bits, one of rank >= 128 must be absent from it, and the whole order is recovered from
mf_recommend alone by peeling (three calls, each excluding what the earlier ones returned)."""
import numpy as np
import pytest

from conftest import set_knob
from mfhip import _lib as L
from mfhip.context import Context

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
COLD, EXCLUDED = L.PAIR_RANK_COLD, L.PAIR_RANK_EXCLUDED


def make_ctx(k, mode):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    return Context(p)


def shuffled_ids(rng, n, scale=3):
    """n distinct ids, about half of them negative, in random order (row order is call order)."""
    return (rng.permutation(n).astype(np.int32) - n // 2) * scale + 1


def chain_scores(P, Q):
    """s[a, b] = the chain over f ascending from 0 (exact for the small integers and specials used here)."""
    S = np.zeros((len(P), len(Q)))
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(P.shape[1]):
            S = S + np.outer(P[:, f], Q[:, f])
    return S


def expected(S, qids, cids, q, c, exclude):
    """(ranks, valid) by the definition: per event the non-excluded other candidates whose key beats it."""
    qpos = {int(x): a for a, x in enumerate(qids)}
    cpos = {int(x): b for b, x in enumerate(cids)}
    ex = np.zeros(S.shape, bool)
    if exclude is not None:
        for a, b in zip(exclude[0].tolist(), exclude[1].tolist()):
            if a in qpos and b in cpos:
                ex[qpos[a], cpos[b]] = True
    ranks, valid = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
    for j, (qa, cb) in enumerate(zip(q.tolist(), c.tolist())):
        if qa not in qpos or cb not in cpos:
            ranks[j] = COLD
            continue
        a, b = qpos[qa], cpos[cb]
        if ex[a, b]:
            ranks[j] = EXCLUDED
            continue
        s, t = S[a], S[a, b]
        first = cids < cids[b]
        if np.isnan(t):
            beat = ~np.isnan(s) | first
        else:
            with np.errstate(invalid="ignore"):
                beat = (s > t) | ((s == t) & first)
        beat &= ~ex[a]
        beat[b] = False
        ranks[j] = int(beat.sum())
        valid[j] = S.shape[1] - int(ex[a].sum())
    return ranks, valid


def int_model(rng, ctx, nq, nc, k, side):
    qids, cids = shuffled_ids(rng, nq), shuffled_ids(rng, nc, 5)
    P = rng.integers(-2, 3, (nq, k)).astype(np.float64)
    Q = rng.integers(-2, 3, (nc, k)).astype(np.float64)
    ctx.set_factors(side, qids, P)
    ctx.set_factors(1 - side, cids, Q)
    return qids, cids, P, Q


def events(rng, qids, cids, n):
    """n events over few distinct queries (they repeat within a wave's 32 columns), some repeated whole."""
    few = qids[: max(1, min(len(qids), 5))]
    q = rng.choice(few, n).astype(np.int32)
    c = rng.choice(cids, n).astype(np.int32)
    if n >= 4:
        q[-1], c[-1] = q[0], c[0]
        q[-2], c[-2] = q[1], c[1]
    return q, c


def exclusions(rng, qids, cids, frac=0.3):
    """~frac of the grid, duplicates, unknown ids on either side."""
    m = rng.random((len(qids), len(cids))) < frac
    a, b = np.nonzero(m)
    eq = np.concatenate([qids[a], qids[a][:5], [99_000_000, qids[0]]]).astype(np.int32)
    ec = np.concatenate([cids[b], cids[b][:5], [cids[0], 88_000_000]]).astype(np.int32)
    return eq, ec


# (k, candidates, events): every k on both sides of the 16-wide chunk and of the float4 path, every
# candidate count around one tile of 128, every event count around a wave's 32 columns and a workgroup
SHAPES = [(1, 1, 1), (5, 2, 31), (16, 127, 32), (17, 128, 33), (64, 129, 129), (100, 300, 257), (128, 300, 33),
          (256, 129, 31), (5, 300, 257), (16, 1, 33)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,nc,n", SHAPES)
def test_exact_ranks_on_integer_models(monkeypatch, mode, k, nc, n):
    rng = np.random.default_rng(1000 * k + 10 * nc + n)
    side = L.SIDE_USER if (k + nc) % 2 == 0 else L.SIDE_ITEM
    with make_ctx(k, mode) as ctx:
        qids, cids, P, Q = int_model(rng, ctx, 9, nc, k, side)
        S = chain_scores(P, Q)
        q, c = events(rng, qids, cids, n)
        for excl in (None, exclusions(rng, qids[:5], cids)):
            want_r, want_v = expected(S, qids, cids, q, c, excl)
            got = []
            for split, batch in ((None, None), (1, 7), (3, None), (3, 7)):
                if split is not None:
                    set_knob(monkeypatch, "pr_split", split)
                if batch is not None:
                    set_knob(monkeypatch, "pr_batch", batch)
                r, v, s = ctx.pair_ranks(q, c, side=side, exclude=excl, scores=True)
                monkeypatch.delenv("MFHIP_TEST", raising=False)
                assert np.array_equal(r, want_r), (split, batch, np.argwhere(r != want_r)[:5].ravel(), r[:8], want_r[:8])
                assert np.array_equal(v, want_v), (split, batch)
                ok = r >= 0
                a = np.array([np.nonzero(qids == x)[0][0] for x in q[ok]], int)
                b = np.array([np.nonzero(cids == x)[0][0] for x in c[ok]], int)
                assert np.array_equal(s[ok], S[a, b]) and not s[~ok].any()
                got.append((r, v, s))
            for r, v, s in got[1:]:
                assert np.array_equal(r, got[0][0]) and np.array_equal(s.view(np.uint64), got[0][2].view(np.uint64))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nw", [1, 2, 4])
def test_every_workgroup_shape_of_the_f32_walk(monkeypatch, mode, nw):
    """pr_nw = 1, 2, 4 waves per workgroup (the deterministic walk ignores it): the same exact ranks."""
    rng = np.random.default_rng(40 + nw)
    set_knob(monkeypatch, "pr_nw", nw)
    with make_ctx(20, mode) as ctx:
        qids, cids, P, Q = int_model(rng, ctx, 9, 300, 20, L.SIDE_USER)
        q, c = events(rng, qids, cids, 257)
        excl = exclusions(rng, qids[:5], cids)
        want_r, want_v = expected(chain_scores(P, Q), qids, cids, q, c, excl)
        r, v, _ = ctx.pair_ranks(q, c, exclude=excl)
        assert np.array_equal(r, want_r) and np.array_equal(v, want_v)


@pytest.mark.parametrize("mode", MODES)
def test_special_values_order_as_recommend(mode):
    """NaN rows (one, then two that tie and fall to the id), +inf, -inf, and a row of -0.0 entries among
    rows scoring +0.0: the ranks follow the definition, and the top list of mf_recommend agrees."""
    k, nc = 4, 40
    rng = np.random.default_rng(7)
    with make_ctx(k, mode) as ctx:
        qids, cids = shuffled_ids(rng, 6), shuffled_ids(rng, nc, 5)
        P = rng.integers(-2, 3, (6, k)).astype(np.float64)
        P[:, 0] = 1.0  # column 0 of every query is positive: an infinite entry there stays infinite
        Q = rng.integers(-2, 3, (nc, k)).astype(np.float64)
        Q[3] = [np.inf, 0, 0, 0]
        Q[4] = [-np.inf, 0, 0, 0]
        Q[5] = [-0.0, -0.0, -0.0, -0.0]
        Q[6] = Q[7] = Q[8] = 0.0  # score +0.0: tied with row 5, broken by id
        for nan_rows in ([10], [10, 20]):
            Qn = Q.copy()
            for x in nan_rows:
                Qn[x, 1] = np.nan
            ctx.set_factors(L.SIDE_USER, qids, P)
            ctx.set_factors(L.SIDE_ITEM, cids, Qn)
            S = chain_scores(P, Qn)
            q = np.repeat(qids, nc).astype(np.int32)
            c = np.tile(cids, 6).astype(np.int32)
            want_r, want_v = expected(S, qids, cids, q, c, None)
            r, v, s = ctx.pair_ranks(q, c, scores=True)
            assert np.array_equal(r, want_r), np.argwhere(r != want_r)[:5].ravel()
            assert (v == nc).all()
            # every query's ranks are a permutation, and recommend lists the candidates in that order
            ids, sc, cnt = ctx.recommend(qids, nc)
            for a in range(6):
                ra = r[a * nc:(a + 1) * nc]
                assert sorted(ra.tolist()) == list(range(nc))
                assert np.array_equal(ids[a][ra], cids)
                assert np.array_equal(sc[a][ra].view(np.uint64), s[a * nc:(a + 1) * nc].view(np.uint64))
                assert np.isnan(s[a * nc + nan_rows[0]]) and ra[nan_rows[0]] >= nc - len(nan_rows)


@pytest.mark.parametrize("mode", MODES)
def test_exclusion_corners_and_cold_events(mode):
    k, nc = 8, 70
    rng = np.random.default_rng(11)
    with make_ctx(k, mode) as ctx:
        qids, cids, P, Q = int_model(rng, ctx, 4, nc, k, L.SIDE_USER)
        S = chain_scores(P, Q)
        unknown_q, unknown_c = np.int32(55_000_000), np.int32(-66_000_000)
        # user 0: everything but the target excluded; user 1: the target itself excluded; user 2: some;
        # user 3: none.  Plus pairs naming unknown ids, a user that is in the model but not in the batch
        # ... and duplicates
        eq = [qids[0]] * (nc - 1) + [qids[1]] * 3 + [qids[2]] * 20 + [unknown_q, qids[2], qids[2]]
        ec = cids[1:].tolist() + [cids[5], cids[5], cids[6]] + cids[10:30].tolist() + [cids[0], unknown_c, cids[10]]
        excl = (np.array(eq, np.int32), np.array(ec, np.int32))
        q = np.array([qids[0], qids[1], qids[1], qids[2], qids[2], qids[3], unknown_q, qids[3], unknown_q], np.int32)
        c = np.array([cids[0], cids[5], cids[7], cids[3], cids[12], cids[9], cids[1], unknown_c, unknown_c], np.int32)
        want_r, want_v = expected(S, qids, cids, q, c, excl)
        assert want_r[0] == 0 and want_v[0] == 1 and want_r[1] == EXCLUDED and want_r[4] == EXCLUDED
        assert want_r[6:].tolist() == [COLD] * 3 and want_v[2] == nc - 2 and want_v[3] == nc - 20
        r, v, s = ctx.pair_ranks(q, c, exclude=excl, scores=True)
        assert np.array_equal(r, want_r) and np.array_equal(v, want_v)
        assert not s[r < 0].any() and not v[r < 0].any()
        # exclusions of a user that no event names change nothing
        r2, v2, _ = ctx.pair_ranks(q[5:6], c[5:6], exclude=excl)
        assert r2[0] == want_r[5] and v2[0] == nc
        # n == 0
        r0, v0, _ = ctx.pair_ranks(np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert len(r0) == 0 and len(v0) == 0


def test_state_errors():
    with make_ctx(4, L.MODE_FAST_F32) as ctx:
        with pytest.raises(L.MFError) as e:
            ctx.pair_ranks([1], [1])
        assert e.value.code == L.MF_ERR_NOT_FITTED
        ctx.set_factors(L.SIDE_USER, [1], np.ones((1, 4)))
        r, v, _ = ctx.pair_ranks([1, 2], [1, 1])  # the item side holds no row: cold
        assert r.tolist() == [COLD, COLD] and v.tolist() == [0, 0]
        with pytest.raises(L.MFError) as e:
            ctx.pair_ranks([1], [1], side=3)
        assert e.value.code == L.MF_ERR_INVALID


# ---- against mf_recommend ---------------------------------------------------------------------
REC_SEED = 2024  # picked on the CPU: 257 uniform targets over 300 candidates, both classes well above a quarter


def recommend_case(mode):
    rng = np.random.default_rng(REC_SEED)
    k, nq, nc, n = 24, 40, 300, 257
    ctx = make_ctx(k, mode)
    qids, cids = shuffled_ids(rng, nq), shuffled_ids(rng, nc, 5)
    ctx.set_factors(L.SIDE_USER, qids, rng.standard_normal((nq, k)))
    ctx.set_factors(L.SIDE_ITEM, cids, rng.standard_normal((nc, k)))
    q = rng.choice(qids, n).astype(np.int32)
    c = rng.choice(cids, n).astype(np.int32)
    excl = exclusions(rng, qids, cids, 0.1)
    return ctx, qids, cids, q, c, excl


@pytest.mark.parametrize("mode", MODES)
def test_agrees_with_recommend_and_its_peeled_order(mode):
    ctx, qids, cids, q, c, excl = recommend_case(mode)
    with ctx:
        r, v, s = ctx.pair_ranks(q, c, exclude=excl, scores=True)
        ranked = r >= 0
        low, high = ranked & (r < 128), ranked & (r >= 128)
        assert low.sum() >= len(q) / 4 and high.sum() >= len(q) / 4, (low.sum(), high.sum())
        ids, sc, cnt = ctx.recommend(q, 128, exclude=excl)
        assert np.array_equal(cnt[ranked], np.minimum(v[ranked], 128))
        for j in np.nonzero(low)[0]:
            assert ids[j, r[j]] == c[j]
            assert sc[j, r[j]].view(np.uint64) == s[j].view(np.uint64)
        for j in np.nonzero(high)[0]:
            assert c[j] not in ids[j, :cnt[j]]
        for j in np.nonzero(r == EXCLUDED)[0]:
            assert c[j] not in ids[j, :cnt[j]]
        # the full order from mf_recommend alone: three peels of 128 cover the 300 candidates
        users = np.unique(q)
        eq, ec = excl
        order = {int(u): [] for u in users}
        for _ in range(3):
            pid, _, pcnt = ctx.recommend(users, 128, exclude=(eq, ec), scores=False)
            for a, u in enumerate(users):
                order[int(u)] += pid[a, :pcnt[a]].tolist()
            eq = np.concatenate([eq, np.repeat(users, pcnt)]).astype(np.int32)
            ec = np.concatenate([ec] + [pid[a, :pcnt[a]] for a in range(len(users))]).astype(np.int32)
        for j in np.nonzero(ranked)[0]:
            lst = order[int(q[j])]
            assert len(lst) == v[j]
            assert lst[r[j]] == c[j], (j, r[j])
