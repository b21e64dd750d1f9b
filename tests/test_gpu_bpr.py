"""BPR training on the device (csrc/bpr.cpp, csrc/kernels_bpr.hip) against mfhip/bpr.py, the numpy statement of
the contract in include/mfhip.h, bit for bit: the arithmetic of a step through mf_bpr_step_triples, the draw
through mf_debug_bpr_triples, mf_bpr_run against both, the state rules, and a small problem it must learn.

The refusal on a context over two devices runs only where the machine has two."""
import numpy as np
import pytest

from conftest import set_knob
from mfhip import SEEN, bpr
from mfhip import _lib as L
from mfhip.context import Context

pytestmark = pytest.mark.gpu

F64, F32 = L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32
MODES = [F64, F32]
SCALES = [L.BPR_SCALE_SUM, L.BPR_SCALE_MEAN]
USER, ITEM = L.SIDE_USER, L.SIDE_ITEM
NU, NI = 300, 120
UNKNOWN = 99_000_001


def make_ctx(k, mode, **kw):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    for a, b in kw.items():
        setattr(p, a, b)
    return Context(p)


def dtype_of(mode):
    return np.float64 if mode == F64 else np.float32


def shuffled_ids(rng, n, scale=3):
    """n distinct ids, about half of them negative, in random order (row order is call order)."""
    return (rng.permutation(n).astype(np.int32) - n // 2) * scale + 1


class Model:
    """A context with NU x NI factors under shuffled signed ids; row r of a side is ids[r]."""

    def __init__(self, k, mode, seed=1, nu=NU, ni=NI, lo=-0.5, hi=0.5):
        rng = np.random.default_rng(seed)
        self.k, self.mode, self.T = k, mode, dtype_of(mode)
        self.uid, self.iid = shuffled_ids(rng, nu), shuffled_ids(rng, ni, 5)
        self.P = rng.uniform(lo, hi, (nu, k)).astype(self.T)
        self.Q = rng.uniform(lo, hi, (ni, k)).astype(self.T)
        self.ctx = make_ctx(k, mode)
        self.ctx.set_factors(USER, self.uid, self.P.astype(np.float64))
        self.ctx.set_factors(ITEM, self.iid, self.Q.astype(np.float64))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def device(self):
        """(P, Q) as the device holds them, in row order, in the context's precision."""
        return (self.ctx.lookup(USER, self.uid)[0].astype(self.T), self.ctx.lookup(ITEM, self.iid)[0].astype(self.T))

    def ids(self, u, i, j):
        """Triples of rows as ids; a void slot (-1) becomes a triple naming an unknown user."""
        u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
        live = u >= 0
        return (np.where(live, self.uid[np.where(live, u, 0)], UNKNOWN).astype(np.int32),
                self.iid[np.where(live, i, 0)], self.iid[np.where(live, j, 0)])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(a, b):
    d = np.argwhere(a != b)
    return None if not len(d) else (tuple(d[0]), a[tuple(d[0])], b[tuple(d[0])], len(d))


def random_triples(rng, n, nu=NU, ni=NI):
    u = rng.integers(0, nu, n)
    i = rng.integers(0, ni, n)
    j = (i + 1 + rng.integers(0, ni - 1, n)) % ni
    return u, i, j


def check_steps(m, batches, lr, lam, scale, chunk=bpr.CHUNK):
    """Every batch of (u, i, j, extra void triples as ids) as one device step; the model after each must equal the
    replay's, which started from the model the previous step left."""
    P, Q = m.P, m.Q
    p = Context.bpr_params(lr, lam, batch=0, scale=scale, redraws=99, seed=-7)  # batch, redraws, seed: not read
    for u, i, j in batches:
        st = m.ctx.bpr_step_triples(p, *m.ids(u, i, j))
        P, Q, want = bpr.replay_step(P, Q, u, i, j, lr, lam, scale, chunk)
        dP, dQ = m.device()
        assert same_bits(dP, P), ("users", first_difference(dP, P))
        assert same_bits(dQ, Q), ("items", first_difference(dQ, Q))
        live = np.asarray(u) >= 0                                # the stats against counts made here
        assert st == want == dict(slots=len(u), void_slots=int((~live).sum()),
                                  user_rows_written=len(set(np.asarray(u)[live].tolist())),
                                  item_rows_written=len(set(np.asarray(i)[live].tolist()) |
                                                        set(np.asarray(j)[live].tolist())))
    return P, Q


# ---- the arithmetic, through mf_bpr_step_triples -----------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 63, 64, 65, 128, 129, 200, 255, 256])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_three_steps_equal_the_replay(mode, scale, k):
    rng = np.random.default_rng(100 + k)
    with Model(k, mode, seed=k) as m:
        batches = []
        for n in (1000, 1000, 777):
            u, i, j = random_triples(rng, n, 250, 100)           # the last 50 users and 20 items: never named
            u[rng.integers(0, n, 9)] = -1                        # unknown ids in some slots
            batches.append((u, i, j))
        P, Q = check_steps(m, batches, 0.05 if scale == L.BPR_SCALE_SUM else 0.5, 0.01, scale)
        assert not same_bits(P, m.P) and not same_bits(Q, m.Q)
        dP, dQ = m.device()                                      # rows that no slot names keep their bits
        assert same_bits(dP[250:], m.P[250:]) and same_bits(dQ[100:], m.Q[100:])
        assert (dP[:250] != m.P[:250]).any(1).sum() > 200 and (dQ[:100] != m.Q[:100]).any(1).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("mode", MODES)
def test_triple_counts(mode, n):
    rng = np.random.default_rng(n)
    with Model(40, mode, seed=3) as m:
        first, second = random_triples(rng, n), random_triples(rng, n)
        P, Q = check_steps(m, [first], 0.1, 0.02, L.BPR_SCALE_SUM)
        if n == 1:                                               # one triple writes one user row and two item rows
            assert (P != m.P).any(1).sum() == 1 and (Q != m.Q).any(1).sum() == 2
        m.P, m.Q = P, Q
        check_steps(m, [second], 0.1, 0.02, L.BPR_SCALE_SUM)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_crafted_batches(mode, scale):
    rng = np.random.default_rng(5)
    n = 600
    with Model(33, mode, seed=9) as m:
        u, i, j = random_triples(rng, n)
        one_user = (np.full(n, 17), i, j)                        # one user in every slot
        i2, j2 = i.copy(), j.copy()
        half = rng.random(n) < 0.5                               # one item: positive in some slots, negative in others
        i2[half], j2[~half] = 5, 5
        j2[half & (j2 == 5)] = 6
        i2[~half & (i2 == 5)] = 6
        one_item = (u, i2, j2)
        assert (i2 != j2).all() and ((i2 == 5) | (j2 == 5)).all() and (i2 == 5).any() and (j2 == 5).any()
        check_steps(m, [one_user, one_item], 0.05, 0.01, scale)
        # unknown ids on each of the three sides and pos == neg: void, counted, and with no other effect
        p = Context.bpr_params(0.05, 0.01, scale=scale)
        before = m.device()
        uu, ii, jj = m.ids(u[:8], i[:8], j[:8])
        uu[0], ii[1], jj[2] = UNKNOWN, UNKNOWN, UNKNOWN
        jj[3] = ii[3]
        live = np.array([0, 0, 0, 0, 1, 1, 1, 1], bool)
        st = m.ctx.bpr_step_triples(p, uu, ii, jj)
        assert st["slots"] == 8 and st["void_slots"] == 4
        P, Q, want = bpr.replay_step(*before, np.where(live, u[:8], -1), i[:8], j[:8], 0.05, 0.01, scale)
        assert st == want
        after = m.device()
        assert same_bits(after[0], P) and same_bits(after[1], Q)
        st = m.ctx.bpr_step_triples(p, uu[:4], ii[:4], jj[:4])  # nothing but void slots
        assert st == dict(slots=4, void_slots=4, user_rows_written=0, item_rows_written=0)
        assert all(same_bits(a, b) for a, b in zip(m.device(), after))
        assert m.ctx.bpr_step_triples(p, [], [], []) == dict(slots=0, void_slots=0, user_rows_written=0,
                                                             item_rows_written=0)


def long_segments(rng, lengths, user0=10, item0=20):
    """A batch in which user row user0 + x and item row item0 + x are each named by lengths[x] slots: neighbouring
    rows, so the segments lie side by side after the sort.  The item is the positive in its even slots and the
    negative in its odd ones; everything else is drawn among the rows outside the two ranges."""
    u, i, j = [], [], []
    hi_u, hi_i = user0 + len(lengths), item0 + len(lengths)
    for x, n in enumerate(lengths):
        a, b, c = random_triples(rng, n, NU - hi_u, NI - hi_i)
        u += [user0 + x] * n                                     # the user's segment
        i += (b + hi_i).tolist()
        j += (c + hi_i).tolist()
        u += (a + hi_u).tolist()                                 # the item's
        other = c + hi_i
        odd = np.arange(n) % 2 == 1
        i += np.where(odd, other, item0 + x).tolist()
        j += np.where(odd, item0 + x, other).tolist()
    perm = rng.permutation(len(u))
    return np.array(u)[perm], np.array(i)[perm], np.array(j)[perm]


def check_lengths(batch, lengths, user0=10, item0=20):
    u, i, j = batch
    for x, n in enumerate(lengths):
        assert (u == user0 + x).sum() == n and ((i == item0 + x) | (j == item0 + x)).sum() == n


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_segments_around_the_chunk_length(mode, scale):
    lengths = [1023, 1024, 1025, 2049]
    rng = np.random.default_rng(11)
    batch = long_segments(rng, lengths)
    check_lengths(batch, lengths)
    with Model(8, mode, seed=4, lo=-0.2, hi=0.2) as m:
        check_steps(m, [batch, long_segments(rng, lengths[::-1])], 0.001, 0.01, scale)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_segments_around_a_chunk_of_16(monkeypatch, mode, scale):
    """MFHIP_TEST bpr_chunk=16: the same rule at 15 / 16 / 17 / 33, and segments of several chunks side by side."""
    set_knob(monkeypatch, "bpr_chunk", 16)
    rng = np.random.default_rng(12)
    lengths = [15, 16, 17, 33, 17, 40, 32, 1, 48, 49]
    batch = long_segments(rng, lengths)
    check_lengths(batch, lengths)
    with Model(70, mode, seed=6) as m:
        P, Q = check_steps(m, [batch, long_segments(rng, lengths[::-1])], 0.01, 0.01, scale, chunk=16)
        other = bpr.replay_step(m.P, m.Q, *batch, 0.01, 0.01, scale, bpr.CHUNK)[0]
        assert not same_bits(other, bpr.replay_step(m.P, m.Q, *batch, 0.01, 0.01, scale, 16)[0])  # the chunk matters


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_long_segments_in_a_batch_smaller_than_the_user_side(monkeypatch, mode, scale):
    """Fewer slots than user rows: the new user rows wait in a scratch indexed by their segment's first sorted
    position, not by row.  With bpr_chunk=16, users of 40, 17 and 33 slots among 180 slots and 300 user rows."""
    set_knob(monkeypatch, "bpr_chunk", 16)
    rng = np.random.default_rng(13)
    lengths = [40, 17, 33]
    batch = long_segments(rng, lengths)
    check_lengths(batch, lengths)
    assert len(batch[0]) == 180 < NU
    with Model(70, mode, seed=7) as m:
        check_steps(m, [batch, long_segments(rng, lengths[::-1])], 0.01, 0.01, scale, chunk=16)


# ---- the sampled path --------------------------------------------------------------------------------------
def seen_problem(m, rng):
    """6,000 synthetic pairs, plus user row 3 who has seen every item but row 77 and user row 4 who has seen all."""
    u = rng.integers(5, NU, 6000)
    i = np.minimum((rng.random(6000) ** 2 * NI).astype(np.int64), NI - 1)
    u = np.concatenate([u, np.full(NI - 1, 3), np.full(NI, 4)])
    i = np.concatenate([i, np.delete(np.arange(NI), 77), np.arange(NI)])
    m.ctx.seen_set(m.uid[u], m.iid[i])
    return u, i


def expected_triples(m, seed, step, batch, redraws):
    rid, off, ent, _ = m.ctx.debug_seen_csr(USER)
    assert np.array_equal(rid, m.uid)
    z = bpr.draws(seed, step, batch, redraws, int(off[-1]), NI)
    assert np.array_equal(z, bpr.device_draws(seed, step, batch, redraws, int(off[-1]), NI))
    return bpr.triples(z, off, ent, NI), off, ent


@pytest.mark.parametrize("redraws", [0, 1, 62])
@pytest.mark.parametrize("mode", MODES)
def test_last_steps_triples_are_the_draws_resolved_against_the_table(mode, redraws):
    batch = 1500
    with Model(16, mode, seed=2) as m:
        seen_problem(m, np.random.default_rng(3))
        p = Context.bpr_params(0.05, 0.01, batch=batch, redraws=redraws, seed=41)
        st = m.ctx.bpr_run(p, 6, 1)
        (u, i, j), off, ent = expected_triples(m, 41, 6, batch, redraws)
        du, di, dj = m.ctx.debug_bpr_triples()
        assert np.array_equal(du, u) and np.array_equal(di, i) and np.array_equal(dj, j)
        assert st["slots"] == batch and st["void_slots"] == int((u < 0).sum())
        z = bpr.draws(41, 6, batch, redraws, int(off[-1]), NI)
        e = z[:, 0].astype(np.int64)
        all_seen = (e >= off[4]) & (e < off[5])                  # the positive is one of user row 4's entries
        assert all_seen.sum() > 5 and (u[all_seen] == -1).all()
        almost = (e >= off[3]) & (e < off[4])
        assert almost.sum() > 5 and (j[almost & (u >= 0)] == 77).all()
        if redraws == 62:
            assert (u[almost] >= 0).any()                        # 63 draws among 119 rows find row 77 in 4 slots of 10
        live = u >= 0
        assert (i[live] != j[live]).all()
        held = {(a, b) for a in range(NU) for b in ent[off[a]:off[a + 1]].tolist()}
        assert all((a, b) in held and (a, c) not in held for a, b, c in zip(u[live], i[live], j[live]))
        P, Q, want = bpr.replay_step(m.P, m.Q, u, i, j, 0.05, 0.01, L.BPR_SCALE_SUM)
        dP, dQ = m.device()
        assert same_bits(dP, P) and same_bits(dQ, Q) and st == want


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_run_of_three_steps_equals_three_runs_and_the_replayed_triples(mode, scale):
    batch, seed = 900, -12345
    p = Context.bpr_params(0.2, 0.01, batch=batch, scale=scale, redraws=3, seed=seed)
    with Model(24, mode, seed=8) as a, Model(24, mode, seed=8) as b, Model(24, mode, seed=8) as c:
        for m in (a, b, c):
            seen_problem(m, np.random.default_rng(3))
        sa = a.ctx.bpr_run(p, 10, 3)
        total = dict(slots=0, void_slots=0, user_rows_written=0, item_rows_written=0)
        P, Q = c.P, c.Q
        for t in (10, 11, 12):
            sb = b.ctx.bpr_run(p, t, 1)
            (u, i, j), _, _ = expected_triples(c, seed, t, batch, 3)
            sc = c.ctx.bpr_step_triples(p, *c.ids(u, i, j))
            P, Q, want = bpr.replay_step(P, Q, u, i, j, 0.2, 0.01, scale)
            assert sb == sc == want
            total = {n: total[n] + sb[n] for n in total}
        assert sa == total
        for m in (a, b, c):
            dP, dQ = m.device()
            assert same_bits(dP, P) and same_bits(dQ, Q)
        for x, y in zip(a.ctx.debug_bpr_triples(), b.ctx.debug_bpr_triples()):
            assert np.array_equal(x, y)


def test_pool_of_one_an_empty_set_and_no_steps():
    p = Context.bpr_params(0.05, 0.01, batch=64, redraws=2, seed=1)
    void = dict(slots=128, void_slots=128, user_rows_written=0, item_rows_written=0)
    with Model(8, F32, ni=1) as m:                               # one item: no negative to draw
        m.ctx.seen_set(m.uid[:50], np.repeat(m.iid, 50))
        assert m.ctx.seen_count() == 50
        assert m.ctx.bpr_run(p, 0, 2) == void
        assert all(same_bits(x, y) for x, y in zip(m.device(), (m.P, m.Q)))
    with Model(8, F64) as m:
        m.ctx.seen_set([], [])                                   # an empty set: no positive to draw
        assert m.ctx.bpr_run(p, 0, 2) == void
        with pytest.raises(L.MFError) as e:                      # no kernel ran: there are no triples to show
            m.ctx.debug_bpr_triples()
        assert e.value.code == L.MF_ERR_STATE
        seen_problem(m, np.random.default_rng(3))
        assert m.ctx.bpr_run(p, 4, 0) == dict(slots=0, void_slots=0, user_rows_written=0, item_rows_written=0)
        assert all(same_bits(x, y) for x, y in zip(m.device(), (m.P, m.Q)))
        with pytest.raises(L.MFError) as e:
            m.ctx.debug_bpr_triples()
        assert e.value.code == L.MF_ERR_STATE
        m.ctx.bpr_run(p, 4, 1)                                   # a step, then no steps: the step's triples stay
        shown = m.ctx.debug_bpr_triples()
        after = m.device()
        assert len(shown[0]) == 64 and (shown[0] >= 0).any()
        assert m.ctx.bpr_run(p, 5, 0) == dict(slots=0, void_slots=0, user_rows_written=0, item_rows_written=0)
        assert all(np.array_equal(x, y) for x, y in zip(shown, m.ctx.debug_bpr_triples()))
        assert all(same_bits(x, y) for x, y in zip(m.device(), after))
        m.ctx.seen_set([], [])                                   # ... and a call on an empty set leaves none
        m.ctx.bpr_run(p, 6, 1)
        with pytest.raises(L.MFError) as e:
            m.ctx.debug_bpr_triples()
        assert e.value.code == L.MF_ERR_STATE


def test_state_errors():
    p = Context.bpr_params(0.05, 0.01, batch=8)
    with make_ctx(8, F32) as ctx:
        with pytest.raises(L.MFError) as e:                      # no model
            ctx.bpr_step_triples(p, [1], [2], [3])
        assert e.value.code == L.MF_ERR_NOT_FITTED
        with pytest.raises(L.MFError) as e:                      # no seen set
            ctx.bpr_run(p, 0, 1)
        assert e.value.code == L.MF_ERR_STATE and "seen set" in str(e.value)
    with Model(8, F64) as m:
        with pytest.raises(L.MFError) as e:
            m.ctx.bpr_run(p, 0, 1)
        assert e.value.code == L.MF_ERR_STATE
        m.ctx.seen_set(m.uid[:3], m.iid[:3])
        m.ctx.seen_clear()
        with pytest.raises(L.MFError) as e:
            m.ctx.bpr_run(p, 0, 1)
        assert e.value.code == L.MF_ERR_STATE
        assert all(same_bits(x, y) for x, y in zip(m.device(), (m.P, m.Q)))
    rng = np.random.default_rng(4)
    uid, iid = shuffled_ids(rng, 20), shuffled_ids(rng, 10, 5)
    new_u, new_i = np.array([7001, 7002], np.int32), np.array([8001, 8002], np.int32)

    def all_three(ctx, code, word):
        """bpr_run, bpr_step_triples and bpr_fit each refuse with `code`; the rows and their bits stay."""
        P, Q = rng.random((20, ctx.k)), rng.random((10, ctx.k))
        ctx.set_factors(USER, uid, P)
        ctx.set_factors(ITEM, iid, Q)
        before = (ctx.lookup(USER, uid)[0], ctx.lookup(ITEM, iid)[0])
        for call in (lambda: ctx.bpr_run(p, 0, 1), lambda: ctx.bpr_step_triples(p, uid[:3], iid[:3], iid[3:6]),
                     lambda: ctx.bpr_fit(new_u, new_i, p, 1)):     # (fit would insert four rows)
            with pytest.raises(L.MFError) as e:
                call()
            assert e.value.code == code and word in str(e.value)
        assert ctx.num_factors(USER) == 20 and ctx.num_factors(ITEM) == 10
        assert not ctx.lookup(USER, new_u)[1].any() and not ctx.lookup(ITEM, new_i)[1].any()
        assert np.array_equal(before[0], ctx.lookup(USER, uid)[0]) and np.array_equal(before[1], ctx.lookup(ITEM, iid)[0])

    for mode in MODES:
        with make_ctx(257, mode) as ctx:                         # a rank the kernels do not cover
            all_three(ctx, L.MF_ERR_INVALID, "256")
        q = L.default_params()
        q.num_factors = 8
        q.mode = mode
        with Context(q, rank=(0, 1, 0, b"")) as ctx:             # a rank-mode context (one rank)
            all_three(ctx, L.MF_ERR_STATE, "single-process")
        if L.device_count() >= 2:                                # one process on two devices
            q.num_blocks = 2
            with Context(q, n_devices=2) as ctx:
                all_three(ctx, L.MF_ERR_STATE, "one device")
    with Model(8, F64) as m:                                     # a refusal leaves the seen set as it was
        m.ctx.seen_set(m.uid[:3], m.iid[:3])
        table = m.ctx.debug_seen_csr(USER)
        with pytest.raises(L.MFError) as e:
            m.ctx.bpr_run(Context.bpr_params(0.05, 0.01, batch=8, redraws=63), 0, 1)
        assert e.value.code == L.MF_ERR_INVALID
        assert m.ctx.seen_count() == 3 and all(np.array_equal(x, y) for x, y in zip(table, m.ctx.debug_seen_csr(USER)))
        assert all(same_bits(x, y) for x, y in zip(m.device(), (m.P, m.Q)))


def test_nothing_else_in_the_context_moves():
    rng = np.random.default_rng(21)
    p = Context.bpr_params(0.05, 0.01, batch=500, redraws=2, seed=5)
    how = dict(lam=0.1)
    with Model(8, F64) as m:
        u, i = rng.integers(0, NU, 4000), rng.integers(0, NI, 4000)
        m.ctx.als_prepare(m.uid[u], m.iid[i], rng.integers(1, 6, 4000).astype(np.float64))
        m.ctx.als_run_nonneg(1, **how)                           # the counter is odd now: the user side is next
        m.ctx.seen_from_als()

        def snapshot():
            return ([m.ctx.debug_seen_csr(s) for s in (USER, ITEM)], [m.ctx.als_csr(s) for s in (USER, ITEM)],
                    m.ctx.als_nonneg_stats(), m.ctx.seen_count(), m.ctx.num_factors(USER), m.ctx.num_factors(ITEM))

        def same(x, y):
            if isinstance(x, (list, tuple)):
                return len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
            return np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y

        before = snapshot()
        assert m.ctx.bpr_run(p, 0, 2)["user_rows_written"] > 0
        uu, ii, jj = random_triples(rng, 300)
        m.ctx.bpr_step_triples(p, *m.ids(uu, ii, jj))
        assert same(before, snapshot())
        items = m.ctx.lookup(ITEM, m.iid)[0]
        users = m.ctx.lookup(USER, m.uid)[0]
        m.ctx.als_run(1, **how)                                  # the half-sweep counter: the user side is solved
        assert np.array_equal(items, m.ctx.lookup(ITEM, m.iid)[0])
        assert not np.array_equal(users, m.ctx.lookup(USER, m.uid)[0])
    # a prepared DSGD schedule
    params = dict(num_blocks=2, iterations=2, seed=3)
    with make_ctx(64, F32, **params) as ctx:                     # (the pair schedule: k = 64)
        uid, iid = shuffled_ids(rng, 200), shuffled_ids(rng, 80, 5)
        u, i = rng.integers(0, 200, 5000), rng.integers(0, 80, 5000)
        ctx.prepare(uid[u], iid[i], rng.random(5000))
        ctx.run(1)
        ctx.seen_set(uid[u], iid[i])
        dig, done = ctx.plan_digest(), ctx.superstep
        assert ctx.bpr_run(p, 0, 2)["item_rows_written"] > 0
        assert ctx.plan_digest() == dig and ctx.superstep == done == 1
        ctx.run(1)
        assert ctx.superstep == 2


def test_fit_inserts_scaled_rows_sets_the_seen_set_and_runs():
    rng = np.random.default_rng(31)
    uid, iid = shuffled_ids(rng, 60), shuffled_ids(rng, 40, 5)
    u, i = rng.integers(0, 60, 700), rng.integers(0, 40, 700)
    p = Context.bpr_params(0.05, 0.01, batch=256, redraws=1, seed=9)
    held = np.full((1, 6), 0.25)
    for mode in MODES:
        T = dtype_of(mode)
        with make_ctx(6, mode, seed=17) as a, make_ctx(6, mode, seed=17) as b, make_ctx(6, F64, seed=17) as ref:
            for ctx in (a, b, ref):
                ctx.set_factors(USER, uid[u[:1]], held)          # a row already held is kept
            assert a.bpr_fit(uid[u], iid[i], p, 0, init_scale=0.1) == dict(slots=0, void_slots=0, user_rows_written=0,
                                                                           item_rows_written=0)
            # mf_als_prepare's rows and values in f64, scaled there, then rounded to the context's precision
            ref.als_prepare(uid[u], iid[i], np.ones(700))
            for side in (USER, ITEM):
                (ia, va), (ir, vr) = a.factors(side), ref.factors(side)
                want = (vr * 0.1).astype(T).astype(np.float64)
                if side == USER:
                    want[ir == uid[u[0]]] = held
                assert np.array_equal(ia, ir) and np.array_equal(va, want)
                assert np.array_equal(a.lookup(side, ir)[0], want)
            assert a.seen_count() == len(set(zip(u.tolist(), i.tolist())))
            st = a.bpr_run(p, 0, 3)
            assert st["slots"] == 768 and st["user_rows_written"] > 0
            assert b.bpr_fit(uid[u], iid[i], p, 3, init_scale=0.1) == st   # the whole call at once
            for side in (USER, ITEM):
                (ia, va), (ib, vb) = a.factors(side), b.factors(side)
                assert np.array_equal(ia, ib) and np.array_equal(va, vb)
            for x, y in zip(a.debug_seen_csr(USER), b.debug_seen_csr(USER)):
                assert np.array_equal(x, y)


# ---- it learns ---------------------------------------------------------------------------------------------
def group_problem():
    """200 users and 100 items in 4 groups (user u in group u mod 4, items 25 g .. 25 g + 24): per user 12
    training items and 3 held-out items of its group."""
    rng = np.random.default_rng(0)
    tu, ti, hu, hi = [], [], [], []
    for u in range(200):
        own = 25 * (u % 4) + rng.permutation(25)[:15]
        tu += [u] * 12
        ti += own[:12].tolist()
        hu += [u] * 3
        hi += own[12:].tolist()
    return (np.array(x, np.int32) for x in (tu, ti, hu, hi))


@pytest.mark.parametrize("scale,lr,batch", [(L.BPR_SCALE_MEAN, 0.5, 2400), (L.BPR_SCALE_SUM, 0.05, 512)])
def test_it_learns_the_groups(scale, lr, batch):
    """Hit rate at 10 per held-out pair over the unseen items.  Chance is 10 of 88 unseen items (0.114), the
    ceiling 10 of the 13 unseen items of the group (0.769); the bound is halfway, 0.44."""
    tu, ti, hu, hi = group_problem()
    rng = np.random.default_rng(1)
    k, lam, steps = 8, 0.01, 200
    P = rng.uniform(0, 0.1, (200, k)).astype(np.float32)
    Q = rng.uniform(0, 0.1, (100, k)).astype(np.float32)
    uid, iid = np.arange(200, dtype=np.int32), np.arange(100, dtype=np.int32)
    p = Context.bpr_params(lr, lam, batch=batch, scale=scale, redraws=2, seed=77)
    with make_ctx(k, F32) as ctx:
        ctx.set_factors(USER, uid, P.astype(np.float64))
        ctx.set_factors(ITEM, iid, Q.astype(np.float64))
        ctx.seen_set(tu, ti)
        st = ctx.bpr_run(p, 0, steps)
        assert st["slots"] == steps * batch and st["void_slots"] < st["slots"] // 100
        ids, _, counts = ctx.recommend(uid, 10, exclude=SEEN, scores=False)
        assert (counts == 10).all()
        hits = np.mean([hi[x] in ids[hu[x]] for x in range(len(hu))])
        print(f"hit rate at 10: {hits:.4f} (scale {scale}, lr {lr}, batch {batch})")
        assert hits > 0.44
        # the same model on the CPU
        rid, off, ent, _ = ctx.debug_seen_csr(USER)
        assert np.array_equal(rid, uid) and off[-1] == 2400
        for t in range(steps):
            u, i, j = bpr.triples(bpr.device_draws(77, t, batch, 2, 2400, 100), off, ent, 100)
            P, Q, _ = bpr.replay_step(P, Q, u, i, j, lr, lam, scale)
        assert same_bits(ctx.lookup(USER, uid)[0].astype(np.float32), P)
        assert same_bits(ctx.lookup(ITEM, iid)[0].astype(np.float32), Q)
        scores = P.astype(np.float64) @ Q.astype(np.float64).T
        scores[tu, ti] = -np.inf
        top = np.argsort(-scores, axis=1, kind="stable")[:, :10]
        assert np.mean([hi[x] in top[hu[x]] for x in range(len(hu))]) > 0.44
