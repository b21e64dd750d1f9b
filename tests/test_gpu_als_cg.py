"""The conjugate-gradient ALS half-sweeps (csrc/kernels_als_cg.hip; mf_als_run_cg, mf_als_run_implicit_cg).

One code path serves every rank, so RANKS walks the edges of what the kernels do differ by: the 64
lanes of a rating's dot product (63, 64, 65, 127, 128, 129, 192, 255, 256), the row-wise and the flat
gather (below and from 64), the 32-column padding of G (31, 32, 33) and tiny ranks (1, 3).  Every rank
runs three ways: whole rows whose vectors stay in LDS where the budget holds them, als_cg_stage=0
(gathered again in every pass) and als_chunk=16 (long rows: chunk kernels + the update kernel).

  hook        A v and b through mf_debug_als_cg_matvec on integer data equal the host's integers bit for bit.
  one step    systems with A = 4 I (explicit) and 16 I (implicit): one CG step lands on b / 4 (b / 16)
              exactly, and five steps return the same bits, which needs the rs == 0 stop.
  replay      real-valued data against a numpy replay of the documented algorithm.  The bound is not a
              constant: 4 x the distance between two f64 replays that differ in the order of the rating
              sums (deterministic mode), 4 x the distance of an f32 replay from the f64 one (fast mode).
  the rest    invariance under als_batch, als_cg_stage and from run to run; untouched rows; the
              objective on the smoke data; the shared half-sweep counter; NaN containment; arguments.
"""
import functools

import numpy as np
import pytest

import mfhip
from als_support import FILLERS, MODES, REGS, TINY, bits, dtype_of, frozen, make_ctx, rows_of, shuffled_ids
from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth
from mfhip.context import Context

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 16, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 192, 255, 256]
REPLAY_RANKS = [3, 33, 64, 128, 160, 256]
WAYS = (None, ("als_cg_stage", 0), ("als_chunk", 16))
EXACT = 1 << 24     # f32 holds every integer up to here


# ---------------------------------------------------------------------------------------------
# 1. the hook: A v and b on integer data

@functools.lru_cache(maxsize=None)
def hook_problem(k):
    """max(k, 5) users with factors in {-3..3}, FILLERS zero-vector users, one user in the model but not
    in the data; items with 5, k, k + 1 and k + 200 ratings (fillers make up the excess), ratings in
    {-2..5} with every sign, v in {-2..2}.  Every sum the device can form is bounded in integers here."""
    rng = np.random.default_rng(4000 + k)
    real = max(k, 5)
    nu = real + FILLERS + 1
    P = np.zeros((nu, k), np.int64)
    P[:real] = rng.integers(-3, 4, (real, k))
    P[-1] = 2                                          # not in the data: takes no part in G
    pu, pi = [], []
    for t, (n_real, extra) in enumerate(((5, 0), (k, 0), (k, 1), (k, FILLERS))):
        pu += list(range(n_real)) + (real + rng.choice(FILLERS, extra, replace=False)).tolist()
        pi += [t] * (n_real + extra)
    pu, pi = np.array(pu), np.array(pi)
    r = rng.integers(-2, 6, len(pu))
    r[:3] = [-1, 0, 2]
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    irows = rows_of(pi, 5)
    assert [len(x) for x in irows] == [5, k, k + 1, k + FILLERS, 0]
    v = rng.integers(-2, 3, k)
    rated = np.unique(pu)
    assert set(range(real)) <= set(rated.tolist())
    G = P[rated].T @ P[rated]
    want = {}
    for t in range(4):
        Qm, rt = P[pu[irows[t]]], r[irows[t]]
        for implicit in (False, True):
            w = np.abs(rt) if implicit else np.ones_like(rt)          # alpha = 1
            c = np.where(rt > 0, 1 + np.abs(rt), 0) if implicit else rt
            Mv = Qm.T @ (w * (Qm @ v)) + (G @ v if implicit else 0)
            bound = np.abs(Qm).T @ (np.abs(w) * np.abs(Qm @ v)) + (np.abs(G) @ np.abs(v) if implicit else 0)
            assert bound.max() + 2 * (k + FILLERS) * 2 < EXACT and (np.abs(Qm).T @ np.abs(c)).max() < EXACT
            want[t, implicit] = (Mv, Qm.T @ c, int((rt > 0).sum()) if implicit else len(rt))
    return frozen(dict(pu=pu, pi=pi, r=r.astype(np.float64), P=P.astype(np.float64), v=v.astype(np.float64),
                       Q0=rng.integers(1, 4, (5, k)).astype(np.float64), uids=shuffled_ids(rng, nu),
                       iids=shuffled_ids(rng, 5, 5))), want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", RANKS)
def test_hook_is_exact_on_integer_data(monkeypatch, mode, k):
    """A v and b of the four rated items, explicit and implicit (alpha 1), staged, gathered again and
    split, equal the host's integers bit for bit.  lambda: 1e-300 with both regs (the device's own
    lambda' v in the context's precision is added on the host: it vanishes against every non-zero
    integer), and 2 (plain) and 1 (weighted), where lambda' v is an integer and a lost lambda' p shows."""
    d, want = hook_problem(k)
    T = dtype_of(mode)
    for way in WAYS:
        with monkeypatch.context() as mp:
            if way:
                set_knob(mp, *way)
            with make_ctx(k, mode) as ctx:
                assert ctx.als_cg_capacity() >= 5     # the 5-rating row is staged at every rank
                ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
                ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q0"])
                ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
                for (t, implicit), (Mv, b, n) in want.items():
                    for lam, reg in ((TINY, L.ALS_REG_WEIGHTED), (TINY, L.ALS_REG_PLAIN), (2.0, L.ALS_REG_PLAIN),
                                     (1.0, L.ALS_REG_WEIGHTED)):
                        lam_row = T(lam) * T(n) if reg == L.ALS_REG_WEIGHTED else T(lam)
                        Av = Mv.astype(T) + lam_row * d["v"].astype(T)
                        gAv, gb = ctx.als_cg_matvec(L.SIDE_ITEM, d["iids"][t], lam, d["v"],
                                                    alpha=1.0 if implicit else -1.0, reg=reg)
                        assert np.array_equal(bits(gAv), bits(Av)), (k, mode, way, t, implicit, lam, reg)
                        assert np.array_equal(bits(gb), bits(b)), (k, mode, way, t, implicit, lam, reg)
                with pytest.raises(mfhip.MFError):    # no rating in the data
                    ctx.als_cg_matvec(L.SIDE_ITEM, d["iids"][4], 1.0, d["v"])
                assert np.array_equal(bits(ctx.lookup(L.SIDE_ITEM, d["iids"])[0]), bits(d["Q0"]))  # nothing changed
                assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, d["uids"])[0]), bits(d["P"]))


# ---------------------------------------------------------------------------------------------
# 2. systems one CG step solves exactly

N_ONE = 6


@functools.lru_cache(maxsize=None)
def onestep_problem(k, implicit):
    """Users: 2 e_f for every factor f but one, four users e_f for that one, in permuted order, FILLERS
    zero-vector users, one user not in the data; so sum q q^T over them is 4 I.  N_ONE items rate all of
    them plus 0, 1 or 200 fillers; two items have no rating.  Explicit: ratings in {1..5}, A = 4 I,
    x = b / 4.  Implicit (alpha 1): ratings +-3, G + 3 sum q q^T = 16 I, x = b / 16; item 0 has no
    positive rating."""
    rng = np.random.default_rng(7000 + 2 * k + implicit)
    f4 = int(rng.integers(k))
    vecs = [2 * np.eye(k, dtype=np.int64)[f] for f in range(k) if f != f4] + [np.eye(k, dtype=np.int64)[f4]] * 4
    real = len(vecs)
    nu = real + FILLERS + 1
    P = np.zeros((nu, k), np.int64)
    P[:real] = np.array(vecs)[rng.permutation(real)]
    P[-1] = 2
    extras = [1, 0, FILLERS, 0, 1, FILLERS]
    pu, pi, r = [], [], []
    for t in range(N_ONE):
        fill = real + rng.choice(FILLERS, extras[t], replace=False)
        n = real + extras[t]
        pu += list(range(real)) + fill.tolist()
        pi += [t] * n
        rt = 3 * rng.choice([-1, 1], n) if implicit else rng.integers(1, 6, n)
        if implicit and t == 0:
            rt = -np.abs(rt)
        r += rt.tolist()
    pu, pi, r = np.array(pu), np.array(pi), np.array(r, np.int64)
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    irows = rows_of(pi, N_ONE + 2)
    X0 = rng.integers(-3, 4, (N_ONE + 2, k))
    rated = np.unique(pu)
    G = P[rated].T @ P[rated]
    assert np.array_equal(G, 4 * np.eye(k, dtype=np.int64))
    X = np.zeros((N_ONE, k))
    for t in range(N_ONE):
        Qm, rt = P[pu[irows[t]]], r[irows[t]]
        if implicit:
            A = G + (Qm * np.abs(rt)[:, None]).T @ Qm
            b = Qm.T @ np.where(rt > 0, 1 + np.abs(rt), 0)
        else:
            A, b = Qm.T @ Qm, Qm.T @ rt
        s = 16 if implicit else 4
        assert np.array_equal(A, s * np.eye(k, dtype=np.int64))
        X[t] = b / s
        assert np.array_equal(X[t] * s, b)               # b / s is exact
        res = b - s * X0[t]
        assert s * (res @ res) < EXACT
    assert not implicit or (not (r[irows[0]] > 0).any() and not X[0].any())
    return frozen(dict(pu=pu, pi=pi, r=r.astype(np.float64), P=P.astype(np.float64), X0=X0.astype(np.float64), X=X,
                       uids=shuffled_ids(rng, nu), iids=shuffled_ids(rng, N_ONE + 2, 5)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("k", RANKS)
def test_one_step_solves_a_scaled_identity(monkeypatch, mode, implicit, k):
    """cg_steps = 1 returns b / 4 (implicit: b / 16) bit for bit from an integer start, and cg_steps = 5
    the same bits: after the first step r is exactly 0, and only the rs == 0 stop keeps 0 / 0 out of x.
    The implicit item without a positive rating is +0; the items without ratings and the whole user side
    stay bitwise as set."""
    d = onestep_problem(k, implicit)
    for way in WAYS:
        with monkeypatch.context() as mp:
            if way:
                set_knob(mp, *way)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
                for steps in (1, 5):
                    for reg in REGS:
                        ctx.set_factors(L.SIDE_ITEM, d["iids"], d["X0"])
                        ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
                        if implicit:
                            ctx.als_run_implicit_cg(1, TINY, 1.0, reg, cg_steps=steps)
                        else:
                            ctx.als_run_cg(1, TINY, reg, cg_steps=steps)
                        X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
                        assert np.array_equal(bits(X[:N_ONE]), bits(d["X"])), (k, mode, way, steps, reg)
                        assert np.array_equal(bits(X[N_ONE:]), bits(d["X0"][N_ONE:]))
                        assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, d["uids"])[0]), bits(d["P"]))


# ---------------------------------------------------------------------------------------------
# 3. real-valued data against a numpy replay of the documented algorithm

NI, NU = 30, 200


@functools.lru_cache(maxsize=None)
def real_problem(k):
    """NI items with 3k/2 ratings each (at least 2) drawn from NU users with repetition (duplicate pairs are
    legal), one item and one user without ratings; ratings in {-2..5}; factors N(0, 1/k)."""
    rng = np.random.default_rng(11000 + k)
    per = max(2, 3 * k // 2)
    pi = np.repeat(np.arange(NI), per)
    pu = rng.integers(0, NU, NI * per)
    r = rng.integers(-2, 6, NI * per).astype(np.float64)
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    P = rng.normal(0, 1 / np.sqrt(k), (NU + 1, k))
    Q = rng.normal(0, 1 / np.sqrt(k), (NI + 1, k))
    return frozen(dict(pu=pu, pi=pi, r=r, P=P, Q=Q, uids=shuffled_ids(rng, NU + 1), iids=shuffled_ids(rng, NI + 1, 5),
                       irows=np.array(rows_of(pi, NI), dtype=np.int64)))


def replay(Qm, rt, x, lam, weighted, S, T, G=None, alpha=None, rev=False):
    """mfhip.h's algorithm for one row in precision T, the rating sums in CSR or in reversed order."""
    Qm, rt, x = Qm.astype(T), rt.astype(T), x.astype(T)
    if rev:
        Qm, rt = Qm[::-1], rt[::-1]
    if alpha is None:
        w, c, n = np.ones_like(rt), rt, len(rt)
    else:
        w = T(alpha) * np.abs(rt)
        c, n = np.where(rt > 0, T(1) + w, T(0)).astype(T), int((rt > 0).sum())
        if n == 0:
            return np.zeros_like(x)
    lam = T(lam) * T(n) if weighted else T(lam)
    G = None if G is None else G.astype(T)
    colsum = lambda e: (e[:, None] * Qm).sum(axis=0, dtype=T)
    gv = lambda v: G @ v if G is not None else T(0)
    r = colsum(c - w * (Qm @ x)) - gv(x) - lam * x
    p, rs = r.copy(), r @ r
    for _ in range(S):
        if not np.isfinite(rs):
            return np.full_like(x, np.nan)
        if rs == 0:
            break
        Ap = colsum(w * (Qm @ p)) + gv(p) + lam * p
        pAp = p @ Ap
        if not np.isfinite(pAp):
            return np.full_like(x, np.nan)
        if pAp == 0:
            break
        a = rs / pAp
        x, r = x + a * p, r - a * Ap
        rsn = r @ r
        p, rs = r + (rsn / rs) * p, rsn
    return x if np.isfinite(rs) else np.full_like(x, np.nan)


def replay_side(d, S, lam, reg, alpha, T, rev=False):
    rated = np.unique(d["pu"])
    G = None if alpha is None else d["P"][rated].T @ d["P"][rated]
    return np.array([replay(d["P"][d["pu"][pos]], d["r"][pos], d["Q"][t], lam, reg == L.ALS_REG_WEIGHTED, S, T, G,
                            alpha, rev).astype(np.float64) for t, pos in enumerate(d["irows"])])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", REPLAY_RANKS)
def test_half_sweep_matches_the_numpy_replay(mode, k):
    """One item half-sweep, S in {1, 3}, both regs, explicit and implicit (alpha 0.5), lambda 0.1, against the
    f64 replay.  Deterministic mode: within 4 x the largest difference between the forward and the
    reversed-order f64 replay; fast mode: within 4 x the largest difference between an f32 replay and the
    f64 one.  The ratios seen are printed (DESIGN 4.7.3 records them)."""
    d = real_problem(k)
    lam = 0.1
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
        for alpha in (None, 0.5):
            for S in (1, 3):
                for reg in REGS:
                    ref = replay_side(d, S, lam, reg, alpha, np.float64)
                    if mode == L.MODE_DETERMINISTIC_F64:
                        dist = np.abs(replay_side(d, S, lam, reg, alpha, np.float64, rev=True) - ref).max()
                    else:
                        dist = np.abs(replay_side(d, S, lam, reg, alpha, np.float32) - ref).max()
                    ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q"])
                    ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
                    if alpha is None:
                        ctx.als_run_cg(1, lam, reg, cg_steps=S)
                    else:
                        ctx.als_run_implicit_cg(1, lam, alpha, reg, cg_steps=S)
                    X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
                    err = np.abs(X[:NI] - ref).max()
                    print(f"replay k={k} mode={mode} alpha={alpha} S={S} reg={reg}: err {err:.3e} dist {dist:.3e} "
                          f"ratio {err / dist if dist else float('inf'):.2f}")
                    assert np.abs(X[:NI] - d["Q"][:NI]).max() > 1e-3          # the sweep moved the rows
                    assert err <= 4 * dist, (k, mode, alpha, S, reg, err, dist)
                    assert np.array_equal(bits(X[NI]), bits(d["Q"][NI].astype(dtype_of(mode))))  # unrated: as set


# ---------------------------------------------------------------------------------------------
# 4. invariances

def two_half_sweeps(ctx, d, alpha):
    ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
    ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q"])
    ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
    if alpha is None:
        ctx.als_run_cg(2, 0.1, cg_steps=3)
    else:
        ctx.als_run_implicit_cg(2, 0.1, alpha, cg_steps=3)
    return ctx.lookup(L.SIDE_ITEM, d["iids"])[0], ctx.lookup(L.SIDE_USER, d["uids"])[0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [33, 128])
def test_results_do_not_depend_on_launches_staging_or_the_run(monkeypatch, mode, k):
    """Two half-sweeps (S = 3), explicit and implicit: bitwise the same with als_batch=5 (many launches),
    with als_cg_stage=0 and when run again.  At k = 128 the item rows (192 ratings) exceed the LDS budget
    and the user rows fit it, so both forms run in the default pass."""
    d = real_problem(k)
    for alpha in (None, 0.5):
        with make_ctx(k, mode) as ctx:
            cap = ctx.als_cg_capacity()
            base = two_half_sweeps(ctx, d, alpha)
            again = two_half_sweeps(ctx, d, alpha)
        counts = np.bincount(d["pu"])
        assert (counts[counts > 0] <= cap).any()      # staged rows exist
        assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(base, again))
        for knob in (("als_batch", 5), ("als_cg_stage", 0)):
            with monkeypatch.context() as mp:
                set_knob(mp, *knob)
                with make_ctx(k, mode) as ctx:
                    got = two_half_sweeps(ctx, d, alpha)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(base, got)), (k, mode, alpha, knob)
        T = dtype_of(mode)                            # the rows without ratings: as set, in the context's precision
        assert np.array_equal(bits(base[0][NI]), bits(d["Q"][NI].astype(T)))
        assert np.array_equal(bits(base[1][NU]), bits(d["P"][NU].astype(T)))


# ---------------------------------------------------------------------------------------------
# 5. end to end on the smoke data

@functools.lru_cache(maxsize=None)
def smoke_data():
    d = synth.generate(300, 120, 6000, seed=3)
    return np.asarray(d.u, np.int32), np.asarray(d.i, np.int32), np.asarray(d.r, np.float64)


def objective(ctx, u, i, r, lam, alpha=None):
    """The weighted-lambda objective whose row-wise quadratics the half-sweeps minimise."""
    uid, ui = np.unique(u, return_inverse=True)
    iid, ii = np.unique(i, return_inverse=True)
    Pu, Qi = ctx.lookup(L.SIDE_USER, uid)[0], ctx.lookup(L.SIDE_ITEM, iid)[0]
    pred = np.einsum("jf,jf->j", Pu[ui], Qi[ii])
    if alpha is None:
        nu_, ni_ = np.bincount(ui), np.bincount(ii)
        fit = ((r - pred) ** 2).sum()
    else:
        pos = r > 0
        nu_, ni_ = np.bincount(ui, pos, len(uid)), np.bincount(ii, pos, len(iid))
        w = alpha * np.abs(r)
        fit = ((Pu @ Qi.T) ** 2).sum() + (w * pred ** 2 - 2 * np.where(pos, 1 + w, 0) * pred).sum()
    return fit + lam * ((nu_ * (Pu ** 2).sum(1)).sum() + (ni_ * (Qi ** 2).sum(1)).sum())


@pytest.mark.parametrize("implicit", [False, True])
def test_objective_falls_in_every_half_sweep(implicit):
    """k = 16, lambda 0.1, S = 3, 5 iterations, deterministic mode: CG from the row's current value cannot
    raise the row's quadratic, so the objective must fall in each of the 10 half-sweeps.  The final
    training RMSE is printed beside mf_als_run's (reported, not gated)."""
    u, i, r = smoke_data()
    alpha = 1.0 if implicit else None
    if implicit:
        r = r - 3.0
    p = L.default_params()
    p.num_factors = 16
    p.has_seed, p.seed = 1, 11
    with Context(p) as ctx, Context(p) as chol:
        ctx.als_prepare(u, i, r)
        obj = [objective(ctx, u, i, r, 0.1, alpha)]
        for _ in range(10):
            if implicit:
                ctx.als_run_implicit_cg(1, 0.1, alpha, cg_steps=3)
            else:
                ctx.als_run_cg(1, 0.1, cg_steps=3)
            obj.append(objective(ctx, u, i, r, 0.1, alpha))
        if implicit:
            chol.als_fit_implicit(u, i, r, 5, 0.1, alpha)
        else:
            chol.als_fit(u, i, r, 5, 0.1)
        print(f"smoke data implicit={implicit}: objective {obj[0]:.6g} -> {obj[-1]:.6g} (Cholesky "
              f"{objective(chol, u, i, r, 0.1, alpha):.6g}); training rmse CG {ctx.rmse(u, i, r)[0]:.6f} "
              f"Cholesky {chol.rmse(u, i, r)[0]:.6f}")
    assert all(b < a for a, b in zip(obj, obj[1:])), obj


def test_solvers_share_the_half_sweep_counter():
    """als_run, als_run_cg, als_run: item side, user side, item side -- each call changes exactly one side."""
    u, i, r = smoke_data()
    uid, iid = np.unique(u), np.unique(i)
    p = L.default_params()
    p.num_factors = 16
    p.has_seed, p.seed = 1, 11
    with Context(p) as ctx:
        ctx.als_prepare(u, i, r)
        state = [(ctx.lookup(L.SIDE_USER, uid)[0], ctx.lookup(L.SIDE_ITEM, iid)[0])]
        for call in (lambda: ctx.als_run(1, 0.1), lambda: ctx.als_run_cg(1, 0.1, cg_steps=3), lambda: ctx.als_run(1, 0.1),
                     lambda: ctx.als_run_implicit_cg(1, 0.1, 0.5, cg_steps=2)):
            call()
            state.append((ctx.lookup(L.SIDE_USER, uid)[0], ctx.lookup(L.SIDE_ITEM, iid)[0]))
    for h in range(4):
        same, moved = (0, 1) if h % 2 == 0 else (1, 0)    # even half-sweeps solve the item side
        assert np.array_equal(bits(state[h + 1][same]), bits(state[h][same])), h
        assert not np.array_equal(state[h + 1][moved], state[h][moved]), h


# ---------------------------------------------------------------------------------------------
# 6. bad input and arguments

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("way", WAYS)
def test_a_nan_reaches_exactly_the_rows_that_rate_it(monkeypatch, mode, way):
    d = real_problem(33)
    P = d["P"].copy()
    P[7, 5] = np.nan
    hit = np.zeros(NI + 1, bool)
    hit[np.unique(d["pi"][d["pu"] == 7])] = True
    assert hit.any() and not hit[:NI].all()
    with monkeypatch.context() as mp:
        if way:
            set_knob(mp, *way)
        with make_ctx(33, mode) as ctx:
            ctx.set_factors(L.SIDE_USER, d["uids"], P)
            ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q"])
            ctx.als_prepare(d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"])
            ctx.als_run_cg(1, 0.1, cg_steps=3)
            X = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
    assert np.isnan(X[hit]).all() and np.isfinite(X[~hit]).all()


def test_arguments_are_validated():
    """cg_steps outside 1..256, lambda, reg and alpha as the Cholesky calls check them, a run before prepare."""
    d = real_problem(3)
    u, i, r = d["uids"][d["pu"]], d["iids"][d["pi"]], d["r"]
    W = L.ALS_REG_WEIGHTED

    def code(fn, *a, **kw):
        with pytest.raises(mfhip.MFError) as e:
            fn(*a, **kw)
        return e.value.code

    with make_ctx(3, L.MODE_DETERMINISTIC_F64) as ctx:
        assert code(ctx.als_run_cg, 1, 0.1) == L.MF_ERR_STATE
        assert code(ctx.als_run_implicit_cg, 1, 0.1, 1.0) == L.MF_ERR_STATE
        assert code(ctx.als_cg_matvec, L.SIDE_ITEM, int(d["iids"][0]), 0.1, np.zeros(3)) == L.MF_ERR_STATE
        for steps in (0, -1, 257):
            assert code(ctx.als_fit_cg, u, i, r, 1, 0.1, W, steps) == L.MF_ERR_INVALID
            assert code(ctx.als_fit_implicit_cg, u, i, r, 1, 0.1, 1.0, W, steps) == L.MF_ERR_INVALID
        assert code(ctx.als_run_cg, 1, 0.1) == L.MF_ERR_STATE     # the rejected fits prepared nothing
        ctx.als_prepare(u, i, r)
        for steps in (0, -1, 257):
            assert code(ctx.als_run_cg, 1, 0.1, W, steps) == L.MF_ERR_INVALID
            assert code(ctx.als_run_implicit_cg, 1, 0.1, 1.0, W, steps) == L.MF_ERR_INVALID
        for lam in (0.0, -1.0, float("nan"), float("inf")):
            assert code(ctx.als_run_cg, 1, lam) == L.MF_ERR_INVALID
            assert code(ctx.als_run_implicit_cg, 1, lam, 1.0) == L.MF_ERR_INVALID
        for alpha in (-0.5, float("nan"), float("inf")):
            assert code(ctx.als_run_implicit_cg, 1, 0.1, alpha) == L.MF_ERR_INVALID
        assert code(ctx.als_run_cg, 1, 0.1, 7) == L.MF_ERR_INVALID
        assert code(ctx.als_run_cg, -1, 0.1) == L.MF_ERR_INVALID
        before = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
        ctx.als_run_cg(0, 0.1, cg_steps=256)               # the bounds themselves are valid
        ctx.als_run_implicit_cg(0, 0.1, 0.0, cg_steps=1)
        assert np.array_equal(bits(ctx.lookup(L.SIDE_ITEM, d["iids"])[0]), bits(before))
    model = mfhip.ALS.withSolver("cg", cg_steps=2).train((u, i, r), rank=3, iterations=2, lambda_=0.1)
    assert np.isfinite(model.predict(int(u[0]), int(i[0])))
    model.close()
