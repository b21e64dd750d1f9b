"""ALS on the device (mf_als_prepare / mf_als_run / mf_als_fit, csrc/kernels_als.hip).

The reference is numpy f64 on the host: per row A = Q^T Q + lambda' I, b = Q^T r over the row's
ratings, solved with np.linalg.solve, half-sweeps alternating with the item side first."""
import os

import numpy as np
import pytest

import mf_oracle as O
import mfhip
from als_support import (MODES, REGS, bits, make_ctx, normal_eq_reference, numpy_half_sweep, objective, rows_of,
                         shuffled_ids, small_problem)
from conftest import golden, set_knob
from mfhip import _lib as L
from mfhip import synth
from mfhip.context import Context

pytestmark = pytest.mark.gpu



# ---------------------------------------------------------------------------------------------
# 1. exact normal equations through the hook

def int_problem(rng, k):
    """Integer factors and ratings; item rows with 1000, 31, 33 and 1 ratings, user rows with 33, 31
    and 1..4, one duplicated (user, item) pair, shuffled signed ids, one id per side that is in the
    model but not in the data.  Returns dense indices, ids and factors."""
    nu, ni = 1002, 44
    pu, pi = [], []
    for item, users in ((0, range(1000)), (1, range(31)), (2, range(33)), (3, [5])):
        pu += list(users)
        pi += [item] * len(users)
    pu += [1000] * 33 + [1001] * 31   # two long user rows over items 10..42 / 10..40
    pi += list(range(10, 43)) + list(range(10, 41))
    pu.append(5)                      # (5, 3) a second time
    pi.append(3)
    pu, pi = np.array(pu), np.array(pi)
    perm = rng.permutation(len(pu))
    pu, pi = pu[perm], pi[perm]
    r = rng.integers(1, 6, len(pu)).astype(np.float64)
    uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, ni + 1, 5)
    P = rng.integers(-3, 4, (nu + 1, k)).astype(np.float64)
    Q = rng.integers(-3, 4, (ni + 1, k)).astype(np.float64)
    return pu, pi, r, uids, iids, P, Q


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 3, 10, 64, 100, 128])
def test_normal_equations_exact(monkeypatch, mode, k):
    """Entries in {-3..3}, ratings in {1..5}, lambda 0.5: every product and sum is exact in f32, so the
    device's A and b must equal numpy's exactly for every row of both sides -- whole rows and rows
    split over 16 chunks alike, under any batching.  A dropped or doubled rating shows here."""
    rng = np.random.default_rng(100 + k)
    pu, pi, r, uids, iids, P, Q = int_problem(rng, k)
    urows, irows = rows_of(pu, len(uids)), rows_of(pi, len(iids))
    assert sorted({len(x) for x in irows} & {1, 31, 33, 1000}) == [1, 31, 33, 1000]
    assert len(urows[-1]) == 0 and len(irows[-1]) == 0  # in the model, not in the data
    lam = 0.5
    sides = ((L.SIDE_USER, uids, urows, Q, pi), (L.SIDE_ITEM, iids, irows, P, pu))
    first_half = []
    for knob in (None, ("als_chunk", 64), ("als_batch", 7)):
        with monkeypatch.context() as mp:
            if knob:
                set_knob(mp, *knob)
            with make_ctx(k, mode) as ctx:
                ctx.set_factors(L.SIDE_USER, uids, P)
                ctx.set_factors(L.SIDE_ITEM, iids, Q)
                ctx.als_prepare(uids[pu], iids[pi], r)
                for side, ids, rows, F_other, other_index in sides:
                    for a, pos in enumerate(rows):
                        if not len(pos):
                            continue
                        for reg in REGS:
                            A, b = normal_eq_reference(F_other, other_index, r, pos, lam, reg, k)
                            gA, gb = ctx.als_normal_eq(side, ids[a], lam, reg)
                            assert np.array_equal(gA, A), (knob, reg, side, a)
                            assert np.array_equal(gb, b), (knob, reg, side, a)
                # the hook changes nothing
                assert np.array_equal(ctx.lookup(L.SIDE_USER, uids)[0], P)
                assert np.array_equal(ctx.lookup(L.SIDE_ITEM, iids)[0], Q)
                with pytest.raises(mfhip.MFError):  # no rating in the data
                    ctx.als_normal_eq(L.SIDE_ITEM, iids[-1], lam)
                # identical systems give identical solutions: the first half-sweep is bitwise the same
                # whole or in chunks
                ctx.als_run(1, lam)
                first_half.append(ctx.lookup(L.SIDE_ITEM, iids)[0])
                assert np.array_equal(first_half[-1][-1], Q[-1])
    for x in first_half[1:]:
        assert np.array_equal(bits(x), bits(first_half[0]))


# ---------------------------------------------------------------------------------------------
# 2. the solve, within the backward-error bound of a Cholesky solve

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,rows,lo,hi", [(3, 40, 33, 33), (10, 70, 5, 60), (64, 40, 100, 100), (128, 20, 200, 200),
                                          (33, 40, 40, 40), (80, 30, 120, 120), (100, 20, 150, 150)])
def test_solve_within_backward_error_bound(mode, k, rows, lo, hi):
    """One half-sweep (items from users).  Per solved row, with A = Q^T Q + lambda' I and b = Q^T r in
    numpy f64: ||b - A x|| <= 2 u c (||A|| ||x|| + || |Q|^T |r| ||), c = k (n + 2) + 4 k (3 k + 1) + 2:
    accumulation over n terms, Higham's bound for a Cholesky solve, the final rounding of x; the factor
    2 covers second-order terms.  Measured on an MI355X, the largest residual / bound over the rows
    of a case: k = 3: 4.3e-3 (f64) / 2.7e-3 (f32), k = 10: 2.9e-4 / 2.8e-4, k = 64: 7.5e-6 / 8.3e-6,
    k = 128: 1.8e-6 / 2.0e-6; at the other rank buckets (real-valued data where tests/test_gpu_als_ranks.py
    has the exact systems) k = 33: 2.5e-5 / 2.9e-5, k = 80: 4.2e-6 / 5.2e-6, k = 100: 3.2e-6 / 3.2e-6
    (DESIGN.md section 4.7).  The bound is sound, not sharp: in f32 at k = 128 it admits a solve with
    a trailing update of the factorisation left out; the exact systems are the sharp check."""
    rng = np.random.default_rng(7 * k + rows)
    f32 = mode == L.MODE_FAST_F32
    u_round = 2.0 ** -24 if f32 else 2.0 ** -53
    nu = 256
    counts = rng.integers(lo, hi + 1, rows)
    pu = np.concatenate([rng.choice(nu, c, replace=False) for c in counts])
    pi = np.repeat(np.arange(rows), counts)
    perm = rng.permutation(len(pu))
    pu, pi = pu[perm], pi[perm]
    r = rng.integers(1, 11, len(pu)) / 2.0
    uids, iids = shuffled_ids(rng, nu + 1), shuffled_ids(rng, rows + 2, 5)  # one user, two items unrated
    P, Q = rng.standard_normal((nu + 1, k)), rng.standard_normal((rows + 2, k))
    if f32:
        P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    irows = rows_of(pi, len(iids))
    lam = 0.1
    worst = 0.0
    for reg in REGS:
        with make_ctx(k, mode) as ctx:
            ctx.set_factors(L.SIDE_USER, uids, P)
            ctx.set_factors(L.SIDE_ITEM, iids, Q)
            ctx.als_prepare(uids[pu], iids[pi], r)
            ctx.als_run(1, lam, reg)
            X = ctx.lookup(L.SIDE_ITEM, iids)[0]
            assert np.array_equal(bits(ctx.lookup(L.SIDE_USER, uids)[0]), bits(P))  # the side not solved
            assert np.array_equal(bits(X[rows:]), bits(Q[rows:]))                    # rows with no rating
        for a in range(rows):
            pos = irows[a]
            n = len(pos)
            A, b = normal_eq_reference(P, pu, r, pos, lam, reg, k)
            x = X[a]
            assert np.isfinite(x).all()
            c = k * (n + 2) + 4 * k * (3 * k + 1) + 2
            bound = 2 * u_round * c * (np.linalg.norm(A, 2) * np.linalg.norm(x) +
                                       np.linalg.norm(np.abs(P[pu[pos]]).T @ np.abs(r[pos])))
            res = np.linalg.norm(b - A @ x)
            worst = max(worst, res / bound)
            assert res <= bound, (reg, a, res, bound)
    print(f"als residual / bound: mode {mode} k {k}: {worst:.3e}")


# ---------------------------------------------------------------------------------------------
# 3. half-sweep order and the counter

@pytest.mark.parametrize("mode", MODES)
def test_half_sweep_order_and_counter(mode):
    rng = np.random.default_rng(21)
    k, lam = 5, 0.1
    u, i, r = small_problem(rng)
    uids, iids = np.unique(u), np.unique(i)
    Q0 = rng.random((len(iids), k))
    with make_ctx(k, mode) as ctx:
        ctx.set_factors(L.SIDE_USER, uids, np.zeros((len(uids), k)))
        ctx.set_factors(L.SIDE_ITEM, iids, Q0)
        ctx.als_prepare(u, i, r)
        ctx.als_run(1, lam)  # items from the (zero) users first: a zero right-hand side
        assert not ctx.lookup(L.SIDE_ITEM, iids)[0].any()
        assert not ctx.lookup(L.SIDE_USER, uids)[0].any()
        ctx.als_run(1, lam)  # then users from the (now zero) items
        assert not ctx.lookup(L.SIDE_USER, uids)[0].any()

    def start():
        ctx = make_ctx(k, mode)
        ctx.set_factors(L.SIDE_USER, uids, rng_u)
        ctx.set_factors(L.SIDE_ITEM, iids, Q0)
        return ctx

    def both(ctx):
        return bits(ctx.factors(L.SIDE_USER)[1]), bits(ctx.factors(L.SIDE_ITEM)[1])

    rng_u = rng.random((len(uids), k))
    with start() as a, start() as b, start() as c, start() as d:
        a.als_prepare(u, i, r)
        a.als_run(2, lam)
        b.als_prepare(u, i, r)
        b.als_run(1, lam)
        b.als_run(1, lam)
        for x, y in zip(both(a), both(b)):
            assert np.array_equal(x, y)
        T = 3
        c.als_fit(u, i, r, T, lam)
        d.als_prepare(u, i, r)
        d.als_run(2 * T, lam)
        for x, y in zip(both(c), both(d)):
            assert np.array_equal(x, y)
        # the counter continues: one more half-sweep solves the item side again
        before_u = both(d)[0]
        d.als_run(1, lam)
        assert np.array_equal(both(d)[0], before_u)


# ---------------------------------------------------------------------------------------------
# 4. end to end against a numpy f64 ALS

@pytest.fixture(scope="module")
def smoke_als():
    """The smoke data, dense indices and the numpy ALS result (per mode: its start is rounded to f32
    in fast mode, as the device stores it)."""
    d = synth.generate(300, 120, 6000, seed=3)
    uids, pu = np.unique(d.u, return_inverse=True)
    iids, pi = np.unique(d.i, return_inverse=True)
    rng = np.random.default_rng(4)
    k, lam, T = 16, 0.1, 5
    P0, Q0 = rng.random((len(uids), k)), rng.random((len(iids), k))
    urows, irows = rows_of(pu, len(uids)), rows_of(pi, len(iids))
    ref = {}
    for mode in MODES:
        P, Q = P0.copy(), Q0.copy()
        if mode == L.MODE_FAST_F32:
            P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
        for _ in range(T):
            numpy_half_sweep(Q, P, irows, pu, d.r, lam)
            numpy_half_sweep(P, Q, urows, pi, d.r, lam)
        err = d.r - np.einsum("nk,nk->n", P[pu], Q[pi])
        ref[mode] = float(np.sqrt(err @ err / len(err)))
    return dict(d=d, uids=uids, iids=iids, pu=pu, pi=pi, k=k, lam=lam, T=T, P0=P0, Q0=Q0, ref=ref)


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_against_numpy_als(smoke_als, mode):
    """Measured on an MI355X: training RMSE 0.422266994 on the device and in numpy f64; the relative
    difference is 3.9e-16 in deterministic mode and 3.6e-9 in fast mode."""
    s = smoke_als
    d, k, lam, T = s["d"], s["k"], s["lam"], s["T"]

    def start():
        ctx = make_ctx(k, mode)
        ctx.set_factors(L.SIDE_USER, s["uids"], s["P0"])
        ctx.set_factors(L.SIDE_ITEM, s["iids"], s["Q0"])
        ctx.als_prepare(d.u, d.i, d.r)
        return ctx

    with start() as ctx, start() as twin:
        _, P = ctx.factors(L.SIDE_USER)
        _, Q = ctx.factors(L.SIDE_ITEM)
        obj = [objective(P, Q, s["pu"], s["pi"], d.r, lam)]
        for _ in range(2 * T):
            ctx.als_run(1, lam)
            _, P = ctx.factors(L.SIDE_USER)
            _, Q = ctx.factors(L.SIDE_ITEM)
            obj.append(objective(P, Q, s["pu"], s["pi"], d.r, lam))
        print("als objective per half-sweep:", " ".join(f"{x:.6f}" for x in obj))
        assert all(b < a for a, b in zip(obj, obj[1:])), obj  # (a)
        rmse, matched = ctx.rmse(d.u, d.i, d.r)
        rel = abs(rmse - s["ref"][mode]) / s["ref"][mode]
        print(f"als rmse: mode {mode} device {rmse:.9f} numpy {s['ref'][mode]:.9f} rel {rel:.3e}")
        assert matched == len(d.u)
        assert rel < 0.005  # (b) the project's fast-mode band
        for _ in range(2 * T):  # (c) the same calls on a second context
            twin.als_run(1, lam)
        for side in (L.SIDE_USER, L.SIDE_ITEM):
            assert np.array_equal(bits(twin.factors(side)[1]), bits(ctx.factors(side)[1]))


# ---------------------------------------------------------------------------------------------
# 5. unseen ids and the calls downstream of a fit

@pytest.mark.parametrize("mode", MODES)
def test_unseen_ids_and_downstream_calls(mode, tmp_path):
    d = synth.generate(300, 120, 6000, seed=3)
    k, lam = 16, 0.1
    uids, iids = np.unique(d.u), np.unique(d.i)
    with make_ctx(k, mode, seed=11) as a, make_ctx(k, mode, seed=11) as b:
        a.als_prepare(d.u, d.i, d.r)  # no half-sweep: the inserted rows as initialised
        b.prepare(d.u, d.i, d.r)      # mf_dsgd_prepare's initial factors
        for side, ids in ((L.SIDE_USER, uids), (L.SIDE_ITEM, iids)):
            va, fa = a.lookup(side, ids)
            vb, fb = b.lookup(side, ids)
            assert fa.all() and fb.all()
            assert np.array_equal(bits(va), bits(vb))
    with make_ctx(k, mode, seed=11) as ctx:
        ctx.als_fit(d.u, d.i, d.r, 3, lam)
        assert np.array_equal(ctx.factors(L.SIDE_USER)[0], uids)
        pred, found = ctx.predict(d.u[:200], d.i[:200])
        assert found.all() and np.isfinite(pred).all()
        rmse, matched = ctx.rmse(d.u, d.i, d.r)
        assert matched == len(d.u) and rmse < 1.0
        # recommend's scores against predict, under the rule mfhip.h states for each mode
        q = uids[:33]
        ids, sc, cnt = ctx.recommend(q, 10)
        assert (cnt == 10).all()
        pr, fd = ctx.predict(np.repeat(q, 10), ids.reshape(-1))
        assert fd.all()
        if mode == L.MODE_DETERMINISTIC_F64:
            assert np.array_equal(bits(pr), bits(sc.reshape(-1)))
        else:
            Pq = ctx.lookup(L.SIDE_USER, np.repeat(q, 10))[0]
            Qc = ctx.lookup(L.SIDE_ITEM, ids.reshape(-1))[0]
            eps = 2 * k * 2.0 ** -24 * (np.abs(Pq) * np.abs(Qc)).sum(1)  # two k-term f32 chains
            assert (np.abs(pr - sc.reshape(-1)) <= eps).all()
        path = os.path.join(tmp_path, "als.mfsnap")
        ctx.save(path)
        with make_ctx(k, mode, seed=11) as other:
            other.load(path)
            for side in (L.SIDE_USER, L.SIDE_ITEM):
                ia, va = ctx.factors(side)
                ib, vb = other.factors(side)
                assert np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))
        before = ctx.lookup(L.SIDE_USER, d.u[:50])[0]
        tu, ti = ctx.online_update(d.u[:50], d.i[:50], d.r[:50])
        assert tu == len(np.unique(d.u[:50])) and ti == len(np.unique(d.i[:50]))
        assert not np.array_equal(ctx.lookup(L.SIDE_USER, d.u[:50])[0], before)
        # a warm start: a further fit on the fitted context keeps working and inserts new ids
        ctx.als_fit(np.append(d.u, 9999).astype(np.int32), np.append(d.i, 7777).astype(np.int32),
                    np.append(d.r, 3.0), 1, lam)
        assert ctx.lookup(L.SIDE_USER, [9999])[1].all() and ctx.lookup(L.SIDE_ITEM, [7777])[1].all()


# ---------------------------------------------------------------------------------------------
# 6. errors

@pytest.mark.parametrize("mode", MODES)
def test_errors(mode):
    rng = np.random.default_rng(2)
    u, i, r = small_problem(rng)
    with make_ctx(4, mode) as ctx:
        for lam in (0.0, -1.0, float("nan")):
            with pytest.raises(mfhip.MFError) as e:
                ctx.als_fit(u, i, r, 1, lam)
            assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit(u, i, r, 1, 0.1, 7)
        assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit(u, i, r, -1, 0.1)
        assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_run(1, 0.1)
        assert e.value.code == L.MF_ERR_STATE
        assert ctx.num_factors(L.SIDE_USER) == 0  # nothing above touched the context
        # n = 0: a no-op
        e0 = np.empty(0, np.int32)
        ctx.als_fit(e0, e0, np.empty(0), 3, 0.1)
        assert ctx.num_factors(L.SIDE_USER) == 0 and ctx.num_factors(L.SIDE_ITEM) == 0
        ctx.als_prepare(u, i, r)
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_run(-1, 0.1)
        assert e.value.code == L.MF_ERR_INVALID
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_run(1, 0.1, 7)
        assert e.value.code == L.MF_ERR_INVALID
        ctx.als_run(2, 0.1)
        # a DSGD prepare rebuilds the rows: the ALS data must be prepared again
        ctx.prepare(u, i, r)
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_run(1, 0.1)
        assert e.value.code == L.MF_ERR_STATE
    with make_ctx(L.ALS_MAX_RANK + 1, mode) as ctx:
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit(u, i, r, 1, 0.1)
        assert e.value.code == L.MF_ERR_INVALID and str(L.ALS_MAX_RANK) in str(e.value)
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_prepare(u, i, r)
        assert e.value.code == L.MF_ERR_INVALID


def test_singular_system_gives_nan_and_returns():
    """A pivot that is not a positive finite number: the row is NaN and the kernel finishes."""
    k = 4
    with make_ctx(k, L.MODE_DETERMINISTIC_F64) as ctx:
        ctx.set_factors(L.SIDE_USER, [1, 2], np.full((2, k), np.inf))
        ctx.set_factors(L.SIDE_ITEM, [5, 6], np.ones((2, k)))
        ctx.als_prepare([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
        ctx.als_run(1, 0.1)
        assert np.isnan(ctx.lookup(L.SIDE_ITEM, [5, 6])[0]).all()


def test_two_device_context_is_refused():
    if L.device_count() < 2:
        pytest.skip("needs two GPUs")
    p = L.default_params()
    p.num_factors = 4
    p.num_blocks = 2
    rng = np.random.default_rng(2)
    u, i, r = small_problem(rng)
    with Context(p, n_devices=2) as ctx:
        with pytest.raises(mfhip.MFError) as e:
            ctx.als_fit(u, i, r, 1, 0.1)
        assert e.value.code == L.MF_ERR_STATE


# ---------------------------------------------------------------------------------------------
# 7. the mirror API

@pytest.mark.parametrize("mode", ["deterministic", "fast"])
def test_als_train_agrees_with_the_context(mode):
    d = synth.generate(300, 120, 6000, seed=3)
    model = mfhip.ALS.train((d.u, d.i, d.r), rank=16, iterations=3, lambda_=0.1, mode=mode, seed=11)
    try:
        with make_ctx(16, L.MODE_FAST_F32 if mode == "fast" else L.MODE_DETERMINISTIC_F64, seed=11) as ctx:
            ctx.als_fit(d.u, d.i, d.r, 3, 0.1)
            uf, pf = model.userFeatures(), model.productFeatures()
            ids, vecs = ctx.factors(L.SIDE_USER)
            assert [x for x, _ in uf] == ids.tolist()
            assert np.array_equal(bits(np.array([v for _, v in uf])), bits(vecs))
            assert [x for x, _ in pf] == ctx.factors(L.SIDE_ITEM)[0].tolist()
            pairs = list(zip(d.u[:20].tolist(), d.i[:20].tolist()))
            got = model.predict(pairs)
            want, found = ctx.predict(d.u[:20], d.i[:20])
            assert found.all() and [p[:2] for p in got] == pairs
            assert np.array_equal(bits([p[2] for p in got]), bits(want))
            assert model.predict(*pairs[0]) == want[0]
            user = int(d.u[0])
            rp = model.recommendProducts(user, 5)
            rid, rsc, rcnt = ctx.recommend([user], 5)
            assert [(a, b) for a, b, _ in rp] == [(user, int(x)) for x in rid[0, :rcnt[0]]]
            assert np.array_equal(bits([c for _, _, c in rp]), bits(rsc[0, :rcnt[0]]))
            ru = model.recommendUsers(int(d.i[0]), 5)
            assert len(ru) == 5 and all(b == int(d.i[0]) for _, b, _ in ru)
            every = model.recommendProductsForUsers(3)
            assert sorted(every) == ids.tolist() and every[user] == model.recommendProducts(user, 3)
    finally:
        model.close()


def spark_example_batches():
    g = golden("spark_example_online_spark_p2")
    out, start = [], 0
    for sz in g["batch_sizes"].tolist():
        sl = slice(start, start + sz)
        out.append((g["u"][sl], g["i"][sl], g["r"][sl]))
        start += sz
    return g, out


def test_online_offline_spark_als():
    from mfhip.combined import OnlineOfflineSpark
    g, batches = spark_example_batches()
    assert len(batches) == 3 and sum(len(b[0]) for b in batches) == 47
    k, lr, P, iters = int(g["k"]), float(g["lr"]), int(g["partitions"]), 4
    m = OnlineOfflineSpark(k, lr, num_partitions=P, offline_every=2, iterations=iters, offline_algorithm="ALS")
    try:
        flags = []
        for b, (u, i, r) in enumerate(batches, start=1):
            uu, iu, offline = m.process(u, i, r)
            flags.append(offline)
            if offline:  # ALS.train(history, k, iterations, 0.1): every vector is emitted
                hu, hi, hr = (np.concatenate([x[c] for x in batches[:b]]) for c in range(3))
                assert set(uu) == set(hu.tolist()) and set(iu) == set(hi.tolist())
                with make_ctx(k, L.MODE_DETERMINISTIC_F64) as ctx:
                    ctx.als_fit(hu, hi, hr, iters, 0.1)
                    for side, got in ((L.SIDE_USER, uu), (L.SIDE_ITEM, iu)):
                        ids, vecs = ctx.factors(side)
                        for x, v in zip(ids.tolist(), vecs):
                            assert np.array_equal(bits(got[x]), bits(v))
            else:
                assert set(uu) == set(u.tolist()) and set(iu) == set(i.tolist())
        assert flags == [False, True, False]
    finally:
        m.close()
    with pytest.raises(ValueError):
        OnlineOfflineSpark(k, lr, offline_algorithm="SVD")


def test_online_offline_spark_dsgd_unchanged():
    """offline_algorithm="DSGD" (and the default) keep the behaviour from before the ALS branch: the
    recorded factors of the online-only run, and the oracle's sweeps around an offline refit."""
    from mfhip.combined import OnlineOfflineSpark
    g, batches = spark_example_batches()
    k, lr, P, iters = int(g["k"]), float(g["lr"]), int(g["partitions"]), 1
    for kw in ({}, {"offline_algorithm": "DSGD"}):
        m = OnlineOfflineSpark(k, lr, num_partitions=P, offline_every=10, **kw)
        for u, i, r in batches:
            assert m.process(u, i, r)[2] is False
        ids, vecs = m.ctx.factors(L.SIDE_USER)
        assert np.array_equal(ids, g["user_ids"]) and np.array_equal(vecs, g["user_factors"])
        ids, vecs = m.ctx.factors(L.SIDE_ITEM)
        assert np.array_equal(ids, g["item_ids"]) and np.array_equal(vecs, g["item_factors"])
        m.close()
    m = OnlineOfflineSpark(k, lr, num_partitions=P, offline_every=2, iterations=iters, offline_algorithm="DSGD")
    users, items, hist = {}, {}, []
    for b, (u, i, r) in enumerate(batches, start=1):
        rs = list(zip(u.tolist(), i.tolist(), r.tolist()))
        hist += rs
        uu, iu, offline = m.process(u, i, r)
        assert offline == (b == 2)
        if offline:
            users, items = {}, {}
            O.spark_sweep(hist, users, items, k, lr, P, iters)
        else:
            O.spark_sweep(rs, users, items, k, lr, P, 1)
        for x, v in uu.items():
            assert np.isfinite(v).all() and np.array_equal(v, np.array(users[x])), (b, "user", x)
        for x, v in iu.items():
            assert np.isfinite(v).all() and np.array_equal(v, np.array(items[x])), (b, "item", x)
    m.close()
