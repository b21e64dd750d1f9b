"""Parity of the HIP DSGD path (libmfhip on the GPU) against the CPU oracle."""
import numpy as np
import pytest

import coracle
import mf_oracle as O
import mfhip
from conftest import experiments_built, golden, set_knob
from mfhip import _lib as L
from mfhip import synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def needs_experiments():
    """Hot-item replicas (MFHIP_ITEM_SPLIT) exist only in an EXPERIMENTS=1 build of libmfhip."""
    if not experiments_built():
        pytest.skip("libmfhip built without MFHIP_EXPERIMENTS (make EXPERIMENTS=1)")


def params(k, iterations, nb, seed, mode=L.MODE_DETERMINISTIC_F64, lam=1.0, lr=0.001, fast_waves=0, has_seed=1,
           blocking=L.BLOCKING_REFERENCE):
    p = L.default_params()
    p.num_factors, p.iterations, p.num_blocks, p.seed, p.mode = k, iterations, nb, seed, mode
    p.lambda_, p.learning_rate, p.fast_waves, p.has_seed = lam, lr, fast_waves, has_seed
    p.fast_blocking = blocking
    return p


def assert_factors_equal(ctx, g):
    ids, vecs = ctx.factors(L.SIDE_USER)
    assert np.array_equal(ids, g["user_ids"])
    assert np.array_equal(vecs, g["user_factors"]), np.abs(vecs - g["user_factors"]).max()
    ids, vecs = ctx.factors(L.SIDE_ITEM)
    assert np.array_equal(ids, g["item_ids"])
    assert np.array_equal(vecs, g["item_factors"]), np.abs(vecs - g["item_factors"]).max()


@pytest.mark.parametrize("name", ["spark_example_dsgd_n1", "spark_example_dsgd_n2", "spark_example_dsgd_n3",
                                  "synthetic1k_dsgd_n3", "synthetic1k_dsgd_n4_seed_neg", "ml100k_like_dsgd_n4"])
def test_deterministic_fit_bit_exact_vs_golden(name):
    g = golden(name)
    with mfhip.Context(params(int(g["k"]), int(g["iterations"]), int(g["n_blocks"]), int(g["seed"]),
                              lam=float(g["lam"]), lr=float(g["lr"]))) as ctx:
        ctx.fit(g["u"], g["i"], g["r"])
        assert_factors_equal(ctx, g)
        if "test_u" in g:
            pred, found = ctx.predict(g["pred_u"], g["pred_i"])
            assert found.all() and np.array_equal(pred, g["pred"])  # predictRating ddot, bit-exact
            rm, cnt = ctx.rmse(g["test_u"], g["test_i"], g["test_r"])
            assert cnt == int(g["test_matched"]) and abs(rm - float(g["test_rmse"])) <= 1e-12 * max(1, rm)
            risk = ctx.empirical_risk(g["test_u"], g["test_i"], g["test_r"], float(g["lam"]))
            assert abs(risk - float(g["risk"])) <= 1e-9 * abs(float(g["risk"]))


def test_mirror_api_round_trip():
    g = golden("spark_example_dsgd_n3")
    ratings = list(zip(g["u"].tolist(), g["i"].tolist(), g["r"].tolist()))
    sgd = mfhip.DSGDforMF().setNumFactors(4).setIterations(10).setBlocks(3).setSeed(0)
    sgd.fit(ratings)
    users, items = sgd.factorsOption
    assert [f.id for f in users] == g["user_ids"].tolist()
    assert np.array_equal(np.stack([f.vector for f in items]), g["item_factors"])
    out = sgd.predict([(2, 13), (1, 1), (99, 1)])   # unknown user dropped (inner join)
    assert [(a, b) for a, b, _ in out] == [(2, 13), (1, 1)]


@pytest.mark.parametrize("k,nb,seed", [(1, 2, 0), (64, 4, 5), (100, 2, 1), (128, 8, 0), (130, 3, 2), (256, 2, 9)])
def test_deterministic_vs_c_oracle_shapes(k, nb, seed):
    d = synth.generate(700, 300, 15000, seed=seed + 10)
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=k, iterations=2, n_blocks=nb, seed=seed, lam=0.9, lr=0.002, threads=4)
    with mfhip.Context(params(k, 2, nb, seed, lam=0.9, lr=0.002)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        for side in (0, 1):
            ids, vecs = ctx.factors(side)
            rids, rvecs = m.factors(side)
            assert np.array_equal(ids, rids)
            assert np.array_equal(vecs, rvecs)


@pytest.mark.parametrize("mode,k,seed", [(L.MODE_DETERMINISTIC_F64, 10, 0), (L.MODE_DETERMINISTIC_F64, 130, -77),
                                         (L.MODE_FAST_F32, 128, 3), (L.MODE_FAST_F32, 64, 0)])
def test_device_factor_init_bit_exact(mode, k, seed):
    """Initial rows generated on the GPU (launch_jvm_init_rows, LCG jump-ahead) equal k x nextDouble
    of new Random(id ^ seed) (DSGDforMF.scala:548-549) -- f64 bitwise, f32 = the rounded double --
    incl. negative ids and seed, before any superstep runs."""
    d = synth.generate(500, 200, 6000, seed=21)
    u = d.u.copy()
    u[::97] = -u[::97] - 5  # negative ids
    with mfhip.Context(params(k, 1, 3, seed, mode=mode)) as ctx:
        ctx.prepare(u, d.i, d.r)
        ctx.sync()
        for side in (0, 1):
            ids, vecs = ctx.factors(side)
            want = np.array([O.random_factors(k, O.JavaRandom(int(x) ^ seed)) for x in ids])
            if mode == L.MODE_FAST_F32:
                want = want.astype(np.float32).astype(np.float64)
            assert np.array_equal(vecs, want)


@pytest.mark.parametrize("method,arg", [(1, 0.0), (2, 50.0), (3, 0.5), (4, 0.7)])
def test_learning_rate_methods_bit_exact(method, arg):
    d = synth.generate(200, 100, 4000, seed=4)
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=8, iterations=3, n_blocks=2, seed=1, lr=0.003, lr_method=method,
                         lr_arg=arg)
    p = params(8, 3, 2, 1, lr=0.003)
    p.lr_method, p.lr_arg = method, arg
    with mfhip.Context(p) as ctx:
        ctx.fit(d.u, d.i, d.r)
        assert np.array_equal(ctx.factors(0)[1], m.factors(0)[1])


@pytest.mark.parametrize("shards", [2, 4])
def test_multi_shard_ring_bit_exact(shards):
    """n blocks over several shards (here virtual shards on device 0): the item-block ring must give the
    same bits as one device (deterministic results identical at 1/2/4/8 GPUs)."""
    d = synth.generate(900, 400, 30000, seed=21)
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=32, iterations=2, n_blocks=4, seed=3, threads=4)
    with mfhip.Context(params(32, 2, 4, 3), devices=[0] * shards) as ctx:
        ctx.fit(d.u, d.i, d.r)
        for side in (0, 1):
            assert np.array_equal(ctx.factors(side)[1], m.factors(side)[1])
        pred, found = ctx.predict(d.u[:500], d.i[:500])
        rp, rf = m.predict(d.u[:500], d.i[:500])
        assert np.array_equal(pred, rp) and np.array_equal(found, rf)


def test_staged_run_and_resume_equal_one_shot():
    d = synth.generate(300, 150, 8000, seed=2)
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=16, iterations=3, n_blocks=3, seed=4)
    with mfhip.Context(params(16, 3, 3, 4)) as ctx:
        ctx.prepare(d.u, d.i, d.r)
        ctx.run(4)
        assert ctx.superstep == 4
        uids, uv = ctx.factors(0)
        iids, iv = ctx.factors(1)
    with mfhip.Context(params(16, 3, 3, 4)) as ctx2:   # checkpoint restore
        ctx2.prepare(d.u, d.i, d.r)
        ctx2.set_factors(0, uids, uv)
        ctx2.set_factors(1, iids, iv)
        ctx2.superstep = 4
        ctx2.run(5)
        for side in (0, 1):
            assert np.array_equal(ctx2.factors(side)[1], m.factors(side)[1])


def test_staged_runs_take_over_prebuilt_supersteps():
    """A deterministic run builds the next run's first supersteps ahead (dsgd_det.cpp det_run): staged runs of
    1-3 supersteps each take them over, a restart or a factor upload drops them, and every path equals the
    oracle's one-shot fit bit for bit."""
    d = synth.generate(300, 150, 8000, seed=2)
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=16, iterations=3, n_blocks=3, seed=4)
    with mfhip.Context(params(16, 3, 3, 4)) as ctx:
        ctx.prepare(d.u, d.i, d.r)
        for n in (2, 1, 3, 3):
            ctx.run(n)
        assert ctx.superstep == 9
        for side in (0, 1):
            assert np.array_equal(ctx.factors(side)[1], m.factors(side)[1])
        ctx.restart()  # superstep 0 again: the builds made for superstep 10 are dropped
        ctx.run(4)
        uids, uv = ctx.factors(0)
        iids, iv = ctx.factors(1)
        ctx.set_factors(0, uids, uv)  # same values back: the layouts may change, builds are dropped
        ctx.set_factors(1, iids, iv)
        ctx.run(5)
        for side in (0, 1):
            assert np.array_equal(ctx.factors(side)[1], m.factors(side)[1])


def test_snapshot_file_resume_bit_exact(tmp_path):
    """mf_save_model / mf_load_model (TemporaryPath persistence, DSGDforMF.scala:291-296, 330-349):
    4 supersteps, snapshot to disk, a fresh context resumes and finishes == the oracle's one-shot fit;
    with more than 64 rows per side the load takes the bulk-upload path."""
    d = synth.generate(300, 150, 8000, seed=2)
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=16, iterations=3, n_blocks=3, seed=4)
    snap = str(tmp_path / "model.mfsnap")
    with mfhip.Context(params(16, 3, 3, 4)) as ctx:
        ctx.prepare(d.u, d.i, d.r)
        ctx.run(4)
        ctx.save(snap)
    with mfhip.Context(params(16, 3, 3, 4)) as ctx2:
        ctx2.prepare(d.u, d.i, d.r)
        step = ctx2.load(snap)
        assert step == 4
        ctx2.superstep = step
        ctx2.run(5)
        for side in (0, 1):
            ids, vecs = ctx2.factors(side)
            rids, rvecs = m.factors(side)
            assert np.array_equal(ids, rids) and np.array_equal(vecs, rvecs)
    with mfhip.Context(params(8, 1, 1, 0)) as bad:
        with pytest.raises(mfhip.MFError, match="rank"):
            bad.load(snap)


@pytest.mark.parametrize("k,kern", [(12, "sweep"), (64, "sweep"), (64, "level"), (128, "sweep")])
def test_block_update_exact(monkeypatch, k, kern):
    """mf_block_update (the Flink-resident updateLocalFactors, DSGDforMF.scala:378-418) == the C
    oracle's sequential order, bitwise: on the persistent split sweep at k = 64 / 128 (the one-block
    superstep), and one launch per dependency level at k = 12 and with MFHIP_TEST det_kernel=level."""
    set_knob(monkeypatch, "det_kernel", kern)
    rng = np.random.default_rng(8)
    nu, ni, n = 30, 20, 400
    uidx = rng.integers(0, nu, n).astype(np.int32)
    iidx = rng.integers(0, ni, n).astype(np.int32)
    r = rng.random(n) * 5
    users, items = rng.random((nu, k)), rng.random((ni, k))
    uom = np.bincount(uidx, minlength=nu).astype(np.int32) + 1
    iom = np.bincount(iidx, minlength=ni).astype(np.int32) + 1
    a = mfhip.block_update(r, uidx, iidx, users, uom, items, iom, k, 2, 7, 5, 0.01, 0, 0.0, 1.0)
    b = coracle.block_update(r, uidx, iidx, users, uom, items, iom, k, 2, 7, 5, 0.01, 0, 0.0, 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_block_update_1m_hot_block_bit_exact():
    """One NFLX-shaped rating block of 1.2M ratings (Zipf users and items, one item in ~4% of the
    ratings, heavy users) through mf_block_update at k = 128: one persistent split-sweep launch,
    bitwise the C oracle's block update (new Random(iteration ^ ratingBlockId ^ seed) shuffle, F2J
    fold, no FMA)."""
    k = 128
    d = synth.generate(60000, 2200, 1_200_000, seed=17, test_fraction=0.0)
    rng = np.random.default_rng(17)
    uidx, iidx, r = d.u.copy(), d.i.copy(), d.r.copy()
    iidx[rng.random(len(iidx)) < 0.04] = 5  # a hot item: a ~48k-update chain
    nu, ni = int(uidx.max()) + 1, int(iidx.max()) + 1
    users, items = rng.random((nu, k)) * 0.3, rng.random((ni, k)) * 0.3
    uom = np.bincount(uidx, minlength=nu).astype(np.int32) + 1
    iom = np.bincount(iidx, minlength=ni).astype(np.int32) + 1
    p = L.default_params()
    p.num_factors = k
    with mfhip.Context(p) as ctx:
        a = mfhip.block_update(r, uidx, iidx, users, uom, items, iom, k, 3, 9, 42, 0.001, 0, 0.0, 1.0, ctx=ctx)
        st = ctx.stats()
    assert st["kernel_launches"] == 1 and st["levels"] == 0  # the persistent sweep ran
    b = coracle.block_update(r, uidx, iidx, users, uom, items, iom, k, 3, 9, 42, 0.001, 0, 0.0, 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])



def test_edge_cases():
    with mfhip.Context(params(4, 2, 3, 0)) as ctx:   # empty input: empty model
        ctx.fit(np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0))
        assert ctx.num_factors(0) == 0
        pred, found = ctx.predict([1], [1])
        assert not found.any()
    # more blocks than ids -> empty rating blocks pass through (DSGDforMF.scala:482-487)
    R = [(1, 1, 3.0), (2, 2, 4.0), (3, 1, 5.0)]
    us, it = O.dsgd_fit(R, k=3, iterations=4, n_blocks=7, seed=1)
    with mfhip.Context(params(3, 4, 7, 1)) as ctx:
        ctx.fit([a for a, _, _ in R], [b for _, b, _ in R], [c for _, _, c in R])
        ids, vecs = ctx.factors(0)
        assert np.array_equal(vecs, np.array([us[x] for x in ids.tolist()]))
    with pytest.raises(mfhip.MFError):
        mfhip.Context(params(4, 1, 3, 0), devices=[0, 0])  .fit([1], [1], [1.0])  # 3 blocks on 2 shards


def fast_replay_reference(d, k, nb, seed, G, iterations, lam, lr):
    """Serialise the fast plan (superstep, sub-step, group, position) and replay it in f64."""
    from test_schedule import fast_plan_window, fast_schedule
    b, t, g, p = fast_schedule(d.u, d.i, nb, seed, G, window=fast_plan_window(k), k=k)
    uids = np.unique(d.u); iids = np.unique(d.i)
    urow = np.searchsorted(uids, d.u).astype(np.int32)
    irow = np.searchsorted(iids, d.i).astype(np.int32)
    U = np.stack([O.random_factors(k, O.JavaRandom(int(x) ^ seed)) for x in uids])
    I = np.stack([O.random_factors(k, O.JavaRandom(int(x) ^ seed)) for x in iids])
    ru = lam / np.bincount(urow).astype(np.float64)
    ri = lam / np.bincount(irow).astype(np.float64)
    for s in range(1, iterations * nb + 1):
        eta = O.learning_rate(0, lr, s // nb + 1, lam)
        in_stratum = ((b // nb + s - 1) % nb) == (b % nb)
        idx = np.where(in_stratum)[0]
        order = idx[np.lexsort((p[idx], g[idx], b[idx], t[idx]))]
        coracle.dsgd_apply(urow[order], irow[order], d.r[order], U, I, ru, ri, k, eta)
    return uids, U, iids, I


def fast_split_replay_reference(d, k, nb, seed, G, iterations, lam, lr, split):
    """fast_replay_reference with hot-item replicas: per superstep every replica row starts as a
    copy of its item's row, takes its chain of updates, and the item ends as the mean of its R
    chains (plan.hpp SplitItem)."""
    from test_schedule import fast_plan_window, fast_schedule_split
    b, t, g, p, rep = fast_schedule_split(d.u, d.i, nb, seed, G, split, window=fast_plan_window(k), k=k)
    uids = np.unique(d.u); iids = np.unique(d.i)
    urow = np.searchsorted(uids, d.u).astype(np.int32)
    irow = np.searchsorted(iids, d.i).astype(np.int32)
    U = np.stack([O.random_factors(k, O.JavaRandom(int(x) ^ seed)) for x in uids])
    I = np.stack([O.random_factors(k, O.JavaRandom(int(x) ^ seed)) for x in iids])
    ru = lam / np.bincount(urow).astype(np.float64)
    ri = lam / np.bincount(irow).astype(np.float64)
    # one physical row per (rating block, item, replica >= 1), appended after the items
    keys = sorted({(int(x), int(y), int(z)) for x, y, z in zip(b[rep > 0], irow[rep > 0], rep[rep > 0])})
    extra = {kk: len(iids) + n for n, kk in enumerate(keys)}
    prow = irow.copy()
    for j in np.where(rep > 0)[0]:
        prow[j] = extra[(int(b[j]), int(irow[j]), int(rep[j]))]
    Ix = np.concatenate([I, np.zeros((len(keys), k))])
    rix = np.concatenate([ri, np.array([ri[kk[1]] for kk in keys])])
    for s in range(1, iterations * nb + 1):
        eta = O.learning_rate(0, lr, s // nb + 1, lam)
        in_stratum = ((b // nb + s - 1) % nb) == (b % nb)
        live = [kk for kk in keys if ((kk[0] // nb + s - 1) % nb) == (kk[0] % nb)]
        for kk in live:
            Ix[extra[kk]] = Ix[kk[1]]
        idx = np.where(in_stratum)[0]
        order = idx[np.lexsort((p[idx], g[idx], b[idx], t[idx]))]
        coracle.dsgd_apply(urow[order], prow[order], d.r[order], U, Ix, ru, rix, k, eta)
        chains = {}
        for kk in live:
            chains.setdefault((kk[0], kk[1]), []).append(extra[kk])
        for (_, it), rows in chains.items():
            Ix[it] = (Ix[it] + Ix[rows].sum(0)) / (len(rows) + 1)
    return uids, U, iids, Ix[:len(iids)]


def hot_item_data(seed=5):
    """A synthetic with one item rated by most users (and some users rating it twice), so some
    cells are a single long item run (the pair kernel's lean path) next to mixed cells."""
    d = synth.generate(400, 120, 12000, seed=seed)
    rng = np.random.default_rng(seed)
    hu = np.concatenate([rng.permutation(400)[:350], rng.integers(0, 400, 40)]).astype(np.int32)
    d.u = np.concatenate([d.u, hu])
    d.i = np.concatenate([d.i, np.full(len(hu), 7, np.int32)])
    d.r = np.concatenate([d.r, rng.integers(1, 6, len(hu)).astype(np.float64)])
    return d


@pytest.mark.parametrize("k,nb,G,hot", [(64, 2, 8, False), (128, 3, 4, False), (40, 2, 4, False), (256, 1, 8, False),
                                        (128, 1, 4, True), (64, 2, 8, True)])
def test_fast_kernel_equals_its_schedule(k, nb, G, hot):
    """The f32 sweep kernel (register ring, forwarding, item runs, pairs) == sequential replay of its plan."""
    d = hot_item_data(k) if hot else synth.generate(400, 120, 12000, seed=k)
    seed, lam, lr, iters = 3, 1.0, 0.002, 2
    uids, U, iids, I = fast_replay_reference(d, k, nb, seed, G, iters, lam, lr)
    with mfhip.Context(params(k, iters, nb, seed, mode=L.MODE_FAST_F32, lam=lam, lr=lr, fast_waves=-G,
                              blocking=L.BLOCKING_REFERENCE)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        a_ids, a_u = ctx.factors(0)
        b_ids, a_i = ctx.factors(1)
    assert np.array_equal(a_ids, uids) and np.array_equal(b_ids, iids)
    np.testing.assert_allclose(a_u, U, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(a_i, I, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("k,nb,G,split", [(128, 1, 4, 60), (64, 2, 8, 40), (256, 1, 8, 100), (40, 2, 4, 50)])
@pytest.mark.usefixtures("needs_experiments")
def test_hot_item_replicas_equal_their_schedule(monkeypatch, k, nb, G, split):
    """MFHIP_ITEM_SPLIT (experiment): fork (replica rows), the sweep over replica rows, and the averaging join
    == a sequential f64 replay of the same plan with the same fork/join."""
    d = hot_item_data(k)
    seed, lam, lr, iters = 3, 1.0, 0.002, 2
    uids, U, iids, I = fast_split_replay_reference(d, k, nb, seed, G, iters, lam, lr, split)
    monkeypatch.setenv("MFHIP_ITEM_SPLIT", str(split))
    with mfhip.Context(params(k, iters, nb, seed, mode=L.MODE_FAST_F32, lam=lam, lr=lr, fast_waves=-G)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        a_ids, a_u = ctx.factors(0)
        b_ids, a_i = ctx.factors(1)
    assert np.array_equal(a_ids, uids) and np.array_equal(b_ids, iids)
    np.testing.assert_allclose(a_u, U, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(a_i, I, rtol=2e-4, atol=2e-5)


@pytest.mark.usefixtures("needs_experiments")
def test_hot_item_replicas_systolic_equals_substep(monkeypatch):
    """Replicas under the systolic sweep (automatic per-block groups) == per-sub-step launches, bitwise."""
    d = synth.generate(20000, 3000, 400_000, seed=4)
    outs = []
    set_knob(monkeypatch, "block_groups", "0")  # the same uniform G for both drivers
    monkeypatch.setenv("MFHIP_ITEM_SPLIT", "300")
    for sys_on in ("1", "0"):
        set_knob(monkeypatch, "pair_sys", sys_on)
        with mfhip.Context(params(128, 2, 4, 1, mode=L.MODE_FAST_F32)) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1], ctx.stats()["kernel_launches"]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2] < outs[1][2]


@pytest.mark.usefixtures("needs_experiments")
def test_hot_item_replicas_multi_shard_matches_single(monkeypatch):
    """Replica rows are per-shard scratch outside the rotated item blocks: virtual shards agree."""
    d = synth.generate(3000, 600, 100_000, seed=12)
    outs = []
    monkeypatch.setenv("MFHIP_ITEM_SPLIT", "200")
    for devs in ([0], [0, 0]):
        with mfhip.Context(params(64, 2, 4, 1, mode=L.MODE_FAST_F32), devices=devs) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.usefixtures("needs_experiments")
def test_hot_item_replicas_rmse_within_one_percent_of_reference(monkeypatch):
    """Replicas relax the hot items' sequential chains, so they change the trajectory (averaged
    chains): an opt-in with a looser bar than the default fast mode -- held-out RMSE after 10
    epochs within 1% of the f64 reference order (measured: +0.73% here; on the NFLX-shaped
    synthetic replicas land 8% BELOW the reference, 0.699 vs 0.7575)."""
    d = synth.generate(20000, 3000, 1_000_000, seed=11)
    (tu, ti, tr), (eu, ei, er) = d.split()
    m = coracle.dsgd_fit(tu, ti, tr, k=64, iterations=10, n_blocks=4, seed=0, threads=4)
    ref, _ = m.rmse(eu, ei, er)
    monkeypatch.setenv("MFHIP_ITEM_SPLIT", "500")
    with mfhip.Context(params(64, 10, 4, 0, mode=L.MODE_FAST_F32)) as ctx:
        ctx.fit(tu, ti, tr)
        fast, cnt = ctx.rmse(eu, ei, er)
    assert abs(fast - ref) / ref < 0.01, (fast, ref)


@pytest.mark.parametrize("k", [32, 64])
def test_fast_mode_rmse_within_half_percent_of_reference(k):
    """North-star fast-mode bar: held-out RMSE after 10 epochs within 0.5% of the f64 reference order
    (k=32: one-update-per-step kernel, k=64: pair kernel)."""
    d = synth.generate(20000, 3000, 1_000_000, seed=11)
    (tu, ti, tr), (eu, ei, er) = d.split()
    m = coracle.dsgd_fit(tu, ti, tr, k=k, iterations=10, n_blocks=4, seed=0, threads=4)
    ref, _ = m.rmse(eu, ei, er)
    with mfhip.Context(params(k, 10, 4, 0, mode=L.MODE_FAST_F32)) as ctx:
        ctx.fit(tu, ti, tr)
        fast, cnt = ctx.rmse(eu, ei, er)
    assert abs(fast - ref) / ref < 0.005, (fast, ref)


@pytest.mark.parametrize("shards", [2, 4])
def test_fast_multi_shard_matches_single(shards):
    d = synth.generate(2000, 500, 60000, seed=9)
    outs = []
    for devs in ([0], [0] * shards):
        with mfhip.Context(params(64, 2, 4, 1, mode=L.MODE_FAST_F32, fast_waves=-8), devices=devs) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_profiling_stats():
    d = synth.generate(3000, 800, 50000, seed=5)
    with mfhip.Context(params(128, 1, 2, 0, mode=L.MODE_FAST_F32)) as ctx:
        ctx.prepare(d.u, d.i, d.r)
        ctx.set_profiling(True)
        ctx.run(2)
        st = ctx.stats()
    # (java.util.Random's first draw for small consecutive ids is nearly constant, so with n=2
    # the reference's blocking puts almost every id in one block: some supersteps are empty)
    assert st["updates"] == 50000 and st["supersteps"] == 2
    assert st["kernel_launches"] > 0 and st["kernel_ms"] > 0
    assert st["algorithmic_bytes"] == 50000 * (16 * 128 + 20)


@pytest.mark.parametrize("k,nb,G,hot,n", [(64, 2, 8, False, 12000), (128, 3, 4, True, 12000), (256, 1, 8, True, 12000),
                                          (64, 4, 0, False, 1_000_000), (128, 8, 0, True, 400_000)])
def test_systolic_sweep_equals_substep_launches(monkeypatch, k, nb, G, hot, n):
    """k_sweep_pair_sys (one launch per superstep, neighbour hand-offs through progress words and
    sc1 user-row traffic) runs exactly the cells of the per-sub-step launches in the same order:
    factors must be bitwise equal.  A stale user row read across a hand-off would break this."""
    if hot:
        d = hot_item_data(k)
        if n > 20000:  # scale up: many users, one very hot item among a Zipf tail
            big = synth.generate(n // 20, 2000, n, seed=k)
            hu = np.arange(0, n // 20, 2, dtype=np.int32)
            d.u = np.concatenate([big.u, hu])
            d.i = np.concatenate([big.i, np.full(len(hu), 7, np.int32)])
            d.r = np.concatenate([big.r, np.ones(len(hu))])
    else:
        d = synth.generate(max(400, n // 50), max(120, n // 300), n, seed=k)
    outs = []
    set_knob(monkeypatch, "block_groups", "0")  # the same uniform G for both drivers
    for sys_on in ("0", "1"):
        set_knob(monkeypatch, "pair_sys", sys_on)
        with mfhip.Context(params(k, 2, nb, 3, mode=L.MODE_FAST_F32, fast_waves=-G if G else 0,
                                  blocking=L.BLOCKING_REFERENCE)) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1], ctx.stats()["kernel_launches"]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[1][2] < outs[0][2]  # the systolic path really ran (one launch per superstep)


@pytest.mark.parametrize("config,scale,pair_sys", [("ML20M", 0.1, 1), ("NFLX", 0.05, 1), ("YAHOO", 0.05, 1),
                                                   ("YAHOO", 0.05, 0)])
def test_fast_fit_repeats_itself_after_restart(monkeypatch, config, scale, pair_sys):
    """A fast fit has no atomics and a fixed plan, so mf_dsgd_restart + the same epochs must give
    the same factors bit for bit (k = 64 / 128 / 256 through the BASELINE-shaped synthetics, whose
    Zipf heads make single-run cells; the systolic launch and the per-sub-step launches).  The
    round-4 k = 256 lean single-run path did not: its compiled code rewrote the data VGPRs of
    16-B user-row stores right behind the store, which gfx950 does not survive under load
    (profiles/r05_store_data_hazard.txt); the stores now pin two wait states."""
    set_knob(monkeypatch, "pair_sys", str(pair_sys))
    d = synth.config(config, scale)
    (u, i, r), _ = d.split()
    _, _, _, k, nb = synth.CONFIGS[config]
    p = L.default_params()
    p.num_factors, p.num_blocks, p.iterations, p.seed, p.mode = k, nb, 2, 0, L.MODE_FAST_F32
    with mfhip.Context(p) as ctx:
        ctx.fit(u, i, r)
        first = (ctx.factors(0)[1], ctx.factors(1)[1])
        for _ in range(2):
            ctx.restart()
            ctx.run(2 * nb)
            again = (ctx.factors(0)[1], ctx.factors(1)[1])
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("k", [64, 128, 256])
@pytest.mark.parametrize("pair_sys", [0, 1])
def test_fast_fit_repeats_itself_hot_item(monkeypatch, k, pair_sys):
    """The lean single-run path (one long item run per cell) and the generic step repeat themselves
    after a restart, bit for bit, at every row width and in both launch forms."""
    set_knob(monkeypatch, "pair_sys", str(pair_sys))
    d = hot_item_data(k)
    with mfhip.Context(params(k, 3, 2, 3, mode=L.MODE_FAST_F32, lam=1.0, lr=0.002, fast_waves=-4,
                              blocking=L.BLOCKING_REFERENCE)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        first = (ctx.factors(0)[1], ctx.factors(1)[1])
        for _ in range(2):
            ctx.restart()
            ctx.run(3 * 2)
            assert np.array_equal(first[0], ctx.factors(0)[1]) and np.array_equal(first[1], ctx.factors(1)[1])


def test_systolic_multi_shard_matches_single(monkeypatch):
    set_knob(monkeypatch, "pair_sys", "1")
    d = synth.generate(2000, 500, 60000, seed=9)
    outs = []
    for devs in ([0], [0, 0]):
        with mfhip.Context(params(64, 2, 4, 1, mode=L.MODE_FAST_F32, fast_waves=-8), devices=devs) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("k,nb,waves,hot", [(64, 2, 64, False), (128, 3, 96, True), (64, 4, 256, True)])
def test_systolic_per_block_groups_equal_their_schedule(monkeypatch, k, nb, waves, hot):
    """Automatic G: every rating block of a superstep gets its own G_j x G_j rotation
    (choose_block_groups, budget `waves` per superstep); the kernel == sequential replay of that plan."""
    set_knob(monkeypatch, "sys_waves", str(waves))
    d = hot_item_data(k) if hot else synth.generate(3000, 600, 60000, seed=k)
    seed, lam, lr, iters = 3, 1.0, 0.002, 2
    uids, U, iids, I = fast_replay_reference(d, k, nb, seed, -waves, iters, lam, lr)
    with mfhip.Context(params(k, iters, nb, seed, mode=L.MODE_FAST_F32, lam=lam, lr=lr, fast_waves=0,
                              blocking=L.BLOCKING_REFERENCE)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        a_ids, a_u = ctx.factors(0)
        b_ids, a_i = ctx.factors(1)
        assert ctx.stats()["kernel_launches"] <= iters * nb  # one systolic launch per superstep
    assert np.array_equal(a_ids, uids) and np.array_equal(b_ids, iids)
    np.testing.assert_allclose(a_u, U, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(a_i, I, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("build", ["device", "host", "mixed"])
@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("k,nb,shards", [(64, 4, 1), (128, 4, 2), (100, 3, 1), (256, 2, 2)])
def test_deterministic_persistent_sweep_bit_exact_hot_items(monkeypatch, k, nb, shards, split, build):
    """k_det_sweep (one persistent launch per superstep; items owned by waves, per-user tickets)
    == the C oracle's sequential reference order, bitwise, on data with a very hot item (long
    same-item runs kept in registers) and heavy users (long ticket chains), on 1 or 2 shards.
    split=1 (default, k = 64/128/256): single-item chains run as a chain wave + a helper wave
    (k_det_sweep_split); split=0: one wave each (k_det_sweep2).  build: the superstep's entries
    built on the device from the host's shuffle (det_device_build), on the host (build_det_step), or
    on the host and then, from the third superstep on, on the device (the auto mode's switch)."""
    set_knob(monkeypatch, "det_split", split)
    set_knob(monkeypatch, "det_build", build)
    d = hot_item_data(k)
    big = synth.generate(3000, 500, 60000, seed=k)
    d.u = np.concatenate([d.u, big.u + 1000])
    d.i = np.concatenate([d.i, big.i])
    d.r = np.concatenate([d.r, big.r])
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=k, iterations=2, n_blocks=nb, seed=7, threads=4)
    with mfhip.Context(params(k, 2, nb, 7), devices=[0] * shards) as ctx:
        ctx.fit(d.u, d.i, d.r)
        assert ctx.stats()["kernel_launches"] <= 2 * nb * shards  # the persistent sweep ran
        for side in (0, 1):
            ids, vecs = ctx.factors(side)
            rids, rvecs = m.factors(side)
            assert np.array_equal(ids, rids) and np.array_equal(vecs, rvecs)


def test_det_split_many_blocks_cu_isolation_bitwise(monkeypatch):
    """The split sweep's slot table past one CU period (det_slot_table): with ~1000 waves a superstep
    has several hundred blocks, so the longest chains' CU-sharing positions b + cus*m are left empty
    (det_alone=1, the default) -- factors bitwise the C oracle's with and without that isolation."""
    k, nb = 64, 1
    d = synth.generate(6000, 3000, 150000, seed=21)
    rng = np.random.default_rng(21)
    hot = np.repeat(np.arange(12, dtype=np.int32), 900)  # a dozen long single-item chains
    d.u = np.concatenate([d.u, rng.integers(0, 6000, len(hot)).astype(np.int32)])
    d.i = np.concatenate([d.i, hot])
    d.r = np.concatenate([d.r, rng.integers(1, 6, len(hot)).astype(np.float64)])
    m = coracle.dsgd_fit(d.u, d.i, d.r, k=k, iterations=2, n_blocks=nb, seed=3, threads=4)
    set_knob(monkeypatch, "det_waves", 1000)
    for alone in ("1", "0"):
        set_knob(monkeypatch, "det_alone", alone)
        with mfhip.Context(params(k, 2, nb, 3)) as ctx:
            ctx.fit(d.u, d.i, d.r)
            assert ctx.stats()["kernel_launches"] <= 2 * nb  # the persistent sweep ran
            for side in (0, 1):
                ids, vecs = ctx.factors(side)
                rids, rvecs = m.factors(side)
                assert np.array_equal(ids, rids) and np.array_equal(vecs, rvecs), (alone, side)


@pytest.mark.parametrize("shards,nb", [(2, 4), (2, 8), (4, 8)])
def test_ring_overlap_split_launches_bitwise(monkeypatch, shards, nb):
    """c = nb/shards >= 2 user blocks per shard: each superstep runs as launch A (blocks 0..c-2) on
    the compute stream and launch B (block c-1) on a second stream behind the arriving item block,
    while the leaving block moves on a third stream as soon as A is done (the north star's ring
    exchange overlapped with compute).  Scheduling only: factors bitwise equal to the same plan
    without the overlap and to one shard."""
    set_knob(monkeypatch, "pair_sys", "1")
    set_knob(monkeypatch, "block_groups", "0")  # the same uniform G on every path
    d = hot_item_data(64)
    big = synth.generate(4000, 900, 120000, seed=31)
    d.u = np.concatenate([d.u, big.u + 500])
    d.i = np.concatenate([d.i, big.i + 200])
    d.r = np.concatenate([d.r, big.r])
    outs = []
    for devs, ov in (([0], "1"), ([0] * shards, "0"), ([0] * shards, "1")):
        set_knob(monkeypatch, "ring_overlap", ov)
        with mfhip.Context(params(64, 2, nb, 5, mode=L.MODE_FAST_F32, fast_waves=-8), devices=devs) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1], ctx.stats()["kernel_launches"]))
    for o in outs[1:]:
        assert np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1])
    assert outs[2][2] > outs[1][2]  # the overlapped path really split the launches


@pytest.mark.parametrize("mode,k,nb,seed", [(L.MODE_DETERMINISTIC_F64, 16, 4, 3), (L.MODE_DETERMINISTIC_F64, 8, 7, -9),
                                            (L.MODE_FAST_F32, 64, 8, 0), (L.MODE_FAST_F32, 128, 3, 11)])
def test_device_blocking_equals_host_blocking(monkeypatch, mode, k, nb, seed):
    """Blocking on the GPU (kernels_block.hip: radix sorts, scans, the JVM block draw per id) ==
    the host's build_side + build_rating_blocks bit for bit: the deterministic fit replays the
    reference's shuffled order inside each rating block and the fast plan depends on every row's
    position, so any difference in blocks, rows or in-block order changes the factors.  Data with
    negative ids, duplicate (user, item) pairs and ids far apart (the host's sparse path)."""
    d = synth.generate(1500, 400, 40000, seed=nb)
    u = d.u.copy()
    u[::53] = -u[::53] - 7
    u[::211] += 1_500_000_000
    i = d.i.copy()
    i[::97] = -i[::97] - 1
    u = np.concatenate([u, u[:3000]])
    i = np.concatenate([i, i[:3000]])
    r = np.concatenate([d.r, d.r[:3000][::-1]])
    outs = []
    for host in ("1", "0"):
        set_knob(monkeypatch, "host_blocking", host)
        with mfhip.Context(params(k, 2, nb, seed, mode=mode)) as ctx:
            ctx.fit(u, i, r)
            outs.append([ctx.factors(s) for s in (0, 1)])
    for s in (0, 1):
        assert np.array_equal(outs[0][s][0], outs[1][s][0])
        assert np.array_equal(outs[0][s][1], outs[1][s][1])


@pytest.mark.parametrize("k,nb,kind", [(64, 4, "zipf"), (128, 8, "zipf"), (128, 2, "hot"), (256, 4, "zipf"),
                                       (64, 8, "tiny")])
def test_device_plan_equals_host_plan(monkeypatch, k, nb, kind):
    """The fast schedule built on the device (kernels_plan.hip: the per-cell emission and pair
    records, and with MFHIP_TEST device_plan=2 the cell-major order and spreading too) is bitwise the host's (plan.cpp build_fast_plan + build_pair_plan):
    same pair records, wave and systolic tables (digest), same padding and requested bytes, and
    so the same factors after a fit."""
    if kind == "hot":
        d = hot_item_data(11)
    elif kind == "tiny":  # empty rating blocks and empty cells
        d = synth.generate(60, 40, 300, seed=23)
    else:
        d = synth.generate(6000, 1500, 400000, seed=17)
    res = {}
    for flag in ("0", "1", "2"):  # host / device emission / whole schedule on the device
        set_knob(monkeypatch, "device_plan", flag)
        with mfhip.Context(params(k, 2, nb, 5, mode=L.MODE_FAST_F32)) as ctx:
            ctx.prepare(d.u, d.i, d.r)
            dig = ctx.plan_digest()
            st = ctx.stats()
            ctx.run(2 * nb)
            res[flag] = (dig, st["pads"], st["groups"], ctx.factors(0)[1], ctx.factors(1)[1])
    h = res["0"]
    assert h[0][1] > 0
    for flag in ("1", "2"):
        g = res[flag]
        assert h[0] == g[0], (flag, h[0], g[0])
        assert h[1:3] == g[1:3], flag
        assert np.array_equal(h[3], g[3]) and np.array_equal(h[4], g[4]), flag
