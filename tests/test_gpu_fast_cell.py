"""The generic fast sweep (csrc/kernels_fast.hip) at every rank bucket and edge.

Fast f32 mode runs k = 64 / 128 / 256 through the pair kernels and every other rank from 1 to 512
through k_fast_substep<KPL, FULL, D>: KPL = 1 / 2 / 4 / 8 for k <= 64 / 128 / 256 / 512, FULL (vector
b32 / b64 / b128 row I/O) when k == 64 * KPL and masked otherwise, ring depth D = 8 (4 at KPL = 8).
MFHIP_TEST fast_kernel=cell sends 64 / 128 / 256 through it too, fast_kernel=persistent runs the
same cells from k_fast_superstep (one launch per superstep).  Which test drives which instance:

  test_cell_kernel_equals_its_schedule    k_fast_substep, all eight instances: masked <1> k = 1, 3, 63;
                                          <2> 65, 100, 127; <4> 129, 200, 255; <8, D = 4> 257, 300, 511;
                                          FULL <1> 64, <2> 128, <4> 256 (knob), <8, D = 4> 512
  test_masked_rows_equal_padded_full_rows masked <KPL> against FULL <KPL> bitwise, KPL = 1, 2, 4, 8
  test_cell_fit_repeats_itself            FULL <4> (256), FULL <8> (512), masked <8> (300): the b128 store
  test_cell_virtual_shards_match_single   masked <2> (100) on two virtual shards
  test_persistent_driver_equals_cell      k_fast_superstep masked <1> (40), <2> (100), <8> (300)

The CPU tests (not marked gpu) establish what the GPU tests rely on: the project tolerance holds
for a plain float32 replay of each plan with a factor 8 to spare, it does not hide a frozen tail
element or a dropped record, and the cell plan does not depend on the rank."""
import numpy as np
import pytest

import coracle
import mf_oracle as O
import mfhip
from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth
from test_gpu_dsgd import fast_replay_reference, hot_item_data, params
from test_schedule import fast_plan_window, fast_schedule

gpu = pytest.mark.gpu

# the project's tolerance of a fast f32 fit against the f64 replay of its plan (test_gpu_dsgd.py)
RTOL, ATOL = 2e-4, 2e-5
SEED, LAM, LR, ITERS = 3, 1.0, 0.002, 2

# (k, nb, G, data, fast_kernel=cell): every rank bucket, its edges, nb in {1, 2, 3}, G in {4, 8};
# hot data at least once per KPL, masked and FULL; "tiny": cells shorter than the ring, empty
# cells and empty rating blocks
CASES = [
    (1, 2, 4, "plain", False), (3, 1, 8, "hot", False), (63, 3, 4, "plain", False), (64, 2, 8, "hot", True),
    (65, 1, 4, "plain", False), (100, 2, 8, "hot", False), (127, 3, 8, "plain", False), (128, 3, 4, "hot", True),
    (129, 2, 4, "plain", False), (200, 3, 8, "hot", False), (255, 1, 8, "plain", False), (256, 2, 4, "hot", True),
    (257, 3, 4, "plain", False), (300, 1, 8, "hot", False), (511, 2, 8, "plain", False), (512, 1, 4, "hot", False),
    (100, 4, 8, "tiny", False),
]
CASE_IDS = [f"k{k}-nb{nb}-G{G}-{data}{'-cell' if cell else ''}" for k, nb, G, data, cell in CASES]

# Host float32 replay of each case's plan against its f64 replay, in units of the tolerance
# (max |x32 - x64| / (ATOL + RTOL |x64|)), as test_project_tolerance_holds_for_a_float32_replay
# measures and prints it: the largest of the 17 cases is 0.100 (k = 200, hot data), then 0.084 (256),
# 0.078 (64), 0.074 (512); the other ranks above 256 give 0.032 (257), 0.040 (300), 0.039 (511).  So the
# project tolerance is at least 10x the reference's own f32 error and no case needs a wider one.
HOST_F32_MARGIN = 8.0


def case_data(k, data):
    if data == "tiny":
        return synth.generate(60, 40, 300, seed=23)
    return hot_item_data(k) if data == "hot" else synth.generate(400, 120, 12000, seed=k)


def tol_units(x, ref):
    """Largest distance of x from ref in units of the tolerance: <= 1 passes assert_allclose."""
    return float((np.abs(x - ref) / (ATOL + RTOL * np.abs(ref))).max())


def host_replay(d, k, nb, G, dtype, freeze_user_tail=False, skip=None, seed=SEED, iterations=ITERS, lam=LAM, lr=LR):
    """The plan of fast_replay_reference replayed in numpy at `dtype`, with the kernel's form of the
    update (kernels_fast.hip sweep_cell): w = eta r - eta p.q, p' = w q + (1 - eta ru) p,
    q' = w p + (1 - eta ri) q.  Cells of one sub-step share no row, so the records at one
    position of all its cells are applied together.  freeze_user_tail: element k-1 of a user row is
    never written; skip: the index of a rating whose update is dropped once, in the first epoch."""
    b, t, g, p = fast_schedule(d.u, d.i, nb, seed, G, window=fast_plan_window(k), k=k)
    uids, iids = np.unique(d.u), np.unique(d.i)
    urow, irow = np.searchsorted(uids, d.u), np.searchsorted(iids, d.i)
    U = np.stack([coracle.next_double(int(x) ^ seed, k) for x in uids]).astype(dtype)
    I = np.stack([coracle.next_double(int(x) ^ seed, k) for x in iids]).astype(dtype)
    ru = (lam / np.bincount(urow).astype(np.float64)).astype(dtype)
    ri = (lam / np.bincount(irow).astype(np.float64)).astype(dtype)
    r = d.r.astype(dtype)
    one = dtype(1)
    for s in range(1, iterations * nb + 1):
        eta = dtype(O.learning_rate(0, lr, s // nb + 1, lam))
        idx = np.where(((b // nb + s - 1) % nb) == (b % nb))[0]
        if skip is not None and s <= nb:
            idx = idx[idx != skip]
        key = t[idx].astype(np.int64) * (int(p.max()) + 1) + p[idx]
        order = idx[np.argsort(key, kind="stable")]
        cuts = np.flatnonzero(np.diff(np.sort(key))) + 1
        for grp in np.split(order, cuts):
            ur, ir = urow[grp], irow[grp]
            P, Q = U[ur], I[ir]
            w = eta * r[grp] - eta * (P * Q).sum(1, dtype=dtype)
            Pn = w[:, None] * Q + (one - eta * ru[ur])[:, None] * P
            Qn = w[:, None] * P + (one - eta * ri[ir])[:, None] * Q
            if freeze_user_tail:
                Pn[:, k - 1] = P[:, k - 1]
            U[ur], I[ir] = Pn, Qn
            assert Pn.dtype == dtype and Qn.dtype == dtype
    return U.astype(np.float64), I.astype(np.float64)


_refs = {}


def reference(monkeypatch, case):
    """The f64 replay of the case's plan, computed once (with the case's knob set) and shared."""
    k, nb, G, data, cell = case
    if cell:
        set_knob(monkeypatch, "fast_kernel", "cell")
    if case not in _refs:
        out = fast_replay_reference(case_data(k, data), k, nb, SEED, G, ITERS, LAM, LR)
        for a in out:
            a.setflags(write=False)
        _refs[case] = out
    return _refs[case]


# ---- CPU: what the GPU tests rely on ---------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_project_tolerance_holds_for_a_float32_replay(monkeypatch, case):
    """The tolerance of (a) comes from the reference alone: a float32 replay of the plan on the host
    stays 8x inside rtol=2e-4, atol=2e-5 of the f64 replay (the factor covers a host summation
    order against the device's DPP tree; both obey the same a-priori bound)."""
    k, nb, G, data, cell = case
    uids, U, iids, I = reference(monkeypatch, case)
    U32, I32 = host_replay(case_data(k, data), k, nb, G, np.float32)
    dist = max(tol_units(U32, U), tol_units(I32, I))
    print(f"host float32 replay, k={k} nb={nb} G={G} {data}: {dist:.4f} of the tolerance")
    assert dist * HOST_F32_MARGIN <= 1.0, dist


def test_tolerance_sees_a_frozen_tail_element_and_a_dropped_record(monkeypatch):
    """The same host replay in f64 equals the oracle's replay to rounding, and each of the two defects
    the GPU tests are there to catch -- the last element of the user rows never stored, one record
    of one cell skipped -- puts it outside the tolerance of (a)."""
    case = (100, 2, 8, "hot", False)
    k, nb, G, data, _ = case
    d = case_data(k, data)
    uids, U, iids, I = reference(monkeypatch, case)
    U64, I64 = host_replay(d, k, nb, G, np.float64)
    assert max(tol_units(U64, U), tol_units(I64, I)) < 1e-6  # the replay itself is the oracle's
    Uf, If = host_replay(d, k, nb, G, np.float64, freeze_user_tail=True)
    assert tol_units(Uf[:, k - 1], U[:, k - 1]) > 1.0
    assert not np.allclose(Uf, U, rtol=RTOL, atol=ATOL)
    skip = len(d.u) // 2  # one rating of the plain part: one record of one cell
    Us, Is = host_replay(d, k, nb, G, np.float64, skip=skip)
    urow, irow = np.searchsorted(uids, d.u[skip]), np.searchsorted(iids, d.i[skip])
    assert tol_units(Us[urow], U[urow]) > 1.0 and tol_units(Is[irow], I[irow]) > 1.0
    assert not np.allclose(Us, U, rtol=RTOL, atol=ATOL) and not np.allclose(Is, I, rtol=RTOL, atol=ATOL)


# (k', K, nb, G, data, fast_kernel=cell): a masked rank and the FULL rank of its KPL
PAD_CASES = [(40, 64, 2, 4, "plain", True), (1, 64, 1, 8, "hot", True), (100, 128, 3, 4, "hot", True),
             (130, 256, 2, 8, "plain", True), (200, 256, 1, 4, "hot", True), (300, 512, 2, 4, "hot", False)]
PAD_IDS = [f"k{kp}-in-{K}" for kp, K, *_ in PAD_CASES]


@pytest.mark.parametrize("case", PAD_CASES, ids=PAD_IDS)
def test_cell_plan_does_not_depend_on_the_rank(monkeypatch, case):
    """build_fast_plan uses k only for the row byte offsets (plan.cpp), and the cell kernel's window is
    kHazardWindow at every rank: ranks k' and K sweep the same records in the same cells and order."""
    kp, K, nb, G, data, cell = case
    if cell:
        set_knob(monkeypatch, "fast_kernel", "cell")
    d = case_data(kp, data)
    assert fast_plan_window(kp) == fast_plan_window(K)
    a = fast_schedule(d.u, d.i, nb, SEED, G, window=fast_plan_window(kp), k=kp)
    b = fast_schedule(d.u, d.i, nb, SEED, G, window=fast_plan_window(K), k=K)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- GPU -------------------------------------------------------------------------------------

def fast_params(k, nb, G, iters=ITERS, seed=SEED):
    return params(k, iters, nb, seed, mode=L.MODE_FAST_F32, lam=LAM, lr=LR, fast_waves=-G,
                  blocking=L.BLOCKING_REFERENCE)


@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cell_kernel_equals_its_schedule(monkeypatch, case):
    """k_fast_substep (register ring, run forwarding, chunk swap, masked or vector row I/O) == the
    sequential f64 replay of its plan, at the project's tolerance (justified on the host above)."""
    k, nb, G, data, cell = case
    uids, U, iids, I = reference(monkeypatch, case)  # sets fast_kernel=cell before the context exists
    d = case_data(k, data)
    assert L.lib().mf_fast_kernel_name(k) == b"k_fast_substep"
    with mfhip.Context(fast_params(k, nb, G)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        a_ids, a_u = ctx.factors(0)
        b_ids, a_i = ctx.factors(1)
    assert np.array_equal(a_ids, uids) and np.array_equal(b_ids, iids)
    print(f"device, k={k}: {max(tol_units(a_u, U), tol_units(a_i, I)):.4f} of the tolerance")
    np.testing.assert_allclose(a_u, U, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a_i, I, rtol=RTOL, atol=ATOL)


@gpu
@pytest.mark.parametrize("case", PAD_CASES, ids=PAD_IDS)
def test_masked_rows_equal_padded_full_rows(monkeypatch, case):
    """A lane holds elements [lane KPL, lane KPL + KPL) in both forms, so the masked kernel at rank
    k' does the arithmetic of the vector kernel at K = 64 KPL on rows whose columns k'..K-1 are
    zero: the partial products add exact zeros, wave_sum sees the same 64 values, zero columns
    stay zero.  Same plan (checked on the host above), same starting factors: bitwise equal."""
    kp, K, nb, G, data, cell = case
    if cell:
        set_knob(monkeypatch, "fast_kernel", "cell")
    d = case_data(kp, data)
    uids, iids = np.unique(d.u), np.unique(d.i)
    rng = np.random.default_rng(kp)
    start = [rng.random((len(ids), kp)).astype(np.float32).astype(np.float64) for ids in (uids, iids)]
    out = {}
    for k in (kp, K):
        assert L.lib().mf_fast_kernel_name(k) == b"k_fast_substep"
        with mfhip.Context(fast_params(k, nb, G)) as ctx:
            ctx.prepare(d.u, d.i, d.r)
            for side, ids in ((0, uids), (1, iids)):
                rows = np.zeros((len(ids), k))
                rows[:, :kp] = start[side]
                ctx.set_factors(side, ids, rows)
            ctx.run(2 * nb)
            out[k] = (ctx.factors(0)[1], ctx.factors(1)[1])
    for side in (0, 1):
        narrow, wide = out[kp][side], out[K][side]
        assert not np.array_equal(narrow, start[side])  # the fit ran
        assert np.array_equal(narrow.view(np.uint64), wide[:, :kp].copy().view(np.uint64))
        assert not wide[:, kp:].any()


@gpu
@pytest.mark.parametrize("k,cell", [(256, True), (512, False), (300, False)])
def test_cell_fit_repeats_itself(monkeypatch, k, cell):
    """No atomics and a fixed plan: restart + the same epochs give the same bits.  The guard of the
    store-data-hazard pin behind store_row's 16-B stores (FULL KPL = 4 and 8), as
    test_fast_fit_repeats_itself_hot_item is for the pair kernels, plus the masked KPL = 8 stores."""
    if cell:
        set_knob(monkeypatch, "fast_kernel", "cell")
    assert L.lib().mf_fast_kernel_name(k) == b"k_fast_substep"
    d = hot_item_data(k)
    with mfhip.Context(fast_params(k, 2, 4, iters=3)) as ctx:
        ctx.fit(d.u, d.i, d.r)
        first = (ctx.factors(0)[1], ctx.factors(1)[1])
        for _ in range(2):
            ctx.restart()
            ctx.run(3 * 2)
            assert np.array_equal(first[0], ctx.factors(0)[1]) and np.array_equal(first[1], ctx.factors(1)[1])


@gpu
def test_cell_virtual_shards_match_single():
    d = synth.generate(2000, 500, 60000, seed=9)
    outs = []
    for devs in ([0], [0, 0]):
        with mfhip.Context(params(100, 2, 4, 1, mode=L.MODE_FAST_F32, fast_waves=-8), devices=devs) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@gpu
@pytest.mark.parametrize("k,nb,G", [(40, 2, 4), (100, 1, 8), (300, 2, 4)])
def test_persistent_driver_equals_cell(monkeypatch, k, nb, G):
    """k_fast_superstep (MFHIP_TEST fast_kernel=persistent: one launch per superstep, waves hand
    user groups on through progress words) sweeps the cells of the per-sub-step launches in the
    same order: bitwise the same factors, in fewer launches.  nb G <= 16 waves per launch, all
    resident; a wave that waited over 1 s would fail the fit through fast_err."""
    d = synth.generate(400, 120, 12000, seed=k)
    outs = []
    for kern, name in (("cell", b"k_fast_substep"), ("persistent", b"k_fast_superstep")):
        set_knob(monkeypatch, "fast_kernel", kern)
        assert L.lib().mf_fast_kernel_name(k) == name
        with mfhip.Context(fast_params(k, nb, G)) as ctx:
            ctx.fit(d.u, d.i, d.r)
            outs.append((ctx.factors(0)[1], ctx.factors(1)[1], ctx.stats()["kernel_launches"]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[1][2] < outs[0][2]
