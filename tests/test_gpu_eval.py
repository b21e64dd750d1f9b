"""mf_predict, mf_rmse and mf_empirical_risk (k_predict, csrc/kernels_det.hip) against the host.

Every quality gate of the project is a number this kernel returned, so it is checked here against
plain numpy / math.fsum on models uploaded with set_factors, in both instantiations: double
(CE = 16 elements per staged row chunk, 4 pairs per load instruction) and float (CE = 32, 2 pairs).
Which test drives which path:

  test_predict_is_the_sequential_dot   both instantiations at the chunk edges k = 1, 15..17, 31..33, 100, 130,
                                       512 and n = 1, 63, 64, 65, 257, 1000: partial last chunk, partial last
                                       wave group, waves holding known and unknown pairs, a wave of unknown ones
  test_rmse_and_risk_match_fsum        the sse / cnt / risk sums and their butterfly + 4-wave + per-workgroup
                                       reduction, pp / qq over several chunks, multiplicity 2 and 3, lambda 0 / 0.7
  test_grid_stride_path                n = 1,200,000 > 4096 * 256: every workgroup makes more than one pass
  test_rmse_after_a_cell_kernel_fit    the float instantiation on the factors k_fast_substep left at k = 100

predict is compared bitwise: the kernel sums pq = pq + a * b in f64 in the order f = 0..k-1.  In fast
mode a and b are widened f32 values, so every product is exact in f64; in f64 mode it is the
project's ddot parity (the file is compiled with -ffp-contract=off).

The sums: the device adds non-negative terms, each bitwise the host's, in a fixed tree, so
|sum_dev - sum_ref| <= n 2^-53 sum_ref with sum_ref from math.fsum: a sum of non-negative terms is
within (additions on its longest path) x 2^-53 of the exact one, to first order, and that path (a
lane's passes x multiplicity, 6 butterfly steps, 3 wave adds, one add per workgroup) is never longer
than n here.  mf_empirical_risk returns its sum and is held to that bound as it stands.  mf_rmse returns sqrt(sse / cnt), so its bound is the same one carried through the
square root, which halves a relative error: n/2 2^-53 from the sum, 1.5 2^-53 for the device's
division and square root, 1.5 2^-53 for the same two roundings of the reference."""
import math

import numpy as np
import pytest

import mfhip
from mfhip import _lib as L
from mfhip import synth
from test_gpu_dsgd import params
from test_gpu_recommend import make_ctx, shuffled_ids

pytestmark = pytest.mark.gpu

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
MODE_IDS = ["f64", "f32"]
KS = [1, 15, 16, 17, 31, 32, 33, 100, 130, 512]
NS = [1, 63, 64, 65, 257, 1000]
U = 2.0 ** -53


def load_model(ctx, rng, nu, ni, k, mode):
    """Random factors under signed shuffled ids (users = 1 mod 3, items = 1 mod 5), as the device holds them."""
    uids, iids = shuffled_ids(rng, nu), shuffled_ids(rng, ni, 5)
    P, Q = rng.standard_normal((nu, k)), rng.standard_normal((ni, k))
    if mode == L.MODE_FAST_F32:
        P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    ctx.set_factors(L.SIDE_USER, uids, P)
    ctx.set_factors(L.SIDE_ITEM, iids, Q)
    return uids, iids, P, Q


def draw_pairs(rng, uids, iids, n):
    """n (user, item) pairs by row: about a fifth with an unknown user, an unknown item or both, spread
    at random so that a wave's 64 pairs hold both kinds; from n = 257 on, pairs 64..127 (one whole wave)
    are all unknown.  Pairs 0 and 1 are known.  Returns (u, i, user row, item row, known)."""
    ur, ir = rng.integers(0, len(uids), n), rng.integers(0, len(iids), n)
    kind = rng.random(n)
    bad_u = (kind < 0.07) | ((kind >= 0.14) & (kind < 0.2))
    bad_i = (kind >= 0.07) & (kind < 0.2)
    if n >= 257:
        bad_u[64:128] = kind[64:128] < 0.6
        bad_i[64:128] = kind[64:128] >= 0.3
    bad_u[:2] = bad_i[:2] = False
    u = np.where(bad_u, uids[ur] + 1, uids[ur]).astype(np.int32)  # 2 mod 3: no such user
    i = np.where(bad_i, iids[ir] + 2, iids[ir]).astype(np.int32)  # 3 mod 5: no such item
    known = ~(bad_u | bad_i)
    if n >= 257:
        assert not known[64:128].any() and bad_u[64:128].any() and bad_i[64:128].any()
    return u, i, ur, ir, known


def mixed_waves(known):
    g = [known[x:x + 64] for x in range(0, len(known), 64)]
    return sum(1 for w in g if w.any() and not w.all())


def seq_dot(A, B):
    """sum_f A[:, f] * B[:, f] as a left fold over f from 0.0, every product and sum rounded to f64."""
    acc = np.zeros(A.shape[0])
    for f in range(A.shape[1]):
        acc = acc + A[:, f] * B[:, f]
    return acc


def host_terms(P, Q, ur, ir, known, r, lam):
    """Per known pair, as k_predict forms them: (r - p.q)^2 and that plus lam (p.p + q.q)."""
    A, B = P[ur[known]], Q[ir[known]]
    d = r[known] - seq_dot(A, B)
    se = d * d
    return se, se + lam * (seq_dot(A, A) + seq_dot(B, B))


def multiplicity(u, i):
    """How often each row's (user, item) pair occurs in the list (the reference's join on the pair)."""
    key = (u.astype(np.int64) << 32) | (i.astype(np.int64) & 0xFFFFFFFF)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return cnt[inv]


def check_sums(ctx, P, Q, u, i, ur, ir, known, r, lams):
    n = len(u)
    se, _ = host_terms(P, Q, ur, ir, known, r, 0.0)
    rm, cnt = ctx.rmse(u, i, r)
    assert cnt == int(known.sum())
    if cnt == 0:
        assert math.isnan(rm)
    else:
        ref = math.sqrt(math.fsum(se.tolist()) / cnt)
        print(f"n={n}: rmse off by {abs(rm - ref) / ref / U:.2f} x 2^-53, bound {n / 2 + 3}")
        assert abs(rm - ref) <= (n / 2 + 3) * U * ref, (rm, ref)
    mult = multiplicity(u, i)[known]
    for lam in lams:
        _, term = host_terms(P, Q, ur, ir, known, r, lam)
        ref = math.fsum(np.repeat(term, mult).tolist())  # a pair occurring m times counts m times per row
        risk = ctx.empirical_risk(u, i, r, lam)
        if cnt == 0:
            assert risk == 0.0
        else:
            print(f"n={n} lambda={lam}: risk off by {abs(risk - ref) / ref / U:.2f} x 2^-53, bound {n}")
            assert abs(risk - ref) <= n * U * ref, (lam, risk, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", KS)
def test_predict_is_the_sequential_dot(mode, k):
    rng = np.random.default_rng(100 * k + mode)
    with make_ctx(k, mode) as ctx:
        uids, iids, P, Q = load_model(ctx, rng, 70, 50, k, mode)
        mixed = 0
        for n in NS:
            u, i, ur, ir, known = draw_pairs(rng, uids, iids, n)
            mixed += mixed_waves(known)
            pred, found = ctx.predict(u, i)
            want = np.where(known, seq_dot(P[ur], Q[ir]), 0.0)
            assert np.array_equal(found, known)
            assert np.array_equal(pred.view(np.uint64), want.view(np.uint64)), (n, np.abs(pred - want).max())
            assert not pred[~known].any()
        assert mixed >= 4  # waves holding known and unknown pairs


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", KS)
def test_rmse_and_risk_match_fsum(mode, k):
    rng = np.random.default_rng(100 * k + mode + 7)
    with make_ctx(k, mode) as ctx:
        uids, iids, P, Q = load_model(ctx, rng, 70, 50, k, mode)
        for n in NS:
            u, i, ur, ir, known = draw_pairs(rng, uids, iids, n)
            if n >= 63:  # pair 0 twice, pair 1 three times (both known), with ratings of their own
                for dst, src in ((n - 1, 0), (n - 2, 1), (n - 3, 1)):
                    u[dst], i[dst], ur[dst], ir[dst], known[dst] = u[src], i[src], ur[src], ir[src], True
                mult = multiplicity(u, i)
                assert mult[0] >= 2 and mult[1] >= 3
            r = rng.integers(1, 11, n) / 2.0  # half-integers
            check_sums(ctx, P, Q, u, i, ur, ir, known, r, (0.0, 0.7))
        # no pair matches: NaN and 0.0
        u = (uids[:5] + 1).astype(np.int32)
        i = iids[:5].astype(np.int32)
        rm, cnt = ctx.rmse(u, i, np.ones(5))
        assert cnt == 0 and math.isnan(rm)
        assert ctx.empirical_risk(u, i, np.ones(5), 0.7) == 0.0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_grid_stride_path(mode):
    """n above 4096 workgroups x 256 pairs: the grid-stride loop every workload-sized evaluation takes."""
    k, n = 3, 1_200_000
    assert n > 4096 * 256
    rng = np.random.default_rng(31 + mode)
    with make_ctx(k, mode) as ctx:
        uids, iids, P, Q = load_model(ctx, rng, 2000, 500, k, mode)
        u, i, ur, ir, known = draw_pairs(rng, uids, iids, n)
        pred, found = ctx.predict(u, i)
        want = np.where(known, seq_dot(P[ur], Q[ir]), 0.0)
        assert np.array_equal(found, known)
        assert np.array_equal(pred.view(np.uint64), want.view(np.uint64))
        r = rng.integers(1, 11, n) / 2.0
        check_sums(ctx, P, Q, u, i, ur, ir, known, r, (0.7,))


def test_rmse_after_a_cell_kernel_fit():
    """The judge on the model it judges: a fast fit at k = 100 (k_fast_substep, masked KPL = 2), then
    ctx.rmse on the held-out pairs against the host formula applied to ctx.factors."""
    k, nb = 100, 2
    d = synth.generate(400, 120, 12000, seed=100)
    (tu, ti, tr), (eu, ei, er) = d.split()
    assert L.lib().mf_fast_kernel_name(k) == b"k_fast_substep"
    with mfhip.Context(params(k, 2, nb, 3, mode=L.MODE_FAST_F32, lam=1.0, lr=0.002)) as ctx:
        ctx.fit(tu, ti, tr)
        uids, P = ctx.factors(L.SIDE_USER)
        iids, Q = ctx.factors(L.SIDE_ITEM)
        assert np.array_equal(P, P.astype(np.float32).astype(np.float64))
        ur = np.minimum(np.searchsorted(uids, eu), len(uids) - 1)
        ir = np.minimum(np.searchsorted(iids, ei), len(iids) - 1)
        known = (uids[ur] == eu) & (iids[ir] == ei)
        assert 0 < known.sum()
        check_sums(ctx, P, Q, eu.astype(np.int32), ei.astype(np.int32), ur, ir, known, er, (0.0, 1.0))
