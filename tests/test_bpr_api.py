"""BPR training (mf_bpr_run / mf_bpr_step_triples / mf_bpr_draws / mf_bpr_fit): the surface that needs no GPU --
exports, argument checks (each raised before the context is read), the draw against its Python statement, and the
contract's exponential against numpy.  The state errors need a context and are in tests/test_gpu_bpr.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mfhip import _lib as L
from mfhip import bpr

HEADER = os.path.join(ROOT, "include", "mfhip.h")
TESTING = os.path.join(ROOT, "include", "mfhip_testing.h")
FAKE = C.c_void_p(8)  # an opaque non-null handle, never dereferenced: each call below fails an argument check first
PUBLIC = ("mf_bpr_run", "mf_bpr_step_triples", "mf_bpr_draws", "mf_bpr_fit")


def test_symbols_are_exported_declared_and_wrapped():
    lib = L.lib()
    text = open(HEADER).read()
    for name in PUBLIC:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    assert "mf_debug_bpr_triples" in L.TESTING_EXPORTS and hasattr(lib, "mf_debug_bpr_triples")
    assert re.search(r"^int\s+mf_debug_bpr_triples\s*\(", open(TESTING).read(), flags=re.M)
    assert C.sizeof(L.mf_bpr_params) == 56 and C.sizeof(L.mf_bpr_stats) == 32
    import mfhip
    for name in ("bpr_run", "bpr_step_triples", "bpr_fit", "bpr_params"):
        assert hasattr(mfhip.Context, name)
    java = open(os.path.join(ROOT, "jni", "MfHip.java")).read()
    shim = open(os.path.join(ROOT, "jni", "mfhip_jni.c")).read()
    for jname, cname in (("bprRun", "mf_bpr_run"), ("bprStepTriples", "mf_bpr_step_triples"), ("bprFit", "mf_bpr_fit")):
        assert re.search(r"public static native \w+(\[\])? " + jname + r"\(", java), jname
        assert "JFN(" + jname + ")" in shim and cname + "(" in shim


def params(lr=0.05, lam=0.01, batch=8, scale=L.BPR_SCALE_SUM, redraws=1, seed=3):
    p = L.mf_bpr_params()
    p.lr, p.lambda_, p.batch, p.scale, p.redraws, p.seed = lr, lam, batch, scale, redraws, seed
    return p


def run(ctx=FAKE, p=True, first=0, steps=1, **kw):
    return L.lib().mf_bpr_run(ctx, C.byref(params(**kw)) if p else None, first, steps, None)


def step(ctx=FAKE, p=True, n=2, arrays=True, **kw):
    a = (C.c_int32 * 4)()
    return L.lib().mf_bpr_step_triples(ctx, C.byref(params(**kw)) if p else None, a if arrays else None, a, a, n, None)


def fit(ctx=FAKE, p=True, n=2, arrays=True, init_scale=0.1, steps=1, **kw):
    a = (C.c_int32 * 4)()
    return L.lib().mf_bpr_fit(ctx, a if arrays else None, a, n, init_scale, C.byref(params(**kw)) if p else None, steps,
                              None)


SHARED = [  # refused by all three context calls
    (dict(ctx=None), "null"), (dict(p=False), "null"),
    (dict(lr=0.0), "lr"), (dict(lr=-1.0), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr=float("inf")), "lr"),
    (dict(lam=-0.1), "lambda"), (dict(lam=float("nan")), "lambda"),
    (dict(scale=2), "scale"), (dict(scale=-1), "scale"),
]
SAMPLED = [  # ... by the two that draw
    (dict(batch=0), "batch"), (dict(batch=(1 << 24) + 1), "batch"), (dict(redraws=-1), "redraws"),
    (dict(redraws=63), "redraws"), (dict(steps=-1), "step"), (dict(steps=(1 << 26) + 1), "step"),
]
CASES = ([(run, kw, w) for kw, w in SHARED + SAMPLED] +
         [(run, dict(first=-1), "step"), (run, dict(first=1 << 26, steps=1), "step")] +
         [(step, kw, w) for kw, w in SHARED] +
         [(step, dict(n=-1), "count"), (step, dict(n=(1 << 24) + 1), "2^24"), (step, dict(arrays=False), "null")] +
         [(fit, kw, w) for kw, w in SHARED + SAMPLED] +
         [(fit, dict(n=-1), "count"), (fit, dict(arrays=False), "null"), (fit, dict(n=2 ** 31 - 1), "2^31"),
          (fit, dict(init_scale=float("inf")), "init_scale"), (fit, dict(init_scale=float("nan")), "init_scale")])


@pytest.mark.parametrize("fn,kw,word", CASES, ids=[f"{f.__name__}-{k}" for f, k, _ in CASES])
def test_argument_checks_come_before_the_context_is_read(fn, kw, word):
    assert fn(**kw) == L.MF_ERR_INVALID
    assert word in L.lib().mf_last_error().decode()


def test_step_triples_does_not_read_batch_redraws_or_seed():
    """... so a bad value of those is no argument error there: the call gets as far as the (null) context."""
    assert step(ctx=None, batch=0, redraws=99) == L.MF_ERR_INVALID
    assert "null" in L.lib().mf_last_error().decode()


@pytest.mark.parametrize("kw", [dict(batch=0), dict(batch=(1 << 24) + 1), dict(redraws=-1), dict(redraws=63),
                                dict(step=-1), dict(step=1 << 26), dict(pairs=-1), dict(pool=0),
                                dict(pool=2 ** 31 + 1), dict(out=False)])
def test_draws_argument_checks(kw):
    a = dict(seed=1, step=0, batch=4, redraws=1, pairs=10, pool=5, out=True)
    a.update(kw)
    buf = (C.c_uint64 * 64)()
    st = L.lib().mf_bpr_draws(a["seed"], a["step"], a["batch"], a["redraws"], a["pairs"], a["pool"],
                              buf if a["out"] else None)
    assert st == L.MF_ERR_INVALID
    if "batch" in kw or "redraws" in kw or "step" in kw:
        with pytest.raises(ValueError):
            bpr.draws(a["seed"], a["step"], a["batch"], a["redraws"], a["pairs"], a["pool"])


# ---- the draw ------------------------------------------------------------------------------------------
def test_known_answers():
    """Worked by hand from the header's formula (Python integers), not from the library."""
    assert bpr.draw_bits(0, 0, 0, 0) == 0xE220A8397B1DCDAF  # SplitMix64's first output for seed 0
    assert bpr.draw_bits(0, 0, 0, 1) == 0x6E789E6AA1B965F4  # ... and its second
    z = bpr.device_draws(0, 0, 1, 0, 1 << 32, 1 << 16)
    assert int(z[0, 0]) == 0xE220A8397B1DCDAF >> 32         # (z * 2^32) >> 64
    assert int(z[0, 1]) == ((0x6E789E6AA1B965F4 >> 32) * 65535) >> 32
    # state = seed + gamma * (t * 2^38 + s * 64 + r + 1): step 1, slot 0, draw 0 is step 0's index 2^38
    g = 0x9E3779B97F4A7C15
    st = (5 + g * ((1 << 38) + 3 * 64 + 2 + 1)) % (1 << 64)
    st = ((st ^ (st >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    st = ((st ^ (st >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    st ^= st >> 31
    assert bpr.draw_bits(5, 1, 3, 2) == st
    assert int(bpr.device_draws(5, 1, 4, 1, 1000, 77)[3, 2]) == ((st >> 32) * 76) >> 32


@pytest.mark.parametrize("seed,step,batch,redraws,pairs,pool", [
    (7, 3, 50, 2, 6000, 120), (-1, 0, 1, 0, 1, 2), (2 ** 63 - 1, 2 ** 26 - 1, 65, 62, 2 ** 40, 2 ** 31),
    (-2 ** 63, 12345, 64, 5, 90_400_000, 17770), (11, 9, 33, 3, 0, 1),
])
def test_library_draws_equal_the_python_statement(seed, step, batch, redraws, pairs, pool):
    a, b = bpr.draws(seed, step, batch, redraws, pairs, pool), bpr.device_draws(seed, step, batch, redraws, pairs, pool)
    assert a.shape == b.shape == (batch, 2 + redraws) and a.dtype == b.dtype == np.uint64
    assert np.array_equal(a, b)
    if pairs:
        assert int(a[:, 0].max()) < pairs
    assert int(a[:, 1:].max()) < max(pool - 1, 1)


def test_last_slot_of_the_largest_batch():
    s = (1 << 24) - 1
    z = bpr.device_draws(-5, 2 ** 26 - 1, 1 << 24, 1, 2 ** 40, 2 ** 31)
    assert np.array_equal(z[[0, s]], bpr.draws(-5, 2 ** 26 - 1, 1 << 24, 1, 2 ** 40, 2 ** 31, slots=[0, s]))


def test_a_draw_depends_on_seed_step_slot_and_draw_alone():
    big = bpr.device_draws(9, 4, 300, 6, 5000, 90)
    small = bpr.device_draws(9, 4, 17, 6, 5000, 90)
    assert np.array_equal(big[:17], small)                      # not on the batch
    few = bpr.device_draws(9, 4, 300, 2, 5000, 90)
    assert np.array_equal(big[:, :4], few)                      # not on the redraws
    assert not np.array_equal(big, bpr.device_draws(9, 5, 300, 6, 5000, 90))
    assert not np.array_equal(big, bpr.device_draws(10, 4, 300, 6, 5000, 90))
    # slot s of step t and slot 0 of step t + 1 are 2^38 - 64 s indices apart: no two (t, s, r) share a state
    assert len({bpr.draw_bits(9, t, s, r) for t in (0, 1) for s in (0, 1, (1 << 24) - 1) for r in (0, 1, 63)}) == 18


def test_positives_and_negatives_are_uniform():
    """Chi-square of 200,000 draws over 100 cells against the uniform law: the 99.9% point of chi2(99) is 149."""
    pairs, pool, n = 100, 101, 50_000
    z = np.concatenate([bpr.device_draws(21, t, n, 0, pairs, pool) for t in range(4)])
    for col in (0, 1):
        cnt = np.bincount(z[:, col].astype(np.int64), minlength=100)
        assert len(cnt) == 100
        exp = len(z) / 100
        assert ((cnt - exp) ** 2 / exp).sum() < 149.0, col
    # and the two are independent enough: the 100 x 100 table's chi-square against its 9,999 degrees of freedom
    # (mean 9,999, sd 141: five sd)
    tab = np.zeros((100, 100))
    np.add.at(tab, (z[:, 0].astype(np.int64), z[:, 1].astype(np.int64)), 1)
    e = len(z) / 10_000
    assert abs(((tab - e) ** 2 / e).sum() - 9999) < 5 * 141.4


def test_triples_resolve_against_a_table():
    """Three users: row 0 holds items {0, 2}, row 1 nothing, row 2 every item but 1 (pool 4)."""
    off = np.array([0, 2, 2, 5], np.int64)
    ent = np.array([0, 2, 0, 2, 3], np.int32)
    z = np.array([[0, 0, 0], [1, 1, 2], [3, 0, 1], [4, 2, 2], [2, 1, 0]], np.uint64)
    u, i, j = bpr.triples(z, off, ent, 4)
    # slot 0: entry 0 = (row 0, item 0); c = 0 -> row 1 (skips the positive), not held
    # slot 1: entry 1 = (row 0, item 2); c = 1 -> 1; slot 2: entry 3 = (row 2, item 2); c = 0 -> 0 held, c = 1 -> 1
    # slot 3: entry 4 = (row 2, item 3); c = 2 -> 2 held twice: void; slot 4: entry 2 = (row 2, item 0); c = 1 -> 2
    # held, c = 0 -> 1
    assert u.tolist() == [0, 0, 2, -1, 2] and i.tolist() == [0, 2, 2, -1, 0] and j.tolist() == [1, 1, 1, -1, 1]
    for a in bpr.triples(z, off, ent, 1) + bpr.triples(z[:, :1], off, ent, 4):
        assert a.tolist() == [-1] * 5


# ---- the gradient weight ---------------------------------------------------------------------------------
def test_exponential_is_within_2_to_the_minus_40_of_numpys():
    x = np.concatenate([np.linspace(-40.0, 40.0, 400_001), np.array([-40.0, 40.0, 0.0, -0.0, 1e-300, -1e-300]),
                        np.random.default_rng(5).uniform(-40, 40, 100_000)])
    e, ref = bpr.exp_contract(x), np.exp(x)
    assert np.max(np.abs(e - ref) / ref) < 2.0 ** -40
    assert bpr.exp_contract(0.0) == 1.0


def test_sigmoid_on_a_grid_at_the_clamp_and_beyond():
    x = np.linspace(-40.0, 40.0, 160_001)
    ref = 1.0 / (1.0 + np.exp(-x))
    s = bpr.sigmoid(x)
    assert np.max(np.abs(s - ref) / ref) < 2.0 ** -40
    assert bpr.sigmoid(0.0) == 0.5 and bpr.weight(0.0) == 0.5
    assert np.array_equal(bpr.weight(x), bpr.sigmoid(-x))
    for big in (40.0, 41.0, 1e3, 1e300, np.inf):               # beyond the clamp: the value at the clamp
        assert bpr.sigmoid(big) == bpr.sigmoid(40.0) == 1.0 / (1.0 + bpr.exp_contract(-40.0))
        assert bpr.sigmoid(-big) == bpr.sigmoid(-40.0) == 1.0 / (1.0 + bpr.exp_contract(40.0))
    assert 0.0 < bpr.sigmoid(-40.0) < 1e-17 and bpr.sigmoid(40.0) == 1.0
    assert np.isnan(bpr.sigmoid(np.nan)) and np.isnan(bpr.weight(np.nan))


def test_replay_leaves_its_inputs_and_untouched_rows_alone():
    rng = np.random.default_rng(2)
    P, Q = rng.random((6, 5)).astype(np.float32), rng.random((7, 5)).astype(np.float32)
    P0, Q0 = P.copy(), Q.copy()
    P2, Q2, st = bpr.replay_step(P, Q, [1, -1, 1, 4], [2, -1, 3, 2], [0, -1, 2, 6], 0.1, 0.01, bpr.SCALE_MEAN)
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)
    assert st == dict(slots=4, void_slots=1, user_rows_written=2, item_rows_written=4)
    assert np.array_equal(P2[[0, 2, 3, 5]], P0[[0, 2, 3, 5]]) and np.array_equal(Q2[[1, 4, 5]], Q0[[1, 4, 5]])
    assert not np.array_equal(P2[1], P0[1]) and not np.array_equal(Q2[6], Q0[6])
    # one slot, SUM, lambda 0, by hand
    p, qi, qj = P0[4].astype(np.float64), Q0[2].astype(np.float64), Q0[6].astype(np.float64)
    P3, Q3, _ = bpr.replay_step(P, Q, [4], [2], [6], 0.1, 0.0, bpr.SCALE_SUM)
    g = 1.0 / (1.0 + np.exp(np.float32(np.dot(p, qi - qj))))
    assert np.allclose(P3[4], p + 0.1 * g * (qi - qj), rtol=1e-5) and np.allclose(Q3[2], qi + 0.1 * g * p, rtol=1e-5)
    assert np.allclose(Q3[6], qj - 0.1 * g * p, rtol=1e-5)
