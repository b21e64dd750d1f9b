"""mf_negative_draws / mf_online_update_sampled / mf_online_prequential_sampled: the surface that needs
no GPU -- the draw's known answers, the library's draws (csrc/neg_sample.hpp, through mf_negative_draws)
against the definition of record in plain Python integers (mfhip/negsample.py draws), range and
uniformity of the draw, argument checks, and the Python signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mfhip
from conftest import ROOT
from mfhip import _lib as L
from mfhip import negsample as NS
from mfhip.prequential import PrequentialEvaluator

HEADER = os.path.join(ROOT, "include", "mfhip.h")
NAMES = ("mf_negative_draws", "mf_online_update_sampled", "mf_online_prequential_sampled")
SEEDS = (0, 1, -7, 2**40 + 3)


def test_symbols_are_exported_and_declared():
    lib = L.lib()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in L.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    m = re.search(r"^#define\s+MF_NEG_MAX\s+(\d+)", text, flags=re.M)
    assert m and int(m.group(1)) == L.NEG_MAX == NS.NEG_MAX == 64
    assert hasattr(mfhip, "negsample")


def test_known_answers():
    assert NS.draw_bits(0, 0, 0) == 0xE220A8397B1DCDAF
    assert NS.draw_bits(5, 7, 2) == 0xC82574DD60113C09
    want = [[8, 4, 0, 9], [1, 2, 2, 5], [6, 9, 2, 9]]
    assert NS.draws(0, 0, [3, 3, 3], 10, 4).tolist() == want
    assert NS.device_draws(0, 0, [3, 3, 3], 10, 4).tolist() == want


def test_first_event_shifts_the_stream():
    pos = np.arange(8) % 5
    whole = NS.device_draws(9, 100, pos, 5, 3)
    assert np.array_equal(NS.device_draws(9, 103, pos[3:], 5, 3), whole[3:])
    assert np.array_equal(NS.draws(9, 103, pos[3:], 5, 3), whole[3:])


@pytest.mark.parametrize("seed, first_event, pool, negatives",
                         [(0, 0, 2, 0), (1, 1, 3, 1), (-7, 2**40, 17, 5), (2**40 + 3, 2**62, 1000, 64)])
def test_library_draws_match_the_definition(seed, first_event, pool, negatives):
    n = 97
    pos = (np.arange(n, dtype=np.int64) * 7 + 3) % pool
    pos[:2] = (0, pool - 1)
    want = NS.draws(seed, first_event, pos, pool, negatives)
    got = NS.device_draws(seed, first_event, pos, pool, negatives)
    assert got.shape == want.shape == (n, negatives)
    assert np.array_equal(got, want)
    assert ((got >= 0) & (got < pool)).all()
    assert (got != pos[:, None]).all()


def test_two_rows_always_give_the_other():
    pos = np.arange(50) % 2
    for seed in SEEDS:
        got = NS.device_draws(seed, 11, pos, 2, 6)
        assert np.array_equal(got, np.repeat((1 - pos)[:, None], 6, axis=1))


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_are_uniform_over_the_other_rows(seed):
    """pool = 64, 20,000 events x 5, pos_row = t % 64: every row is drawn 100,000 / 64 = 1562.5 times in
    expectation (each row is excluded in 1/64 of the events and drawn with 1/63 in the others), standard
    deviation ~39; +-10 % is about four of them."""
    n, pool, neg = 20000, 64, 5
    pos = np.arange(n) % pool
    got = NS.device_draws(seed, 0, pos, pool, neg)
    assert ((got >= 0) & (got < pool)).all() and (got != pos[:, None]).all()
    counts = np.bincount(got.reshape(-1), minlength=pool)
    expected = n * neg / pool
    print(seed, counts.min() / expected, counts.max() / expected, ((counts - expected) ** 2 / expected).sum())
    assert counts.min() >= 0.9 * expected and counts.max() <= 1.1 * expected
    # the definition of record on a slice of the same stream
    assert np.array_equal(NS.draws(seed, 1000, pos[1000:1200], pool, neg), got[1000:1200])


def _draws(seed=0, first=0, n=1, neg=1, pool=4, null=False):
    p = (C.c_int32 * 1)(0)
    o = (C.c_int32 * 64)()
    return L.lib().mf_negative_draws(seed, first, n, neg, pool, None if null else p, None if null else o)


def _last():
    return L.lib().mf_last_error().decode()


def test_negative_draws_argument_errors():
    assert _draws() == L.MF_OK
    assert _draws(neg=65) == L.MF_ERR_INVALID and "negatives" in _last()
    assert _draws(neg=-1) == L.MF_ERR_INVALID
    assert _draws(pool=0) == L.MF_ERR_INVALID and "pool" in _last()
    assert _draws(pool=-3) == L.MF_ERR_INVALID
    assert _draws(pool=2**31 + 1) == L.MF_ERR_INVALID
    assert _draws(n=-1) == L.MF_ERR_INVALID and "count" in _last()
    assert _draws(first=-1) == L.MF_ERR_INVALID and "first_event" in _last()
    assert _draws(null=True) == L.MF_ERR_INVALID
    assert _draws(pool=1) == L.MF_ERR_INVALID and "one row" in _last()      # nothing to draw from
    assert _draws(pool=1, neg=0) == L.MF_OK and _draws(pool=1, n=0) == L.MF_OK
    p = (C.c_int32 * 1)(4)
    o = (C.c_int32 * 1)()
    assert L.lib().mf_negative_draws(0, 0, 1, 1, 4, p, o) == L.MF_ERR_INVALID and "pos_row" in _last()
    for bad in (dict(negatives=65), dict(first_event=-1), dict(pool=0)):
        kw = dict(seed=0, first_event=0, pos_rows=[0], pool=4, negatives=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            NS.draws(**kw)
    with pytest.raises(ValueError):
        NS.draws(0, 0, [0], 1, 1)
    with pytest.raises(ValueError):
        NS.draws(0, 0, [4], 4, 1)


def _update(ctx=None, n=1, neg=1, rating=0.0, first=0):
    q = (C.c_int32 * 1)(1)
    d = (C.c_double * 1)(1.0)
    return L.lib().mf_online_update_sampled(ctx, q, q, d, n, L.ONLINE_NEXT_FACTORS, neg, rating, 0, first, None, None,
                                            None)


def _prequential(ctx=None, n=1, neg=1, rating=0.0, first=0):
    q = (C.c_int32 * 1)(1)
    d = (C.c_double * 1)(1.0)
    o = L.mf_prequential()
    return L.lib().mf_online_prequential_sampled(ctx, q, q, d, n, L.ONLINE_NEXT_FACTORS, 10, q, q, 0, C.byref(o), None,
                                                 None, None, neg, rating, 0, first, None)


@pytest.mark.parametrize("call", [_update, _prequential])
def test_sampled_calls_argument_errors(call):
    assert call() == L.MF_ERR_INVALID and "null context" in _last()
    assert call(neg=65) == L.MF_ERR_INVALID and "negatives" in _last()
    assert call(neg=-1) == L.MF_ERR_INVALID and "negatives" in _last()
    assert call(rating=float("nan")) == L.MF_ERR_INVALID and "negative_rating" in _last()
    assert call(rating=float("inf")) == L.MF_ERR_INVALID and "negative_rating" in _last()
    assert call(first=-1) == L.MF_ERR_INVALID and "first_event" in _last()


def test_expand_layout():
    u, i, r = [7, -2], [5, 9], [1.0, 0.5]
    U, I, R = NS.expand(u, i, r, [[1, 2, 1], [3, 3, 4]], -0.25)
    assert U.tolist() == [7, 7, 7, 7, -2, -2, -2, -2] and U.dtype == np.int32
    assert I.tolist() == [5, 1, 2, 1, 9, 3, 3, 4] and I.dtype == np.int32
    assert R.tolist() == [1.0, -0.25, -0.25, -0.25, 0.5, -0.25, -0.25, -0.25] and R.dtype == np.float64
    U, I, R = NS.expand(u, i, r, np.zeros((2, 0), np.int32), 0.0)
    assert (U.tolist(), I.tolist(), R.tolist()) == (u, i, r)
    U, I, R = NS.expand([], [], [], np.zeros((0, 5), np.int32), 0.0)
    assert len(U) == len(I) == len(R) == 0


def test_python_signatures():
    def names(f):
        return list(inspect.signature(f).parameters)
    assert names(NS.draws) == ["seed", "first_event", "pos_rows", "pool", "negatives"]
    assert names(NS.expand) == ["u", "i", "r", "sampled_ids", "negative_rating"]
    got = names(mfhip.Context.online_update_sampled)
    assert got[:8] == ["self", "u", "i", "r", "negatives", "negative_rating", "seed", "first_event"]
    got = names(mfhip.Context.online_prequential_sampled)
    assert got[:9] == ["self", "u", "i", "r", "top_n", "negatives", "negative_rating", "seed", "first_event"]
    sig = inspect.signature(PrequentialEvaluator.__init__).parameters
    assert (sig["negatives"].default, sig["negative_rating"].default, sig["seed"].default) == (0, 0.0, 0)
    assert list(sig)[:5] == ["self", "ctx", "top_n", "flavour", "num_partitions"]   # today's calls keep their meaning
