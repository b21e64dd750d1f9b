"""Negative sampling of the online path (mf_online_update_sampled, include/mfhip.h) stated on the host.

draws is the definition of record: plain Python integers, the formula of the header line by line.  The
device expansion, the library's host expansions and mf_negative_draws (device_draws below) share one C++
header, csrc/neg_sample.hpp, and are compared with it bit for bit.

    rows = draws(seed, first_event, pos_rows, pool, negatives)      # [n, negatives] factor rows
    U, I, R = expand(u, i, r, sampled_ids, negative_rating)         # the batch mf_online_update would take
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

NEG_MAX = L.NEG_MAX
_M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def draw_bits(seed: int, t: int, s: int) -> int:
    """The 64 bits of negative s of stream event t: SplitMix64 at state seed + GAMMA * (t * 64 + s + 1)."""
    z = (int(seed) + GAMMA * (int(t) * NEG_MAX + int(s) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def pick_row(z: int, pool: int, pos_row: int) -> int:
    """One of the pool - 1 rows other than pos_row, from the top 32 bits of z."""
    c = ((z >> 32) * (pool - 1)) >> 32
    return c + (1 if c >= pos_row else 0)


def _check(first_event: int, pool: int, negatives: int) -> None:
    if not 0 <= int(negatives) <= NEG_MAX:
        raise ValueError(f"negatives must be in [0, {NEG_MAX}]")
    if int(first_event) < 0:
        raise ValueError("first_event must not be negative")
    if not 1 <= int(pool) <= 2**31:
        raise ValueError("pool must be in [1, 2^31]")


def draws(seed: int, first_event: int, pos_rows, pool: int, negatives: int) -> np.ndarray:
    """rows[j, s]: the factor row of negative s of event first_event + j, whose own item has row
    pos_rows[j] < pool.  pool: the item rows of the model after the batch's new ids have theirs."""
    _check(first_event, pool, negatives)
    pos = [int(x) for x in pos_rows]
    out = np.zeros((len(pos), int(negatives)), np.int32)
    if not pos or not negatives:
        return out
    if pool < 2:
        raise ValueError("a pool of one row holds no negative")
    for j, p in enumerate(pos):
        if not 0 <= p < pool:
            raise ValueError("pos_row outside the pool")
        for s in range(int(negatives)):
            out[j, s] = pick_row(draw_bits(seed, int(first_event) + j, s), int(pool), p)
    return out


def device_draws(seed: int, first_event: int, pos_rows, pool: int, negatives: int) -> np.ndarray:
    """mf_negative_draws: the same rows from the library's own header (no GPU needed)."""
    pos = np.ascontiguousarray(pos_rows, dtype=np.int32)
    n = len(pos)
    m = n * max(int(negatives), 0)
    out = np.zeros(max(m, 1), np.int32)
    L.check(L.lib().mf_negative_draws(int(seed), int(first_event), n, int(negatives), int(pool),
                                      L.ptr(pos, C.c_int32), L.ptr(out, C.c_int32)))
    return out[:m].reshape(n, int(negatives))


def expand(u, i, r, sampled_ids, negative_rating: float):
    """The expanded batch in arrival order: event j, then (u[j], sampled_ids[j, s], negative_rating) for s
    ascending.  sampled_ids: [n, negatives] item ids.  Returns (users int32, items int32, ratings f64)."""
    u, i, r = L.as_i32(u), L.as_i32(i), L.as_f64(r)
    n = L.same_length(u, i, r)
    ids = np.asarray(sampled_ids, dtype=np.int32)
    ids = ids.reshape(n, ids.size // n if n else 0)
    per = 1 + ids.shape[1]
    U = np.repeat(u, per)
    I = np.empty((n, per), np.int32)
    I[:, 0] = i
    I[:, 1:] = ids
    R = np.full((n, per), float(negative_rating), np.float64)
    R[:, 0] = r
    return U, I.reshape(-1), R.reshape(-1)
