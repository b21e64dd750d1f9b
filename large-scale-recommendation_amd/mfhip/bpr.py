"""BPR training (mf_bpr_run / mf_bpr_step_triples, include/mfhip.h) stated on the host.

These functions restate the header's text in Python integers and numpy elementwise arithmetic; they are the
definition of record the device is compared with bit for bit, not a port of the kernels.

    z = draws(seed, step, batch, redraws, pairs, pool)            # [batch, 2 + redraws]: entry, then ranks c
    u, i, j = triples(z, off, ent, pool)                          # rows per slot, -1 for a void slot
    g = weight(x)                                                 # 1 / (1 + E(x)), f64
    P2, Q2, stats = replay_step(P, Q, u, i, j, lr, lam, scale)    # one step; P, Q in the context's precision
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

SCALE_SUM = L.BPR_SCALE_SUM
SCALE_MEAN = L.BPR_SCALE_MEAN
MAX_REDRAWS = L.BPR_MAX_REDRAWS
CHUNK = 1024
_M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def draw_bits(seed: int, t: int, s: int, r: int) -> int:
    """Draw r of slot s of step t: SplitMix64 at state seed + GAMMA * (t * 2^38 + s * 64 + r + 1)."""
    z = (int(seed) + GAMMA * ((int(t) << 38) + int(s) * 64 + int(r) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _check(step: int, batch: int, redraws: int, pairs: int, pool: int) -> None:
    if not 1 <= int(batch) <= L.BPR_MAX_BATCH:
        raise ValueError("batch must lie in 1 .. 2^24")
    if not 0 <= int(redraws) <= MAX_REDRAWS:
        raise ValueError(f"redraws must lie in 0 .. {MAX_REDRAWS}")
    if not 0 <= int(step) < 2**26:
        raise ValueError("step must lie in 0 .. 2^26 - 1")
    if int(pairs) < 0:
        raise ValueError("negative pair count")
    if not 1 <= int(pool) <= 2**31:
        raise ValueError("pool must be in [1, 2^31]")


def draws(seed: int, step: int, batch: int, redraws: int, pairs: int, pool: int, slots=None) -> np.ndarray:
    """z[s, 0] = the positive's entry (z * pairs) >> 64, z[s, r] = c = ((z >> 32) * (pool - 1)) >> 32 of negative
    draw r = 1 .. 1 + redraws.  slots: only these slots (rows in that order); the values do not depend on it."""
    _check(step, batch, redraws, pairs, pool)
    which = range(int(batch)) if slots is None else [int(s) for s in slots]
    out = np.zeros((len(which), 2 + int(redraws)), np.uint64)
    for row, s in enumerate(which):
        out[row, 0] = (draw_bits(seed, step, s, 0) * int(pairs)) >> 64
        for r in range(1, 2 + int(redraws)):
            out[row, r] = ((draw_bits(seed, step, s, r) >> 32) * (int(pool) - 1)) >> 32
    return out


def device_draws(seed: int, step: int, batch: int, redraws: int, pairs: int, pool: int) -> np.ndarray:
    """mf_bpr_draws: the same values from the library's own header (no GPU needed)."""
    per = 2 + max(int(redraws), 0)
    out = np.zeros(max(int(batch), 1) * per, np.uint64)
    L.check(L.lib().mf_bpr_draws(int(seed), int(step), int(batch), int(redraws), int(pairs), int(pool),
                                 L.ptr(out, C.c_uint64)))
    return out[:int(batch) * per].reshape(int(batch), per)


def triples(z: np.ndarray, off: np.ndarray, ent: np.ndarray, pool: int):
    """The draws resolved against the seen set's user-major table (off [rows + 1], ent: item rows, ascending per
    row): per slot (user row, positive row, negative row), -1 in all three for a void slot."""
    n = len(z)
    u = np.full(n, -1, np.int32)
    i = np.full(n, -1, np.int32)
    j = np.full(n, -1, np.int32)
    pairs = int(off[-1]) if len(off) else 0
    if pairs == 0 or pool < 2:
        return u, i, j
    off = np.asarray(off, np.int64)
    ent = np.asarray(ent, np.int64)
    e = z[:, 0].astype(np.int64)
    row = np.searchsorted(off[:-1], e, side="right") - 1  # the largest row with off[row] <= e
    pos = ent[e]
    # (row, item) held <=> its key is among the table's, which ascend: rows ascend and so do a row's entries
    keys = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off)) * int(pool) + ent
    open_ = np.ones(n, bool)
    for r in range(1, z.shape[1]):  # the first negative the row does not hold
        c = z[:, r].astype(np.int64)
        cand = c + (c >= pos)
        key = row * int(pool) + cand
        at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        take = open_ & (keys[at] != key)
        u[take], i[take], j[take] = row[take], pos[take], cand[take]
        open_ &= ~take
    return u, i, j


_LOG2E = 1.4426950408889634
_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10


def _coefficients():
    c, f = [], 1.0
    for i in range(14):
        if i:
            f *= i  # i! is exact in f64 up to 18!
        c.append(1.0 / f)
    return c


_COEF = _coefficients()


def exp_contract(x) -> np.ndarray:
    """E(x) of the header, f64 elementwise."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        xc = np.where(x < -40.0, -40.0, np.where(x > 40.0, 40.0, x))  # a NaN stays
        n = np.rint(xc * _LOG2E)
        r = (xc - n * _LN2_HI) - n * _LN2_LO
        p = np.full_like(r, _COEF[13])
        for i in range(12, -1, -1):
            m = p * r
            p = m + _COEF[i]
        ni = np.where(np.isnan(n), 0, n).astype(np.int32)
        return np.ldexp(p, ni)


def weight(x) -> np.ndarray:
    """g = 1 / (1 + E(x)) in f64."""
    with np.errstate(invalid="ignore"):
        return 1.0 / (1.0 + exp_contract(x))


def sigmoid(x) -> np.ndarray:
    """1 / (1 + E(-x)): the logistic function by the contract's exponential (weight(x) = sigmoid(-x))."""
    return weight(-np.asarray(x, np.float64))


def _dot64(p: np.ndarray, d: np.ndarray) -> np.ndarray:
    """Step 2 for n slots at once: p, d [n, k] of dtype T -> x [n]."""
    n, k = p.shape
    v = np.zeros((n, 64), p.dtype)
    for f0 in range(0, k, 64):
        w = min(64, k - f0)
        m = p[:, f0:f0 + w] * d[:, f0:f0 + w]
        v[:, :w] = v[:, :w] + m
    lanes = np.arange(64)
    for b in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ b]
    return v[:, 0]


def _row_sums(rows: np.ndarray, terms: np.ndarray, chunk: int):
    """Steps 4 and 5's sums: entry e (in order) adds terms[e] to row rows[e].  Per row a chain from 0 over its
    entries in order; a row of more than `chunk` entries takes one chain per `chunk` consecutive entries and adds
    the chain results to 0 in order.  All chains advance together, one entry each per pass, which changes no
    chain's order.  Returns (the distinct rows ascending, their entry counts, their sums [rows, k])."""
    order = np.argsort(rows, kind="stable")
    uniq, start, counts = np.unique(rows[order], return_index=True, return_counts=True)
    seg = np.repeat(np.arange(len(uniq)), counts)
    pos = np.arange(len(rows)) - start[seg]
    nch = (counts + chunk - 1) // chunk
    base = np.concatenate([[0], np.cumsum(nch)[:-1]]).astype(np.int64)
    cid = base[seg] + pos // chunk
    step = pos % chunk
    t_sorted = terms[order]
    acc = np.zeros((int(nch.sum()), terms.shape[1]), terms.dtype)
    for t in range(int(step.max()) + 1):
        sel = step == t
        acc[cid[sel]] = acc[cid[sel]] + t_sorted[sel]
    out = acc[base].copy()  # a row of one chain: the chain itself
    many = np.nonzero(nch > 1)[0]
    if len(many):
        tot = np.zeros((len(many), terms.shape[1]), terms.dtype)
        for c in range(int(nch[many].max())):
            sel = nch[many] > c
            tot[sel] = tot[sel] + acc[base[many][sel] + c]
        out[many] = tot
    return uniq, counts, out


def replay_step(P: np.ndarray, Q: np.ndarray, u, i, j, lr: float, lam: float, scale: int, chunk: int = CHUNK):
    """One step on triples of rows (a slot with u < 0 is void).  P [users, k], Q [items, k] of dtype float32 or
    float64 are the model as the step finds it; returns (P', Q', stats) and leaves P, Q unchanged."""
    T = P.dtype.type
    assert Q.dtype == P.dtype and P.dtype in (np.float32, np.float64)
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    live = np.nonzero(u >= 0)[0]
    stats = {"slots": int(len(u)), "void_slots": int(len(u) - len(live)), "user_rows_written": 0,
             "item_rows_written": 0}
    P2, Q2 = P.copy(), Q.copy()
    if len(live) == 0:
        return P2, Q2, stats
    lrT, lamT = T(lr), T(lam)

    def finish(old, acc, counts):
        cnt = counts.astype(P.dtype)[:, None]
        one = np.ones_like(cnt)
        c, lm = (one / cnt, lamT * one) if scale == SCALE_MEAN else (one, lamT * cnt)
        t1 = c * acc
        t2 = lm * old
        t3 = t1 - t2
        t4 = lrT * t3
        return old + t4

    with np.errstate(over="ignore", invalid="ignore"):
        ul, il, jl = u[live], i[live], j[live]
        d = Q[il] - Q[jl]                                    # 1
        x = _dot64(P[ul], d)                                 # 2
        g = weight(x.astype(np.float64)).astype(P.dtype)     # 3
        gd = g[:, None] * d
        gp = g[:, None] * P[ul]
        rows, counts, acc = _row_sums(ul, gd, chunk)         # 4 (live slots ascend in s)
        P2[rows] = finish(P[rows], acc, counts)
        stats["user_rows_written"] = int(len(rows))
        # 5: entries in ascending (s, positive before negative); acc - m == acc + (-m) in IEEE arithmetic
        rows, counts, acc = _row_sums(np.stack([il, jl], 1).reshape(-1),
                                      np.stack([gp, -gp], 1).reshape(-1, P.shape[1]), chunk)
        Q2[rows] = finish(Q[rows], acc, counts)
        stats["item_rows_written"] = int(len(rows))
    return P2, Q2, stats
