"""Host replays of the online micro-batch's f32 arithmetic, in numpy (no GPU, no library).

The f32 online kernels apply SGDUpdater.nextFactors (core/FactorUpdater.scala:37-45) in a fixed,
fully specified order, so a host replay can be bitwise:

  tree_replay  csrc/online_f32.hpp as written -- k_online_f32 (kernels_online_sweep.hip) and
               k_level / k_level_out at k <= 256 (kernels_det.hip): every lane folds its own KPL
               products with fused multiply-adds, a fixed butterfly sums the 64 lane partials, the
               row updates are fused multiply-adds;
  fold_replay  the plain f32 statement of k_online_sweep<float> and k_level<float, 8> /
               k_level_out<float, 8> (compiled with -ffp-contract=off): rounded products, a left
               fold from 0, rounded multiply then add in the row updates.

fma32 is a correctly rounded f32 fused multiply-add (the product is exact in f64, the f64 sum is
rounded to odd with its exact TwoSum error, so the conversion to f32 rounds once).  The f64
reference of the same operation stays coracle.online_apply / mf_oracle.online_sequential.

standard_batch is the batch tests/test_online_emu.py and tests/test_gpu_online_ranks.py share.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """Correctly rounded float32 a * b + c (one rounding), elementwise with broadcasting."""
    a = np.asarray(a, F32).astype(np.float64)
    b = np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b  # exact: 24 x 24 bits, and no f32 product leaves the f64 exponent range
        s = p + c
        bb = s - p  # TwoSum (Knuth): s + err == p + c exactly
        err = (p - (s - bb)) + (c - bb)
        shape = s.shape
        s = np.ascontiguousarray(np.atleast_1d(s))
        err = np.atleast_1d(err)
        # round to odd: an inexact sum whose last bit is even moves to the odd neighbour on the
        # side of the exact value, so the f32 conversion below sees on which side of a tie it lies
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32).reshape(shape)


def fma32_naive(a, b, c):
    """a * b + c in f64, then rounded to f32: rounds twice (kept to show that the checks see it)."""
    a = np.asarray(a, F32).astype(np.float64)
    b = np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    with np.errstate(over="ignore"):
        return (a * b + c).astype(F32)


def lane_elements(k: int, layout: Optional[str] = None) -> np.ndarray:
    """(64, KPL) element index of lane l's c-th value, k where the lane holds a zero.
    layout None: online_f32.hpp's choice -- contiguous (l * KPL + c) when k == 64 KPL and KPL != 3,
    else strided (l + 64 c); "contiguous" / "strided" force one (the defect checks)."""
    kpl = (k + 63) // 64
    if layout is None:
        layout = "contiguous" if (k == 64 * kpl and kpl != 3) else "strided"
    lane, c = np.meshgrid(np.arange(64), np.arange(kpl), indexing="ij")
    idx = lane * kpl + c if layout == "contiguous" else lane + 64 * c
    return np.where(idx < k, idx, k)


def wave_sum(x: np.ndarray) -> np.float32:
    """f32_wave_sum: lanes l + (l ^ 32), then l ^ 16, l ^ 1, l ^ 2, quad 0 + quad 1 within 8, then
    the halves of 16 (every add a commutative f32 add, so all lanes agree)."""
    s = np.asarray(x, F32).reshape(2, 2, 2, 2, 2, 2)  # lane bits 5, 4, 3, 2, 1, 0
    s = s[0] + s[1]  # bit 5 -> axes (4, 3, 2, 1, 0)
    s = s[0] + s[1]  # bit 4 -> axes (3, 2, 1, 0)
    s = s[..., 0] + s[..., 1]  # bit 0 -> (3, 2, 1)
    s = s[..., 0] + s[..., 1]  # bit 1 -> (3, 2)
    s = s[..., 0] + s[..., 1]  # bit 2 -> (3,)
    return F32(s[0] + s[1])  # bit 3


def tree_dot(p: np.ndarray, q: np.ndarray, idx: np.ndarray) -> np.float32:
    """f32_lane_dot + f32_wave_sum: part = p0 q0 rounded, then fmaf(p[c], q[c], part)."""
    pz, qz = np.append(p, F32(0)), np.append(q, F32(0))
    pl, ql = pz[idx], qz[idx]
    part = pl[:, 0] * ql[:, 0]
    for c in range(1, idx.shape[1]):
        part = fma32(pl[:, c], ql[:, c], part)
    return wave_sum(part)


def fold_dot(p: np.ndarray, q: np.ndarray) -> np.float32:
    """((0 + p0 q0) + p1 q1) + ...: rounded products, one f32 add each, in order f = 0..k-1."""
    return np.cumsum(np.concatenate([np.zeros(1, F32), p * q]), dtype=F32)[-1]


def _replay(step: Callable, U, I, urow, irow, r, k, records, freeze_user_tail):
    U = np.array(U, dtype=F32).reshape(-1, k)
    I = np.array(I, dtype=F32).reshape(-1, k)
    urow, irow = np.asarray(urow), np.asarray(irow)
    r32 = np.asarray(r, np.float64).astype(F32)
    n = len(r32)
    kinds = {None: (), "next": ("next",), "delta": ("delta",), "both": ("next", "delta")}[records]
    out = {kd: (np.empty((n, k)), np.empty((n, k))) for kd in kinds}
    for j in range(n):
        u, i = int(urow[j]), int(irow[j])
        p, q = U[u].copy(), I[i].copy()
        le, pn, qn = step(p, q, r32[j])
        if "next" in out:
            out["next"][0][j], out["next"][1][j] = pn, qn
        if "delta" in out:
            di = le * p  # one f32 rounding; p before the update (k_level_out, OUT == 2)
            out["delta"][0][j], out["delta"][1][j] = p + di, di
        if freeze_user_tail:
            pn[k - 1] = p[k - 1]
        U[u], I[i] = pn, qn
    if records is None:
        return U, I
    if records == "both":
        return U, I, out
    return U, I, out[records][0], out[records][1]


def tree_replay(U, I, urow, irow, r, lr, k, records=None, layout=None, freeze_user_tail=False):
    """The updates (urow[j], irow[j], r[j]) in order on copies of U and I (rows x k, rounded to f32)
    with online_f32.hpp's arithmetic.  Returns (U, I) as float32, and with records "next" /
    "delta" the per-rating records widened to f64: (p', q') / (p + f32(le p), f32(le p)) with p
    before the update; "both": a dict of the two.  layout / freeze_user_tail: deliberate defects
    for the sensitivity checks (a forced lane layout; the last element of the user rows never
    stored)."""
    assert 1 <= k <= 256
    idx = lane_elements(k, layout)
    eta = F32(lr)

    def step(p, q, r32):
        le = eta * (r32 - tree_dot(p, q, idx))  # f32_err: two f32 roundings
        return le, fma32(le, q, p), fma32(le, p, q)

    return _replay(step, U, I, urow, irow, r, k, records, freeze_user_tail)


def fold_replay(U, I, urow, irow, r, lr, k, records=None, freeze_user_tail=False):
    """As tree_replay with the unfused f32 arithmetic of k_online_sweep<float> / k_level<float, 8>:
    e = r - dot (left fold), le = eta e, p' = p + f32(le q), q' = q + f32(le p)."""
    eta = F32(lr)

    def step(p, q, r32):
        le = eta * (r32 - fold_dot(p, q))
        return le, p + le * q, q + le * p

    return _replay(step, U, I, urow, irow, r, k, records, freeze_user_tail)


def row_rel_err(a, b) -> float:
    """max over rows of ||a - b|| / ||b|| (test_gpu_configs.py's ONLINE_F32_TOL measure)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.linalg.norm(b, axis=1), 1e-30)
    return float((np.linalg.norm(a - b, axis=1) / den).max())


@dataclass
class Batch:
    """A micro-batch over a model: uid / iid / r the ratings (ids, arrival order); split: the second
    online_update call starts there; known_u / known_i: the ids loaded before the batch, in row
    order, with factors U0 / I0 (f32-representable f64); new_u / new_i: the ids first seen in the
    batch, in first-touch order (their rows follow the known ones); urow / irow: each rating's row."""
    k: int
    lr: float
    uid: np.ndarray
    iid: np.ndarray
    r: np.ndarray
    split: int
    known_u: np.ndarray
    known_i: np.ndarray
    U0: np.ndarray
    I0: np.ndarray
    new_u: np.ndarray
    new_i: np.ndarray
    urow: np.ndarray
    irow: np.ndarray

    def start(self, init: Callable, f32: bool):
        """The factor matrices in row order before the batch: the loaded rows, then the new ids'
        first-touch values init(id, k), rounded to f32 when f32."""
        def side(F0, new):
            fresh = np.array([init(int(x), self.k) for x in new], np.float64).reshape(-1, self.k)
            if f32:
                fresh = fresh.astype(F32).astype(np.float64)
            return np.concatenate([F0, fresh])
        return side(self.U0, self.new_u), side(self.I0, self.new_i)

    def reorder(self, order):
        """The same batch with its ratings in another sequence (rows unchanged)."""
        order = np.asarray(order)
        return (self.urow[order], self.irow[order], self.r[order])


def _first_touch(ids, known):
    seen = set(int(x) for x in known)
    new = []
    for x in ids.tolist():
        if x not in seen:
            seen.add(x)
            new.append(x)
    return np.array(new, np.int32)


def make_batch(k, uidx, iidx, r, nu, ni, rng, lr=0.01, split=None, new_frac=0.05, signed=True) -> Batch:
    """A Batch from user / item indices in [0, nu) / [0, ni): every index gets a distinct id (signed
    and shuffled, or non-negative and shuffled), the last new_frac of the indices stay out of the
    loaded model (the ratings decide whether and when they are first touched), and the loaded ids
    get factors standard_normal / k**0.25 rounded to f32, in a shuffled row order."""
    n = len(r)
    def ids_for(m):
        lo = -2**31 if signed else 0
        while True:
            ids = np.unique(rng.integers(lo, 2**31 - 1, 2 * m + 8))
            if len(ids) >= m:
                return rng.permutation(ids)[:m].astype(np.int32)
    umap, imap = ids_for(nu), ids_for(ni)
    nku, nki = nu - int(round(nu * new_frac)), ni - int(round(ni * new_frac))
    known_u, known_i = rng.permutation(umap[:nku]), rng.permutation(imap[:nki])
    scale = float(k) ** 0.25
    U0 = (rng.standard_normal((nku, k)) / scale).astype(F32).astype(np.float64)
    I0 = (rng.standard_normal((nki, k)) / scale).astype(F32).astype(np.float64)
    uid, iid = umap[np.asarray(uidx)], imap[np.asarray(iidx)]
    new_u, new_i = _first_touch(uid, known_u), _first_touch(iid, known_i)
    urows = {int(x): j for j, x in enumerate(np.concatenate([known_u, new_u]).tolist())}
    irows = {int(x): j for j, x in enumerate(np.concatenate([known_i, new_i]).tolist())}
    urow = np.array([urows[int(x)] for x in uid], np.int32)
    irow = np.array([irows[int(x)] for x in iid], np.int32)
    return Batch(k, lr, uid.astype(np.int32), iid.astype(np.int32), np.asarray(r, np.float64),
                 n // 2 if split is None else split, known_u, known_i, U0, I0, new_u, new_i, urow, irow)


def standard_batch(k: int, signed: bool = True) -> Batch:
    """n = 3000 ratings of 300 users and 100 items, one hot item on every 5th rating, ratings in
    1..5, lr 0.01.  The first 1500 ratings use only the loaded ids (95 % of each side); the second
    1500 draw from all of them, so the second call brings ids the model has not seen."""
    rng = np.random.default_rng(1000 + k)
    n, nu, ni, hot = 3000, 300, 100, 17
    h = n // 2
    uidx = np.concatenate([rng.integers(0, 285, h), rng.integers(0, nu, n - h)])
    iidx = np.concatenate([rng.integers(0, 95, h), rng.integers(0, ni, n - h)])
    iidx[::5] = hot
    r = rng.integers(1, 6, n).astype(np.float64)
    return make_batch(k, uidx, iidx, r, nu, ni, rng, signed=signed)
