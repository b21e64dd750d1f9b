"""Prequential (test-then-train) evaluation of the online path: the definitions of
mf_online_prequential (include/mfhip.h) stated on the host, and the evaluator that keeps the
"online DCG" curve of a stream.

host_prequential is the definition of record: plain Python over the ranks and list lengths
mf_pair_ranks returns, with ranking.GAIN / IDCG (the table the device reads), every sum taken in the
device's order, so the device's sums can be compared with it bit for bit.

    ev = PrequentialEvaluator(ctx, top_n=10, flavour=ONLINE_NEXT_FACTORS)
    for u, i, r in stream:
        ev.process(u, i, r)          # ranks the batch, then learns it
    ev.ndcg, ev.mpr                   # cumulative;  ev.curve("ndcg") per batch
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import _lib as L
from .context import Context, Prequential
from .ranking import GAIN, IDCG, MAX_TOP

SLICE = 1024


def slice_tree_sum(values) -> float:
    """The fixed-order sum of the device: slices of 1024 values (zero-padded); inside a slice the
    pairwise tree v[t] = v[t] + v[t + d] for every t < d, d = 512, 256, ..., 1; the slice sums added
    to 0.0 in ascending slice order."""
    total = 0.0
    n = len(values)
    for s0 in range(0, n, SLICE):
        v = [float(x) for x in values[s0:s0 + SLICE]]
        v += [0.0] * (SLICE - len(v))
        d = SLICE // 2
        while d >= 1:
            for t in range(d):
                v[t] = v[t] + v[t + d]
            d //= 2
        total = total + v[0]
    return total


def host_prequential(ranks, valid, top_n: int) -> Tuple[np.ndarray, Tuple[float, float, float]]:
    """Per-event values and their sums for ranks / valid as mf_pair_ranks lays them out (a negative
    rank: a cold or excluded event, which contributes 0.0 everywhere).  For an evaluated event with
    rank r and list length V, N = top_n:
        ndcg = GAIN[r] / IDCG[1] if r < N else 0      rr = 1 / (r + 1) if r < N else 0
        hit  = 1 if r < N else 0                      pr = r / (V - 1), 0 when V == 1
    Returns (values [n, 4] float64 = ndcg, rr, hit, pr; (sum_ndcg, sum_rr, sum_pr) in the device's
    slice-and-tree order)."""
    top_n = int(top_n)
    if not 1 <= top_n <= MAX_TOP:
        raise ValueError(f"top_n must be in [1, {MAX_TOP}]")
    n = len(ranks)
    out = np.zeros((n, 4), np.float64)
    for j in range(n):
        r, v = int(ranks[j]), int(valid[j])
        if r < 0:
            continue
        hit = r < top_n
        out[j] = (GAIN[r] / IDCG[1] if hit else 0.0, 1.0 / (r + 1) if hit else 0.0, 1.0 if hit else 0.0,
                  r / (v - 1) if v > 1 else 0.0)
    sums = (slice_tree_sum(out[:, 0].tolist()), slice_tree_sum(out[:, 1].tolist()), slice_tree_sum(out[:, 3].tolist()))
    return out, sums


class PrequentialEvaluator:
    """Test-then-train over a stream of micro-batches on one Context: process() is one
    mf_online_prequential, and one record per batch is kept (`batches`).  The cumulative values are
    sums over the records' sums divided by the evaluated events, so adding batches is exact in the
    counts and a plain left-to-right f64 sum of the per-batch sums.
    negatives > 0 (implicit feedback): the training step is mf_online_update_sampled -- every event is
    followed by `negatives` sampled updates (user, another item, negative_rating) drawn with `seed`; the
    evaluator counts the events it has processed and passes that count as first_event."""

    def __init__(self, ctx: Context, top_n: int, flavour: int = L.ONLINE_NEXT_FACTORS, num_partitions: int = 0,
                 negatives: int = 0, negative_rating: float = 0.0, seed: int = 0):
        self.ctx = ctx
        self.top_n = int(top_n)
        self.flavour = flavour
        self.num_partitions = num_partitions
        self.negatives = int(negatives)
        self.negative_rating = float(negative_rating)
        self.seed = int(seed)
        self.first_event = 0  # of the next batch: the events processed so far
        self.batches: List[Prequential] = []

    def process(self, u, i, r, exclude=None, ranks: bool = False) -> Prequential:
        if self.negatives > 0:
            rec = self.ctx.online_prequential_sampled(u, i, r, self.top_n, self.negatives, self.negative_rating,
                                                      self.seed, self.first_event, self.flavour, exclude=exclude,
                                                      ranks=ranks)
        else:
            rec = self.ctx.online_prequential(u, i, r, self.top_n, self.flavour, self.num_partitions,
                                              exclude=exclude, ranks=ranks)
        self.first_event += rec.events
        self.add(rec)
        return rec

    def add(self, rec: Prequential) -> None:
        """Append a record taken elsewhere (e.g. against a model that was then replaced)."""
        self.batches.append(rec)

    # -- cumulative ------------------------------------------------------------
    def _count(self, name: str) -> int:
        return sum(int(getattr(b, name)) for b in self.batches)

    def _sum(self, name: str) -> float:
        total = 0.0
        for b in self.batches:
            total = total + float(getattr(b, name))
        return total

    def _mean(self, total: float) -> float:
        ev = self.evaluated
        return total / ev if ev > 0 else 0.0

    events = property(lambda self: self._count("events"))
    evaluated = property(lambda self: self._count("evaluated"))
    cold = property(lambda self: self._count("cold"))
    excluded = property(lambda self: self._count("excluded"))
    hits = property(lambda self: self._count("hits"))
    sum_ndcg = property(lambda self: self._sum("sum_ndcg"))
    sum_rr = property(lambda self: self._sum("sum_rr"))
    sum_pr = property(lambda self: self._sum("sum_pr"))
    ndcg = property(lambda self: self._mean(self.sum_ndcg))
    mrr = property(lambda self: self._mean(self.sum_rr))
    hit_rate = property(lambda self: self._mean(float(self.hits)))
    mpr = property(lambda self: self._mean(self.sum_pr))

    # -- per batch -------------------------------------------------------------
    def curve(self, name: str = "ndcg") -> np.ndarray:
        """One value per batch: "ndcg", "mrr", "hit_rate" or "mpr" (the online-DCG curve)."""
        if name not in ("ndcg", "mrr", "hit_rate", "mpr"):
            raise ValueError(f"unknown metric {name!r}")
        return np.array([getattr(b, name) for b in self.batches], np.float64)


def evaluate_only(ctx: Context, u, i, top_n: int, exclude=None) -> Prequential:
    """The record mf_online_prequential would give for a batch, without the update: the ranks from
    pair_ranks, the metrics from host_prequential.  For a batch whose training step is not an online
    update (an offline refit: evaluate against the model as it stands, then refit)."""
    u, i = L.as_i32(u), L.as_i32(i)
    n = L.same_length(u, i)
    try:
        ranks, valid, _ = ctx.pair_ranks(u, i, side=L.SIDE_USER, exclude=exclude)
    except L.MFError as e:
        if e.code != L.MF_ERR_NOT_FITTED:
            raise
        ranks, valid = np.full(n, L.PAIR_RANK_COLD, np.int32), np.zeros(n, np.int32)
    vals, sums = host_prequential(ranks, valid, top_n)
    ev = int((ranks >= 0).sum())
    hits = int(vals[:, 2].sum())
    div = float(ev) if ev else 1.0
    return Prequential(events=n, evaluated=ev, cold=int((ranks == L.PAIR_RANK_COLD).sum()),
                       excluded=int((ranks == L.PAIR_RANK_EXCLUDED).sum()), hits=hits, sum_ndcg=sums[0], sum_rr=sums[1],
                       sum_pr=sums[2], ndcg=sums[0] / div if ev else 0.0, mrr=sums[1] / div if ev else 0.0,
                       hit_rate=hits / div if ev else 0.0, mpr=sums[2] / div if ev else 0.0)
