"""Ranking metrics: the definitions of mf_rank_eval (include/mfhip.h) stated on the host, and the
mirror of MLlib's RankingMetrics over a fitted model.

host_metrics is the definition of record: plain Python over mf_recommend's output with math.log,
every sum taken sequentially over ascending list position, so the device's per-query values can be
compared with it bit for bit (the device reads gains and their prefix sums the host computed with
the same libm log).

    metrics = model.rankingMetrics(heldout_pairs, exclude=train_pairs)
    metrics.precisionAt(10); metrics.ndcgAt(10); metrics.meanAveragePrecisionAt(10)
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np

from . import _lib as L
from .context import Context, RankMetrics

MAX_TOP = L.RECOMMEND_MAX_TOP
# gain_i = 1 / log(i + 2); IDCG[m] = gain_0 + ... + gain_{m-1}, added in that order
GAIN = [1.0 / math.log(i + 2) for i in range(MAX_TOP)]
IDCG = [0.0]
for _g in GAIN:
    IDCG.append(IDCG[-1] + _g)


def host_metrics(ids, counts, gt: Sequence, top_n: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-query ranking metrics of top-N lists as mf_recommend lays them out: row j of ids holds
    counts[j] valid candidate ids, best first, and gt[j] is that query's ground truth (any iterable of
    candidate ids, duplicates counting once, at least one).  Only the first min(counts[j], top_n)
    entries of a row are read.  Returns (counts [n, 2] int32 = (hits, g), values [n, 6] float64 =
    precision, recall, ap, ndcg, rr, hit)."""
    top_n = int(top_n)
    if not 1 <= top_n <= MAX_TOP:
        raise ValueError(f"top_n must be in [1, {MAX_TOP}]")
    ids = np.asarray(ids)
    n = len(gt)
    out_c = np.zeros((n, 2), np.int32)
    out_v = np.zeros((n, L.RANK_NMETRICS), np.float64)
    for j in range(n):
        truth = set(int(x) for x in gt[j])
        g = len(truth)
        if g == 0:
            raise ValueError(f"query {j} has no ground truth")
        c = min(int(counts[j]), top_n)
        hits, first = 0, -1
        ap = dcg = 0.0
        for i in range(c):
            if int(ids[j][i]) in truth:
                hits += 1
                if first < 0:
                    first = i
                ap += hits / (i + 1)
                dcg += GAIN[i]
        out_c[j] = (hits, g)
        out_v[j] = (hits / top_n, hits / g, ap / g, dcg / IDCG[min(g, top_n)],
                    1.0 / (first + 1) if first >= 0 else 0.0, 1.0 if hits > 0 else 0.0)
    return out_c, out_v


def ground_truth_sets(queries, cands) -> Dict[int, set]:
    """{query id: set of candidate ids} of a pair list."""
    out: Dict[int, set] = {}
    for q, c in zip(np.asarray(queries).tolist(), np.asarray(cands).tolist()):
        out.setdefault(int(q), set()).add(int(c))
    return out


class RankingMetrics:
    """org.apache.spark.mllib.evaluation.RankingMetrics over a fitted Context: the held-out pairs are the
    labels, the model's top-k lists (exclude = pairs never recommended, e.g. the training pairs) the
    predictions.  Every method is one mf_rank_eval at top_n = k, cached per k.  Unlike MLlib, queries
    without labels do not exist here (a query is evaluated because a held-out pair names it), and
    meanAveragePrecisionAt takes the average precision of the k-list."""

    def __init__(self, ctx: Context, gt_queries, gt_cands, exclude=None, side: int = L.SIDE_USER):
        self._ctx = ctx
        self._gq, self._gc = L.as_i32(gt_queries), L.as_i32(gt_cands)
        L.same_length(self._gq, self._gc)
        self._exclude = None if exclude is None else (L.as_i32(exclude[0]), L.as_i32(exclude[1]))
        self._side = side
        self._cache: Dict[int, RankMetrics] = {}

    def at(self, k: int) -> RankMetrics:
        k = int(k)
        if k not in self._cache:
            self._cache[k] = self._ctx.rank_eval(self._gq, self._gc, k, side=self._side, exclude=self._exclude)
        return self._cache[k]

    def precisionAt(self, k: int) -> float:
        return self.at(k).precision

    def recallAt(self, k: int) -> float:
        return self.at(k).recall

    def ndcgAt(self, k: int) -> float:
        return self.at(k).ndcg

    def meanAveragePrecisionAt(self, k: int) -> float:
        return self.at(k).map
