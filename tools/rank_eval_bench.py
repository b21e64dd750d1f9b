#!/usr/bin/env python3
"""Ranking metrics of a held-out split, two ways, on the NFLX- and ML20M-shaped synthetics.

The model is seeded random factors (the time does not depend on their values), the synth 90/10 split
gives the pairs: the training pairs are the exclusions, the test pairs the ground truth, top_n = 10.
Timed in one process, median of --reps calls each:

  (a) what a caller did before mf_rank_eval: Context.recommend for the test users with the exclusions
      (ids only), then the metrics of mfhip.ranking.host_metrics vectorised in numpy;
  (b) Context.rank_eval;
  both again without exclusions; the mf_recommend call of (a) is also reported alone.

One more rank_eval call per setting runs with MFHIP_TIMING=1 and the library's phase lines on stderr
are read back: how (b) splits into the pair tables (id lookup on the host, upload, device build), the
batch loop (score, select, metrics, sums; one wait at its end) and the results (the copy back).

Recorded condition: without exclusions (b) does not exceed the mf_recommend call alone by more than
that call's run-to-run spread (max - min of its repetitions).

Writes profiles/rank_eval_bench.json.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-recommendation_amd"))

SIGN = np.uint64(0x80000000)


def pack(pos, ids):
    return (pos.astype(np.uint64) << np.uint64(32)) | ((ids.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) ^ SIGN)


def numpy_metrics(ids, cnt, users, gt_u, gt_i, top_n):
    """host_metrics over all rows at once: the means of precision, recall, ap, ndcg, rr, hit."""
    from mfhip.ranking import GAIN, IDCG
    n = len(users)
    truth = np.unique(pack(np.searchsorted(users, gt_u), gt_i))
    g = np.bincount((truth >> np.uint64(32)).astype(np.int64), minlength=n).astype(np.float64)
    keys = pack(np.repeat(np.arange(n), top_n), ids.reshape(-1))
    at = np.searchsorted(truth, keys)
    hit = (truth[np.minimum(at, len(truth) - 1)] == keys).reshape(n, top_n)
    hit &= np.arange(top_n)[None, :] < cnt[:, None]
    hits = hit.sum(axis=1)
    ap = (hit * np.cumsum(hit, axis=1) / np.arange(1, top_n + 1)).sum(axis=1) / g
    dcg = (hit * np.array(GAIN[:top_n])).sum(axis=1)
    ndcg = dcg / np.array(IDCG)[np.minimum(g, top_n).astype(np.int64)]
    rr = np.where(hits > 0, 1.0 / (hit.argmax(axis=1) + 1), 0.0)
    return [float(x.mean()) for x in (hits / top_n, hits / g, ap, ndcg, rr, (hits > 0).astype(np.float64))]


def phases(ctx, args, kw):
    """One rank_eval call with the library's phase clock on; its stderr lines as {phase: ms}."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["MFHIP_TIMING"] = "1"
        try:
            ctx.rank_eval(*args, **kw)
        finally:
            os.environ.pop("MFHIP_TIMING", None)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        txt = f.read().decode(errors="replace")
    return {m.group(1).strip().replace(" ", "_"): float(m.group(2))
            for m in re.finditer(r"\[mfhip\] rank_eval: (.*?)\s+([0-9.]+) ms", txt)}


def stats(t):
    return {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
            "all_ms": [x * 1e3 for x in t]}


def run_shape(name, scale, top_n, reps):
    from mfhip import _lib as L
    from mfhip import synth
    from mfhip.context import Context

    nu, ni, nr, k, _ = synth.CONFIGS[name]
    data = synth.config(name, scale)
    (tu, ti, _), (su, si, _) = data.split()
    rng = np.random.default_rng(5)
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_FAST_F32
    res = {"shape": name, "scale": scale, "k": k, "top_n": top_n, "train_pairs": len(tu), "test_pairs": len(su),
           "reps": reps}
    with Context(p) as ctx:
        for side, col in ((L.SIDE_USER, data.u), (L.SIDE_ITEM, data.i)):
            ids = np.unique(col)
            ctx.set_factors(side, ids, rng.standard_normal((len(ids), k), dtype=np.float32) * np.float32(0.3))
        users = np.unique(su).astype(np.int32)
        res["queries"] = len(users)
        for label, excl in (("with_exclusions", (tu, ti)), ("without_exclusions", None)):
            rec, host, dev = [], [], []
            ctx.recommend(users[:1000], top_n, scores=False)  # warm-up: buffers, kernels loaded
            ctx.rank_eval(su[:1000], si[:1000], top_n)
            for _ in range(reps):
                t0 = time.perf_counter()
                ids, _, cnt = ctx.recommend(users, top_n, exclude=excl, scores=False)
                t1 = time.perf_counter()
                means_a = numpy_metrics(ids, cnt, users, su, si, top_n)
                t2 = time.perf_counter()
                rec.append(t1 - t0)
                host.append(t2 - t0)
            for _ in range(reps):
                t0 = time.perf_counter()
                m = ctx.rank_eval(su, si, top_n, exclude=excl)
                dev.append(time.perf_counter() - t0)
            means_b = [m.precision, m.recall, m.map, m.ndcg, m.mrr, m.hit_rate]
            assert m.queries == len(users) and np.allclose(means_a, means_b, rtol=1e-9, atol=0), (means_a, means_b)
            r = {"a_recommend_plus_numpy": stats(host), "a_recommend_alone": stats(rec), "b_rank_eval": stats(dev),
                 "b_phases_ms": phases(ctx, (su, si, top_n), {"exclude": excl}), "ndcg": m.ndcg, "hits": m.hits}
            r["speedup_b_over_a"] = r["a_recommend_plus_numpy"]["median_ms"] / r["b_rank_eval"]["median_ms"]
            if excl is None:
                spread = r["a_recommend_alone"]["max_ms"] - r["a_recommend_alone"]["min_ms"]
                r["recommend_spread_ms"] = spread
                r["b_within_recommend_plus_spread"] = bool(
                    r["b_rank_eval"]["median_ms"] <= r["a_recommend_alone"]["median_ms"] + spread)
            res[label] = r
            print(f"{name} {label}: (a) {r['a_recommend_plus_numpy']['median_ms']:.1f} ms (mf_recommend alone "
                  f"{r['a_recommend_alone']['median_ms']:.1f} ms), (b) {r['b_rank_eval']['median_ms']:.1f} ms, "
                  f"phases {r['b_phases_ms']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="ML20M,NFLX")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetics (rehearsal only)")
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_eval_bench.json"))
    a = ap.parse_args()
    from mfhip import _lib as L
    try:
        if L.device_count() < 1:
            raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
    except L.MFNoDeviceError:
        sys.exit("rank_eval_bench needs a GPU: there is no CPU path to time")
    out = {"runs": []}
    for name in a.shapes.split(","):
        out["runs"].append(run_shape(name, a.scale, a.top_n, a.reps))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
