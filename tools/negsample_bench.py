#!/usr/bin/env python3
"""Sampled online updates of 1M-event micro-batches on the NFLX-shaped model (k = 128), f32 and f64.

The model is seeded random factors of the NFLX synthetic's users and items; the events are the first
--events pairs of the synth's test split, every rating 1 (implicit feedback), --negatives sampled
negatives per event.  Two contexts with the same factors, timed in one process after a warm-up call,
median of --reps calls each, the stream counter advancing from call to call:

  device   Context.online_update_sampled: the events go up, the device draws and expands
  host     negsample.expand (the ids the device path drew, taken beforehand with sampled=True) followed
           by Context.online_update of the expanded batch -- the path a caller has without the feature;
           the expansion and the update are also reported apart, and drawing the ids on the host
           (a vectorised numpy statement of negsample.draws) is reported beside them, not added in
  phases   one more call of each with MFHIP_TIMING=1: the library's own laps (host clock)

The library calls return after their last device wait, so the host clock around a call is the end to end
time.  Both paths leave the same model (checked on the factors after the last call).

Writes profiles/negsample_bench.json.
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


def stats(t):
    return {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
            "all_ms": [x * 1e3 for x in t]}


def phases(fn):
    """One call with the library's phase clock on; its stderr lines as [[phase, ms], ...] in order."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["MFHIP_TIMING"] = "1"
        try:
            fn()
        finally:
            os.environ.pop("MFHIP_TIMING", None)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        txt = f.read().decode(errors="replace")
    return [[m.group(1).strip(), float(m.group(2))] for m in re.finditer(r"\[mfhip\] online: (.*?)\s+([0-9.]+) ms", txt)]


def numpy_draws(seed, first_event, pos_rows, pool, negatives):
    """negsample.draws on uint64 arrays (the products wrap mod 2^64 as the definition asks)."""
    with np.errstate(over="ignore"):
        t = np.uint64(first_event) + np.arange(len(pos_rows), dtype=np.uint64)
        idx = t[:, None] * np.uint64(64) + np.arange(1, negatives + 1, dtype=np.uint64)[None, :]
        z = np.uint64(seed & (2**64 - 1)) + np.uint64(0x9E3779B97F4A7C15) * idx
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        c = ((z >> np.uint64(32)) * np.uint64(pool - 1)) >> np.uint64(32)
    c = c.astype(np.int64)
    return (c + (c >= np.asarray(pos_rows, np.int64)[:, None])).astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="NFLX")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic (rehearsal only)")
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "negsample_bench.json"))
    a = ap.parse_args()
    from mfhip import _lib as L
    from mfhip import negsample as NS
    from mfhip import synth
    from mfhip.context import Context
    try:
        if L.device_count() < 1:
            raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
    except L.MFNoDeviceError:
        sys.exit("negsample_bench needs a GPU: there is no CPU path to time")

    k = synth.CONFIGS[a.shape][3]
    data = synth.config(a.shape, a.scale)
    _, (su, si, _) = data.split()
    n = min(a.events, len(su))
    eu, ei, er = su[:n].copy(), si[:n].copy(), np.ones(n)
    uids, iids = np.unique(data.u), np.unique(data.i)
    rng = np.random.default_rng(5)
    P = rng.random((len(uids), k)) * 0.2
    Q = rng.random((len(iids), k)) * 0.2
    neg = a.negatives
    res = {"shape": a.shape, "scale": a.scale, "k": k, "events": int(n), "negatives": neg, "updates": int(n * (1 + neg)),
           "users": len(uids), "items": len(iids), "reps": a.reps}
    print(res, flush=True)
    # numpy_draws against the library's draws, then timed: what generating the ids on the host costs
    pos = np.searchsorted(iids, ei).astype(np.int32)   # set_factors gives rows in this order
    assert np.array_equal(numpy_draws(a.seed, 3, pos[:5000], len(iids), neg), NS.device_draws(a.seed, 3, pos[:5000], len(iids), neg))
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        iids[numpy_draws(a.seed, 0, pos, len(iids), neg)]
        t.append(time.perf_counter() - t0)
    res["host_draw_numpy"] = stats(t)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    for label, mode in (("f32", L.MODE_FAST_F32), ("f64", L.MODE_DETERMINISTIC_F64)):
        p = L.default_params()
        p.num_factors, p.mode = k, mode
        r = {"upload_mb": {"device": n * (12 if label == "f32" else 16) / 1e6,
                           "host": n * (1 + neg) * (12 if label == "f32" else 16) / 1e6}}
        with Context(p) as dev, Context(p) as host:
            for ctx in (dev, host):
                ctx.set_factors(L.SIDE_USER, uids, P)
                ctx.set_factors(L.SIDE_ITEM, iids, Q)
            t_dev, t_host, t_exp, t_upd = [], [], [], []
            first = 0
            for rep in range(a.reps + 2):   # call 0 warms up, the last one runs under the phase clock
                # the ids of this call (untimed): a probe of the draws, not an update
                ids = iids[NS.device_draws(a.seed, first, pos, len(iids), neg)] if rep == 0 else \
                    iids[numpy_draws(a.seed, first, pos, len(iids), neg)]
                last = rep == a.reps + 1

                def run_dev():
                    return dev.online_update_sampled(eu, ei, er, neg, 0.0, a.seed, first)

                def run_host():
                    U, I, R = NS.expand(eu, ei, er, ids, 0.0)
                    tx = time.perf_counter()
                    out = host.online_update(U, I, R)
                    return out, tx

                if last:
                    r["device_phases_ms"] = phases(run_dev)
                    r["host_phases_ms"] = phases(run_host)
                else:
                    t0 = time.perf_counter()
                    td = run_dev()
                    t1 = time.perf_counter()
                    th, tx = run_host()
                    t2 = time.perf_counter()
                    assert td == th, (td, th)
                    if rep > 0:
                        t_dev.append(t1 - t0)
                        t_host.append(t2 - t1)
                        t_exp.append(tx - t1)
                        t_upd.append(t2 - tx)
                first += n
            same = all(np.array_equal(x, y) for side in (L.SIDE_USER, L.SIDE_ITEM)
                       for x, y in zip(dev.factors(side), host.factors(side)))
        r.update(device=stats(t_dev), host=stats(t_host), host_expand=stats(t_exp), host_update=stats(t_upd),
                 same_model=bool(same))
        r["host_over_device"] = r["host"]["median_ms"] / r["device"]["median_ms"]
        r["updates_per_s"] = {"device": n * (1 + neg) / (r["device"]["median_ms"] / 1e3),
                              "host": n * (1 + neg) / (r["host"]["median_ms"] / 1e3)}
        res[label] = r
        print(label, "device", r["device"]["median_ms"], "host", r["host"]["median_ms"], "(expand",
              r["host_expand"]["median_ms"], "update", r["host_update"]["median_ms"], ") ratio", r["host_over_device"],
              "same model", same, flush=True)
        print(" device phases", r["device_phases_ms"], "\n host phases", r["host_phases_ms"], flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
