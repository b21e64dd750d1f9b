#!/usr/bin/env python3
"""Prequential evaluation of 1M-event micro-batches on the NFLX-shaped model (k = 128, fast mode).

The model is seeded random factors of the NFLX synthetic's users and items (the time does not depend on
their values); the synth 90/10 split gives the stream: the events are the first --events test pairs,
the exclusions the training pairs of the batch's users.  Timed in one process, after a warm-up call,
median of --reps calls each, with and without the exclusions:

  end to end   Context.online_prequential (rank the batch, sum the metrics, then learn the batch)
  ranking      Context.pair_ranks alone (ids resolved, exclusion table, targets, walk, subtraction, copy back)
  update       Context.online_update alone
  phases       one more pair_ranks call with MFHIP_TIMING=1: the library's own split into the tables and
               the batch loop (a wait at the end of each, host clock)

The library calls return after their last device wait, so the host clock around a call is the end to end
time; the torch comparison is timed with device events.  Two comparisons in the same process:

  (i)  torch: what a user would write -- P[u] @ Q.T in batches that fit memory, compared against the
       gathered target score, row-summed (no exclusions, no tie rule);
  (ii) mf_recommend at top 10 for the same query rows: the same product plus a selection.  mf_recommend
       scores each distinct user once, so both are reported per scored column.

Also: the f32 walk at 1, 2 and 4 waves per workgroup (MFHIP_TEST pr_nw) and at three batch sizes
(pr_batch), without exclusions, which is how the defaults were chosen.

Writes profiles/prequential_bench.json.
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


def timed(fn, reps):
    fn()  # warm-up: buffers sized, kernels loaded
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return stats(out)


def phases(fn):
    """One call with the library's phase clock on; its stderr lines as {phase: ms}."""
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
    return {m.group(1).strip().replace(" ", "_"): float(m.group(2))
            for m in re.finditer(r"\[mfhip\] pair_ranks: (.*?)\s+([0-9.]+) ms", txt)}


def with_knob(key, value, fn):
    old = os.environ.get("MFHIP_TEST")
    os.environ["MFHIP_TEST"] = f"{key}={value}"
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("MFHIP_TEST", None)
        else:
            os.environ["MFHIP_TEST"] = old


def torch_ranks(P, Q, urow, irow, reps, chunk):
    """(i): the count of items scoring above the event's item, per event, with device events."""
    import torch
    dev = torch.device("cuda:0")
    Pt, Qt = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
    ur, ir = torch.from_numpy(urow.astype(np.int64)).to(dev), torch.from_numpy(irow.astype(np.int64)).to(dev)

    def run():
        out = torch.empty(len(urow), dtype=torch.int64, device=dev)
        for b in range(0, len(urow), chunk):
            u, i = ur[b:b + chunk], ir[b:b + chunk]
            s = Pt[u] @ Qt.T
            t = s.gather(1, i[:, None])
            out[b:b + chunk] = (s > t).sum(dim=1)
        return out

    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 1e3)
    res = out.cpu().numpy()
    del Pt, Qt, ur, ir, out
    torch.cuda.empty_cache()
    return stats(ms), res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="NFLX")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic (rehearsal only)")
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prequential_bench.json"))
    a = ap.parse_args()
    try:  # torch's HIP runtime has to come up before libmfhip's, or it finds no device afterwards
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda:0")
    except ImportError:
        pass
    from mfhip import _lib as L
    from mfhip import synth
    from mfhip.context import Context
    try:
        if L.device_count() < 1:
            raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
    except L.MFNoDeviceError:
        sys.exit("prequential_bench needs a GPU: there is no CPU path to time")

    k = synth.CONFIGS[a.shape][3]
    data = synth.config(a.shape, a.scale)
    (tu, ti, _), (su, si, sr) = data.split()
    n = min(a.events, len(su))
    eu, ei, er = su[:n].copy(), si[:n].copy(), sr[:n].copy()
    keep = np.isin(tu, np.unique(eu))
    xu, xi = tu[keep], ti[keep]
    rng = np.random.default_rng(5)
    uids, iids = np.unique(data.u), np.unique(data.i)
    P = rng.standard_normal((len(uids), k), dtype=np.float32) * np.float32(0.3)
    Q = rng.standard_normal((len(iids), k), dtype=np.float32) * np.float32(0.3)
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_FAST_F32
    res = {"shape": a.shape, "scale": a.scale, "k": k, "top_n": a.top_n, "events": int(n), "users": len(uids),
           "items": len(iids), "distinct_event_users": int(len(np.unique(eu))), "exclusion_pairs": int(len(xu)),
           "reps": a.reps}
    print(res, flush=True)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    with Context(p) as ctx:
        ctx.set_factors(L.SIDE_USER, uids, P)
        ctx.set_factors(L.SIDE_ITEM, iids, Q)
        # the ranking part, and the comparisons, on the model as set (no update in between)
        for label, excl in (("without_exclusions", None), ("with_exclusions", (xu, xi))):
            r = {"ranking": timed(lambda: ctx.pair_ranks(eu, ei, exclude=excl), a.reps),
                 "ranking_phases_ms": phases(lambda: ctx.pair_ranks(eu, ei, exclude=excl))}
            res[label] = r
            print(label, "ranking", r["ranking"]["median_ms"], r["ranking_phases_ms"], flush=True)
            save()
        ranks, valid, _ = ctx.pair_ranks(eu, ei)
        users = np.unique(eu).astype(np.int32)
        rec = timed(lambda: ctx.recommend(users, a.top_n, scores=False), a.reps)
        loop_ms = res["without_exclusions"]["ranking_phases_ms"].get("batch_loop")
        res["recommend_top_n"] = dict(rec, columns=len(users), ns_per_column=rec["median_ms"] * 1e6 / len(users))
        res["pair_ranks_ns_per_column"] = {
            "call": res["without_exclusions"]["ranking"]["median_ms"] * 1e6 / n,
            "batch_loop": loop_ms * 1e6 / n if loop_ms else None}
        print("recommend", res["recommend_top_n"]["median_ms"], res["recommend_top_n"]["ns_per_column"],
              res["pair_ranks_ns_per_column"], flush=True)
        save()
        res["walk_shapes_without_exclusions"] = {}
        for key, values in (("pr_nw", (1, 2, 4)), ("pr_batch", (8192, 32768, 131072))):
            for v in values:
                ph = with_knob(key, v, lambda: (ctx.pair_ranks(eu, ei), phases(lambda: ctx.pair_ranks(eu, ei)))[1])
                res["walk_shapes_without_exclusions"][f"{key}={v}"] = ph
                print(key, v, ph, flush=True)
        save()
        # end to end and the update part: these learn the batch, so they come last
        for label, excl in (("without_exclusions", None), ("with_exclusions", (xu, xi))):
            res[label]["update"] = timed(lambda: ctx.online_update(eu, ei, er), a.reps)
            res[label]["end_to_end"] = timed(lambda: ctx.online_prequential(eu, ei, er, a.top_n, exclude=excl), a.reps)
            m = ctx.online_prequential(eu, ei, er, a.top_n, exclude=excl)
            res[label]["record"] = {"evaluated": m.evaluated, "cold": m.cold, "excluded": m.excluded, "hits": m.hits,
                                    "ndcg": m.ndcg, "mpr": m.mpr}
            print(label, "update", res[label]["update"]["median_ms"], "end to end",
                  res[label]["end_to_end"]["median_ms"], res[label]["record"], flush=True)
            save()
        # (i) torch, on the same rows (the factors as they were set)
        urow, irow = np.searchsorted(uids, eu), np.searchsorted(iids, ei)
        try:
            tstats, above = torch_ranks(P, Q, urow, irow, a.reps, a.torch_chunk)
            # the torch count ignores the tie rule: equal only where no score ties with the target
            res["torch"] = dict(tstats, chunk=a.torch_chunk, equal_ranks=int((above == ranks).sum()))
            print("torch", tstats["median_ms"], res["torch"]["equal_ranks"], flush=True)
        except Exception as e:  # the comparison is a courtesy: the library's numbers stand without it
            res["torch"] = {"error": repr(e)}
            print("torch failed:", e, flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
