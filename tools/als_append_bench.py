#!/usr/bin/env python3
"""Incremental ALS on the NFLX-shaped synthetic (480,189 x 17,770, the training split), k = 128, fast mode.

The model is prepared on all but the last 1M ratings of the split and trained for --fit-iters iterations.
The last 1M are then the stream.  Everything is timed with the host clock around blocking calls, in one
process, medians of --reps:

  append    mf_als_append of a batch of 1k / 10k / 100k / 1M events, against mf_als_prepare of the whole
            concatenation (the prepared part ++ that batch) on a second context -- what a caller had to do
            for the same job before mf_als_append existed.
  update    mf_als_update(rounds = 1) taken apart into its three calls (mf_als_append, mf_als_run_rows of the
            batch's users, mf_als_run_rows of its items) with the rows solved per side, against one full
            iteration (mf_als_run(2)) on the same context.
  quality   the RMSE on the 1M streamed ratings after streaming them in 100k batches with rounds = 1, then
            after mf_als_run(2) and after 20 half-sweeps in all on the resident data (no upload).

For the batches below 1M every repetition appends another slice of the stream to the same context (the
CSR grows by at most 0.6 % on the way); for 1M the context is prepared and trained again before every
repetition.  Nothing here is a threshold.  Writes profiles/als_append_bench.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-recommendation_amd"))


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=5)
    ap.add_argument("--stream", type=int, default=1_000_000, help="ratings held back as the stream")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic (rehearsal only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_append_bench.json"))
    a = ap.parse_args()
    from mfhip import _lib as L
    from mfhip import synth
    from mfhip.context import Context, als_solve
    try:
        if L.device_count() < 1:
            raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
    except L.MFNoDeviceError:
        sys.exit("als_append_bench needs a GPU: there is no CPU path to time")
    nu, ni, nr, _, _ = synth.CONFIGS["NFLX"]
    (u, i, r), _ = synth.generate(max(1, int(nu * a.scale)), max(1, int(ni * a.scale)),
                                  max(1, int(nr * a.scale))).split()
    S = min(a.stream, len(u) // 2)
    base = tuple(np.ascontiguousarray(x[:-S]) for x in (u, i, r))
    tail = tuple(np.ascontiguousarray(x[-S:]) for x in (u, i, r))
    p = L.default_params()
    p.num_factors = a.k
    p.mode = L.MODE_FAST_F32
    how = als_solve(a.lam)
    sizes = [n for n in (1_000, 10_000, 100_000) if n * a.reps <= S] + [S]
    res = {"shape": "NFLX", "scale": a.scale, "k": a.k, "lambda": a.lam, "reps": a.reps, "nnz_prepared": len(base[0]),
           "stream": S, "fit_iters": a.fit_iters, "batches": {}}

    def batch(n, rep):
        lo = 0 if n == S else rep * n
        return tuple(x[lo:lo + n] for x in tail)

    def trained(ctx):
        ms, _ = clock(lambda: ctx.als_prepare(*base))
        ctx.als_run(2 * a.fit_iters, a.lam)
        return ms

    with Context(p) as ctx, Context(p) as cold:
        res["prepare_ms"] = trained(ctx)
        res["iteration_ms"] = med([clock(lambda: ctx.als_run(2, a.lam))[0] for _ in range(a.reps)])
        print(f"prepare of {len(base[0])} ratings {res['prepare_ms']:.0f} ms; one full iteration "
              f"{res['iteration_ms']:.1f} ms", flush=True)
        for n in sizes:
            t = {"append": [], "users": [], "items": [], "prepare_concat": []}
            solved = {"users": [], "items": []}
            for rep in range(a.reps):
                if n == S:
                    trained(ctx)
                bu, bi, br = batch(n, rep)
                t["append"].append(clock(lambda: ctx.als_append(bu, bi, br))[0])
                ms, su = clock(lambda: ctx.als_run_rows(L.SIDE_USER, bu, how))
                t["users"].append(ms)
                ms, si = clock(lambda: ctx.als_run_rows(L.SIDE_ITEM, bi, how))
                t["items"].append(ms)
                solved["users"].append(su)
                solved["items"].append(si)
                whole = tuple(np.concatenate([x, y]) for x, y in zip(base, (bu, bi, br)))
                t["prepare_concat"].append(clock(lambda: cold.als_prepare(*whole))[0])
                del whole
            out = {key: {"median": med(v), "all": v} for key, v in t.items()}
            out["update_ms"] = med([x + y + z for x, y, z in zip(t["append"], t["users"], t["items"])])
            out["rows_solved"] = {key: int(np.median(v)) for key, v in solved.items()}
            out["append_speedup_over_prepare"] = out["prepare_concat"]["median"] / out["append"]["median"]
            out["update_share_of_iteration"] = out["update_ms"] / res["iteration_ms"]
            res["batches"][str(n)] = out
            print(f"batch {n:>8}: append {out['append']['median']:.2f} ms (prepare of the concatenation "
                  f"{out['prepare_concat']['median']:.0f} ms, x{out['append_speedup_over_prepare']:.0f}); users "
                  f"{out['users']['median']:.2f} ms ({out['rows_solved']['users']} rows), items "
                  f"{out['items']['median']:.2f} ms ({out['rows_solved']['items']} rows); update "
                  f"{out['update_ms']:.2f} ms = {100 * out['update_share_of_iteration']:.1f} % of a full iteration",
                  flush=True)
        # quality: the stream in 100k batches, then full half-sweeps on the resident data
        trained(ctx)
        q = {"before_stream": ctx.rmse(*tail)[0]}
        step = min(100_000, S)
        for lo in range(0, S, step):
            ctx.als_update(*(x[lo:lo + step] for x in tail), how, 1)
        q["streamed_rounds_1"] = ctx.rmse(*tail)[0]
        ctx.als_run(2, a.lam)
        q["refit_2_half_sweeps"] = ctx.rmse(*tail)[0]
        ctx.als_run(18, a.lam)
        q["refit_20_half_sweeps"] = ctx.rmse(*tail)[0]
        res["stream_rmse"] = q
        print("RMSE on the streamed ratings:", q, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
