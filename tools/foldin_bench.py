#!/usr/bin/env python3
"""Stateless fold-in on the NFLX-shaped synthetic (480,189 x 17,770, the training split), k = 128, fast mode.

--holdout users (100k) are left out of the prepare with all their ratings; the model is prepared on the rest
and trained for --fit-iters iterations.  The sessions are the complete rating lists of the first 1k, 10k and
100k of those users.  Everything is timed with the host clock around blocking calls, the routes alternating in
one process, medians of --reps:

  fused     mf_recommend_foldin(top 10, exclude_rated = 1).
  two_call  mf_als_foldin, the vectors downloaded, then mf_recommend_vectors with the sessions' pairs as
            explicit exclusion arrays (what the fused call saves: the vectors' round trip and the host's
            exclusion table).
  stateful  on a second context prepared and trained alike: mf_als_append of the sessions' ratings,
            mf_als_run_rows of their users, mf_recommend with the pairs as exclusions -- the only route before
            mf_als_foldin.  The rows are removed again (mf_als_remove_rows, not timed) before the next
            repetition; from the second repetition on the users' factor rows exist already, which favours
            this route.
  phases    one more fused call with MFHIP_TIMING=1 (the stream drained after every phase): upload, table
            build, solve, score-and-select, summed over the call's batches.
  length    the fused call on up to 1000 sessions of every length bucket: the per-session cost against the
            session length (whether a dual-form solve for sessions shorter than the rank is worth building).

Nothing here is a threshold.  Writes profiles/foldin_bench.json.
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

TOP = 10
BUCKETS = [(1, 16), (16, 64), (64, 128), (128, 256), (256, 1024), (1024, 1 << 30)]


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def med(x):
    return float(np.median(x))


def span(x):
    return [float(min(x)), float(max(x))]


def phases_of(f):
    """f() with MFHIP_TIMING=1 and the library's stderr captured: {phase: ms summed over the batches}."""
    sys.stderr.flush()
    keep = os.dup(2)
    out = {}
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["MFHIP_TIMING"] = "1"
        try:
            f()
        finally:
            del os.environ["MFHIP_TIMING"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        for line in tmp.read().decode(errors="replace").splitlines():
            m = re.match(r"\[mfhip\] foldin (\w+)\s+([0-9.]+) ms", line)
            if m:
                out[m.group(1)] = out.get(m.group(1), 0.0) + float(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=5)
    ap.add_argument("--holdout", type=int, default=100_000, help="users left out of the prepare")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic (rehearsal only)")
    ap.add_argument("--no-stateful", action="store_true", help="skip the second context")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foldin_bench.json"))
    a = ap.parse_args()
    from mfhip import _lib as L
    from mfhip import synth
    from mfhip.context import Context, als_solve
    try:
        if L.device_count() < 1:
            raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
    except L.MFNoDeviceError:
        sys.exit("foldin_bench needs a GPU: there is no CPU path to time")
    nu, ni, nr, _, _ = synth.CONFIGS["NFLX"]
    (u, i, r), _ = synth.generate(max(1, int(nu * a.scale)), max(1, int(ni * a.scale)),
                                  max(1, int(nr * a.scale))).split()
    users = np.unique(u)
    H = min(a.holdout, len(users) // 2)
    held = np.random.default_rng(17).permutation(users)[:H]
    out_mask = np.isin(u, held)
    base = tuple(np.ascontiguousarray(x[~out_mask]) for x in (u, i, r))
    # the held-out users' complete lists, grouped by user in `held` order, each in arrival order
    hu, hi, hr = (x[out_mask] for x in (u, i, r))
    rank = np.empty(int(held.max()) + 1 - int(held.min()), np.int64)
    rank[held - held.min()] = np.arange(H)
    order = np.argsort(rank[hu - held.min()], kind="stable")
    hu, hi, hr = (np.ascontiguousarray(x[order]) for x in (hu, hi, hr))
    counts = np.bincount(rank[hu - held.min()], minlength=H)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    del u, i, r, out_mask, order

    p = L.default_params()
    p.num_factors = a.k
    p.mode = L.MODE_FAST_F32
    how = als_solve(a.lam)
    sizes = [n for n in (1_000, 10_000, 100_000) if n <= H] or [H]
    res = {"shape": "NFLX", "scale": a.scale, "k": a.k, "lambda": a.lam, "reps": a.reps, "top_n": TOP,
           "nnz_prepared": len(base[0]), "holdout_users": int(H), "holdout_ratings": int(off[-1]),
           "fit_iters": a.fit_iters, "sessions": {}, "by_length": {}}

    def trained(ctx):
        ctx.als_prepare(*base)
        ctx.als_run(2 * a.fit_iters, a.lam)

    def lists(n):
        e = int(off[n])
        return off[:n + 1], hi[:e], hr[:e], hu[:e]

    with Context(p) as ctx:
        trained(ctx)
        cold = None
        if not a.no_stateful:
            cold = Context(p)
            trained(cold)
        print(f"prepared on {len(base[0])} ratings; {H} users held out with {int(off[-1])} ratings", flush=True)
        for n in sizes:
            o, ci, cr, cu = lists(n)
            eq = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
            t = {"fused": [], "two_call": [], "two_call_foldin": [], "two_call_vectors": [], "stateful": [],
                 "stateful_append": [], "stateful_rows": [], "stateful_recommend": []}
            ctx.recommend_foldin(L.SIDE_USER, o, ci, cr, how, TOP)          # scratch sized before the clock starts
            for rep in range(a.reps):
                ms, fused = clock(lambda: ctx.recommend_foldin(L.SIDE_USER, o, ci, cr, how, TOP))
                t["fused"].append(ms)
                m1, (vecs, used) = clock(lambda: ctx.als_foldin(L.SIDE_USER, o, ci, cr, how))
                m2, two = clock(lambda: ctx.recommend_vectors(vecs, TOP, side=L.SIDE_ITEM, exclude=(eq, ci)))
                t["two_call_foldin"].append(m1)
                t["two_call_vectors"].append(m2)
                t["two_call"].append(m1 + m2)
                live = used > 0
                assert np.array_equal(fused[0][live], two[0][live]) and np.array_equal(fused[2][live], two[2][live])
                if cold is not None:
                    ids = held[:n].astype(np.int32)
                    m1, _ = clock(lambda: cold.als_append(cu, ci, cr))
                    m2, _ = clock(lambda: cold.als_run_rows(L.SIDE_USER, ids, how))
                    m3, _ = clock(lambda: cold.recommend(ids, TOP, side=L.SIDE_USER, exclude=(cu, ci)))
                    t["stateful_append"].append(m1)
                    t["stateful_rows"].append(m2)
                    t["stateful_recommend"].append(m3)
                    t["stateful"].append(m1 + m2 + m3)
                    cold.als_remove_rows(L.SIDE_USER, ids)
            out = {key: {"median": med(v), "span": span(v), "all": v} for key, v in t.items() if v}
            out["entries"] = int(o[-1])
            out["phases_ms"] = phases_of(lambda: ctx.recommend_foldin(L.SIDE_USER, o, ci, cr, how, TOP))
            out["fused_us_per_session"] = 1e3 * out["fused"]["median"] / n
            res["sessions"][str(n)] = out
            print(f"sessions {n:>7} ({int(o[-1])} entries): fused {out['fused']['median']:.2f} ms "
                  f"{out['fused']['span']}, two calls {out['two_call']['median']:.2f} ms {out['two_call']['span']} "
                  f"(foldin {out['two_call_foldin']['median']:.2f} + vectors {out['two_call_vectors']['median']:.2f})"
                  + (f", stateful {out['stateful']['median']:.2f} ms (append {out['stateful_append']['median']:.2f} + "
                     f"rows {out['stateful_rows']['median']:.2f} + recommend {out['stateful_recommend']['median']:.2f})"
                     if cold is not None else "") + f"; phases {out['phases_ms']}", flush=True)
        if cold is not None:
            cold.close()
        # the per-session cost against the session length
        for lo, hi_ in BUCKETS:
            pick = np.flatnonzero((counts >= lo) & (counts < hi_))[:1000]
            if len(pick) == 0:
                continue
            o = np.concatenate([[0], np.cumsum(counts[pick])]).astype(np.int64)
            at = np.concatenate([np.arange(off[j], off[j + 1]) for j in pick])
            ci, cr = np.ascontiguousarray(hi[at]), np.ascontiguousarray(hr[at])
            ctx.recommend_foldin(L.SIDE_USER, o, ci, cr, how, TOP)
            ms = [clock(lambda: ctx.recommend_foldin(L.SIDE_USER, o, ci, cr, how, TOP))[0] for _ in range(a.reps)]
            sv = [clock(lambda: ctx.als_foldin(L.SIDE_USER, o, ci, cr, how))[0] for _ in range(a.reps)]
            key = f"{lo}..{hi_ - 1}" if hi_ < (1 << 30) else f"{lo}.."
            res["by_length"][key] = {"sessions": int(len(pick)), "mean_length": float(counts[pick].mean()),
                                     "fused_ms": med(ms), "fused_span": span(ms), "foldin_ms": med(sv),
                                     "fused_us_per_session": 1e3 * med(ms) / len(pick),
                                     "foldin_us_per_session": 1e3 * med(sv) / len(pick)}
            print(f"length {key:>10}: {len(pick)} sessions, mean {counts[pick].mean():.0f}: fused {med(ms):.2f} ms = "
                  f"{1e3 * med(ms) / len(pick):.1f} us per session, foldin alone {1e3 * med(sv) / len(pick):.1f} us",
                  flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
