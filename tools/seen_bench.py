#!/usr/bin/env python3
"""The resident seen set on the NFLX-shaped model (k = 128, fast mode), in one process.

The model is seeded random factors of the NFLX synthetic's users and items (the times do not depend on
their values); the synth 90/10 split gives the pairs: the 90.4M training pairs are the seen set and the
explicit exclusion arrays, the test pairs the ground truth and the stream.  Medians of --reps calls after a
warm-up, the compared calls alternating inside every repetition:

  1. build      mf_seen_from_als (after mf_als_prepare of the training pairs) and mf_seen_set of the same
                pairs; the yardstick is the "pair tables" phase of the explicit-array mf_rank_eval.
  2. readers    mf_rank_eval, mf_pair_ranks and mf_online_prequential (--events events) three ways: with
                the set, with the same pairs as arrays, with no exclusions.
  3. recommend  mf_recommend top 10 for all users with the set against no exclusions.
  4. add        mf_seen_add of 1k / 10k / 100k / 1M events onto the training set against mf_seen_set of
                the union.

  --ab PARENT_LIB   the existing calls only (mf_recommend for all users, mf_rank_eval and
                mf_online_prequential with and without explicit exclusions), this build against another
                libmfhip.so in alternating child processes, --rounds each: medians, and the other
                build's own run-to-run span as the margin.

Writes profiles/seen_bench.json (--ab: profiles/seen_ab.json).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-recommendation_amd"))


def stats(t):
    return {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
            "all_ms": [x * 1e3 for x in t]}


def alternate(calls, reps):
    """calls: {label: fn}.  One warm-up each, then reps rounds in which every call runs once, in order."""
    for fn in calls.values():
        fn()
    out = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            out[k].append(time.perf_counter() - t0)
    return {k: stats(v) for k, v in out.items()}


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
            for m in re.finditer(r"\[mfhip\] (.*?)\s+([0-9.]+) ms", txt)}


def model(shape, scale):
    from mfhip import _lib as L
    from mfhip import synth
    from mfhip.context import Context
    k = synth.CONFIGS[shape][3]
    data = synth.config(shape, scale)
    train, test = data.split()
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_FAST_F32
    ctx = Context(p)
    rng = np.random.default_rng(5)
    for side, col in ((L.SIDE_USER, data.u), (L.SIDE_ITEM, data.i)):
        ids = np.unique(col)
        ctx.set_factors(side, ids, rng.standard_normal((len(ids), k), dtype=np.float32) * np.float32(0.3))
    return ctx, train, test, k


def run_existing(a):
    """The calls that existed before the seen set, as the three benches of tools/ time them."""
    ctx, (tu, ti, _), (su, si, sr), k = model(a.shape, a.scale)
    users = np.unique(su).astype(np.int32)
    n = min(a.events, len(su))
    eu, ei, er = su[:n], si[:n], sr[:n]
    keep = np.isin(tu, np.unique(eu))  # the training pairs of the batch's users (prequential_bench)
    xu, xi = tu[keep], ti[keep]
    calls = {
        "recommend_all_users": lambda: ctx.recommend(users, a.top_n, scores=False),
        "rank_eval_excl": lambda: ctx.rank_eval(su, si, a.top_n, exclude=(tu, ti)),
        "rank_eval_plain": lambda: ctx.rank_eval(su, si, a.top_n),
        "prequential_excl": lambda: ctx.online_prequential(eu, ei, er, a.top_n, exclude=(xu, xi)),
        "prequential_plain": lambda: ctx.online_prequential(eu, ei, er, a.top_n),
    }
    res = alternate(calls, a.reps)
    ctx.close()
    return res


def run_ab(a):
    libs = {"this": os.path.join(ROOT, "large-scale-recommendation_amd", "lib", "libmfhip.so"), "parent": a.ab}
    runs = {k: [] for k in libs}
    for rnd in range(a.rounds):
        for which, lib in libs.items():
            env = dict(os.environ, MFHIP_LIB=lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--existing", "--shape", a.shape, "--scale", str(a.scale),
                   "--events", str(a.events), "--reps", str(a.reps), "--top-n", str(a.top_n)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900).stdout
            runs[which].append(json.loads(out.strip().splitlines()[-1]))
            print(f"round {rnd} {which}: " + ", ".join(f"{k} {v['median_ms']:.1f}" for k, v in runs[which][-1].items()),
                  flush=True)
    table = {}
    for call in runs["this"][0]:
        row = {}
        for which in libs:
            med = [r[call]["median_ms"] for r in runs[which]]
            row[which] = {"median_ms": float(np.median(med)), "min_ms": min(med), "max_ms": max(med), "runs_ms": med}
        row["delta_ms"] = row["this"]["median_ms"] - row["parent"]["median_ms"]
        row["parent_span_ms"] = row["parent"]["max_ms"] - row["parent"]["min_ms"]
        row["within_parent_span"] = bool(row["delta_ms"] <= row["parent_span_ms"])
        table[call] = row
        print(f"{call}: this {row['this']['median_ms']:.1f} ms, parent {row['parent']['median_ms']:.1f} ms, "
              f"delta {row['delta_ms']:+.2f} ms, parent span {row['parent_span_ms']:.2f} ms", flush=True)
    return {"shape": a.shape, "scale": a.scale, "rounds": a.rounds, "reps_per_process": a.reps, "calls": table}


def run_seen(a):
    from mfhip import SEEN
    ctx, (tu, ti, tr), (su, si, sr), k = model(a.shape, a.scale)
    users = np.unique(su).astype(np.int32)
    n = min(a.events, len(su))
    eu, ei, er = su[:n], si[:n], sr[:n]
    res = {"shape": a.shape, "scale": a.scale, "k": k, "top_n": a.top_n, "train_pairs": len(tu), "test_pairs": len(su),
           "events": n, "reps": a.reps}

    # 1. build
    t0 = time.perf_counter()
    ctx.als_prepare(tu, ti, tr)
    res["als_prepare_ms"] = (time.perf_counter() - t0) * 1e3
    res["build"] = alternate({"seen_from_als": ctx.seen_from_als, "seen_set": lambda: ctx.seen_set(tu, ti)}, a.reps)
    res["pairs_held"] = ctx.seen_count()
    res["build"]["rank_eval_phases_explicit_ms"] = phases(lambda: ctx.rank_eval(su, si, a.top_n, exclude=(tu, ti)))
    res["build"]["rank_eval_phases_seen_ms"] = phases(lambda: ctx.rank_eval(su, si, a.top_n, exclude=SEEN))
    print("build:", json.dumps(res["build"]), flush=True)

    # 2. readers: the set, the same pairs as arrays, nothing
    ways = (("seen", SEEN), ("explicit", (tu, ti)), ("plain", None))
    res["rank_eval"] = alternate({w: (lambda e=e: ctx.rank_eval(su, si, a.top_n, exclude=e)) for w, e in ways}, a.reps)
    res["pair_ranks"] = alternate({w: (lambda e=e: ctx.pair_ranks(eu, ei, exclude=e)) for w, e in ways}, a.reps)
    res["pair_ranks"]["phases_seen_ms"] = phases(lambda: ctx.pair_ranks(eu, ei, exclude=SEEN))
    res["pair_ranks"]["phases_explicit_ms"] = phases(lambda: ctx.pair_ranks(eu, ei, exclude=(tu, ti)))
    res["prequential"] = alternate(
        {w: (lambda e=e: ctx.online_prequential(eu, ei, er, a.top_n, exclude=e)) for w, e in ways}, a.reps)
    for name in ("rank_eval", "pair_ranks", "prequential"):
        print(name + ":", {w: round(res[name][w]["median_ms"], 1) for w, _ in ways}, flush=True)

    # 3. recommend for all users
    res["recommend_all_users"] = alternate(
        {"seen": lambda: ctx.recommend(users, a.top_n, exclude=SEEN, scores=False),
         "plain": lambda: ctx.recommend(users, a.top_n, scores=False)}, a.reps)
    print("recommend:", {w: round(v["median_ms"], 1) for w, v in res["recommend_all_users"].items()}, flush=True)

    # 4. add a batch onto the training set / set the union
    res["add"] = {}
    for m in (1_000, 10_000, 100_000, 1_000_000):
        m = min(m, len(su))
        bu, bi = su[:m], si[:m]
        uu, ui = np.concatenate([tu, bu]), np.concatenate([ti, bi])
        add, whole = [], []
        for rep in range(a.reps + 1):
            ctx.seen_set(tu, ti)  # (not timed: back to the training set)
            t0 = time.perf_counter()
            ctx.seen_add(bu, bi)
            t1 = time.perf_counter()
            held = ctx.seen_count()
            t2 = time.perf_counter()
            ctx.seen_set(uu, ui)
            t3 = time.perf_counter()
            assert ctx.seen_count() == held
            if rep:  # the first round warms up
                add.append(t1 - t0)
                whole.append(t3 - t2)
        res["add"][str(m)] = {"seen_add": stats(add), "seen_set_of_union": stats(whole)}
        print(f"add {m}: seen_add {res['add'][str(m)]['seen_add']['median_ms']:.2f} ms, seen_set of the union "
              f"{res['add'][str(m)]['seen_set_of_union']['median_ms']:.1f} ms", flush=True)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="NFLX")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic (rehearsal only)")
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab", metavar="PARENT_LIB", help="compare the existing calls against another libmfhip.so")
    ap.add_argument("--rounds", type=int, default=5, help="--ab: child processes per build")
    ap.add_argument("--existing", action="store_true", help="(the child of --ab) one JSON line on stdout")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.ab:
        res, out = run_ab(a), a.out or os.path.join(ROOT, "profiles", "seen_ab.json")
    else:
        from mfhip import _lib as L
        try:
            if L.device_count() < 1:
                raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
        except L.MFNoDeviceError:
            sys.exit("seen_bench needs a GPU: there is no CPU path to time")
        if a.existing:
            print(json.dumps(run_existing(a)))
            return
        res, out = run_seen(a), a.out or os.path.join(ROOT, "profiles", "seen_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
