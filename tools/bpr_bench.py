#!/usr/bin/env python3
"""BPR training (mf_bpr_run) on the NFLX-shaped data (k = 128, fast mode), in one process.

The synth 90/10 split gives the pairs: the training pairs are the seen set BPR draws from, the test pairs the
held-out ground truth.  Nothing here has a threshold; the numbers are reported as they are.

  1. throughput  triples per second of mf_bpr_run at batches of 64k, 256k and 1M (MEAN scale), the median of
                 --reps calls of a few steps each after a warm-up; beside it a torch step on the same GPU given
                 the same triples (index_select, sigmoid, index_add_), and the 1.3e8 updates/s of the sampled
                 online path for scale.
  2. phases      one call per batch size with MFHIP_TIMING: the step's phases, the stream drained after each.
  3. quality     NDCG at 10 on the held-out pairs, seen pairs excluded, after --epochs epochs of mf_bpr_fit
                 (an epoch = pairs / batch steps), beside mf_als_fit_implicit at the same rank.

Writes profiles/bpr_bench.json.
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

ONLINE_SAMPLED_UPDATES_PER_S = 1.3e8


def stats(t):
    return {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
            "all_ms": [x * 1e3 for x in t]}


def phase_sums(fn):
    """One call with the library's phase clock on; its stderr lines summed per phase, {phase: ms}."""
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
    out = {}
    for m in re.finditer(r"\[mfhip\] (.*?)\s+([0-9.]+) ms", txt):
        key = m.group(1).strip().replace(" ", "_")
        out[key] = out.get(key, 0.0) + float(m.group(2))
    return out


def load_torch():
    """torch with its GPU context made, or the reason there is none.  Called before the library touches the
    device: torch brings a HIP runtime of its own, and it finds the GPU only when it initialises first."""
    try:
        import torch
    except ImportError as e:
        return None, f"import torch: {e}"
    if not torch.cuda.is_available():
        return None, "torch sees no GPU"
    torch.zeros(1, device="cuda:0")
    return torch, None


def torch_step_time(torch, why, ctx, k, nu, ni, reps, lr, lam):
    """A torch step on the triples of the library's last step: gather, sigmoid, scatter-add ({"error": ...} without
    a usable torch)."""
    if torch is None:
        return {"error": why}
    u, i, j = ctx.debug_bpr_triples()
    live = u >= 0
    dev = torch.device("cuda:0")
    u, i, j = (torch.from_numpy(a[live].astype(np.int64)).to(dev) for a in (u, i, j))
    g = torch.Generator(device=dev).manual_seed(1)
    P = torch.rand((nu, k), device=dev, generator=g) * 0.1
    Q = torch.rand((ni, k), device=dev, generator=g) * 0.1

    def step():
        pu, qi, qj = P.index_select(0, u), Q.index_select(0, i), Q.index_select(0, j)
        d = qi - qj
        w = torch.sigmoid(-(pu * d).sum(1)).unsqueeze(1)
        P.index_add_(0, u, lr * (w * d - lam * pu))
        Q.index_add_(0, i, lr * (w * pu - lam * qi))
        Q.index_add_(0, j, lr * (-w * pu - lam * qj))

    step()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / 4)
    return {"step": stats(t), "triples": int(live.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="NFLX")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="65536,262144,1048576")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--als-iterations", type=int, default=3)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpr_bench.json"))
    a = ap.parse_args()

    from mfhip import SEEN, synth
    from mfhip import _lib as L
    from mfhip.context import Context

    torch, why = load_torch()
    k = synth.CONFIGS[a.shape][3]
    data = synth.config(a.shape, a.scale)
    (tu, ti, tr), (su, si, _) = data.split()
    res = {"shape": a.shape, "scale": a.scale, "k": k, "train_pairs": int(len(tu)), "test_pairs": int(len(su)),
           "online_sampled_updates_per_s": ONLINE_SAMPLED_UPDATES_PER_S, "batches": {}}

    p0 = L.default_params()
    p0.num_factors = k
    p0.mode = L.MODE_FAST_F32
    lr, lam = 0.5, 0.01
    with Context(p0) as ctx:
        rng = np.random.default_rng(5)
        nu = ni = 0
        for side, col in ((L.SIDE_USER, data.u), (L.SIDE_ITEM, data.i)):
            ids = np.unique(col)
            ctx.set_factors(side, ids, rng.random((len(ids), k), dtype=np.float32) * np.float32(0.1))
            nu, ni = (len(ids), ni) if side == L.SIDE_USER else (nu, len(ids))
        t0 = time.perf_counter()
        ctx.seen_set(tu, ti)
        res["seen_set_ms"] = (time.perf_counter() - t0) * 1e3
        res["seen_pairs"] = ctx.seen_count()
        first = 0
        for batch in (int(x) for x in a.batches.split(",")):
            steps = max(4, (8 << 20) // batch)
            p = Context.bpr_params(lr, lam, batch=batch, scale=L.BPR_SCALE_MEAN, redraws=2, seed=17)
            st = ctx.bpr_run(p, first, steps)  # warm-up: the scratch is sized here
            first += steps
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.bpr_run(p, first, steps)
                t.append(time.perf_counter() - t0)
                first += steps
            row = {"steps_per_call": steps, "call": stats(t), "triples_per_s": steps * batch / float(np.median(t)),
                   "void_fraction": st["void_slots"] / st["slots"],
                   "user_rows_per_step": st["user_rows_written"] / steps,
                   "item_rows_per_step": st["item_rows_written"] / steps}
            ph = phase_sums(lambda: ctx.bpr_run(p, first, steps))
            first += steps
            row["phases_ms_per_step"] = {name: v / steps for name, v in ph.items() if name != "bpr_run:_scratch"}
            tt = torch_step_time(torch, why, ctx, k, nu, ni, a.reps, 0.05, lam)
            if "error" not in tt:
                tt["triples_per_s"] = tt["triples"] / (tt["step"]["median_ms"] * 1e-3)
            row["torch"] = tt
            res["batches"][str(batch)] = row
            print(f"batch {batch}: {row['triples_per_s']:.3e} triples/s"
                  + (f", torch {tt['triples_per_s']:.3e}" if "error" not in tt else f", torch: {tt['error']}"), flush=True)

    if not a.no_quality:
        batch = 1 << 20
        steps = a.epochs * max(1, len(tu) // batch)
        q = {"epochs": a.epochs, "batch": batch, "steps": steps, "lr": lr, "lambda": lam, "scale": "MEAN",
             "init_scale": 0.1, "top_n": 10}
        with Context(p0) as ctx:
            t0 = time.perf_counter()
            ctx.bpr_fit(tu, ti, Context.bpr_params(lr, lam, batch=batch, scale=L.BPR_SCALE_MEAN, redraws=2, seed=17),
                        steps, init_scale=0.1)
            q["bpr_fit_s"] = time.perf_counter() - t0
            m = ctx.rank_eval(su, si, 10, exclude=SEEN)
            q["bpr"] = {"ndcg": m.ndcg, "hit_rate": m.hit_rate, "mrr": m.mrr, "queries": int(m.queries)}
        with Context(p0) as ctx:
            t0 = time.perf_counter()
            ctx.als_fit_implicit(tu, ti, tr, a.als_iterations, 0.1, 1.0)
            q["als_fit_s"] = time.perf_counter() - t0
            q["als_iterations"] = a.als_iterations
            ctx.seen_from_als()
            m = ctx.rank_eval(su, si, 10, exclude=SEEN)
            q["als_implicit"] = {"ndcg": m.ndcg, "hit_rate": m.hit_rate, "mrr": m.mrr, "queries": int(m.queries)}
        res["quality"] = q
        print(json.dumps(q), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
