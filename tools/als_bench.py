#!/usr/bin/env python3
"""ALS iterations on the NFLX-shaped synthetic (480,189 x 17,770, the training split, k = --k, 128 by
default), fast mode.

mf_als_prepare once (its host time is reported), one warm-up iteration, then --iters full iterations
(item half-sweep + user half-sweep) timed twice over: with the host clock around the blocking
mf_als_run call, and with the library's device events around every half-sweep's launches
(mf_set_profiling).  The Gram accumulation and the solve of a row run in one kernel, so they are not
timed apart; the item and user half-sweeps are.

FLOP convention, per half-sweep: 2 * nnz * k^2 for the normal matrices (the full k x k product per
rating; the kernel computes the lower-triangle 32 x 32 blocks only, 10 of 16 at k = 128) plus
(2/3) * k^3 * rows for the factorisations, rows = the rated rows of the side solved.  TFLOP/s is that
count over the device-event time.

--chunks N[,N...] repeats the measurement with MFHIP_TEST als_chunk=N (ratings per work item of a
long row).  --dsgd also times one fast DSGD epoch (numBlocks 8) on the same data in the same
process, the baseline the README records beside the ALS iteration.  --implicit also times implicit
iterations (mf_als_run_implicit, alpha --alpha) after the explicit ones, on the same data in the same
process with the ratings shifted by -3 so that they straddle zero (all three rating signs occur).  The
two Gram launches of a half-sweep are inside its time; they are also timed alone, through
mf_debug_als_gram under the same device events.

--k K runs at another rank (129..256 take the kernels of kernels_als_wide.hip); --det also times one
deterministic-mode (f64) iteration after one warm-up.

--solver cg --cg-steps S instead compares the conjugate-gradient half-sweeps (mf_als_run_cg, S steps per
row) with mf_als_run in one process: two contexts on the same data, one warm-up iteration each, then
--iters rounds in which the solvers alternate, every half-sweep under the device events (medians are
reported); both then run on to 10 iterations and report the training RMSE (first 2M ratings).  With
--implicit the same for the implicit calls on the shifted ratings, with --det also in deterministic mode.
The result goes under the key "cg" (of "k<K>" at another rank), beside what the file holds.

--solver nnls compares the non-negative half-sweeps (mf_als_run_nonneg / mf_als_run_implicit_nonneg) with
mf_als_run / mf_als_run_implicit in the same way (--implicit and --det as above; --total-iters is the
iteration count both run on to).  Beside the times it prints the mf_als_nonneg_stats struct (mean and
longest solve in iterations per row, rows at the cap, reason-2 and NaN rows), the share of zero entries in
the fitted factors and both training RMSEs.  The result goes under the key "nnls".

Writes profiles/als_bench.json.  At the default rank this run's fields replace the file's own and every
other key of the file stays; at another rank the same fields go under the key "k<K>", beside what it
holds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-recommendation_amd"))

F32_MFMA_PEAK = 157.3e12  # MI355X, v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate)


def als_run(train, k, iters, lam, chunk, alpha=None, det=False):
    """alpha None: explicit iterations; else implicit ones on the ratings as given.  det: deterministic mode."""
    from mfhip import _lib as L
    from mfhip.context import Context

    u, i, r = train
    if chunk:
        os.environ["MFHIP_TEST"] = f"als_chunk={chunk}"
    else:
        os.environ.pop("MFHIP_TEST", None)
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_DETERMINISTIC_F64 if det else L.MODE_FAST_F32
    nnz = len(u)
    rows = {"item": len(np.unique(i)), "user": len(np.unique(u))}
    flop = {s: 2.0 * nnz * k * k + (2.0 / 3.0) * k ** 3 * rows[s] for s in rows}
    res = {"chunk": chunk or "default", "nnz": nnz, "rows": rows, "k": k, "iters": iters, "lambda": lam,
           "flop_per_half_sweep": flop}
    if alpha is not None:
        res["alpha"] = alpha
        res["rating_signs"] = {"negative": int((r < 0).sum()), "zero": int((r == 0).sum()),
                               "positive": int((r > 0).sum())}
    with Context(p) as ctx:
        t0 = time.perf_counter()
        ctx.als_prepare(u, i, r)
        res["prepare_host_s"] = time.perf_counter() - t0
        def run(n):
            if alpha is None:
                ctx.als_run(n, lam)
            else:
                ctx.als_run_implicit(n, lam, alpha)

        run(2)  # warm-up
        ctx.set_profiling(True)
        half = {"item": [], "user": []}
        wall = []
        for _ in range(iters):
            t0 = time.perf_counter()
            for side in ("item", "user"):
                ctx.reset_stats()
                run(1)
                half[side].append(ctx.stats()["kernel_ms"])
            wall.append(time.perf_counter() - t0)
        if alpha is not None:
            # the Gram launches alone: the item half-sweep takes G of the user rows, the user one of the items
            gram = {"item": [], "user": []}
            for _ in range(iters):
                for side, of in (("item", L.SIDE_USER), ("user", L.SIDE_ITEM)):
                    ctx.reset_stats()
                    ctx.als_gram(of)
                    gram[side].append(ctx.stats()["kernel_ms"])
            res["gram_ms"] = {s: {"median": float(np.median(gram[s])), "all": gram[s]} for s in gram}
            res["gram_flop"] = {"item": 2.0 * rows["user"] * k * k, "user": 2.0 * rows["item"] * k * k}
        ctx.set_profiling(False)
        rmse, _ = ctx.rmse(u[:2_000_000], i[:2_000_000], r[:2_000_000])
    res["train_rmse_sample"] = rmse
    ms = {s: float(np.median(half[s])) for s in half}
    res["half_sweep_ms"] = {s: {"median": ms[s], "all": half[s]} for s in half}
    res["iteration_ms_device"] = ms["item"] + ms["user"]
    res["iteration_ms_host_call"] = float(np.median(wall)) * 1e3
    res["tflops"] = {s: flop[s] / (ms[s] * 1e-3) / 1e12 for s in half}
    res["tflops"]["iteration"] = (flop["item"] + flop["user"]) / (res["iteration_ms_device"] * 1e-3) / 1e12
    res["fraction_of_f32_mfma_peak"] = res["tflops"]["iteration"] * 1e12 / F32_MFMA_PEAK
    kind = "ALS" if alpha is None else f"implicit ALS (alpha {alpha})"
    kind += (f" k {k}" if k != 128 else "") + (" deterministic" if det else "")
    print(f"{kind} chunk {res['chunk']}: {res['iteration_ms_device']:.1f} ms / iteration on the device "
          f"(item half {ms['item']:.1f} ms, {res['tflops']['item']:.1f} TFLOP/s; user half {ms['user']:.1f} ms, "
          f"{res['tflops']['user']:.1f} TFLOP/s), host call {res['iteration_ms_host_call']:.1f} ms; "
          f"{res['tflops']['iteration']:.1f} TFLOP/s by 2*nnz*k^2 + (2/3)*k^3*rows per half-sweep = "
          f"{100 * res['fraction_of_f32_mfma_peak']:.1f} % of the f32 MFMA peak; prepare {res['prepare_host_s']:.1f} s; "
          f"rmse {rmse:.4f}", flush=True)
    if alpha is not None:
        g = res["gram_ms"]
        print(f"  of which the Gram launches: item half {g['item']['median']:.3f} ms ({rows['user']} rows), "
              f"user half {g['user']['median']:.3f} ms ({rows['item']} rows)", flush=True)
    return res


def cg_compare(train, k, rounds, lam, steps, alpha=None, det=False, total_iters=10, solver="cg"):
    """mf_als_run against mf_als_run_cg(steps) -- solver "nnls": against mf_als_run_nonneg --, alternating in
    one process; alpha None: explicit."""
    from mfhip import _lib as L
    from mfhip.context import Context

    u, i, r = train
    os.environ.pop("MFHIP_TEST", None)
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_DETERMINISTIC_F64 if det else L.MODE_FAST_F32
    nnls = solver == "nnls"
    res = {"k": k, "lambda": lam, "rounds": rounds, "deterministic": det, "nnz": len(u)}
    if not nnls:
        res["cg_steps"] = steps
    if alpha is not None:
        res["alpha"] = alpha
    with Context(p) as chol, Context(p) as cg:
        if not nnls:
            cap = cg.als_cg_capacity()
            res["staged_capacity"] = cap
            res["staged_share_of_rows"] = {
                side: float((c[c > 0] <= cap).mean())
                for side, c in (("item", np.bincount(i)), ("user", np.bincount(u)))}
        for ctx in (chol, cg):
            ctx.als_prepare(u, i, r)

        def run(ctx, n):
            if ctx is chol:
                ctx.als_run(n, lam) if alpha is None else ctx.als_run_implicit(n, lam, alpha)
            elif nnls:
                ctx.als_run_nonneg(n, lam) if alpha is None else ctx.als_run_implicit_nonneg(n, lam, alpha)
            else:
                ctx.als_run_cg(n, lam, cg_steps=steps) if alpha is None else \
                    ctx.als_run_implicit_cg(n, lam, alpha, cg_steps=steps)

        names = {id(chol): "cholesky", id(cg): solver}
        half = {n: {"item": [], "user": []} for n in names.values()}
        for ctx in (chol, cg):
            run(ctx, 2)  # warm-up
            ctx.set_profiling(True)
        for _ in range(rounds):
            for ctx in (chol, cg):
                for side in ("item", "user"):
                    ctx.reset_stats()
                    run(ctx, 1)
                    half[names[id(ctx)]][side].append(ctx.stats()["kernel_ms"])
        for ctx in (chol, cg):
            ctx.set_profiling(False)
            run(ctx, 2 * max(0, total_iters - 1 - rounds))
            res.setdefault("train_rmse_sample_after_%d" % max(total_iters, 1 + rounds), {})[names[id(ctx)]] = \
                ctx.rmse(u[:2_000_000], i[:2_000_000], r[:2_000_000])[0]
        if nnls:
            st = cg.als_nonneg_stats()
            res["nonneg_stats"] = st
            res["mean_iterations_per_row"] = st["iterations"] / max(st["rows"], 1)
            res["zero_share"] = {side: float((cg.factors(sd)[1] == 0).mean())
                                 for side, sd in (("user", L.SIDE_USER), ("item", L.SIDE_ITEM))}
    res["half_sweep_ms"] = {n: {s: {"median": float(np.median(v)), "all": v} for s, v in half[n].items()} for n in half}
    it = {n: sum(res["half_sweep_ms"][n][s]["median"] for s in ("item", "user")) for n in half}
    res["iteration_ms_device"] = it
    res["cg_speedup" if not nnls else "nnls_speedup"] = it["cholesky"] / it[solver]
    kind = ("explicit" if alpha is None else f"implicit (alpha {alpha})") + (" deterministic" if det else " fast")
    h = res["half_sweep_ms"]
    if nnls:
        st = res["nonneg_stats"]
        print(f"k {k} {kind}: Cholesky {it['cholesky']:.1f} ms / iteration (item {h['cholesky']['item']['median']:.1f}, "
              f"user {h['cholesky']['user']['median']:.1f}), NNLS {it['nnls']:.1f} ms (item "
              f"{h['nnls']['item']['median']:.1f}, user {h['nnls']['user']['median']:.1f}): x{res['nnls_speedup']:.3f}; "
              f"stats {st}; mean {res['mean_iterations_per_row']:.1f} iterations per row; zero share "
              f"{res['zero_share']}; rmse {[v for k_, v in res.items() if k_.startswith('train_rmse')][0]}", flush=True)
        return res
    print(f"k {k} {kind}: Cholesky {it['cholesky']:.1f} ms / iteration (item {h['cholesky']['item']['median']:.1f}, user "
          f"{h['cholesky']['user']['median']:.1f}), CG S={steps} {it['cg']:.1f} ms (item {h['cg']['item']['median']:.1f}, "
          f"user {h['cg']['user']['median']:.1f}): x{res['cg_speedup']:.2f}; staged rows {res['staged_share_of_rows']}; "
          f"rmse {[v for k_, v in res.items() if k_.startswith('train_rmse')][0]}", flush=True)
    return res


def dsgd_epoch(train, k, nb):
    from mfhip import _lib as L
    from mfhip.context import Context

    os.environ.pop("MFHIP_TEST", None)
    p = L.default_params()
    p.num_factors = k
    p.num_blocks = nb
    p.mode = L.MODE_FAST_F32
    with Context(p) as ctx:
        ctx.prepare(*train)
        ctx.run(nb)
        ctx.sync()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.run(nb)
            ctx.sync()
            t.append(time.perf_counter() - t0)
    ms = float(np.median(t)) * 1e3
    print(f"fast DSGD epoch (numBlocks {nb}) on the same data: {ms:.1f} ms", flush=True)
    return {"epoch_ms": ms, "all_s": t, "n_blocks": nb}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--chunks", default="", help="comma-separated als_chunk values (empty: the default only)")
    ap.add_argument("--dsgd", action="store_true", help="also time a fast DSGD epoch on the same data")
    ap.add_argument("--implicit", action="store_true", help="also time implicit iterations on the shifted ratings")
    ap.add_argument("--alpha", type=float, default=1.0, help="the implicit runs' alpha")
    ap.add_argument("--k", type=int, default=128, help="the rank (default 128)")
    ap.add_argument("--det", action="store_true", help="also time one deterministic-mode iteration")
    ap.add_argument("--solver", choices=("cholesky", "cg", "nnls"), default="cholesky",
                    help="cg / nnls: compare mf_als_run_cg / mf_als_run_nonneg with mf_als_run instead of the "
                         "timings above")
    ap.add_argument("--total-iters", type=int, default=10,
                    help="iterations both solvers of a comparison run on to before the RMSE is taken")
    ap.add_argument("--cg-steps", type=int, default=3, help="CG steps per row (with --solver cg)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic (rehearsal only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_bench.json"))
    a = ap.parse_args()
    from mfhip import _lib as L
    from mfhip import synth
    try:
        if L.device_count() < 1:
            raise L.MFNoDeviceError(L.MF_ERR_NO_DEVICE, "no device")
    except L.MFNoDeviceError:
        sys.exit("als_bench needs a GPU: there is no CPU path to time")
    nu, ni, nr, k0, nb = synth.CONFIGS["NFLX"]
    k = a.k
    train, _ = synth.generate(max(1, int(nu * a.scale)), max(1, int(ni * a.scale)), max(1, int(nr * a.scale))).split()
    if a.solver != "cholesky":
        kw = {"total_iters": a.total_iters, "solver": a.solver}
        out = {"scale": a.scale, "runs": [cg_compare(train, k, a.iters, a.lam, a.cg_steps, **kw)]}
        if a.implicit:
            u, i, r = train
            shifted = (u, i, np.asarray(r, np.float64) - 3.0)
            out["runs"].append(cg_compare(shifted, k, a.iters, a.lam, a.cg_steps, a.alpha, **kw))
        if a.det:
            out["runs"].append(cg_compare(train, k, a.iters, a.lam, a.cg_steps, det=True, **kw))
            if a.implicit and a.solver == "nnls":
                out["runs"].append(cg_compare(shifted, k, a.iters, a.lam, a.cg_steps, a.alpha, det=True, **kw))
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        (old if k == k0 else old.setdefault(f"k{k}", {}))[a.solver] = out
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)
        print("wrote", a.out)
        return
    out = {"shape": "NFLX", "scale": a.scale, "runs": []}
    for c in [int(x) for x in a.chunks.split(",") if x] or [0]:
        out["runs"].append(als_run(train, k, a.iters, a.lam, c))
    if a.implicit:
        u, i, r = train
        shifted = (u, i, np.asarray(r, np.float64) - 3.0)
        out["implicit_runs"] = [als_run(shifted, k, a.iters, a.lam, c, a.alpha)
                                for c in [int(x) for x in a.chunks.split(",") if x] or [0]]
    if a.det:
        out["deterministic_run"] = als_run(train, k, 1, a.lam, 0, det=True)
    if a.dsgd:
        out["dsgd_fast"] = dsgd_epoch(train, k, nb)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    old = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
    if k != k0:  # beside what the file holds
        old[f"k{k}"] = out
        out = old
    else:        # the file is this run; whatever else it holds (other ranks, comparisons) stays
        out.update({key: v for key, v in old.items() if key not in out})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
