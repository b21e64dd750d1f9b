#!/usr/bin/env python3
"""Nearest neighbours in factor space: mf_similar and mf_recommend_vectors against torch on the same GPU.

Shape: NFLX (480,189 users x 17,770 items), k = 128 and, for the cosine overhead at a small rank, k = 16.
Factors are seeded random rows set with mf_set_factors (no fit), fast (f32) mode, top_n = 10, batches of
4,096 queries (tools/recommend_bench.py's setting).  Rows:

  items      mf_similar for all items against all items, cosine and dot
  users      mf_similar for a fixed sample of --user-sample users against all users, cosine and dot
  vectors    mf_recommend_vectors for every user's vector against all items, dot and cosine, beside
             mf_recommend for the same users in the same process

The baseline is what a caller could do without these calls: the same f32 matrices on the same GPU in the
same process -- normalise the rows (cosine), torch.matmul of a query batch against all candidates, mask the
diagonal (the query itself), torch.topk.  The user row's torch batch is 1,024 (a 4,096 x 480,189 f32 score
matrix is 7.9 GB).

Timing as tools/recommend_bench.py: one warm-up, then the median of --repeats with the two paths
alternating; device events around each path (the library calls block, so theirs include id lookup,
launches and the copy of the lists to the host) and the host clock around the library call.

Writes profiles/similar_bench.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-recommendation_amd"))

USERS, ITEMS = 480189, 17770


def run_rank(k, users, items, top_n, batch, repeats, user_sample, rows):
    import torch
    from mfhip import _lib as L
    from mfhip.context import Context

    rng = np.random.default_rng(17)
    P = rng.standard_normal((users, k), dtype=np.float32)
    Q = rng.standard_normal((items, k), dtype=np.float32)
    uid = np.arange(users, dtype=np.int32)
    iid = np.arange(items, dtype=np.int32)
    sample = np.sort(rng.choice(users, min(user_sample, users), replace=False)).astype(np.int32)
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_FAST_F32
    os.environ["MFHIP_TEST"] = f"rec_batch={batch}"
    res = {"users": users, "items": items, "k": k, "top_n": top_n, "batch": batch, "repeats": repeats,
           "user_sample": len(sample), "rows": {}}
    dev = torch.device("cuda")
    P64 = P.astype(np.float64)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0

    def torch_top(X, qidx, cosine, tbatch, mask_self):
        """normalise, matmul, mask the diagonal, topk; X: the candidate rows, qidx: the query rows (tensor)"""
        if cosine:
            X = X / X.norm(dim=1, keepdim=True)
        out = []
        for b0 in range(0, len(qidx), tbatch):
            qi = qidx[b0:b0 + tbatch]
            S = X[qi] @ X.T
            if mask_self:
                S[torch.arange(len(qi), device=dev), qi] = float("-inf")
            out.append(torch.topk(S, top_n, dim=1)[1])
        return torch.cat(out)

    def torch_vectors(V, X, cosine):
        if cosine:
            V = V / V.norm(dim=1, keepdim=True)
            X = X / X.norm(dim=1, keepdim=True)
        out = []
        for b0 in range(0, V.shape[0], batch):
            out.append(torch.topk(V[b0:b0 + batch] @ X.T, top_n, dim=1)[1])
        return torch.cat(out)

    def measure(name, fused, torch_fn, nq, nc):
        ids, _, cnt = fused()  # warm-up; the two paths must pick the same rows (f32 sums in another
        tidx = torch_fn().cpu().numpy()  # order: a near-tie may swap neighbours, so compare as sets)
        assert (cnt == min(top_n, nc)).all(), name
        step = max(1, nq // 500)
        same = np.mean([len(set(a) & set(b)) for a, b in zip(ids[::step], tidx[::step])]) / top_n
        t_f, t_w, t_t = [], [], []
        for _ in range(repeats):
            _, ev, wall = timed(fused)
            t_f.append(ev)
            t_w.append(wall)
            _, ev, _ = timed(torch_fn)
            t_t.append(ev)
        flop = 2.0 * nq * nc * k
        row = {"queries": nq, "candidates": nc, "flop": flop, "overlap_with_torch": float(same)}
        for key, t in (("fused", t_f), ("fused_host_call", t_w), ("torch", t_t)):
            m = statistics.median(t)
            row[key] = {"seconds_median": m, "seconds_all": t, "queries_per_s": nq / m, "f32_flops": flop / m}
        row["fused_over_torch"] = row["torch"]["seconds_median"] / row["fused"]["seconds_median"]
        res["rows"][name] = row
        print(f"k={k} {name}: fused {row['fused']['seconds_median'] * 1e3:.2f} ms "
              f"(host call {row['fused_host_call']['seconds_median'] * 1e3:.2f} ms, "
              f"{row['fused']['f32_flops'] / 1e12:.1f} TF), torch {row['torch']['seconds_median'] * 1e3:.2f} ms, "
              f"overlap {same:.3f}", flush=True)

    with Context(p) as ctx:
        ctx.set_factors(L.SIDE_USER, uid, P64)
        ctx.set_factors(L.SIDE_ITEM, iid, Q.astype(np.float64))
        tP, tQ = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
        t_items = torch.arange(items, device=dev)
        t_sample = torch.from_numpy(sample.astype(np.int64)).to(dev)
        for metric, tag in ((L.METRIC_COSINE, "cosine"), (L.METRIC_DOT, "dot")):
            cos = metric == L.METRIC_COSINE
            if "items" in rows:
                measure(f"items_{tag}", lambda: ctx.similar(iid, top_n, side=L.SIDE_ITEM, metric=metric, scores=False),
                        lambda: torch_top(tQ, t_items, cos, batch, True), items, items)
            if "users" in rows:
                measure(f"users_{tag}", lambda: ctx.similar(sample, top_n, side=L.SIDE_USER, metric=metric, scores=False),
                        lambda: torch_top(tP, t_sample, cos, 1024, True), len(sample), users)
            if "vectors" in rows:
                measure(f"vectors_{tag}",
                        lambda: ctx.recommend_vectors(P64, top_n, side=L.SIDE_ITEM, metric=metric, scores=False),
                        lambda: torch_vectors(tP, tQ, cos), users, items)
        if "vectors" in rows:
            measure("recommend", lambda: ctx.recommend(uid, top_n, scores=False), lambda: torch_vectors(tP, tQ, False),
                    users, items)
    over = {}
    for what in ("items", "users", "vectors"):
        a, b = res["rows"].get(f"{what}_cosine"), res["rows"].get(f"{what}_dot")
        if a and b:
            over[what] = a["fused"]["seconds_median"] / b["fused"]["seconds_median"]
    res["cosine_over_dot"] = over
    print(f"k={k} cosine over dot: " + ", ".join(f"{w} {v:.3f}" for w, v in over.items()), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ranks", default="128,16")
    ap.add_argument("--rows", default="items,users,vectors")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--user-sample", type=int, default=8192)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink users and items (rehearsal only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("similar_bench needs a GPU: there is no CPU path to time")
    out = {"device": torch.cuda.get_device_name(0), "ranks": {}}
    for k in (int(x) for x in a.ranks.split(",")):
        out["ranks"][str(k)] = run_rank(k, max(2, int(USERS * a.scale)), max(2, int(ITEMS * a.scale)), a.top, a.batch,
                                        a.repeats, a.user_sample, a.rows.split(","))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
