#!/usr/bin/env python3
"""mf_recommend_among: the top N within candidate lists, against what a caller could do without it.

Shape: NFLX (480,189 users x 17,770 items), k = 128, fast (f32) mode, top_n = 10, seeded random rows set with
mf_set_factors (no fit).  Legs:

  (a) shared   one allow-list of 1 %, 10 % and 50 % of the items for ALL users, against
               - mf_recommend of the same users over the whole catalogue (what the list should undercut), and
               - torch on the same GPU: gather the list's rows once, matmul per query batch, topk.
  (b) lists    per-query lists of 100 and 1,000 random candidates for 100,000 users, against
               - mf_predict of every (user, candidate) pair plus a numpy sort (argpartition + argsort), and
               - torch on the same GPU: gather each batch's candidate rows, bmm, topk.
               The achieved gather rate is entries x k x 4 B over the call's device time (upload of the lists,
               id lookup and the copy of the results included).
  (c) --ab PARENT_LIB   the existing calls only (mf_recommend for all users, mf_similar for all items,
               mf_recommend_vectors for all users), this build's library against another one's in alternating
               child processes; prints the parent's own run-to-run span beside the difference.

Timing as tools/similar_bench.py: one warm-up, then the median of --repeats with the contenders alternating in
one process; device events around each contender (the library calls block) and the host clock.

Writes profiles/among_bench.json (--ab: profiles/among_ab.json).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-recommendation_amd"))

USERS, ITEMS, K = 480189, 17770, 128


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return r, e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0


def contest(torch, calls, repeats):
    """calls: {label: fn}.  One warm-up each (results returned), then `repeats` rounds, every call once per round."""
    first = {name: fn() for name, fn in calls.items()}
    t = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            t[name].append(timed(torch, fn)[1])
    return first, {name: {"seconds_median": statistics.median(v), "seconds_all": v} for name, v in t.items()}


def model(users, items, k, batch):
    from mfhip import _lib as L
    from mfhip.context import Context
    rng = np.random.default_rng(17)
    P = rng.standard_normal((users, k), dtype=np.float32)
    Q = rng.standard_normal((items, k), dtype=np.float32)
    p = L.default_params()
    p.num_factors = k
    p.mode = L.MODE_FAST_F32
    os.environ["MFHIP_TEST"] = f"rec_batch={batch}"
    # ids are not rows: shuffled, about half of them negative, so that the id resolution a call does is part of
    # what the overlap figures check (row r of P / Q carries id uid[r] / iid[r])
    uid = ((rng.permutation(users) - users // 2) * 3 + 1).astype(np.int32)
    iid = ((rng.permutation(items) - items // 2) * 5 + 2).astype(np.int32)
    ctx = Context(p)
    ctx.set_factors(L.SIDE_USER, uid, P.astype(np.float64))
    ctx.set_factors(L.SIDE_ITEM, iid, Q.astype(np.float64))
    return ctx, P, Q, uid, iid, rng


def overlap(a, b, top_n, step):
    return float(np.mean([len(set(x) & set(y)) for x, y in zip(a[::step], b[::step])]) / top_n)


def run_new(a):
    import torch
    users, items = max(2, int(USERS * a.scale)), max(2, int(ITEMS * a.scale))
    ctx, P, Q, uid, iid, rng = model(users, items, a.k, a.batch)
    dev = torch.device("cuda")
    tP, tQ = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
    t_iid = torch.from_numpy(iid.astype(np.int64)).to(dev)
    top = a.top
    res = {"device": torch.cuda.get_device_name(0), "users": users, "items": items, "k": a.k, "top_n": top,
           "batch": a.batch, "repeats": a.repeats, "shared": {}, "lists": {}}

    # (a) one shared list for all users
    for pct in (1, 10, 50):
        n = max(top, items * pct // 100)
        allow_rows = np.sort(rng.choice(items, n, replace=False))
        allow = iid[allow_rows]  # the library gets ids, torch the rows
        t_allow = torch.from_numpy(allow_rows.astype(np.int64)).to(dev)

        def torch_shared():
            Qs = tQ[t_allow]
            out = [torch.topk(tP[b0:b0 + a.batch] @ Qs.T, top, dim=1)[1] for b0 in range(0, users, a.batch)]
            return t_iid[t_allow[torch.cat(out)]]

        first, t = contest(torch, {
            "among": lambda: ctx.recommend_among(uid, top, allow, scores=False),
            "recommend_full": lambda: ctx.recommend(uid, top, scores=False),
            "torch": torch_shared}, a.repeats)
        assert (first["among"][2] == top).all()
        row = dict(t, candidates=n,
                   overlap_with_torch=overlap(first["among"][0], first["torch"].cpu().numpy(), top, max(1, users // 500)))
        row["among_over_full"] = t["among"]["seconds_median"] / t["recommend_full"]["seconds_median"]
        row["among_over_torch"] = t["among"]["seconds_median"] / t["torch"]["seconds_median"]
        res["shared"][f"{pct}%"] = row
        print(f"(a) {pct}% = {n} items: among {t['among']['seconds_median'] * 1e3:.1f} ms, mf_recommend (all items) "
              f"{t['recommend_full']['seconds_median'] * 1e3:.1f} ms, torch {t['torch']['seconds_median'] * 1e3:.1f} ms, "
              f"overlap {row['overlap_with_torch']:.3f}", flush=True)

    # (b) per-query lists
    nq = min(users, max(2, int(100000 * a.scale)))
    q_rows = np.sort(rng.choice(users, nq, replace=False))
    q = uid[q_rows]
    t_q = torch.from_numpy(q_rows.astype(np.int64)).to(dev)
    for length in (100, 1000):
        length = min(length, items)
        # distinct inside a list (the baselines do not remove repeats): a random start and a random step coprime
        # to the item count walk the catalogue without meeting an item twice
        steps = np.array([s for s in range(1, min(items, 4096)) if np.gcd(s, items) == 1], np.int64)
        cand = ((rng.integers(0, items, (nq, 1)) + np.arange(length)[None, :] * rng.choice(steps, (nq, 1))) % items)
        cand_rows = np.ascontiguousarray(cand, np.int64)
        cand = iid[cand_rows]  # the ids of those rows, which is what the library calls get
        off = np.arange(nq + 1, dtype=np.int64) * length
        flat = np.ascontiguousarray(cand.reshape(-1))
        qrep = np.repeat(q, length)
        tb = max(1, (1 << 28) // (length * a.k))  # torch batch: 1 GiB of gathered rows

        def predict_sort():
            s = ctx.predict(qrep, flat)[0].reshape(nq, length)
            part = np.argpartition(-s, top - 1, axis=1)[:, :top]
            order = np.argsort(-np.take_along_axis(s, part, 1), axis=1)
            return np.take_along_axis(cand, np.take_along_axis(part, order, 1), 1)

        def torch_lists():
            out = []
            for b0 in range(0, nq, tb):
                c = torch.from_numpy(cand_rows[b0:b0 + tb]).to(dev)
                s = torch.bmm(tQ[c], tP[t_q[b0:b0 + tb]].unsqueeze(2)).squeeze(2)
                out.append(t_iid[torch.gather(c, 1, torch.topk(s, top, dim=1)[1])])
            return torch.cat(out)

        first, t = contest(torch, {
            "among": lambda: ctx.recommend_among(q, top, flat, offsets=off, scores=False),
            "predict_numpy_sort": predict_sort,
            "torch": torch_lists}, a.repeats)
        step = max(1, nq // 500)
        row = dict(t, queries=nq, list_length=length, entries=int(nq) * length,
                   overlap_with_torch=overlap(first["among"][0], first["torch"].cpu().numpy(), top, step),
                   overlap_with_predict=overlap(first["among"][0], first["predict_numpy_sort"], top, step))
        row["gather_bytes_per_s"] = row["entries"] * a.k * 4 / t["among"]["seconds_median"]
        row["among_over_predict"] = t["among"]["seconds_median"] / t["predict_numpy_sort"]["seconds_median"]
        row["among_over_torch"] = t["among"]["seconds_median"] / t["torch"]["seconds_median"]
        res["lists"][str(length)] = row
        print(f"(b) {nq} users x {length}: among {t['among']['seconds_median'] * 1e3:.1f} ms "
              f"({row['gather_bytes_per_s'] / 1e9:.0f} GB/s of rows), mf_predict + numpy sort "
              f"{t['predict_numpy_sort']['seconds_median'] * 1e3:.1f} ms, torch {t['torch']['seconds_median'] * 1e3:.1f} ms, "
              f"overlap {row['overlap_with_torch']:.3f} / {row['overlap_with_predict']:.3f}", flush=True)
    ctx.close()
    return res


def run_existing(a):
    """(the child of --ab) the existing calls, one JSON line on stdout"""
    import torch
    from mfhip import _lib as L
    users, items = max(2, int(USERS * a.scale)), max(2, int(ITEMS * a.scale))
    ctx, P, Q, uid, iid, _ = model(users, items, a.k, a.batch)
    P64 = P.astype(np.float64)
    _, t = contest(torch, {
        "mf_recommend": lambda: ctx.recommend(uid, a.top, scores=False),
        "mf_similar": lambda: ctx.similar(iid, a.top, side=L.SIDE_ITEM, scores=False),
        "mf_recommend_vectors": lambda: ctx.recommend_vectors(P64, a.top, side=L.SIDE_ITEM, scores=False)}, a.repeats)
    ctx.close()
    print(json.dumps({name: {"median_ms": v["seconds_median"] * 1e3} for name, v in t.items()}))


def run_ab(a):
    libs = [("this", os.path.join(ROOT, "large-scale-recommendation_amd", "lib", "libmfhip.so")), ("parent", a.ab)]
    runs = {which: [] for which, _ in libs}
    for rnd in range(a.rounds):
        for which, lib in (libs if rnd % 2 == 0 else libs[::-1]):  # balanced order
            cmd = [sys.executable, os.path.abspath(__file__), "--existing", "--scale", str(a.scale), "--k", str(a.k),
                   "--top", str(a.top), "--batch", str(a.batch), "--repeats", str(a.repeats)]
            out = subprocess.run(cmd, env=dict(os.environ, MFHIP_LIB=lib), check=True, capture_output=True, text=True,
                                 timeout=600).stdout
            runs[which].append(json.loads(out.strip().splitlines()[-1]))
            print(f"round {rnd} {which}: " + ", ".join(f"{c} {v['median_ms']:.1f}" for c, v in runs[which][-1].items()),
                  flush=True)
    table = {}
    for call in runs["this"][0]:
        row = {}
        for which, _ in libs:
            med = [r[call]["median_ms"] for r in runs[which]]
            row[which] = {"median_ms": float(np.median(med)), "min_ms": min(med), "max_ms": max(med), "runs_ms": med}
        row["delta_ms"] = row["this"]["median_ms"] - row["parent"]["median_ms"]
        row["parent_span_ms"] = row["parent"]["max_ms"] - row["parent"]["min_ms"]
        row["within_parent_span"] = bool(abs(row["delta_ms"]) <= row["parent_span_ms"])
        table[call] = row
        print(f"{call}: this {row['this']['median_ms']:.1f} ms, parent {row['parent']['median_ms']:.1f} ms, "
              f"delta {row['delta_ms']:+.2f} ms, parent span {row['parent_span_ms']:.2f} ms", flush=True)
    return {"scale": a.scale, "k": a.k, "rounds": a.rounds, "repeats_per_process": a.repeats, "calls": table}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=K)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink users and items (rehearsal only)")
    ap.add_argument("--ab", metavar="PARENT_LIB", help="compare the existing calls against another libmfhip.so")
    ap.add_argument("--rounds", type=int, default=4, help="--ab: child processes per build")
    ap.add_argument("--existing", action="store_true", help="(the child of --ab) one JSON line on stdout")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("among_bench needs a GPU: there is no CPU path to time")
    if a.existing:
        run_existing(a)
        return
    res = run_ab(a) if a.ab else run_new(a)
    out = a.out or os.path.join(ROOT, "profiles", "among_ab.json" if a.ab else "among_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
