#!/usr/bin/env python3
"""Filtered search on the headline corpus of bench.py (synthetic 1 M passages, B = 32, k = 1000, two-pass mode): step
time by HIP events and the per-kernel breakdown (clb_profile_read) of the unfiltered search and of filtered search at
selectivity 1.0 / 0.5 / 0.1 / 0.01 in both scopes, a re-rank of 1 000 pids per query, the candidate counts of every case
and the time of clb_filter_create_pids -- one JSON file (default profiles/filtered_search.json).

  --old-lib PATH   another build of the library (the parent commit's: `make SUF=_old` in its csrc/) is loaded into the
                   same process on its own handle; the unfiltered search is timed on both, rounds alternating old / new.

A measurement path only: it needs a GPU and fails without one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per case (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--all-max", type=float, default=1.0, help="largest selectivity run in scope 'all'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_search.json"))
    args = ap.parse_args()
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import _lib, synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_filtered_search: no GPU")

    T, B, k = 32, args.batch, args.k
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    n_docs = int(idx["doclens"].size)
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=768, T=T)
    Qdev = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).cuda()
    n_q = Qdev.shape[0] // B

    new_lib = clb.lib()
    libs = {"new": new_lib}
    if args.old_lib:
        old = C.CDLL(os.path.abspath(args.old_lib))  # a build from before the filter entry points: only what this tool calls
        old.clb_last_error.restype = C.c_char_p
        old.clb_searcher_device_bytes.restype = C.c_int64
        libs["old"] = old

    class On:
        """every library call of the block goes to that build"""
        def __init__(self, name): self.name = name
        def __enter__(self): _lib._lib = libs[self.name]
        def __exit__(self, *exc): _lib._lib = new_lib

    handles = {}
    for name in libs:
        with On(name):
            s = clb.Searcher(index=idx, device=0)
            s.set_mode(1)
            handles[name] = (s, DeviceSearch(s, T, B, k, 2))

    def window(run, filters, scope, steps):
        """ms per batch over `steps` batches between two HIP events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            run(Qdev[(i % n_q) * B:(i % n_q + 1) * B], filters, scope)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def kernels(s, run, filters, scope, steps):
        s.profile_enable(True)
        for i in range(steps):
            run(Qdev[(i % n_q) * B:(i % n_q + 1) * B], filters, scope)
        torch.cuda.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
        return {kn: round(v["ms"] / max(v["launches"], 1), 5) for kn, v in prof.items() if v["launches"]}

    def case(name, filters, scope, steps, rounds, lib_name="new"):
        s, run = handles[lib_name]
        with On(lib_name):
            for i in range(args.warmup):
                run(Qdev[i * B:(i + 1) * B], filters, scope)
            torch.cuda.synchronize()
            nc = run.ncand.cpu().numpy()
            ms = [window(run, filters, scope, steps) for _ in range(rounds)]
            rec = {"case": name, "lib": lib_name, "scope": scope if filters is not None else None, "step_ms": round(float(np.median(ms)), 5),
                   "step_ms_rounds": [round(x, 5) for x in ms], "steps_per_round": steps,
                   "candidates_per_query": {"mean": float(nc.mean()), "min": int(nc.min()), "max": int(nc.max())},
                   "kernels_ms": kernels(s, run, filters, scope, max(steps // 2, 3))}
        rec["kernels_sum_ms"] = round(sum(rec["kernels_ms"].values()), 5)
        print(json.dumps(rec), flush=True)
        return rec

    out = {"tool": "tools/bench_filtered_search.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k,
           "T": T, "nprobe": 2, "mode": "two-pass", "cases": [], "unfiltered_old_vs_new": None, "filter_create_pids_ms": {}}

    # ---- unfiltered: old and new build alternating (same process, same index, same queries)
    if "old" in libs:
        ab = {"old": [], "new": []}
        for name in ("old", "new"):                  # warm both
            with On(name):
                for i in range(args.warmup):
                    handles[name][1](Qdev[i * B:(i + 1) * B])
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name in ("old", "new") if r % 2 == 0 else ("new", "old"):
                with On(name):
                    ab[name].append(window(handles[name][1], None, "candidates", args.steps))
        kern = {}
        for name in ("old", "new"):
            with On(name):
                kern[name] = kernels(handles[name][0], handles[name][1], None, "candidates", args.steps)
        mo, mn = float(np.median(ab["old"])), float(np.median(ab["new"]))
        out["unfiltered_old_vs_new"] = {"old_step_ms": round(mo, 5), "new_step_ms": round(mn, 5), "new_over_old": round(mn / mo, 4),
                                        "old_rounds": [round(x, 5) for x in ab["old"]], "new_rounds": [round(x, 5) for x in ab["new"]],
                                        "kernels_ms": kern}
        print(json.dumps(out["unfiltered_old_vs_new"]), flush=True)
    out["cases"].append(case("unfiltered", None, "candidates", args.steps, args.rounds))

    # ---- filter creation (clb_filter_create_pids: upload, marking kernel, count, one read-back)
    s, run = handles["new"]
    rng = np.random.default_rng(5)
    for n in (1_000, 100_000, 1_000_000):
        pids = rng.integers(1, n_docs + 1, size=n).astype(np.int64)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = s.make_filter(pids=pids)
            ts.append((time.perf_counter() - t0) * 1e3)
            f.close()
        out["filter_create_pids_ms"][str(n)] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4)}
    print(json.dumps(out["filter_create_pids_ms"]), flush=True)

    # ---- filtered, one filter for the whole batch (a tenant); scope "candidates" first: it never grows the workspace
    sels = (1.0, 0.5, 0.1, 0.01)
    masks = {sel: (np.ones(n_docs, bool) if sel == 1.0 else np.random.default_rng(int(sel * 1000)).random(n_docs) < sel) for sel in sels}
    filters = {sel: s.make_filter(mask=masks[sel]) for sel in sels}
    for sel in sels:
        rec = case(f"candidates sel={sel}", filters[sel], "candidates", args.steps, args.rounds)
        rec["selectivity"], rec["filter_count"] = sel, filters[sel].count
        out["cases"].append(rec)
    # a re-rank: 1 000 pids of the caller's per query
    rerank = [s.make_filter(pids=np.random.default_rng(100 + j).integers(1, n_docs + 1, size=1000)) for j in range(B)]
    rec = case("all rerank 1000 pids per query", rerank, "all", args.steps, args.rounds)
    rec["filter_count"] = int(np.mean([f.count for f in rerank]))
    out["cases"].append(rec)
    for sel in reversed(sels):                       # growing sets: the workspace grows with them
        if sel > args.all_max:
            continue
        steps = max(3, int(args.steps * min(1.0, 0.01 / sel)))
        rec = case(f"all sel={sel}", filters[sel], "all", steps, min(args.rounds, 3))
        rec["selectivity"], rec["filter_count"] = sel, filters[sel].count
        out["cases"].append(rec)
    # the handle afterwards: the unfiltered search on the grown workspace
    out["cases"].append(case("unfiltered after the filtered cases", None, "candidates", args.steps, args.rounds))
    out["device_bytes_after"] = s.device_bytes

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
