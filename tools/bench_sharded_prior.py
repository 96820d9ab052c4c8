#!/usr/bin/env python3
"""Sharded search with a score prior against sharded search without one on the headline corpus of bench.py (synthetic 1 M
passages, B = 32, k = 1000, two-pass shards), the corpus cut into 2 and into 4 shards that all live on one GPU
(`ShardedSearcher.from_index`), protocol "two_phase".  Two measurements:

  * default -- on ONE build, in one process: a step with an N(0, 0.5) prior (weight 1) against a step without one.
    ms per step -- one `ShardedSearcher.search_batch` of B queries, host arrays in and out, so the exchanges, the merge and
    the copies are inside -- over `--steps` steps per window: `--rounds` windows per side (default 3), interleaved
    plain / prior / prior / plain ..., the median, the spread and every sample kept; and the length of the re-score list per
    query, summed over the shards (clb_last_batch_stats of every shard), on both sides.
  * `--against LIB` -- the step WITHOUT a prior of this tree's library against another build of the library (the parent
    commit's): fresh child processes, one library each through COLBERT_HIP_LIB, in the order this, this, LIB, this, LIB -- the
    first two give the spread two processes of ONE library differ by, the rest alternate.  Every child runs `--child`: the
    plain side of the default measurement alone.

Writes one JSON file (default profiles/sharded_prior.json, with --against profiles/sharded_prior_parent.json);
profiles/sharded_prior.md is written from them by hand.  A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args, with_prior: bool):
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_sharded_prior: no GPU")
    T, B, k, nprobe = 32, args.batch, args.k, 2
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    n_docs = int(idx["doclens"].size)
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=768, T=T)
    n_q = Q.shape[2] // B
    values = np.random.default_rng(99).normal(0.0, 0.5, n_docs).astype(np.float32)

    def batch(i):
        return np.asfortranarray(Q[:, :, (i % n_q) * B:(i % n_q + 1) * B])

    out = {"tool": "tools/bench_sharded_prior.py", "library": os.path.relpath(clb._lib.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0),
           "docs": n_docs, "K": K, "batch": B, "k": k, "T": T, "nprobe": nprobe, "protocol": "two_phase",
           "prior": "N(0, 0.5), weight 1" if with_prior else None, "steps_per_window": args.steps, "shards": {}}
    for n_shards in args.shards:
        g = clb.ShardedSearcher.from_index(idx, n_shards)
        sides = {"plain": None}
        if with_prior:
            sides["prior"] = g.make_prior(values)

        def step(i, prior):
            more = {} if prior is None else {"prior": prior}
            return g.search_batch(batch(i), k, nprobe, pad_short=True, protocol="two_phase", **more)

        def window(prior):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(i, prior)                         # ends with the copy of the result to the host: synchronous
            return (time.perf_counter() - t0) * 1e3 / args.steps

        def list_length(prior):
            """(candidates, re-scored passages) per query, summed over the shards, over the first 8 batches"""
            for s in g.shards:
                s.profile_enable(True, counters=True)
            cand, resc = [], []
            for i in range(8):
                step(i, prior)
                st = [s.last_batch_stats() for s in g.shards]
                cand.append(sum(x["cand_docs"] for x in st) / B); resc.append(sum(x["rescored_docs"] for x in st) / B)
            for s in g.shards:
                s.profile_enable(False)
            return round(float(np.mean(cand)), 1), round(float(np.mean(resc)), 1)

        for prior in sides.values():
            for i in range(args.warmup):
                step(i, prior)
        ms = {name: [] for name in sides}
        for r in range(args.rounds):
            order = list(sides) if r % 2 == 0 else list(sides)[::-1]
            for name in order:
                ms[name].append(window(sides[name]))
        res = {"sides": {}}
        for name, prior in sides.items():
            cand, resc = list_length(prior)
            res["sides"][name] = {"step_ms": round(float(np.median(ms[name])), 4), "step_ms_windows": [round(x, 4) for x in ms[name]],
                                  "spread_ms": round(float(max(ms[name]) - min(ms[name])), 4), "candidates_per_query": cand,
                                  "nlist_per_query": resc}
        if with_prior:
            a, b = res["sides"]["plain"], res["sides"]["prior"]
            res["prior_over_plain"] = {"step_ms": round(b["step_ms"] / a["step_ms"], 4),
                                       "nlist": round(b["nlist_per_query"] / max(a["nlist_per_query"], 1e-9), 4)}
            sides["prior"].close()
        out["shards"][str(n_shards)] = res
        print(json.dumps({n_shards: res}), flush=True)
        g.close()
    return out


def against(args):
    """Alternating child processes, one library each; nothing is started after a child that failed."""
    mine = os.path.join(ROOT, "colbert.jl_amd", "csrc", "libcolbert_hip.so")
    other = os.path.abspath(args.against)
    if not os.path.exists(other):
        sys.exit(f"bench_sharded_prior: {other} does not exist")
    runs = []
    for name, path in (("this", mine), ("this", mine), ("other", other), ("this", mine), ("other", other)):
        env = dict(os.environ, COLBERT_HIP_LIB=path)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--batch", str(args.batch), "--k", str(args.k),
               "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--shards", *map(str, args.shards)]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
        if p.returncode != 0:
            sys.exit(f"bench_sharded_prior: the child with {path} ended with status {p.returncode}")
        res = json.loads(p.stdout.strip().splitlines()[-1])
        runs.append({"library": name, "path": os.path.relpath(path, ROOT), "shards": {n: r["sides"]["plain"] for n, r in res["shards"].items()}})
        print(json.dumps(runs[-1]), flush=True)
    out = {"tool": "tools/bench_sharded_prior.py --against", "order": [r["library"] for r in runs], "runs": runs, "summary": {}}
    for n in map(str, args.shards):
        ms = lambda which: [r["shards"][n]["step_ms"] for r in runs if r["library"] == which]
        this, oth = ms("this"), ms("other")
        out["summary"][n] = {"this_ms": this, "other_ms": oth, "same_library_spread_ms": round(abs(this[0] - this[1]), 4),
                             "this_median_ms": round(float(np.median(this)), 4), "other_median_ms": round(float(np.median(oth)), 4),
                             "this_over_other": round(float(np.median(this)) / float(np.median(oth)), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--shards", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--against", default=None, help="another build of libcolbert_hip.so: compare the step without a prior")
    ap.add_argument("--child", action="store_true", help="(used by --against) the plain side alone, one JSON line on stdout")
    ap.add_argument("--child-timeout", type=int, default=600, help="seconds one child of --against may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args, with_prior=False)), flush=True)
        return
    out = against(args) if args.against else measure(args, with_prior=True)
    path = args.out or os.path.join(ROOT, "profiles", "sharded_prior_parent.json" if args.against else "sharded_prior.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
