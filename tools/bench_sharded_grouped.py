#!/usr/bin/env python3
"""Grouped sharded search against ungrouped sharded search on the headline corpus of bench.py (synthetic 1 M passages,
B = 32, k = 1000, two-pass shards), on ONE build: documents of `--group-len` consecutive passages (default 4), the corpus cut
into 2 and into 4 shards that all live on one GPU (`ShardedSearcher.from_index`), protocol "two_phase".

  * ms per step -- one `ShardedSearcher.search_batch` of B queries, host arrays in and out, so the exchange, the merge and
    the copies are inside -- over `--steps` steps per window: `--rounds` windows per side (default 3), interleaved
    ungrouped / grouped / grouped / ungrouped ..., the median and every sample kept;
  * the length of the re-score list per query, summed over the shards (clb_last_batch_stats of every shard), on both sides
    and for the single-handle grouped search of the unsharded corpus: what the gathered threshold costs when every shard
    publishes only its k best groups.

Writes one JSON file (default profiles/sharded_grouped.json); profiles/sharded_grouped.md is written from it by hand.
A measurement path only: it needs a GPU and fails without one."""
import argparse
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
    ap.add_argument("--group-len", type=int, default=4)
    ap.add_argument("--shards", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_grouped.json"))
    args = ap.parse_args()
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_sharded_grouped: no GPU")

    T, B, k, nprobe = 32, args.batch, args.k, 2
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    n_docs = int(idx["doclens"].size)
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=768, T=T)
    n_q = Q.shape[2] // B
    lens = np.full(n_docs // args.group_len, args.group_len, np.int64)
    if n_docs % args.group_len:
        lens = np.concatenate([lens, [n_docs % args.group_len]])

    def batch(i):
        return np.asfortranarray(Q[:, :, (i % n_q) * B:(i % n_q + 1) * B])

    out = {"tool": "tools/bench_sharded_grouped.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k,
           "T": T, "nprobe": nprobe, "protocol": "two_phase", "group_len": args.group_len, "groups": int(lens.size),
           "steps_per_window": args.steps, "shards": {}}

    for n_shards in args.shards:
        g = clb.ShardedSearcher.from_index(idx, n_shards)
        gr = g.make_grouping(group_lens=lens)
        sides = {"ungrouped": None, "grouped": gr}
        straddling = sum(1 for r in g.shard_ranges[:-1] if (r.stop - 1) % args.group_len)

        def step(i, grouping):
            return g.search_batch(batch(i), k, nprobe, pad_short=True, protocol="two_phase", grouping=grouping)

        def window(grouping):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(i, grouping)                      # ends with the copy of the result to the host: synchronous
            return (time.perf_counter() - t0) * 1e3 / args.steps

        def list_length(grouping):
            """(candidates, re-scored passages, reported n_cand) per query, summed over the shards, over the first 8 batches"""
            for s in g.shards:
                s.profile_enable(True, counters=True)
            cand, resc, rep = [], [], []
            for i in range(8):
                _, _, n = step(i, grouping)
                st = [s.last_batch_stats() for s in g.shards]
                cand.append(sum(x["cand_docs"] for x in st) / B); resc.append(sum(x["rescored_docs"] for x in st) / B)
                rep.append(float(n.mean()))
            for s in g.shards:
                s.profile_enable(False)
            return round(float(np.mean(cand)), 1), round(float(np.mean(resc)), 1), round(float(np.mean(rep)), 1)

        for grouping in sides.values():
            for i in range(args.warmup):
                step(i, grouping)
        ms = {name: [] for name in sides}
        for r in range(args.rounds):
            for name in (("ungrouped", "grouped") if r % 2 == 0 else ("grouped", "ungrouped")):
                ms[name].append(window(sides[name]))
        res = {"cuts_inside_a_document": straddling, "sides": {}}
        for name, grouping in sides.items():
            cand, resc, rep = list_length(grouping)
            res["sides"][name] = {"step_ms": round(float(np.median(ms[name])), 4), "step_ms_windows": [round(x, 4) for x in ms[name]],
                                  "spread_ms": round(float(max(ms[name]) - min(ms[name])), 4), "candidates_per_query": cand,
                                  "nlist_per_query": resc, "reported_n_cand_per_query": rep}
        a, b = res["sides"]["ungrouped"], res["sides"]["grouped"]
        res["grouped_over_ungrouped"] = {"step_ms": round(b["step_ms"] / a["step_ms"], 4),
                                         "nlist": round(b["nlist_per_query"] / max(a["nlist_per_query"], 1e-9), 4)}
        out["shards"][str(n_shards)] = res
        print(json.dumps({n_shards: res}), flush=True)
        gr.close()
        g.close()

    # the single-handle grouped search of the unsharded corpus: its re-score list is what the exact threshold gives
    s = clb.Searcher(index=idx, device=0)
    s.set_mode(1)
    run = DeviceSearch(s, T, B, k, nprobe)
    sg = s.make_grouping(group_lens=lens)
    s.profile_enable(True, counters=True)
    resc = []
    for i in range(8):
        Qd = torch.from_numpy(np.ascontiguousarray(batch(i).transpose(2, 1, 0))).cuda()
        run(Qd, None, "candidates", sg)
        torch.cuda.synchronize()
        resc.append(s.last_batch_stats()["rescored_docs"] / B)
    s.profile_enable(False)
    out["single_handle_grouped_nlist_per_query"] = round(float(np.mean(resc)), 1)
    for n_shards, res in out["shards"].items():
        res["grouped_nlist_over_single_handle"] = round(res["sides"]["grouped"]["nlist_per_query"] /
                                                        max(out["single_handle_grouped_nlist_per_query"], 1e-9), 4)
    print(json.dumps({"single_handle_grouped_nlist_per_query": out["single_handle_grouped_nlist_per_query"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sg.close()
    s.close()


if __name__ == "__main__":
    main()
