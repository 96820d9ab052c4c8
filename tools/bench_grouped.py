#!/usr/bin/env python3
"""Grouped search against ungrouped search on the headline corpus of bench.py (synthetic 1 M passages, B = 32, k = 1000,
two-pass mode), on ONE build and one handle: documents of `--group-len` consecutive passages (default 4) throughout.

  * ms per step by HIP events around `--steps` batches: `--rounds` windows per side (default 3), interleaved
    ungrouped / grouped / grouped / ungrouped ..., the median and every sample kept;
  * the mean length of the re-score list per query on both sides (clb_last_batch_stats over one batch of each): the grouped
    list is longer, because the threshold sits at the k-th best DOCUMENT, and pass 2 grows with it;
  * the HIP-event time per launch of every profile row (clb_profile_read), the `select_margin` and `topk` rows -- where the
    collapse and the group threshold run -- among them.

Writes one JSON file (default profiles/grouped.json); profiles/grouped.md is written from it by hand.
A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--group-len", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped.json"))
    args = ap.parse_args()
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_grouped: no GPU")

    T, B, k = 32, args.batch, args.k
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    n_docs = int(idx["doclens"].size)
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=768, T=T)
    Qdev = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).cuda()
    n_q = Qdev.shape[0] // B

    s = clb.Searcher(index=idx, device=0)
    s.set_mode(1)
    run = DeviceSearch(s, T, B, k, 2)
    lens = np.full(n_docs // args.group_len, args.group_len, np.int64)
    if n_docs % args.group_len:
        lens = np.concatenate([lens, [n_docs % args.group_len]])
    g = s.make_grouping(group_lens=lens)
    sides = {"ungrouped": None, "grouped": g}

    def batch(i):
        return Qdev[(i % n_q) * B:(i % n_q + 1) * B]

    def window(grouping):
        """ms per batch over `steps` batches between two HIP events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            run(batch(i), None, "candidates", grouping)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def kernels(grouping):
        s.profile_enable(True)
        for i in range(args.steps):
            run(batch(i), None, "candidates", grouping)
        torch.cuda.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
        return {kn: round(v["ms"] / max(v["launches"], 1), 5) for kn, v in prof.items() if v["launches"]}

    def list_length(grouping):
        """(mean candidates, mean re-scored passages, mean reported n_cand) per query over the first 8 batches"""
        s.profile_enable(True, counters=True)
        cand, resc, rep = [], [], []
        for i in range(8):
            run(batch(i), None, "candidates", grouping)
            torch.cuda.synchronize()
            st = s.last_batch_stats()
            cand.append(st["cand_docs"] / B); resc.append(st["rescored_docs"] / B)
            rep.append(float(run.ncand.cpu().numpy().mean()))
        s.profile_enable(False)
        return round(float(np.mean(cand)), 1), round(float(np.mean(resc)), 1), round(float(np.mean(rep)), 1)

    for grouping in sides.values():                # sizes the slot for both (the grouped call grows it once), warms both
        for i in range(args.warmup):
            run(batch(i), None, "candidates", grouping)
    torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for r in range(args.rounds):
        for name in (("ungrouped", "grouped") if r % 2 == 0 else ("grouped", "ungrouped")):
            ms[name].append(window(sides[name]))
    out = {"tool": "tools/bench_grouped.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k, "T": T,
           "nprobe": 2, "mode": "two-pass", "group_len": args.group_len, "groups": g.count, "steps_per_window": args.steps, "sides": {}}
    for name, grouping in sides.items():
        cand, resc, rep = list_length(grouping)
        out["sides"][name] = {"step_ms": round(float(np.median(ms[name])), 5), "step_ms_windows": [round(x, 5) for x in ms[name]],
                              "spread_ms": round(float(max(ms[name]) - min(ms[name])), 5), "candidates_per_query": cand,
                              "nlist_per_query": resc, "reported_n_cand_per_query": rep, "kernels_ms": kernels(grouping)}
        print(json.dumps({name: out["sides"][name]}), flush=True)
    a, b = out["sides"]["ungrouped"], out["sides"]["grouped"]
    out["grouped_over_ungrouped"] = {"step_ms": round(b["step_ms"] / a["step_ms"], 4),
                                     "nlist": round(b["nlist_per_query"] / max(a["nlist_per_query"], 1e-9), 4)}
    print(json.dumps(out["grouped_over_ungrouped"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    g.close()
    s.close()


if __name__ == "__main__":
    main()
