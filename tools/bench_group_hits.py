#!/usr/bin/env python3
"""Hits of a grouped search (`per_group`) against the grouped search of another build of the library, on the headline corpus
of bench.py (synthetic 1 M passages, B = 32, k = 1000, two-pass mode), documents of `--group-len` consecutive passages
(default 4).

A process binds ONE build of the library (COLBERT_HIP_LIB), so the comparison runs as child processes of this tool, one per
window and build, interleaved: parent, tree, tree, parent, parent, tree (`--rounds` pairs, default 3).  A child builds the
corpus, warms up, and times every side its library has over `--steps` batches between two HIP events:

  * `grouped`: the grouped step (both builds);
  * `per_group=1`, `per_group=2`, `per_group=4`: the grouped step with hits (this tree only; a library without
    clb_search_batch_grouped_hits_device_slot runs `grouped` alone).

and reads the re-scored passages per query of every side (clb_last_batch_stats over 8 batches).  The parent reports the
median of its windows per side, every sample and the spread (max - min).

    python tools/bench_group_hits.py --parent-lib /path/to/the/parent/commit's/libcolbert_hip.so

Writes one JSON file (default profiles/group_hits.json); profiles/group_hits.md is written from it by hand.
A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_GROUP = (1, 2, 4)


def child(args):
    """one window of every side this process's library has -> one JSON line on stdout"""
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_group_hits: no GPU")
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
    has_hits = hasattr(clb.lib(), "clb_search_batch_grouped_hits_device_slot")
    sides = {"grouped": None}
    if has_hits:
        sides.update({f"per_group={m}": m for m in PER_GROUP})

    def step(i, m):
        q = Qdev[(i % n_q) * B:(i % n_q + 1) * B]
        if m is None:
            run(q, None, "candidates", g)
        else:
            run(q, None, "candidates", g, m)

    def window(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(i, m)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def rescored(m):
        s.profile_enable(True, counters=True)
        resc = []
        for i in range(8):
            step(i, m)
            torch.cuda.synchronize()
            resc.append(s.last_batch_stats()["rescored_docs"] / B)
        s.profile_enable(False)
        return round(float(np.mean(resc)), 1)

    for m in sides.values():                       # sizes the slot for every side, warms them
        for i in range(args.warmup):
            step(i, m)
    torch.cuda.synchronize()
    order = list(sides) if args.window % 2 == 0 else list(sides)[::-1]
    ms = {name: round(window(sides[name]), 5) for name in order}
    out = {"lib": args.label, "window": args.window, "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "groups": g.count,
           "step_ms": ms, "rescored_per_query": {name: rescored(m) for name, m in sides.items()}}
    g.close()
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--group-len", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="windows per build (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", help="libcolbert_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_hits.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--label", default="tree", help=argparse.SUPPRESS)
    ap.add_argument("--window", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("bench_group_hits: --parent-lib must name the parent commit's build of libcolbert_hip.so")
    results = []
    for r in range(args.rounds):
        for label in (("parent", "tree") if r % 2 == 0 else ("tree", "parent")):
            env = dict(os.environ)
            env.pop("COLBERT_HIP_LIB", None)
            if label == "parent":
                env["COLBERT_HIP_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--window", str(r), "--docs", str(args.docs),
                   "--batch", str(args.batch), "--k", str(args.k), "--group-len", str(args.group_len), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if done.returncode != 0:                            # nothing more is started on the device after a failed child
                sys.exit(f"bench_group_hits: the {label} window {r} ended with status {done.returncode}")
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            results.append(json.loads(line[len("RESULT "):]))
            print(line, flush=True)
    out = {"tool": "tools/bench_group_hits.py", "device": results[0]["device"], "docs": results[0]["docs"], "K": results[0]["K"],
           "batch": args.batch, "k": args.k, "T": 32, "nprobe": 2, "mode": "two-pass", "group_len": args.group_len,
           "groups": results[0]["groups"], "steps_per_window": args.steps, "windows": results, "sides": {}}
    for label in ("parent", "tree"):
        mine = [x for x in results if x["lib"] == label]
        for name in mine[0]["step_ms"]:
            w = [x["step_ms"][name] for x in mine]
            out["sides"][f"{label}: {name}"] = {"step_ms": round(float(np.median(w)), 5), "step_ms_windows": w,
                                                "spread_ms": round(float(max(w) - min(w)), 5),
                                                "rescored_per_query": mine[0]["rescored_per_query"][name]}
    base = out["sides"]["parent: grouped"]["step_ms"]
    out["over_parent_grouped"] = {name: round(v["step_ms"] / base, 4) for name, v in out["sides"].items()}
    print(json.dumps(out["sides"], indent=1), flush=True)
    print(json.dumps(out["over_parent_grouped"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
