#!/usr/bin/env python3
"""Re-ranking given passages (`candidates=`) on the headline corpus of bench.py (synthetic 1 M passages, two-pass mode):
B = 32 queries per step, k = 100, every query a list of 1 000 random pids, `--batches` distinct (queries, lists) batches.

  1. a listed step on the device route, eager (the batch's own list tensors are passed) and under a captured graph (the
     batch's pids and lengths are copied into the captured tensors, then the graph is replayed; the copies are timed with it);
  2. the route it replaces, on the checkout `--old-root` names (the parent commit, its library built): per step 32
     `make_filter(pids=...)`, one `scope="all"` step on the device route, 32 closes -- host clock around the steps, since the
     creations synchronise; and the same on this build;
  3. an unlisted step of this build against `--old-root`'s, each in fresh child processes, alternating new / old / old / new:
     "a call without lists costs what it cost" holds if the difference of the medians lies inside what two processes of one
     library differ by;
  4. a listed step that also asks for the list scores (`candidate_scores=`), eager and under a graph: the price of the
     single exact pass.

In-process sides: HIP events around `--steps` batches, `--rounds` windows per side interleaved with the order rotating; the
median is reported and every window kept.  Writes one JSON file (default profiles/rerank.json); profiles/rerank.md is written
from it by hand.  A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def root_of(argv):
    """--root PATH (children only): the checkout whose package and library this process drives"""
    return os.path.abspath(argv[argv.index("--root") + 1]) if "--root" in argv else HERE


sys.path.insert(0, root_of(sys.argv))


def setup(args):
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_rerank: no GPU")
    B = args.batch
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=B * args.batches, T=32)
    Qdev = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).cuda()
    n_docs = int(idx["doclens"].size)
    rng = np.random.default_rng(99)
    lists = rng.integers(1, n_docs + 1, size=(args.batches, B, args.list_len)).astype(np.int64)      # [batch][query][position]
    s = clb.Searcher(index=idx, device=0)
    s.set_mode(1)
    return torch, clb, s, DeviceSearch, Qdev, lists, n_docs, K


def timed_window(torch, steps, call):
    """ms per batch over `steps` batches between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        call(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def host_window(torch, steps, call):
    """ms per batch over `steps` batches by the host's clock (for sides that synchronise inside a step)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        call(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def child(args):
    """one side in a process of its own, on the checkout --root names: one JSON line of `rounds` windows"""
    torch, clb, s, DeviceSearch, Qdev, lists, _, _ = setup(args)
    B, n_q = args.batch, args.batches
    run = DeviceSearch(s, 32, B, args.k, 2)
    batch = lambda i: Qdev[(i % n_q) * B:(i % n_q + 1) * B]
    if args.child == "plain":
        call, window = (lambda i: run(batch(i))), timed_window
    else:                                               # "filters": the route the lists replace
        def call(i):
            fs = [s.make_filter(pids=lists[i % n_q, b]) for b in range(B)]
            run(batch(i), filters=fs, scope="all")
            torch.cuda.synchronize()                    # the filters must outlive the search that reads them
            for f in fs:
                f.close()
        window = host_window
    for i in range(args.warmup):
        call(i)
    torch.cuda.synchronize()
    print(json.dumps({"windows_ms": [round(window(torch, args.steps, call), 5) for _ in range(args.rounds)]}), flush=True)
    s.close()


def run_child(args, side, root):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--root", root, "--docs", str(args.docs), "--batch", str(args.batch),
           "--k", str(args.k), "--list-len", str(args.list_len), "--steps", str(args.steps), "--rounds", str(args.rounds),
           "--warmup", str(args.warmup), "--batches", str(args.batches)]
    env = dict(os.environ)
    env.pop("COLBERT_HIP_LIB", None)                    # every checkout drives its own library
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"bench_rerank: the {side} child on {root} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["windows_ms"]


def library_ab(args):
    """the unlisted step on this build and on --old-root's, fresh child processes, new / old / old / new"""
    runs = {"new": [], "old": []}
    for side in ("new", "old", "old", "new"):
        runs[side].append(run_child(args, "plain", HERE if side == "new" else os.path.abspath(args.old_root)))
        print(json.dumps({side: runs[side][-1]}), flush=True)
    med = {side: float(np.median(np.concatenate(w))) for side, w in runs.items()}
    same_lib = max(abs(float(np.median(w[0])) - float(np.median(w[1]))) for w in runs.values())
    return {"windows_ms": runs, "median_ms": {k: round(v, 5) for k, v in med.items()}, "new_over_old": round(med["new"] / med["old"], 4),
            "new_minus_old_ms": round(med["new"] - med["old"], 5), "same_library_spread_ms": round(same_lib, 5),
            "unchanged_within_spread": bool(abs(med["new"] - med["old"]) <= same_lib)}


def summary(v):
    return {"step_ms": round(float(np.median(v)), 5), "step_ms_windows": [round(x, 5) for x in v],
            "spread_ms": round(float(max(v) - min(v)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--list-len", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=8, help="distinct (queries, lists) batches the steps cycle through")
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-root", default=None, help="a checkout of the parent commit with its library built: sides 2 and 3")
    ap.add_argument("--child", default=None, choices=("plain", "filters"), help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rerank.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    old = {}
    if args.old_root:                                   # before this process opens the GPU
        old["unlisted_against_parent"] = library_ab(args)
        old["filters_route_parent"] = summary(run_child(args, "filters", os.path.abspath(args.old_root)))
        print(json.dumps({"filters_route_parent": old["filters_route_parent"]}), flush=True)
    old["filters_route_this_build"] = summary(run_child(args, "filters", HERE))
    print(json.dumps({"filters_route_this_build": old["filters_route_this_build"]}), flush=True)

    torch, clb, s, DeviceSearch, Qdev, lists, n_docs, K = setup(args)
    B, k, n_q, L = args.batch, args.k, args.batches, args.list_len
    batch = lambda i: Qdev[(i % n_q) * B:(i % n_q + 1) * B]
    d_lists = [torch.from_numpy(lists[i]).cuda() for i in range(n_q)]                 # int64 [B, L] each
    d_lens = torch.full((B,), L, dtype=torch.int64, device="cuda")
    d_scores = torch.zeros((B, L), dtype=torch.float32, device="cuda")
    run = DeviceSearch(s, 32, B, k, 2)
    # the captured sides: static tensors the graph holds the addresses of
    st_q, st_p, st_n = Qdev[:B].clone(), d_lists[0].clone(), d_lens.clone()
    graphs = {"listed": run.capture(st_q, candidates=(st_p, st_n)),
              "listed_scores": run.capture(st_q, candidates=(st_p, st_n), candidate_scores=d_scores),
              "unlisted": run.capture(st_q)}

    def replay(name):
        def call(i):
            st_q.copy_(batch(i))
            if name != "unlisted":
                st_p.copy_(d_lists[i % n_q]); st_n.copy_(d_lens)
            graphs[name].replay()
        return call
    sides = {"unlisted_eager": lambda i: run(batch(i)),
             "listed_eager": lambda i: run(batch(i), candidates=(d_lists[i % n_q], d_lens)),
             "listed_scores_eager": lambda i: run(batch(i), candidates=(d_lists[i % n_q], d_lens), candidate_scores=d_scores),
             "unlisted_graph": replay("unlisted"), "listed_graph": replay("listed"), "listed_scores_graph": replay("listed_scores")}
    names = list(sides)
    for name in names:
        for i in range(args.warmup):
            sides[name](i)
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for r in range(args.rounds):
        rot = r % len(names)
        for name in names[rot:] + names[:rot]:
            ms[name].append(timed_window(torch, args.steps, sides[name]))
    out = {"tool": "tools/bench_rerank.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k, "T": 32,
           "nprobe": 2, "mode": "two-pass", "list_len": L, "steps_per_window": args.steps, "query_batches": n_q,
           "sides": {name: summary(ms[name]) for name in names}, **old}

    def kernels(call):
        s.profile_enable(True)
        for i in range(args.steps):
            call(i)
        torch.cuda.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
        return {kn: round(v["ms"] / max(v["launches"], 1), 5) for kn, v in prof.items() if v["launches"]}
    for name in ("unlisted_eager", "listed_eager", "listed_scores_eager"):
        out["sides"][name]["kernels_ms"] = kernels(sides[name])
    s.profile_enable(True, counters=True)
    sides["listed_eager"](0)
    torch.cuda.synchronize()
    st = s.last_batch_stats()
    s.profile_enable(False)
    out["listed_candidates_per_query"] = round(st["cand_docs"] / B, 1)
    out["listed_rescored_per_query"] = round(st["rescored_docs"] / B, 1)
    for name in names:
        print(json.dumps({name: out["sides"][name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    s.close()


if __name__ == "__main__":
    main()
