#!/usr/bin/env python3
"""Search after a cursor against search without one on the headline corpus of bench.py (synthetic 1 M passages, B = 32,
k = 1000, two-pass mode), on ONE build and one handle:

  * ms per step by HIP events around `--steps` batches: `--rounds` windows per side (default 3), interleaved between no cursor
    arrays at all, cursors at depth 0 (+Inf: "no cursor" through the new entry point), depth 1 000 and depth 10 000, the order
    rotating from round to round; the median and every sample kept.  The cursor at depth d of a query is the (score, pid) of
    rank d of its plain ranking, taken once from a search with k = 10 000;
  * the mean length of the re-score list per query on each side (clb_last_batch_stats over the batches used);
  * the HIP-event time per launch of every profile row (clb_profile_read): after_cut_kernel runs inside the `select_margin`
    row, after_filter_kernel inside the `topk` row;
  * page 11 by cursor (k = 1 000, depth 10 000) against ONE call with k = 11 000, interleaved in the same way.

With `--old-lib` (another build of the library, e.g. the parent commit's `make SUF=_old`): the step WITHOUT cursors on both
libraries, each in fresh child processes (COLBERT_HIP_LIB), alternating new / old / old / new, before the in-process part --
the path without a cursor must be unchanged within the spread two processes of the same library show.

Writes one JSON file (default profiles/after.json); profiles/after.md is written from it by hand.
A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEEP = 10_000


def setup(args):
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_after: no GPU")
    T, B, k = 32, args.batch, args.k
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=B * args.batches, T=T)
    Qdev = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).cuda()
    s = clb.Searcher(index=idx, device=0)
    s.set_mode(1)
    return torch, s, DeviceSearch, Qdev, int(idx["doclens"].size), K


def timed_window(torch, steps, call):
    """ms per batch over `steps` batches between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        call(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def child(args):
    """the step without cursors on whatever library COLBERT_HIP_LIB names: one JSON line of `rounds` windows"""
    torch, s, DeviceSearch, Qdev, _, _ = setup(args)
    B, n_q = args.batch, args.batches
    run = DeviceSearch(s, 32, B, args.k, 2)
    call = lambda i: run(Qdev[(i % n_q) * B:(i % n_q + 1) * B])
    for i in range(args.warmup):
        call(i)
    torch.cuda.synchronize()
    print(json.dumps({"windows_ms": [round(timed_window(torch, args.steps, call), 5) for _ in range(args.rounds)]}), flush=True)
    s.close()


def library_ab(args):
    """the step without cursors on this build and on --old-lib, fresh child processes, new / old / old / new"""
    runs = {"new": [], "old": []}
    base = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--batch", str(args.batch), "--k", str(args.k),
            "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--batches", str(args.batches)]
    for side in ("new", "old", "old", "new"):
        env = dict(os.environ)
        env.pop("COLBERT_HIP_LIB", None)
        if side == "old":
            env["COLBERT_HIP_LIB"] = os.path.abspath(args.old_lib)
        r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"bench_after: the {side} child failed ({r.returncode}):\n{r.stderr[-2000:]}")
        runs[side].append(json.loads(r.stdout.strip().splitlines()[-1])["windows_ms"])
        print(json.dumps({side: runs[side][-1]}), flush=True)
    med = {side: float(np.median(np.concatenate(w))) for side, w in runs.items()}
    same_lib = max(abs(float(np.median(w[0])) - float(np.median(w[1]))) for w in runs.values())
    return {"windows_ms": runs, "median_ms": {k: round(v, 5) for k, v in med.items()}, "new_over_old": round(med["new"] / med["old"], 4),
            "new_minus_old_ms": round(med["new"] - med["old"], 5), "same_library_spread_ms": round(same_lib, 5),
            "unchanged_within_spread": bool(abs(med["new"] - med["old"]) <= same_lib)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=8, help="distinct query batches the steps cycle through")
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-lib", default=None, help="another build of libcolbert_hip.so to time the step without cursors against")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "after.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    ab = library_ab(args) if args.old_lib else None         # before this process opens the GPU

    torch, s, DeviceSearch, Qdev, n_docs, K = setup(args)
    B, k, n_q = args.batch, args.k, args.batches
    batch = lambda i: Qdev[(i % n_q) * B:(i % n_q + 1) * B]
    deep = DeviceSearch(s, 32, B, DEEP, 2)                  # the plain ranking to depth 10 000: where the cursors come from
    long_page = DeviceSearch(s, 32, B, DEEP + k, 2)         # page 11 the only way there was: one call with k = 11 000
    run = DeviceSearch(s, 32, B, k, 2)
    cursors = {"depth_0": [], "depth_1000": [], "depth_10000": []}
    short = 0
    for i in range(n_q):
        p, sc = deep(batch(i))
        torch.cuda.synchronize()
        cursors["depth_0"].append((torch.full((B,), float("inf"), device=p.device), torch.zeros(B, dtype=torch.int64, device=p.device)))
        for name, d in (("depth_1000", 1000), ("depth_10000", DEEP)):
            cursors[name].append((sc[:, d - 1].clone(), p[:, d - 1].clone()))
        short += int((p[:, DEEP - 1] == 0).sum())           # a query with fewer than 10 000 candidates: its deep page is empty
    sides = {"no_cursor": None, **cursors}

    def call(name):
        cur = sides[name]
        return (lambda i: run(batch(i))) if cur is None else (lambda i: run(batch(i), after=cur[i % n_q]))

    def kernels(name):
        s.profile_enable(True)
        for i in range(args.steps):
            call(name)(i)
        torch.cuda.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
        return {kn: round(v["ms"] / max(v["launches"], 1), 5) for kn, v in prof.items() if v["launches"]}

    def list_length(name):
        """(mean candidates, mean re-scored passages) per query over the batches"""
        s.profile_enable(True, counters=True)
        cand, resc = [], []
        for i in range(n_q):
            call(name)(i)
            torch.cuda.synchronize()
            st = s.last_batch_stats()
            cand.append(st["cand_docs"] / B); resc.append(st["rescored_docs"] / B)
        s.profile_enable(False)
        return round(float(np.mean(cand)), 1), round(float(np.mean(resc)), 1)

    names = list(sides)
    for name in names:                             # sizes the slot (the first call with cursors grows it once), warms every side
        for i in range(args.warmup):
            call(name)(i)
    for i in range(args.warmup):
        long_page(batch(i))
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for r in range(args.rounds):
        rot = r % len(names)
        for name in names[rot:] + names[:rot]:
            ms[name].append(timed_window(torch, args.steps, call(name)))
    out = {"tool": "tools/bench_after.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k, "T": 32,
           "nprobe": 2, "mode": "two-pass", "steps_per_window": args.steps, "query_batches": n_q,
           "queries_with_fewer_than_10000_candidates": short, "sides": {}}
    for name in names:
        cand, resc = list_length(name)
        out["sides"][name] = {"step_ms": round(float(np.median(ms[name])), 5), "step_ms_windows": [round(x, 5) for x in ms[name]],
                              "spread_ms": round(float(max(ms[name]) - min(ms[name])), 5), "candidates_per_query": cand,
                              "nlist_per_query": resc, "kernels_ms": kernels(name)}
        print(json.dumps({name: out["sides"][name]}), flush=True)
    base = out["sides"]["no_cursor"]
    out["over_no_cursor"] = {name: {"step_ms": round(out["sides"][name]["step_ms"] / base["step_ms"], 4),
                                    "minus_ms": round(out["sides"][name]["step_ms"] - base["step_ms"], 5),
                                    "nlist": round(out["sides"][name]["nlist_per_query"] / max(base["nlist_per_query"], 1e-9), 4)}
                             for name in names[1:]}
    print(json.dumps(out["over_no_cursor"]), flush=True)
    # page 11: by cursor against one call with k = 11 000
    pair = {"page_11_by_cursor": call("depth_10000"), "one_call_k_11000": lambda i: long_page(batch(i))}
    pms = {name: [] for name in pair}
    for r in range(args.rounds):
        for name in (list(pair) if r % 2 == 0 else list(pair)[::-1]):
            pms[name].append(timed_window(torch, args.steps, pair[name]))
    out["page_11"] = {name: {"step_ms": round(float(np.median(v)), 5), "step_ms_windows": [round(x, 5) for x in v],
                             "spread_ms": round(float(max(v) - min(v)), 5)} for name, v in pms.items()}
    s.profile_enable(True, counters=True)
    long_page(batch(0))
    torch.cuda.synchronize()
    out["page_11"]["one_call_k_11000"]["nlist_per_query"] = round(s.last_batch_stats()["rescored_docs"] / B, 1)
    s.profile_enable(False)
    out["page_11"]["cursor_over_one_call"] = round(out["page_11"]["page_11_by_cursor"]["step_ms"]
                                                   / out["page_11"]["one_call_k_11000"]["step_ms"], 4)
    print(json.dumps(out["page_11"]), flush=True)
    if ab:
        out["no_cursor_against_old_library"] = ab
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    s.close()


if __name__ == "__main__":
    main()
