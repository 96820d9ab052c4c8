#!/usr/bin/env python3
"""Re-ranking with first-stage scores (`candidate_priors=`) on the headline corpus of bench.py (synthetic 1 M passages,
two-pass mode): B = 32 queries per step, k = 100, every query a list of 1 000 random pids with one N(0, 0.5) value per
position, weight 1, `--batches` distinct (queries, lists, values) batches.

  (a) the listed step with list priors against the listed step without them, on this build, eager (the batch's own tensors
      are passed) and under a captured graph (the batch's pids, lengths and values are copied into the captured tensors,
      then the graph is replayed; the copies are timed with it) -- with the per-kernel times of the eager sides and the
      re-score list length of both;
  (b) the route it replaces, on the checkout `--old-root` names (the parent commit, its library built): a resident prior
      holds ONE value per passage for the whole batch, so per step 32 `make_prior(dense_b)` of n_docs floats (the dense
      vectors are made ahead of the clock), 32 one-query listed steps on the device route with `prior=`, 32 closes -- host
      clock around the steps, since the creations synchronise; and the same on this build;
  (c) a step without lists on this build against `--old-root`'s, each in fresh child processes that drive their own
      checkout's library, alternating new / old / old / new: "a call without list priors costs what it cost" holds if the
      difference of the medians lies inside what two processes of one library differ by.

In-process sides: HIP events around `--steps` batches, `--rounds` windows per side interleaved with the order rotating; the
median is reported and every window kept.  Writes one JSON file (default profiles/list_prior.json); profiles/list_prior.md is
written from it by hand.  A measurement path only: it needs a GPU and fails without one."""
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
        sys.exit("bench_list_prior: no GPU")
    B = args.batch
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=B * args.batches, T=32)
    Qdev = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).cuda()
    n_docs = int(idx["doclens"].size)
    rng = np.random.default_rng(99)
    lists = rng.integers(1, n_docs + 1, size=(args.batches, B, args.list_len)).astype(np.int64)      # [batch][query][position]
    values = rng.normal(0, 0.5, size=lists.shape).astype(np.float32)
    s = clb.Searcher(index=idx, device=0)
    s.set_mode(1)
    return torch, clb, s, DeviceSearch, Qdev, lists, values, n_docs, K


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


def dense_of(n_docs, pids, vals):
    """the per-passage vector a resident prior needs for one query's list: the value of a pid's first occurrence, 0 elsewhere"""
    u, first = np.unique(pids, return_index=True)
    d = np.zeros(n_docs, np.float32)
    d[u - 1] = vals[first]
    return d


def child(args):
    """one side in a process of its own, on the checkout --root names: one JSON line of `rounds` windows"""
    torch, clb, s, DeviceSearch, Qdev, lists, values, n_docs, _ = setup(args)
    B, n_q = args.batch, args.batches
    batch = lambda i: Qdev[(i % n_q) * B:(i % n_q + 1) * B]
    if args.child == "plain":
        run = DeviceSearch(s, 32, B, args.k, 2)
        call, window = (lambda i: run(batch(i))), timed_window
    else:                                               # "priors": the route the list priors replace
        n_d = min(n_q, 2)                               # (dense vectors of two batches: 32 x 4 MB each)
        dense = [[dense_of(n_docs, lists[i, b], values[i, b]) for b in range(B)] for i in range(n_d)]
        d_lists = [torch.from_numpy(lists[i]).cuda() for i in range(n_d)]
        d_lens = torch.full((B,), args.list_len, dtype=torch.int64, device="cuda")
        one = DeviceSearch(s, 32, 1, args.k, 2)

        def call(i):
            j = i % n_d
            ps = [s.make_prior(dense[j][b]) for b in range(B)]
            q = batch(j)
            for b in range(B):
                one(q[b:b + 1], candidates=(d_lists[j][b:b + 1], d_lens[b:b + 1]), prior=ps[b], prior_weight=1.0)
            torch.cuda.synchronize()                    # the priors must outlive the searches that read them
            for p in ps:
                p.close()
        window = host_window
    for i in range(args.warmup):
        call(i)
    torch.cuda.synchronize()
    print(json.dumps({"windows_ms": [round(window(torch, args.steps, call), 5) for _ in range(args.rounds)]}), flush=True)
    s.close()


def run_child(args, side, root, steps=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--root", root, "--docs", str(args.docs), "--batch", str(args.batch),
           "--k", str(args.k), "--list-len", str(args.list_len), "--steps", str(steps or args.steps), "--rounds", str(args.rounds),
           "--warmup", str(args.warmup), "--batches", str(args.batches)]
    env = dict(os.environ)
    env.pop("COLBERT_HIP_LIB", None)                    # every checkout drives its own library
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"bench_list_prior: the {side} child on {root} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["windows_ms"]


def library_ab(args):
    """the step without lists on this build and on --old-root's, fresh child processes, new / old / old / new"""
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
    ap.add_argument("--batches", type=int, default=8, help="distinct (queries, lists, values) batches the steps cycle through")
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--prior-steps", type=int, default=5, help="batches per timed window of side (b): each is 32 make_prior calls")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-root", default=None, help="a checkout of the parent commit with its library built: sides (b) and (c)")
    ap.add_argument("--child", default=None, choices=("plain", "priors"), help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "list_prior.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    old = {}
    if args.old_root:                                   # before this process opens the GPU
        old["unlisted_against_parent"] = library_ab(args)
        old["priors_route_parent"] = summary(run_child(args, "priors", os.path.abspath(args.old_root), args.prior_steps))
        print(json.dumps({"priors_route_parent": old["priors_route_parent"]}), flush=True)
    old["priors_route_this_build"] = summary(run_child(args, "priors", HERE, args.prior_steps))
    print(json.dumps({"priors_route_this_build": old["priors_route_this_build"]}), flush=True)

    torch, clb, s, DeviceSearch, Qdev, lists, values, n_docs, K = setup(args)
    B, k, n_q, L = args.batch, args.k, args.batches, args.list_len
    batch = lambda i: Qdev[(i % n_q) * B:(i % n_q + 1) * B]
    d_lists = [torch.from_numpy(lists[i]).cuda() for i in range(n_q)]                 # int64 [B, L] each
    d_vals = [torch.from_numpy(values[i]).cuda() for i in range(n_q)]                 # float32 [B, L] each
    d_lens = torch.full((B,), L, dtype=torch.int64, device="cuda")
    run = DeviceSearch(s, 32, B, k, 2)
    # the captured sides: static tensors the graph holds the addresses of
    st_q, st_p, st_n, st_v = Qdev[:B].clone(), d_lists[0].clone(), d_lens.clone(), d_vals[0].clone()
    graphs = {"listed": run.capture(st_q, candidates=(st_p, st_n)),
              "listed_prior": run.capture(st_q, candidates=(st_p, st_n), candidate_priors=st_v, prior_weight=1.0)}

    def replay(name):
        def call(i):
            st_q.copy_(batch(i))
            st_p.copy_(d_lists[i % n_q]); st_n.copy_(d_lens)
            if name == "listed_prior":
                st_v.copy_(d_vals[i % n_q])
            graphs[name].replay()
        return call
    sides = {"listed_eager": lambda i: run(batch(i), candidates=(d_lists[i % n_q], d_lens)),
             "listed_prior_eager": lambda i: run(batch(i), candidates=(d_lists[i % n_q], d_lens), candidate_priors=d_vals[i % n_q],
                                                 prior_weight=1.0),
             "listed_graph": replay("listed"), "listed_prior_graph": replay("listed_prior")}
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
    out = {"tool": "tools/bench_list_prior.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k,
           "T": 32, "nprobe": 2, "mode": "two-pass", "list_len": L, "values": "N(0, 0.5)", "weight": 1.0,
           "steps_per_window": args.steps, "prior_route_steps_per_window": args.prior_steps, "query_batches": n_q,
           "sides": {name: summary(ms[name]) for name in names}, **old}

    def kernels(call):
        s.profile_enable(True)
        for i in range(args.steps):
            call(i)
        torch.cuda.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
        return {kn: round(v["ms"] / args.steps, 5) for kn, v in prof.items() if v["launches"]}
    for name in ("listed_eager", "listed_prior_eager"):
        out["sides"][name]["kernels_ms_per_step"] = kernels(sides[name])
        s.profile_enable(True, counters=True)
        sides[name](0)
        torch.cuda.synchronize()
        st = s.last_batch_stats()
        s.profile_enable(False)
        out["sides"][name]["candidates_per_query"] = round(st["cand_docs"] / B, 1)
        out["sides"][name]["rescored_per_query"] = round(st["rescored_docs"] / B, 1)
    for name in names:
        print(json.dumps({name: out["sides"][name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    s.close()


if __name__ == "__main__":
    main()
