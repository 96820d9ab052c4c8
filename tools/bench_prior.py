#!/usr/bin/env python3
"""Search with a score prior against search without one on the headline corpus of bench.py (synthetic 1 M passages, B = 32,
k = 1000, two-pass mode), on ONE build and one handle:

  * ms per step by HIP events around `--steps` batches: `--rounds` windows per side (default 3), interleaved between no prior,
    an all-zero prior and an N(0, 0.5) prior, the order rotating from round to round; the median and every sample kept;
  * the mean length of the re-score list per query on each side (clb_last_batch_stats over eight batches of each);
  * the HIP-event time per launch of every profile row (clb_profile_read): the boost of the approximate scores and the boosted
    threshold run inside the `select_margin` row, the boost of the exact scores inside the `topk` row.

With `--old-lib` (another build of the library, e.g. the parent commit's `make SUF=_old`): the step WITHOUT a prior on both
libraries, each in fresh child processes (COLBERT_HIP_LIB), alternating new / old / old / new, before the in-process part --
the no-prior path must be unchanged within the spread two windows of the same library show.

Writes one JSON file (default profiles/prior.json); profiles/prior.md is written from it by hand.
A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(args):
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    from colbert_jl_amd.distributed import DeviceSearch
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_prior: no GPU")
    T, B, k = 32, args.batch, args.k
    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8))
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=768, T=T)
    Qdev = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).cuda()
    s = clb.Searcher(index=idx, device=0)
    s.set_mode(1)
    return torch, s, DeviceSearch(s, T, B, k, 2), Qdev, int(idx["doclens"].size), K


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
    """the step without a prior on whatever library COLBERT_HIP_LIB names: one JSON line of `rounds` windows"""
    torch, s, run, Qdev, _, _ = setup(args)
    B, n_q = args.batch, Qdev.shape[0] // args.batch
    call = lambda i: run(Qdev[(i % n_q) * B:(i % n_q + 1) * B])
    for i in range(args.warmup):
        call(i)
    torch.cuda.synchronize()
    print(json.dumps({"windows_ms": [round(timed_window(torch, args.steps, call), 5) for _ in range(args.rounds)]}), flush=True)
    s.close()


def library_ab(args):
    """no-prior step on this build and on --old-lib, fresh child processes, new / old / old / new"""
    runs = {"new": [], "old": []}
    base = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--batch", str(args.batch), "--k", str(args.k),
            "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    for side in ("new", "old", "old", "new"):
        env = dict(os.environ)
        env.pop("COLBERT_HIP_LIB", None)
        if side == "old":
            env["COLBERT_HIP_LIB"] = os.path.abspath(args.old_lib)
        r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"bench_prior: the {side} child failed ({r.returncode}):\n{r.stderr[-2000:]}")
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
    ap.add_argument("--steps", type=int, default=40, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side (the median is reported, all are kept)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-lib", default=None, help="another build of libcolbert_hip.so to time the no-prior step against")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    ab = library_ab(args) if args.old_lib else None         # before this process opens the GPU

    torch, s, run, Qdev, n_docs, K = setup(args)
    B, k, n_q = args.batch, args.k, Qdev.shape[0] // args.batch
    rng = np.random.default_rng(5)
    priors = {"no_prior": None, "zero_prior": s.make_prior(np.zeros(n_docs, np.float32)),
              "normal_prior": s.make_prior(rng.normal(0.0, 0.5, n_docs).astype(np.float32))}

    def call(prior):
        return lambda i: run(Qdev[(i % n_q) * B:(i % n_q + 1) * B], prior=prior)

    def kernels(prior):
        s.profile_enable(True)
        for i in range(args.steps):
            call(prior)(i)
        torch.cuda.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
        return {kn: round(v["ms"] / max(v["launches"], 1), 5) for kn, v in prof.items() if v["launches"]}

    def list_length(prior):
        """(mean candidates, mean re-scored passages) per query over the first 8 batches"""
        s.profile_enable(True, counters=True)
        cand, resc = [], []
        for i in range(8):
            call(prior)(i)
            torch.cuda.synchronize()
            st = s.last_batch_stats()
            cand.append(st["cand_docs"] / B); resc.append(st["rescored_docs"] / B)
        s.profile_enable(False)
        return round(float(np.mean(cand)), 1), round(float(np.mean(resc)), 1)

    for prior in priors.values():                  # sizes the slot (the first call with a prior grows it once), warms every side
        for i in range(args.warmup):
            call(prior)(i)
    torch.cuda.synchronize()
    names = list(priors)
    ms = {name: [] for name in names}
    for r in range(args.rounds):
        for name in names[r % 3:] + names[:r % 3]:
            ms[name].append(timed_window(torch, args.steps, call(priors[name])))
    out = {"tool": "tools/bench_prior.py", "device": torch.cuda.get_device_name(0), "docs": n_docs, "K": K, "batch": B, "k": k, "T": 32,
           "nprobe": 2, "mode": "two-pass", "steps_per_window": args.steps, "sides": {}}
    for name, prior in priors.items():
        cand, resc = list_length(prior)
        out["sides"][name] = {"step_ms": round(float(np.median(ms[name])), 5), "step_ms_windows": [round(x, 5) for x in ms[name]],
                              "spread_ms": round(float(max(ms[name]) - min(ms[name])), 5), "candidates_per_query": cand,
                              "nlist_per_query": resc, "kernels_ms": kernels(prior)}
        print(json.dumps({name: out["sides"][name]}), flush=True)
    base = out["sides"]["no_prior"]
    out["over_no_prior"] = {name: {"step_ms": round(out["sides"][name]["step_ms"] / base["step_ms"], 4),
                                   "nlist": round(out["sides"][name]["nlist_per_query"] / max(base["nlist_per_query"], 1e-9), 4)}
                            for name in names[1:]}
    print(json.dumps(out["over_no_prior"]), flush=True)
    if ab:
        out["no_prior_against_old_library"] = ab
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in priors.values():
        if p is not None:
            p.close()
    s.close()


if __name__ == "__main__":
    main()
