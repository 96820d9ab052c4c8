#!/usr/bin/env python3
"""Removing from a resident index against rebuilding it, on the headline corpus of bench.py (synthetic 1 M passages): wall
time of `Searcher.remove_passages` of 1 passage, 1 % and 50 % of the passages of a resident 1 M-passage Searcher, beside
the wall time of `Searcher(index=reduced)` on the reduced host arrays with their IVF already computed -- the route a caller
had to take before (the host-side column deletion and IVF rebuild that route also needs are NOT in its figure).

The baseline is timed with ANOTHER build of the library when --baseline-lib names one (the parent commit's, built with
`make SUF=_old`: README, "A/B against another commit"): a process loads one library, so the baseline runs in a child process of
this tool with COLBERT_HIP_LIB set, on the same card, before this process touches the GPU.  The child regenerates the
corpus from the same seeds.  --baseline-reps baseline runs per case (default 5) give the run-to-run spread the removal time
is held against.  Every figure is a host clock around work that ends in clb_device_synchronize.  Writes one JSON file
(default profiles/remove.json) and prints the table of profiles/remove.md.

A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def removed_pids(n_docs, how, seed=5):
    """the 1-based pids a case removes: "1" -> one passage in the middle, "1%" / "50%" -> that share, at random"""
    if how.endswith("%"):
        n = int(round(n_docs * float(how[:-1]) / 100.0))
        return np.sort(np.random.default_rng(seed).choice(n_docs, n, replace=False)).astype(np.int64) + 1
    return np.arange(n_docs // 2 + 1, n_docs // 2 + 1 + int(how), dtype=np.int64)


def reduced_index(idx, pids, build_ivf):
    gone = np.zeros(idx["doclens"].size, dtype=bool)
    gone[pids - 1] = True
    keep = np.repeat(~gone, idx["doclens"])
    r = dict(idx)
    r["codes"] = np.ascontiguousarray(idx["codes"][keep])
    r["residuals"] = np.asfortranarray(idx["residuals"][:, keep])
    r["doclens"] = np.where(gone, 0, idx["doclens"]).astype(np.int64)
    r["ivf"], r["ivf_lengths"] = build_ivf(r["codes"], idx["ivf_lengths"].size)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="passages resident before the removal")
    ap.add_argument("--remove", nargs="+", default=["1", "1%", "50%"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="the library the rebuild is timed with (default: this build)")
    ap.add_argument("--baseline-timeout", type=float, default=900.0, help="seconds the child process may take: a hang in it ends the run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove.json"))
    ap.add_argument("--rebuild-only", action="store_true", help="(the child process) time Searcher(index=reduced) only")
    args = ap.parse_args()
    child = None            # first of all: the child starts before this process has touched the GPU
    if args.baseline_lib and not args.rebuild_only:
        env = dict(os.environ, COLBERT_HIP_LIB=os.path.abspath(args.baseline_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--rebuild-only", "--docs", str(args.docs), "--baseline-reps",
               str(args.baseline_reps), "--remove"] + list(args.remove)
        done = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=args.baseline_timeout)
        child = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("REBUILD ")][-1][len("REBUILD "):])

    import colbert_jl_amd as clb
    from colbert_jl_amd import codec, synthetic
    from colbert_jl_amd._lib import LIB_PATH, check
    l = clb.lib()
    if l.clb_device_count() < 1:
        sys.exit("bench_remove: no GPU")

    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8), ivf_on_device=True)   # bench.py's corpus
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=32, T=32)

    def timed(fn):
        check(l.clb_device_synchronize(0))
        t0 = time.perf_counter()
        out = fn()
        check(l.clb_device_synchronize(0))
        return (time.perf_counter() - t0) * 1e3, out

    if args.rebuild_only:
        out = {}
        for how in args.remove:
            red = reduced_index(idx, removed_pids(args.docs, how), codec.build_ivf)
            ms = []
            for _ in range(args.baseline_reps):
                t, f = timed(lambda: clb.Searcher(index=red, device=0))
                f.close()
                ms.append(t)
            out[how] = ms
        print("REBUILD " + json.dumps({"lib": LIB_PATH, "ms": out}), flush=True)
        return

    rows = []
    for how in args.remove:
        pids = removed_pids(args.docs, how)
        red = reduced_index(idx, pids, codec.build_ivf)
        t_remove, same = [], None
        for rep in range(args.reps):
            s = clb.Searcher(index=idx, device=0)
            s.search_batch(Q, 1000)                     # a served handle: its workspaces are sized
            ms, n = timed(lambda: s.remove_passages(pids))
            assert n == pids.size
            t_remove.append(ms)
            if rep == 0:                                # the two routes must agree before their times are compared
                got = s.search_batch(Q, 1000, pad_short=True)
                f = clb.Searcher(index=red, device=0)
                want = f.search_batch(Q, 1000, pad_short=True)
                f.close()
                same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))
                assert same, "reduced and rebuilt handles disagree"
            s.close()
        if child is not None:
            t_rebuild = child["ms"][how]
        else:
            t_rebuild = []
            for _ in range(args.baseline_reps):
                ms, f = timed(lambda: clb.Searcher(index=red, device=0))
                f.close()
                t_rebuild.append(ms)
        a, r = statistics.median(t_remove), statistics.median(t_rebuild)
        rows.append({"resident_passages": args.docs, "resident_embeddings": int(idx["codes"].size), "removed": how,
                     "removed_passages": int(pids.size), "embeddings_left": int(red["codes"].size), "remove_ms": t_remove,
                     "rebuild_ms": t_rebuild, "remove_ms_median": a, "rebuild_ms_median": r, "rebuild_ms_min": min(t_rebuild),
                     "rebuild_ms_max": max(t_rebuild), "results_identical": same})
        print(f"| {how} | {pids.size} | {a:.0f} | {r:.0f} | {min(t_rebuild):.0f}-{max(t_rebuild):.0f} | {r / a:.1f} |", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"K": K, "reps": args.reps, "baseline_lib": child["lib"] if child else LIB_PATH, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
