#!/usr/bin/env python3
"""Appending to a resident index against rebuilding it, on the headline corpus of bench.py (synthetic 1 M passages): wall
time of `Searcher.add_compressed` of 1 000 and of 10 000 passages onto a resident 1 M-passage Searcher, beside the wall
time of `Searcher(index=full)` on the concatenated index -- the route a caller had to take before (host arrays with the
full IVF already computed: the host-side concatenation and IVF rebuild that route also needs are NOT in its figure).
Same process, same card; every figure is the median of --reps runs of a host clock around work that ends in
clb_device_synchronize.  Writes one JSON file (default profiles/append.json) and prints the table of profiles/append.md.

A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="passages resident before the append")
    ap.add_argument("--append", type=int, nargs="+", default=[1_000, 10_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append.json"))
    args = ap.parse_args()
    import colbert_jl_amd as clb
    from colbert_jl_amd import codec, synthetic
    from colbert_jl_amd._lib import check
    l = clb.lib()
    if l.clb_device_count() < 1:
        sys.exit("bench_append: no GPU")

    extra = max(args.append)
    K = synthetic.num_partitions_for(args.docs, 80.0)
    # head and tail are generated separately (own RNG streams): the head is bench.py's corpus, passage for passage
    head = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8), ivf_on_device=True)
    more = synthetic.make_index(seed=2025, n_docs=extra, K=K, ivf_on_device=True)
    more_off = np.concatenate([[0], np.cumsum(more["doclens"])])
    n_head = int(head["codes"].size)
    Q = synthetic.make_topic_queries(head["centroids"], seed=77, n_queries=32, T=32)

    def timed(fn):
        check(l.clb_device_synchronize(0))
        t0 = time.perf_counter()
        out = fn()
        check(l.clb_device_synchronize(0))
        return (time.perf_counter() - t0) * 1e3, out

    rows = []
    for n_add in args.append:
        n = int(more_off[n_add])
        tail = (more["codes"][:n], np.asfortranarray(more["residuals"][:, :n]), more["doclens"][:n_add])
        full = dict(head)
        full["codes"] = np.concatenate([head["codes"], tail[0]])
        full["residuals"] = np.asfortranarray(np.concatenate([head["residuals"], tail[1]], axis=1))
        full["doclens"] = np.concatenate([head["doclens"], tail[2]])
        full["ivf"], full["ivf_lengths"] = codec.build_ivf(full["codes"], K)
        t_append, t_rebuild, same = [], [], None
        for rep in range(args.reps):
            s = clb.Searcher(index=head, device=0)
            s.search_batch(Q, 1000)                     # a served handle: its workspaces are sized
            ms, new = timed(lambda: s.add_compressed(*tail))
            assert new == range(args.docs + 1, args.docs + n_add + 1)
            t_append.append(ms)
            got = s.search_batch(Q, 1000) if rep == 0 else None
            s.close()
            ms, f = timed(lambda: clb.Searcher(index=full, device=0))
            t_rebuild.append(ms)
            if rep == 0:                                # the two routes must agree before their times are compared
                want = f.search_batch(Q, 1000)
                same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))
                assert same, "appended and rebuilt handles disagree"
            f.close()
        a, r = statistics.median(t_append), statistics.median(t_rebuild)
        rows.append({"resident_passages": args.docs, "resident_embeddings": n_head, "appended_passages": n_add,
                     "appended_embeddings": n, "append_ms": t_append, "rebuild_ms": t_rebuild, "append_ms_median": a,
                     "rebuild_ms_median": r, "rebuild_over_append": r / a, "results_identical": same})
        print(f"| {n_add} | {a:.0f} | {r:.0f} | {r / a:.1f} |", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"K": K, "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
