#!/usr/bin/env python3
"""Replacing passages of a resident index in place against the two routes a caller had before, on the headline corpus of
bench.py (synthetic 1 M passages): wall time of `Searcher.update_compressed` of 1 000 and of 10 000 passages of a resident
1 M-passage Searcher, beside `remove_passages` + `add_compressed` of the same passages and content on a handle of the same
kind in the same run (the old workaround: the new versions get new pids), and beside `Searcher(index=updated)` on the updated
host arrays with their IVF already computed (the host-side splice and IVF rebuild that route also needs are NOT in its figure).

Every named passage gets the content of another passage of the corpus (its length changes with it).  Every figure is a host
clock around work that ends in clb_device_synchronize, on a handle that has served a search.  Before the times are compared
the updated handle must answer bit for bit as the rebuilt one.  Writes one JSON file (default profiles/update.json) and prints
the table of profiles/update.md.

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


def columns_of(idx, pids):
    """(codes, residuals, doclens) of the passages `pids` (1-based), one after another"""
    off = np.concatenate([[0], np.cumsum(idx["doclens"])])
    lens = idx["doclens"][pids - 1].astype(np.int64)
    start = np.repeat(off[pids - 1], lens)
    rank = np.arange(int(lens.sum())) - np.repeat(np.concatenate([[0], np.cumsum(lens)])[:-1], lens)
    cols = start + rank
    return np.ascontiguousarray(idx["codes"][cols]), np.asfortranarray(idx["residuals"][:, cols]), lens


def updated_index(idx, pids, codes, residuals, doclens, build_ivf):
    """idx with the columns of the passages `pids` (ascending) replaced"""
    off = np.concatenate([[0], np.cumsum(idx["doclens"])])
    new_off = np.concatenate([[0], np.cumsum(doclens)])
    dl = idx["doclens"].astype(np.int64).copy()
    dl[pids - 1] = doclens
    slot = np.full(dl.size, -1, dtype=np.int64)
    slot[pids - 1] = np.arange(pids.size)
    first = np.where(slot >= 0, -1 - new_off[np.maximum(slot, 0)], off[:-1])       # < 0: -1 - the new column
    start = np.repeat(first, dl)
    rank = np.arange(int(dl.sum())) - np.repeat(np.concatenate([[0], np.cumsum(dl)])[:-1], dl)
    new = start < 0
    col = np.where(new, -1 - start, start) + rank
    u = dict(idx)
    u["codes"] = np.where(new, codes[np.where(new, col, 0)], idx["codes"][np.where(new, 0, col)]).astype(idx["codes"].dtype)
    res = np.empty((idx["residuals"].shape[0], col.size), dtype=np.uint8, order="F")
    res[:, new] = residuals[:, col[new]]
    res[:, ~new] = idx["residuals"][:, col[~new]]
    u["residuals"], u["doclens"] = res, dl
    u["ivf"], u["ivf_lengths"] = build_ivf(u["codes"], idx["ivf_lengths"].size)
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="passages resident before the update")
    ap.add_argument("--update", nargs="+", type=int, default=[1_000, 10_000], help="passages replaced per case")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update.json"))
    args = ap.parse_args()

    import colbert_jl_amd as clb
    from colbert_jl_amd import codec, synthetic
    from colbert_jl_amd._lib import check
    l = clb.lib()
    if l.clb_device_count() < 1:
        sys.exit("bench_update: no GPU")

    K = synthetic.num_partitions_for(args.docs, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=args.docs, K=K, n_blocks=8, blocks=range(8), ivf_on_device=True)   # bench.py's corpus
    Q = synthetic.make_topic_queries(idx["centroids"], seed=77, n_queries=32, T=32)
    print(f"corpus: {args.docs} passages, {idx['codes'].size} embeddings, K = {K}", file=sys.stderr, flush=True)

    def timed(fn):
        check(l.clb_device_synchronize(0))
        t0 = time.perf_counter()
        out = fn()
        check(l.clb_device_synchronize(0))
        return (time.perf_counter() - t0) * 1e3, out

    def served():
        s = clb.Searcher(index=idx, device=0)
        s.search_batch(Q, 1000)                         # a served handle: its workspaces are sized
        return s

    rows = []
    for n in args.update:
        rng = np.random.default_rng(5)
        pids = np.sort(rng.choice(args.docs, n, replace=False)).astype(np.int64) + 1
        co, re, dl = columns_of(idx, rng.choice(args.docs, n, replace=False).astype(np.int64) + 1)
        upd = updated_index(idx, pids, co, re, dl, codec.build_ivf)
        print(f"case {n}: {co.size} new rows, {upd['codes'].size} embeddings afterwards", file=sys.stderr, flush=True)
        t_update, t_remove, t_append, same = [], [], [], None
        for rep in range(args.reps):
            s = served()
            ms, changed = timed(lambda: s.update_compressed(pids, co, re, dl))
            assert changed == n
            t_update.append(ms)
            if rep == 0:                                # the two routes must agree before their times are compared
                got = s.search_batch(Q, 1000, pad_short=True)
                f = clb.Searcher(index=upd, device=0)
                want = f.search_batch(Q, 1000, pad_short=True)
                f.close()
                same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))
                assert same, "updated and rebuilt handles disagree"
            s.close()
            s = served()
            ms, _ = timed(lambda: s.remove_passages(pids))
            t_remove.append(ms)
            ms, _ = timed(lambda: s.add_compressed(co, re, dl))
            t_append.append(ms)
            s.close()
        t_rebuild = []
        for _ in range(args.rebuild_reps):
            ms, f = timed(lambda: clb.Searcher(index=upd, device=0))
            f.close()
            t_rebuild.append(ms)
        u, ra, r = statistics.median(t_update), statistics.median([a + b for a, b in zip(t_remove, t_append)]), statistics.median(t_rebuild)
        rows.append({"resident_passages": args.docs, "resident_embeddings": int(idx["codes"].size), "updated_passages": n,
                     "new_embeddings": int(co.size), "embeddings_after": int(upd["codes"].size), "update_ms": t_update,
                     "remove_ms": t_remove, "append_ms": t_append, "rebuild_ms": t_rebuild, "update_ms_median": u,
                     "remove_plus_append_ms_median": ra, "rebuild_ms_median": r, "results_identical": same})
        print(f"| {n} | {co.size} | {u:.0f} | {ra:.0f} | {statistics.median(t_remove):.0f} + {statistics.median(t_append):.0f} | "
              f"{r:.0f} | {ra / u:.2f} | {r / u:.1f} |", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"K": K, "reps": args.reps, "rebuild_reps": args.rebuild_reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
