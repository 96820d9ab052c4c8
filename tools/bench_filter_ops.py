#!/usr/bin/env python3
"""Composing filters on the device against the route it replaces, on the headline corpus of bench.py (synthetic 1 M passages):
wall time of

  a & b                        against  make_filter(mask=ma & mb)
  ~a                           against  make_filter(mask=~ma)
  combine_filters("or", 8)     against  make_filter(mask=np.logical_or.reduce(masks))
  make_range_filter(p, lo, hi) against  make_filter(mask=(v >= lo) & (v <= hi))
  to_mask()                    (the host route keeps its own copy of every mask instead: nothing to time beside it)

Both sides run on this build, in this process; every call synchronises (the count is read back), so the host's clock is the
measure, and closing the filter that was made is timed with making it on both sides.  `--reps` repetitions per side,
interleaved device / host / device / ...; the median is reported with the fastest and the slowest repetition.  The masks have
density 0.5 (0.1 each for the 8-way union), the attribute is uniform on [0, 1) with the range [0.3, 0.9].

Writes profiles/filter_ops.md (and the raw numbers beside it as JSON on stdout).  A measurement path only: it needs a GPU and
fails without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--doclen", type=float, default=80.0, help="mean passage length of the corpus (a filter's cost depends on --docs alone)")
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "filter_ops.md"))
    args = ap.parse_args()

    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import synthetic
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_filter_ops: no GPU")
    n = args.docs
    K = synthetic.num_partitions_for(n, 80.0)
    idx = synthetic.make_index(seed=2024, n_docs=n, K=K, n_blocks=8, blocks=range(8), doclen_mean=args.doclen,
                               doclen_std=args.doclen / 5)
    s = clb.Searcher(index=idx, device=0)
    rng = np.random.default_rng(5)
    ma, mb = rng.random(n) < 0.5, rng.random(n) < 0.5
    m8 = [rng.random(n) < 0.1 for _ in range(8)]
    v = rng.uniform(0, 1, n).astype(np.float32)
    lo, hi = np.float32(0.3), np.float32(0.9)
    a, b, f8, p = s.make_filter(mask=ma), s.make_filter(mask=mb), [s.make_filter(mask=m) for m in m8], s.make_prior(v)

    def host(make_mask):
        return lambda: s.make_filter(mask=make_mask()).close()
    ops = {
        "a & b": (lambda: (a & b).close(), host(lambda: ma & mb)),
        "~a": (lambda: (~a).close(), host(lambda: ~ma)),
        "8-way or": (lambda: s.combine_filters("or", f8).close(), host(lambda: np.logical_or.reduce(m8))),
        "range": (lambda: s.make_range_filter(p, lo, hi).close(), host(lambda: (v >= lo) & (v <= hi))),
        "to_mask": (lambda: a.to_mask(), None),
    }
    # the sides agree before anything is timed
    with a & b as x, ~a as y, s.combine_filters("or", f8) as z, s.make_range_filter(p, lo, hi) as r:
        assert np.array_equal(x.to_mask(), ma & mb) and np.array_equal(y.to_mask(), ~ma)
        assert np.array_equal(z.to_mask(), np.logical_or.reduce(m8)) and np.array_equal(r.to_mask(), (v >= lo) & (v <= hi))
    ms = {name: {"device": [], "host": []} for name in ops}
    for name, (dev, hst) in ops.items():
        for _ in range(args.warmup):
            dev()
            if hst:
                hst()
        for _ in range(args.reps):
            ms[name]["device"].append(timed(dev))
            if hst:
                ms[name]["host"].append(timed(hst))

    def stat(x):
        return None if not x else {"median_ms": round(float(np.median(x)), 4), "min_ms": round(min(x), 4), "max_ms": round(max(x), 4)}
    out = {"tool": "tools/bench_filter_ops.py", "device": torch.cuda.get_device_name(0), "docs": n, "doclen_mean": args.doclen,
           "reps": args.reps, "ops": {name: {side: stat(x) for side, x in d.items()} for name, d in ms.items()}}
    print(json.dumps(out), flush=True)

    def cell(st):
        return "—" if st is None else f"{st['median_ms']:.3f} ({st['min_ms']:.3f} … {st['max_ms']:.3f})"
    lines = ["# Composing filters on the device against numpy + `make_filter(mask=…)`", "",
             f"`tools/bench_filter_ops.py` on {out['device']}: synthetic corpus of {n:,} passages (mean length {args.doclen:g}), wall time per call in",
             f"ms by the host's clock, making and closing one filter; median of {args.reps} interleaved repetitions (fastest … slowest).",
             "Both sides on the same build and handle.  Masks of density 0.5 (0.1 each for the 8-way union); attribute uniform on",
             "[0, 1), range [0.3, 0.9].", "",
             "| operation | on the device | numpy on host masks + `make_filter(mask=…)` | host / device |", "|---|---|---|---|"]
    for name, d in out["ops"].items():
        ratio = "—" if d["host"] is None else f"{d['host']['median_ms'] / d['device']['median_ms']:.1f}×"
        lines.append(f"| `{name}` | {cell(d['device'])} | {cell(d['host'])} | {ratio} |")
    lines += ["", "`to_mask` has no host counterpart: the host route keeps a copy of every mask instead of reading one back.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    for x in [a, b, p] + f8:
        x.close()
    s.close()


if __name__ == "__main__":
    main()
