#!/usr/bin/env python3
"""Dense MaxSim by passage id (`codec.maxsim_batch_device(pids=, store_offsets=)`) against the route it replaces, at the re-ranking
shape of profiles/maxsim_batch.md: B = 32 queries x `--per-query` (1 000) listed passages, doclens N(80, 20), dim 128, T = 32,
owned form, the passages drawn from a resident store of `--store-passages` (1 000 000) so that their rows are cold.  Per
`--dtypes` format (float16, int8, mxfp4, binary), three sides on the same lists:

  listed    the listed call: rows read where they lie in the store;
  gather    the replaced route: row numbers from the two offset arrays, a device gather of rows and scales into contiguous
            tensors (torch), then the contiguous call;
  gathered  the contiguous call alone on rows gathered beforehand: listed - gathered is what indirect addressing costs.

`--lists` different pid lists are cycled through the calls of a window, so a call does not find its rows in the caches its
predecessor filled.  HIP events around `--steps` calls; `--rounds` windows per side, interleaved with the order rotating; medians,
every window and the spread are written.  The listed scores are compared bit for bit with the gathered ones at the timed size.
Writes one JSON file; profiles/maxsim_store.md is written from it by hand.  A measurement path only: it fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--per-query", type=int, default=1000)
    ap.add_argument("--store-passages", type=int, default=1_000_000)
    ap.add_argument("--dtypes", default="float16,int8,mxfp4")
    ap.add_argument("--lists", type=int, default=8)
    ap.add_argument("--steps", type=int, default=24, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "maxsim_store.json"))
    args = ap.parse_args()
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import codec
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_maxsim_store: no GPU")
    dim, T, B, P, N = 128, 32, args.batch, args.store_passages, args.batch * args.per_query
    rng = np.random.default_rng(2025)
    lens = np.clip(np.rint(rng.normal(80, 20, size=P)), 8, 180).astype(np.int64)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
    rows = int(off[-1])
    q = torch.nn.functional.normalize(torch.randn(B, T, dim, device="cuda"), dim=-1)
    owner = torch.arange(B, dtype=torch.int32, device="cuda").repeat_interleave(args.per_query)
    pids = [torch.from_numpy(rng.integers(0, P, size=N)).cuda() for _ in range(args.lists)]
    result = {"tool": "tools/bench_maxsim_store.py", "device": torch.cuda.get_device_name(0), "dim": dim, "T": T, "B": B, "entries": N,
              "store_passages": P, "store_rows": rows, "lists": args.lists, "steps_per_window": args.steps, "formats": {}}

    def row_numbers(pid):
        """the store rows of the listed passages, back to back, and their doclens: what the gather route builds per call"""
        start, n = off[pid], off[pid + 1] - off[pid]
        first = torch.cumsum(n, 0) - n                                   # where each passage begins in the gathered tensor
        return torch.repeat_interleave(start - first, n) + torch.arange(int(n.sum()), device="cuda"), n

    for dtype in args.dtypes.split(","):
        torch.manual_seed(7)
        chunks = [torch.nn.functional.normalize(torch.randn(min(1 << 22, rows - a), dim, device="cuda"), dim=-1) for a in range(0, rows, 1 << 22)] \
            if dtype == "float16" else None
        if dtype == "float16":
            store, scale = torch.cat([c.half() for c in chunks]), None
        else:                                                            # quantised chunk by chunk: the fp32 store is never whole
            quant = {"int8": codec.quantize_rows_device, "binary": codec.binarize_rows_device}.get(dtype) or (lambda x: codec.quantize_mx_device(x, dtype))
            parts = [quant(torch.nn.functional.normalize(torch.randn(min(1 << 22, rows - a), dim, device="cuda"), dim=-1))
                     for a in range(0, rows, 1 << 22)]
            store, scale = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            del parts
        del chunks
        d_type = {"float16": 1, "int8": 3, "mxfp4": 5, "binary": 16}[dtype]
        out = [torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(3)]
        work = torch.empty(int(clb.lib().clb_maxsim_store_work_bytes(N, B, T, dim, d_type)), dtype=torch.uint8, device="cuda")
        work_c = torch.empty(int(max(clb.lib().clb_maxsim_batch_half_work_bytes(N, B, T, dim), clb.lib().clb_maxsim_batch_i8_work_bytes(N, B, T, dim),
                                     clb.lib().clb_maxsim_batch_mx_work_bytes(N, B, T, dim), clb.lib().clb_maxsim_batch_b1_work_bytes(N, B, T, dim))),
                             dtype=torch.uint8, device="cuda")
        ready = []
        for pid in pids:                                                 # the gathered side's operands, made once
            r, n = row_numbers(pid)
            ready.append((store[r], None if scale is None else scale[r], n))

        def listed(i):
            return codec.maxsim_batch_device(q, store, None, owner=owner, out=out[0], work=work, d_scale=scale, pids=pids[i], store_offsets=off)

        def gather(i):
            r, n = row_numbers(pids[i])
            return codec.maxsim_batch_device(q, store[r], n, owner=owner, out=out[1], work=work_c, d_scale=None if scale is None else scale[r])

        def gathered(i):
            d, s, n = ready[i]
            return codec.maxsim_batch_device(q, d, n, owner=owner, out=out[2], work=work_c, d_scale=s)

        sides = {"listed": listed, "gather": gather, "gathered": gathered}
        a, b, c = (f(0).cpu().numpy().view(np.uint32) for f in (listed, gather, gathered))
        assert np.array_equal(a, c) and np.array_equal(b, c), dtype     # the three routes agree bit for bit at the timed size

        def window(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.steps):
                call(k % args.lists)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps

        names = list(sides)
        for n in names:
            for k in range(args.warmup):
                sides[n](k % args.lists)
        ms = {n: [] for n in names}
        for r in range(args.rounds):
            for n in names[r % 3:] + names[:r % 3]:
                ms[n].append(window(sides[n]))
        listed_rows = int(sum(int(x[2].sum()) for x in ready) / args.lists)
        row_bytes = store.shape[1] * store.element_size() + (0 if scale is None else scale.numel() // rows * scale.element_size())
        med = {n: float(np.median(v)) for n, v in ms.items()}
        result["formats"][dtype] = {
            "sides": {n: {"ms": round(med[n], 5), "windows_ms": [round(x, 5) for x in v], "spread_ms": round(max(v) - min(v), 5)} for n, v in ms.items()},
            "rows_per_call": listed_rows, "row_bytes": row_bytes, "listed_gb_s": round(listed_rows * row_bytes / med["listed"] / 1e6, 1),
            "gather_over_listed": round(med["gather"] / med["listed"], 3), "listed_over_gathered": round(med["listed"] / med["gathered"], 3)}
        del store, scale, ready
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
