#!/usr/bin/env python3
"""Dense MaxSim of un-indexed passages (`codec.maxsim_batch_device`) at dim 128, T = 32, two shapes:

  rerank   B = 32 queries, `--per-query` (1 000) passages of ~80 embeddings each per query, owned form;
  pairs    B = 32 queries against `--pairs-passages` (4 096) passages, all-pairs form.

For each: the device call on resident tensors (HIP events around `--steps` calls), and the same work through the route it
replaces on this same build -- `codec.maxsim` once per query from host arrays (host clock: every call uploads and waits).
`--rounds` windows per side, interleaved with the order rotating; medians reported, every window kept, spread stated.
Rates: the bytes the call must read (D, Q, doclens, owners) over its time against `clb_measure_read_rate` taken in the
same run, and 2 dim T rows (x B for pairs) flop over its time against `--mfma-f32-tflops` (what
tools/microbench/mfma_f32_peak.hip printed on the same machine).  Writes one JSON file; profiles/maxsim_batch.md is
written from it by hand.  `--dtype float16 | bfloat16`: the 16-bit kernel (embeddings stored in 16 bits, fp32 queries rounded
on the device) beside the fp32 kernel on the same values, the two interleaved in the same windows; the per-query host route
is left out, the 16-bit bytes and `--mfma-16bit-tflops` (if given) make the rates, and the largest error / bound against the
fp32 call's scores is reported (profiles/maxsim_batch_half.md).  `--dtype int8`: the integer kernel (embeddings stored as int8
with one scale each by `quantize_rows_device`, fp32 queries quantised in the call) beside the fp32 AND the float16 kernel on the
same values, all three interleaved in the same windows; its bytes make the read-rate fraction, and the largest and median
|int8 score - fp32 score| are reported, not asserted: they are the format's (profiles/maxsim_batch_int8.md).  `--dtype mxfp8 |
mxfp4`: the scaled-MFMA kernel (passages quantised by `quantize_mx_device`, fp32 queries quantised to MXFP8 in the call) beside
the fp32, the float16 AND the int8 kernel, all four interleaved; the same figures (profiles/maxsim_batch_mx.md).  `--dtype binary`:
the 1-bit kernel (passages binarised by `binarize_rows_device`, fp32 queries quantised to int8 in the call) beside the fp32, float16,
int8 AND mxfp4 kernels, all five interleaved, with every quantised side's own bytes and share of the read rate
(profiles/maxsim_batch_b1.md).
A measurement path only: it needs a GPU and fails without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def unit(rng, dim, n):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def summary(v):
    return {"ms": round(float(np.median(v)), 5), "windows_ms": [round(x, 5) for x in v], "spread_ms": round(float(max(v) - min(v)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--per-query", type=int, default=1000)
    ap.add_argument("--pairs-passages", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50, help="device calls per timed window")
    ap.add_argument("--old-steps", type=int, default=1, help="passes of the per-query route per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mfma-f32-tflops", type=float, default=None)
    ap.add_argument("--dtype", choices=["float32", "float16", "bfloat16", "int8", "mxfp8", "mxfp4", "binary"], default="float32")
    ap.add_argument("--mfma-16bit-tflops", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    half = args.dtype != "float32"
    args.out = args.out or os.path.join(HERE, "profiles", f"maxsim_batch_{args.dtype}.json" if half else "maxsim_batch.json")
    import torch
    import colbert_jl_amd as clb
    from colbert_jl_amd import codec
    from colbert_jl_amd._lib import measure_read_rate
    if clb.lib().clb_device_count() < 1:
        sys.exit("bench_maxsim_batch: no GPU")
    dim, T, B = 128, 32, args.batch
    rng = np.random.default_rng(2025)
    Q = unit(rng, dim, T * B).reshape(B, T, dim)
    shapes = {}
    for name, N in (("rerank", B * args.per_query), ("pairs", args.pairs_passages)):
        dl = np.clip(np.rint(rng.normal(80, 20, size=N)), 8, 180).astype(np.int64)
        D = unit(rng, dim, int(dl.sum()))
        owner = np.repeat(np.arange(B, dtype=np.int32), args.per_query) if name == "rerank" else None
        shapes[name] = (dl, D, owner)

    sides, work_of = {}, {}
    for name, (dl, D, owner) in shapes.items():
        N, rows = dl.size, int(dl.sum())
        d_Q, d_D, d_l = torch.from_numpy(Q).cuda(), torch.from_numpy(D).cuda(), torch.from_numpy(dl).cuda()
        d_o = None if owner is None else torch.from_numpy(owner).cuda()
        out = torch.empty(N if owner is not None else (B, N), dtype=torch.float32, device="cuda")
        work = torch.empty(int(clb.lib().clb_maxsim_batch_work_bytes(N, B, T)), dtype=torch.uint8, device="cuda")
        sides[name + "_device"] = (lambda d_Q=d_Q, d_D=d_D, d_l=d_l, d_o=d_o, out=out, work=work:
                                   codec.maxsim_batch_device(d_Q, d_D, d_l, owner=d_o, out=out, work=work))
        flop = 2.0 * dim * T * rows * (1 if owner is not None else B)
        mx, b1 = args.dtype in ("mxfp8", "mxfp4"), args.dtype == "binary"
        if args.dtype == "int8" or mx or b1:                 # the same values as int8 + scales, and in fp16: each its own out and work
            d_Dh, out_h, out_8 = d_D.to(torch.float16), torch.empty_like(out), torch.empty_like(out)
            d_D8, d_ds = codec.quantize_rows_device(d_D)
            work_h = torch.empty(int(clb.lib().clb_maxsim_batch_half_work_bytes(N, B, T, dim)), dtype=torch.uint8, device="cuda")
            work_8 = torch.empty(int(clb.lib().clb_maxsim_batch_i8_work_bytes(N, B, T, dim)), dtype=torch.uint8, device="cuda")
            sides[name + "_float16_device"] = (lambda d_Q=d_Q, d_Dh=d_Dh, d_l=d_l, d_o=d_o, out_h=out_h, work_h=work_h:
                                               codec.maxsim_batch_device(d_Q, d_Dh, d_l, owner=d_o, out=out_h, work=work_h))
            sides[name + "_int8_device"] = (lambda d_Q=d_Q, d_D8=d_D8, d_ds=d_ds, d_l=d_l, d_o=d_o, out_8=out_8, work_8=work_8:
                                            codec.maxsim_batch_device(d_Q, d_D8, d_l, owner=d_o, out=out_8, work=work_8, d_scale=d_ds))
            rest = 4.0 * Q.size + 8.0 * N + (4.0 * N if owner is not None else 0)
            byts = 1.0 * dim * rows + 4.0 * rows + rest
            side_bytes = {"int8": byts}
            if mx or b1:                               # the same values as an MX pair: its own out and work
                fmt = "mxfp4" if b1 else args.dtype
                (d_Dm, d_dm), out_m = codec.quantize_mx_device(d_D, fmt), torch.empty_like(out)
                work_m = torch.empty(int(clb.lib().clb_maxsim_batch_mx_work_bytes(N, B, T, dim)), dtype=torch.uint8, device="cuda")
                sides[name + "_" + fmt + "_device"] = (lambda d_Q=d_Q, d_Dm=d_Dm, d_dm=d_dm, d_l=d_l, d_o=d_o, out_m=out_m, work_m=work_m:
                                                       codec.maxsim_batch_device(d_Q, d_Dm, d_l, owner=d_o, out=out_m, work=work_m, d_scale=d_dm))
                byts = side_bytes[fmt] = 1.0 * d_Dm.numel() + d_dm.numel() + rest
            if b1:                                     # the same values as sign bits + scales: its own out and work
                (d_Db, d_db), out_b = codec.binarize_rows_device(d_D), torch.empty_like(out)
                work_b = torch.empty(int(clb.lib().clb_maxsim_batch_b1_work_bytes(N, B, T, dim)), dtype=torch.uint8, device="cuda")
                sides[name + "_binary_device"] = (lambda d_Q=d_Q, d_Db=d_Db, d_db=d_db, d_l=d_l, d_o=d_o, out_b=out_b, work_b=work_b:
                                                  codec.maxsim_batch_device(d_Q, d_Db, d_l, owner=d_o, out=out_b, work=work_b, d_scale=d_db))
                byts = side_bytes["binary"] = 1.0 * d_Db.numel() + 4.0 * d_db.numel() + rest
            diff = np.abs(sides[name + "_" + args.dtype + "_device"]().cpu().numpy().astype(np.float64) - sides[name + "_device"]().cpu().numpy())
            work_of[name] = {"passages": N, "embeddings": rows, "flop": flop, "bytes": byts,
                             "max_abs_difference_from_fp32": float(diff.max()), "median_abs_difference_from_fp32": float(np.median(diff))}
            if b1:
                work_of[name]["side_bytes"] = side_bytes
            continue
        if half:                                       # the same values stored in 16 bits; its own out and work
            d_Dh, out_h = d_D.to(getattr(torch, args.dtype)), torch.empty_like(out)
            work_h = torch.empty(int(clb.lib().clb_maxsim_batch_half_work_bytes(N, B, T, dim)), dtype=torch.uint8, device="cuda")
            sides[name + "_" + args.dtype + "_device"] = (lambda d_Q=d_Q, d_Dh=d_Dh, d_l=d_l, d_o=d_o, out_h=out_h, work_h=work_h:
                                                     codec.maxsim_batch_device(d_Q, d_Dh, d_l, owner=d_o, out=out_h, work=work_h))
            got, want = sides[name + "_" + args.dtype + "_device"]().cpu().numpy(), sides[name + "_device"]().cpu().numpy()
            eps = 2.0 ** (-11 if args.dtype == "float16" else -8)      # unit-norm operands: each dot moves by at most 2 eps + eps^2
            byts = 2.0 * dim * rows + 4.0 * Q.size + 8.0 * N + (4.0 * N if owner is not None else 0)
            work_of[name] = {"passages": N, "embeddings": rows, "flop": flop, "bytes": byts,
                             "max_abs_difference_from_fp32": float(np.abs(got - want).max()),
                             "operand_rounding_bound": T * (2 * eps + eps * eps)}
            assert work_of[name]["max_abs_difference_from_fp32"] <= work_of[name]["operand_rounding_bound"], name
            continue
        Qh = [np.asfortranarray(Q[b].T) for b in range(B)]
        Dh = np.asfortranarray(D.T)
        pids = np.arange(1, N + 1)
        if owner is not None:                          # every query's own passages: a slice of D and of the doclens
            off = np.concatenate([[0], np.cumsum(dl)])
            cut = [(b * args.per_query, (b + 1) * args.per_query) for b in range(B)]
            parts = [(np.asfortranarray(Dh[:, off[a]:off[z]]), dl[a:z], np.arange(1, z - a + 1)) for a, z in cut]
            old = lambda Qh=Qh, parts=parts: np.concatenate([codec.maxsim(Qh[b], *parts[b][::2], parts[b][1]) for b in range(B)])     # noqa: E731
        else:
            old = lambda Qh=Qh, Dh=Dh, pids=pids, dl=dl: np.stack([codec.maxsim(Qh[b], Dh, pids, dl) for b in range(B)])            # noqa: E731
        sides[name + "_per_query_host"] = old
        got, want = sides[name + "_device"]().cpu().numpy(), old()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name      # the two routes agree bit for bit at the timed size
        byts = 4.0 * dim * rows + 4.0 * Q.size + 8.0 * N + (4.0 * N if owner is not None else 0)
        work_of[name] = {"passages": N, "embeddings": rows, "flop": flop, "bytes": byts}

    def device_window(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def host_window(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.old_steps):
            call()
        return (time.perf_counter() - t0) * 1e3 / args.old_steps

    names = list(sides)
    for n in names:
        for _ in range(args.warmup if n.endswith("_device") else 1):
            sides[n]()
    torch.cuda.synchronize()
    read_gbs = measure_read_rate(0)
    ms = {n: [] for n in names}
    for r in range(args.rounds):
        rot = r % len(names)
        for n in names[rot:] + names[:rot]:
            ms[n].append((device_window if n.endswith("_device") else host_window)(sides[n]))
    out = {"tool": "tools/bench_maxsim_batch.py", "device": torch.cuda.get_device_name(0), "dtype": args.dtype, "dim": dim, "T": T, "B": B,
           "steps_per_window": args.steps, "read_rate_gb_s": round(read_gbs, 1), "mfma_f32_tflops": args.mfma_f32_tflops,
           "sides": {n: summary(ms[n]) for n in names}, "shapes": work_of}
    for name, w in work_of.items():
        t32 = out["sides"][name + "_device"]["ms"] * 1e-3
        t = out["sides"][name + "_" + args.dtype + "_device"]["ms"] * 1e-3 if half else t32
        w["device_gb_s"] = round(w["bytes"] / t / 1e9, 1)
        w["fraction_of_read_rate"] = round(w["bytes"] / t / 1e9 / read_gbs, 4)
        w["device_tflops"] = round(w["flop"] / t / 1e12, 2)
        if half:
            for side, sb in w.get("side_bytes", {}).items():      # every quantised side's own bytes over its own time
                w[side + "_fraction_of_read_rate"] = round(sb / (out["sides"][name + "_" + side + "_device"]["ms"] * 1e-3) / 1e9 / read_gbs, 4)
            if mx or b1:
                for other in ("float16", "int8") + (("mxfp4",) if b1 else ()):
                    w[other + "_over_" + args.dtype] = round(out["sides"][name + "_" + other + "_device"]["ms"] * 1e-3 / t, 3)
            elif args.dtype == "int8":
                w["float16_over_int8"] = round(out["sides"][name + "_float16_device"]["ms"] * 1e-3 / t, 3)
            elif args.mfma_16bit_tflops:
                w["fraction_of_mfma_16bit_rate"] = round(w["flop"] / t / 1e12 / args.mfma_16bit_tflops, 4)
            w["fp32_over_" + args.dtype] = round(t32 / t, 3)
            continue
        if args.mfma_f32_tflops:
            w["fraction_of_mfma_f32_rate"] = round(w["flop"] / t / 1e12 / args.mfma_f32_tflops, 4)
        w["per_query_host_over_device"] = round(out["sides"][name + "_per_query_host"]["ms"] / out["sides"][name + "_device"]["ms"], 1)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
