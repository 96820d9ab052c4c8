"""Dense MaxSim by passage id (codec.maxsim_batch_device(pids=, store_offsets=) -> clb_maxsim_store_device), all six formats: bit
for bit against float64 on operands whose every partial sum is exact in fp32, and bit for bit against the contiguous call on the
same rows gathered back to back.  No tolerance anywhere."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec
from tests.test_gpu_maxsim_batch_half import EDGES
from tests.test_gpu_maxsim_batch_mx import exact_pair, same

pytestmark = pytest.mark.gpu
FORMATS = ["float32", "float16", "bfloat16", "int8", "mxfp8", "mxfp4"]
# 60 stored passages: every tile and step edge, one empty, runs of one row, passages longer than a step; the last ends the store
LENS = np.array(EDGES + [0, 255, 256, 257, 7, 9] + list(range(2, 19)), np.int64)
OFF = np.concatenate([[0], np.cumsum(LENS)])
P, B = LENS.size, 3
_rng = np.random.default_rng(1)
# a permutation, a descending list, repeats under one owner and under two, a pid below and one past the store | 4200 entries
# drawn from the store and its two neighbours, so a work-group owns several entries and tiles straddle entries and owners
LISTS = [np.concatenate([_rng.permutation(P), np.arange(P)[::-1], [5, 5, 5, 5, -1, P]]), _rng.integers(-1, P + 1, size=4200)]
# runs of three entries per owner, query 1 owns nothing, one entry in 30 is owned by nobody
OWNERS = [np.where(_rng.random(l.size) < 1 / 30, _rng.choice([-1, B], l.size), np.arange(l.size) // 3 % 2 * 2).astype(np.int32) for l in LISTS]


def operand(fmt, rng, dim, shape, exact):
    """(values, scales or None, float64 decoded or None), embeddings last; exact: {0, +-0.5, +-1, +-2}, small integers under
    power-of-two scales (int8), such codes under scale bytes 125..130 (MX); else unit-norm rows quantised on the host"""
    if exact and fmt.startswith("mx"):
        v, s = exact_pair(rng, fmt, dim, shape)
        return v, s, codec.dequantize_mx(v, s, fmt).astype(np.float64)
    if exact and fmt == "int8":
        v, s = rng.integers(-3, 4, (dim,) + shape).astype(np.int8), np.ldexp(1.0, rng.integers(-2, 2, shape)).astype(np.float32)
        return v, s, v * s.astype(np.float64)
    x = rng.choice(np.float32([0, .5, -.5, 1, -1, 2, -2]), (dim,) + shape) if exact else rng.standard_normal((dim,) + shape)
    x = np.asfortranarray((x / (1 if exact else np.linalg.norm(x, axis=0))).astype(np.float32))
    return (*(codec.quantize_mx(x, fmt) if fmt.startswith("mx") else codec.quantize_rows(x) if fmt == "int8" else (x, None)), x.astype(np.float64))


def dev(a, fmt="float32"):                                       # embeddings first, on the device; floats in the format's 16-bit type
    import torch
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    return t.to(getattr(torch, fmt)) if fmt in ("float16", "bfloat16") and a.dtype == np.float32 else t


def score(q, qs, d, ds, fmt, own, qfmt=None, **kw):              # kw: d_doclens (contiguous) or pids (listed in the store)
    kw = dict(kw, d_doclens=None, pids=dev(kw["pids"]), store_offsets=dev(OFF)) if "pids" in kw else dict(kw, d_doclens=dev(kw["d_doclens"]))
    return codec.maxsim_batch_device(dev(q, qfmt or fmt), dev(d, fmt), owner=dev(own), d_scale=dev(ds), q_scale=dev(qs), **kw).cpu().numpy()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dim,T", [(128, 1), (128, 32), (128, 33), (64, 32), (96, 33)])
def test_every_entry_has_the_bits_of_float64(dim, T, fmt):
    rng = np.random.default_rng([dim, T, FORMATS.index(fmt)])
    (q, qs, Qd), (d, ds, Dd) = operand("mxfp8" if fmt.startswith("mx") else fmt, rng, dim, (T, B), True), operand(fmt, rng, dim, (int(OFF[-1]),), True)
    dots = np.einsum("ktb,kn->btn", Qd, Dd)                                   # exact: integers in units of 2^-6 far below 2^53
    m = np.stack([dots[:, :, a:z].max(axis=2, initial=-np.inf) for a, z in zip(OFF[:-1], OFF[1:])])   # (P, B, T)
    ref = np.zeros((P + 1, B + 1), np.float32) - np.inf                        # row P: no such passage; column B: no such query
    ref[:P, :B] = 0
    for t in range(T):
        ref[:P, :B] = ref[:P, :B] + m[:, :, t].astype(np.float32)             # acc = fl32(acc + m_t), t ascending: exact here
    assert np.isneginf(ref[:P, :B][LENS == 0]).all() and np.isfinite(ref[:P, :B][LENS > 0]).all()
    for pid, own in zip(LISTS, OWNERS):
        row, col = np.where((pid < 0) | (pid >= P), P, pid), np.where((own < 0) | (own >= B), B, own)
        same(score(q, qs, d, ds, fmt, None, pids=pid), ref[row, :B].T, "all pairs")
        same(score(q, qs, d, ds, fmt, own, pids=pid), ref[row, col], "owned")


_random = {}


def random_case(dim, T, fmt):
    if (dim, T, fmt) not in _random:
        rng = np.random.default_rng([dim, T, FORMATS.index(fmt), 7])
        _random[(dim, T, fmt)] = operand("mxfp8" if fmt.startswith("mx") else fmt, rng, dim, (T, B), False) + operand(fmt, rng, dim, (int(OFF[-1]),), False)
    return _random[(dim, T, fmt)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dim,T", [(128, 32), (96, 33)])
def test_same_bits_as_the_contiguous_call_on_the_gathered_rows(dim, T, fmt):
    q, qs, Q64, d, ds, _ = random_case(dim, T, fmt)
    for k, (pid, own) in enumerate(zip(LISTS, OWNERS)):
        ok = (pid >= 0) & (pid < P)
        rows = np.concatenate([np.arange(OFF[p], OFF[p + 1]) for p in pid[ok]])
        lens, gd, gds = np.where(ok, LENS[np.clip(pid, 0, P - 1)], 0), d[:, rows], None if ds is None else ds[..., rows]
        for qq, qqs, qfmt in ((q, qs, fmt), (Q64.astype(np.float32), None, "float32")):      # Q in its format; Q in fp32, converted in the call
            for o in (None, own):
                same(score(qq, qqs, d, ds, fmt, o, qfmt, pids=pid), score(qq, qqs, gd, gds, fmt, o, qfmt, d_doclens=lens),
                     f"list {k}, Q {qfmt}, {'owned' if o is not None else 'all pairs'}")


def test_preallocated_out_and_work_give_the_same_bits():
    import torch
    q, qs, Q64, d, ds, _ = random_case(128, 32, "int8")
    pid, own = LISTS[0], OWNERS[0]
    out = torch.empty(pid.size, dtype=torch.float32, device="cuda")
    work = torch.empty(int(clb.lib().clb_maxsim_store_work_bytes(pid.size, B, 32, 128, 3)), dtype=torch.uint8, device="cuda")
    score(Q64.astype(np.float32), None, d, ds, "int8", own, "float32", pids=pid, out=out, work=work)
    same(out.cpu().numpy(), score(Q64.astype(np.float32), None, d, ds, "int8", own, "float32", pids=pid), "out= and work=")
