"""Dense MaxSim on 1-bit sign embeddings (codec.maxsim_batch(dtype="binary") / maxsim_batch_device on a uint8 d_D with float32
scales) and the quantiser (codec.binarize_rows_device) against a numpy restatement of their definition (include/colbert_hip.h):
bit for bit, no tolerance -- the integer dots are exact."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

pytestmark = pytest.mark.gpu

# a tile's 16 rows and a wave's 64 straddle passage ends, one passage is longer than a work-group's 256-row step
LENS = np.array([1, 15, 16, 17, 63, 65, 300, 2, 31, 33, 1, 1, 7, 64, 5, 16, 48, 3, 9, 130], np.int64)
BIG = np.concatenate([LENS, np.random.default_rng(3).integers(1, 6, size=2081)])     # above 2048 passages a work-group owns two
B = 3


def owners(N):                                                  # runs, then alternating
    return np.concatenate([np.repeat(np.arange(B), N // 6 + 1)[:N // 2], np.arange(N - N // 2) % B]).astype(np.int32)


def operands(dim, T, lens):
    """(q8, qs, bits, ds): query values over the whole -127..127, a row of all ones and one of all zeros, scales that include 0"""
    rng, n = np.random.default_rng(1000 * dim + T), int(lens.sum())
    q8 = np.asfortranarray(rng.integers(-127, 128, size=(dim, T, B)).astype(np.int8))
    v = np.asfortranarray(rng.integers(0, 256, size=(dim // 8, n)).astype(np.uint8))
    qs, ds = rng.uniform(0.5, 2, size=(T, B)).astype(np.float32), rng.uniform(0.5, 2, size=n).astype(np.float32)
    q8[:2, 0, 0], v[:, 0], v[:, 1], qs[0, 0], ds[3] = (127, -127), 255, 0, 0, 0
    return q8, qs, v, ds


def unpacked(v):
    return np.unpackbits(v, axis=0, bitorder="little").astype(np.int8) * 2 - 1


def reference(q8, qs, v, ds, dl):
    """(N, B): exact int64 dots with the bits as +-1, one float32 multiply by the row's scale, the maximum, the scaled ordered sum"""
    (dim, T, nb), first = q8.shape, np.concatenate([[0], np.cumsum(dl)[:-1]])
    i = q8.reshape(dim, T * nb, order="F").T.astype(np.int64) @ unpacked(v).astype(np.int64)
    m = np.maximum.reduceat(ds[None, :] * i.astype(np.float32), first, axis=1).reshape(nb, T, dl.size)
    acc = np.zeros((nb, dl.size), np.float32)
    for t in range(T):
        acc = acc + qs[t, :, None] * m[:, t, :]
    return acc.T


def same(got, want, what=""):
    got, want = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, np.float32) for a in (got, want))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), what)          # bit for bit; shapes included


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("T", [1, 17, 32, 33, 128])
@pytest.mark.parametrize("dim", [128, 256, 384])
def test_both_forms_equal_the_restatement(dim, T):
    pytest.importorskip("torch")
    q8, qs, v, ds = operands(dim, T, LENS)
    ref, N, own = reference(q8, qs, v, ds, LENS), LENS.size, owners(LENS.size)
    same(codec.maxsim_batch((q8, qs), (v, ds), LENS, dtype="binary"), ref, "host route, all pairs")
    same(codec.maxsim_batch((q8, qs), (v, ds), LENS, own, dtype="binary"), ref[np.arange(N), own], "host route, owned")
    kw = dict(d_scale=dev(ds), q_scale=dev(qs.T))
    d_q, d_v = dev(q8.transpose(2, 1, 0)), dev(v.T)
    lens = np.concatenate([LENS[:-1], [LENS[-1] + 40, 0, 7]])          # the last passage overruns n_D; an empty one; one wholly past n_D
    got = codec.maxsim_batch_device(d_q, d_v, dev(lens), **kw).cpu().numpy().T
    same(got[:N], ref, "device route, all pairs")
    assert np.all(np.isneginf(got[N:]))
    bad, want = own.copy(), ref[np.arange(N), own]
    bad[[0, 9]], want[[0, 9]] = (-1, B), -np.inf
    same(codec.maxsim_batch_device(d_q, d_v, dev(LENS), owner=dev(bad), **kw), want, "device route, owned, owners outside the batch")


@pytest.mark.parametrize("dim,T", [(128, 32), (384, 33)])
def test_every_route_gives_the_same_bits(dim, T):
    """The int8 kernel on the unpacked +-1 values, and fp32 queries against queries quantised first; two passages per work-group"""
    pytest.importorskip("torch")
    q8, qs, v, ds = operands(dim, T, BIG)
    d_q, d_v, d_8, d_l, kw = dev(q8.transpose(2, 1, 0)), dev(v.T), dev(unpacked(v).T), dev(BIG), dict(d_scale=dev(ds), q_scale=dev(qs.T))
    for ow in (None, dev(owners(BIG.size))):
        same(codec.maxsim_batch_device(d_q, d_v, d_l, owner=ow, **kw), codec.maxsim_batch_device(d_q, d_8, d_l, owner=ow, **kw), "int8 path")
    Q = np.random.default_rng(dim).standard_normal((dim, T, B)).astype(np.float32)
    g8, gs = codec.quantize_rows(Q)
    same(codec.maxsim_batch_device(dev(Q.transpose(2, 1, 0)), d_v, d_l, d_scale=kw["d_scale"]),
         codec.maxsim_batch_device(dev(g8.transpose(2, 1, 0)), d_v, d_l, d_scale=kw["d_scale"], q_scale=dev(gs.T)), "fp32 queries")


@pytest.mark.parametrize("owned", [False, True])
def test_by_id_equals_the_contiguous_call_on_the_gathered_rows(owned):
    pytest.importorskip("torch")
    q8, qs, v, ds = operands(256, 17, LENS)
    off = np.insert(np.concatenate([[0], np.cumsum(LENS)]), 5, int(LENS[:5].sum()))       # stored passage 5 is empty
    P = off.size - 1
    pids = np.array([7, 7, 0, -1, P, 5, 20, 6, 3, 6, 12, 1, 7, 19, 2, 14, 18, 9], np.int64)  # repeats, outside 0..P-1, empty
    ok = np.array([0 <= p < P and off[p + 1] > off[p] for p in pids])
    rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in pids[ok]])
    own = owners(pids.size)
    kw, d_q = dict(q_scale=dev(qs.T)), dev(q8.transpose(2, 1, 0))
    want = np.full(pids.size if owned else (B, pids.size), -np.inf, np.float32)
    want[..., ok] = codec.maxsim_batch_device(d_q, dev(v.T[rows]), dev((off[1:] - off[:-1])[pids[ok]]), owner=dev(own[ok]) if owned else None,
                                              d_scale=dev(ds[rows]), **kw).cpu().numpy()
    same(codec.maxsim_batch_device(d_q, dev(v.T), None, owner=dev(own) if owned else None, d_scale=dev(ds), pids=dev(pids), store_offsets=dev(off), **kw), want)


@pytest.mark.parametrize("dim", [128, 256, 1024])
def test_binarize_rows_device_equals_binarize_rows(dim):
    """the bits exactly; the scale within an fp32 sum of dim non-negative terms in any order, one division and the host's rounding"""
    pytest.importorskip("torch")
    X = np.random.default_rng(dim).standard_normal((dim, 70)).astype(np.float32)
    X[:, 1], X[::3, 2] = 0, -0.0
    v, s = codec.binarize_rows(X)
    gv, gs = codec.binarize_rows_device(dev(X.T))
    np.testing.assert_array_equal(gv.cpu().numpy().T, v)
    assert np.all(np.abs(gs.cpu().numpy().astype(np.float64) - s) <= (dim + 2) * 2.0 ** -24 * s) and gs[1] == 0


def test_graph_replay_after_refilling_in_place():
    torch = pytest.importorskip("torch")
    _, _, v, ds = operands(128, 17, LENS)
    Q = np.random.default_rng(5).standard_normal((2, 128, 17, B)).astype(np.float32)
    d_Q, own = dev(Q[0].transpose(2, 1, 0)), owners(LENS.size)                                 # fp32 queries: the quantiser is captured too
    out = torch.empty(LENS.size, dtype=torch.float32, device="cuda")
    work = torch.empty(int(clb.lib().clb_maxsim_batch_b1_work_bytes(LENS.size, B, 17, 128)), dtype=torch.uint8, device="cuda")
    d_v, d_s, d_l, d_o = dev(v.T), dev(ds), dev(LENS), dev(own)
    call = lambda: codec.maxsim_batch_device(d_Q, d_v, d_l, owner=d_o, out=out, work=work, d_scale=d_s)   # noqa: E731
    call()                                                                                     # (the kernels are loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    d_Q.copy_(dev(Q[1].transpose(2, 1, 0)))
    want = codec.maxsim_batch(codec.quantize_rows(Q[1]), (v, ds), LENS, own, dtype="binary")
    for rep in range(3):
        out.fill_(0)
        graph.replay()
        same(out, want, f"replay {rep}")
    same(call(), want, "eager")
