"""Dense MaxSim on MX block-scaled embeddings (codec.maxsim_batch(dtype="mxfp8" / "mxfp4"), maxsim_batch_device on uint8 pairs) and
the quantiser (codec.quantize_mx / quantize_mx_device) against float64 on the decoded operands (include/colbert_hip.h): bit for bit
where every partial sum is exact in fp32, within the derived bound on random data.  The bound's u is what the bare instruction was measured at
(tools/microbench/mfma_scale_mx.hip, profiles/maxsim_batch_mx.md): largest |error| / sum|q d| = 2^-11.53 over random blocks of every
code (2^-23.0 where a block's codes lie in its top two binades), twice that rounded up to a power of two: u = 2^-10."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

pytestmark = pytest.mark.gpu

S = 64                                                          # rows of one wave's step, both formats
# empty passages, tiles that straddle passages, a passage across waves (S + 3) and one across steps of 4 waves (4 S + 5)
DOCLENS = np.array([0, 1, 15, 16, 17, 0, S + 3, 4 * S + 5], np.int64)
B = 3
U = 2.0 ** -10


def maxima(qh, dh, dl):
    """(B, T, N) float64: per passage the largest dot of each token with its rows, -inf for an empty passage"""
    dim, T, nb = qh.shape
    dots = qh.reshape(dim, T * nb, order="F").T @ dh                                          # (T nb, n), row = t + T b
    off = np.concatenate([[0], np.cumsum(dl)])
    m = np.stack([dots[:, a:z].max(axis=1, initial=-np.inf) for a, z in zip(off[:-1], off[1:])], axis=1)
    return m.reshape(nb, T, dl.size)


def ordered_sum(m):
    """(N, B) float32: acc = 0; acc = fl32(acc + fl32(m_t)), t ascending"""
    acc = np.zeros((m.shape[0], m.shape[2]), np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(m.shape[1]):
            acc = acc + m[:, t, :].astype(np.float32)
    return acc.T


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), what)          # bit for bit; shapes included


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_pair(torch, pair):
    """a host (values, scales) pair, embeddings last, as the device route takes it: embeddings first"""
    return tuple(cuda(torch, np.moveaxis(a, 0, -1) if a.ndim == 2 else a.transpose(2, 1, 0)) for a in pair)


def exact_pair(rng, fmt, dim, shape):
    """codes of elements drawn from {0, +-0.5, +-1, +-2} and a scale byte from 125..130 for every block"""
    lut = np.array([0x00, 0x30, 0x38, 0x40, 0xB0, 0xB8, 0xC0] if fmt == "mxfp8" else [0, 1, 2, 4, 9, 10, 12], np.uint8)
    v = lut[rng.integers(0, 7, size=(dim,) + shape)]
    if fmt == "mxfp4":
        v = v[0::2] | (v[1::2] << np.uint8(4))
    return np.asfortranarray(v), np.asfortranarray(rng.integers(125, 131, size=(dim // 32,) + shape).astype(np.uint8))


_exact = {}


def exact_case(dim, T, fmt, dl):
    key = (dim, T, fmt, dl.size)
    if key not in _exact:
        rng = np.random.default_rng([dim, T, fmt == "mxfp4", dl.size])
        q, d = exact_pair(rng, "mxfp8", dim, (T, B)), exact_pair(rng, fmt, dim, (int(dl.sum()),))
        qh, dh = codec.dequantize_mx(*q, "mxfp8").astype(np.float64), codec.dequantize_mx(*d, fmt).astype(np.float64)
        qi, di = np.rint(qh * 8).astype(np.int64), np.rint(dh * 8).astype(np.int64)          # in units of 2^-3: integers
        assert np.array_equal(qi, qh * 8) and np.array_equal(di, dh * 8)
        # every term of a dot is a multiple of 2^-6 and the sum of their magnitudes stays below 2^24 of it: every partial sum, in
        # any order, is exact in fp32
        assert (np.abs(qi).reshape(dim, -1, order="F").T @ np.abs(di)).max() < 2 ** 24
        m = maxima(qi.astype(np.float64), di.astype(np.float64), dl) / 64                     # exact: integers below 2^53
        _exact[key] = (q, d, ordered_sum(m))
    return _exact[key]


@pytest.mark.parametrize("owned", [False, True])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("T", [1, 17, 32, 33, 128])
@pytest.mark.parametrize("dim", [32, 96, 128, 160, 256])
def test_exact_products_and_sums_have_the_bits_of_float64(dim, T, fmt, owned):
    torch = pytest.importorskip("torch")
    q, d, ref = exact_case(dim, T, fmt, DOCLENS)
    owner = (np.arange(DOCLENS.size) // 2 % B).astype(np.int32)                              # runs of two passages per query
    (dq, dqs), (dd, dds) = device_pair(torch, q), device_pair(torch, d)
    got = codec.maxsim_batch_device(dq, dd, cuda(torch, DOCLENS), owner=cuda(torch, owner) if owned else None, d_scale=dds, q_scale=dqs)
    same(got.cpu().numpy() if owned else got.cpu().numpy().T, ref[np.arange(DOCLENS.size), owner] if owned else ref)
    assert np.all(np.isneginf(ref[DOCLENS == 0]))


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_exact_with_two_passages_per_work_group(fmt):
    torch = pytest.importorskip("torch")
    dl = np.random.default_rng(5).integers(1, 4, size=2049).astype(np.int64)
    q, d, ref = exact_case(128, 17, fmt, dl)
    (dq, dqs), (dd, dds) = device_pair(torch, q), device_pair(torch, d)
    same(codec.maxsim_batch_device(dq, dd, cuda(torch, dl), d_scale=dds, q_scale=dqs).cpu().numpy().T, ref)


_random = {}


def random_case(dim, fmt):
    """unit-norm fp32 operands, their host quantisation, float64 maxima of the decoded operands"""
    if (dim, fmt) not in _random:
        rng = np.random.default_rng(dim)
        dl = DOCLENS[DOCLENS > 0]
        unit = lambda x: np.asfortranarray((x / np.linalg.norm(x, axis=0, keepdims=True)).astype(np.float32))   # noqa: E731
        Q, D = unit(rng.standard_normal((dim, 33, B))), unit(rng.standard_normal((dim, int(dl.sum()))))
        q, d = codec.quantize_mx(Q, "mxfp8"), codec.quantize_mx(D, fmt)
        qh, dh = codec.dequantize_mx(*q, "mxfp8").astype(np.float64), codec.dequantize_mx(*d, fmt).astype(np.float64)
        _random[(dim, fmt)] = (Q, D, q, d, dl, qh, dh, maxima(qh, dh, dl))
    return _random[(dim, fmt)]


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("dim", [128, 160])
def test_routes_agree_bit_for_bit_and_lie_within_the_bound(dim, fmt):
    torch = pytest.importorskip("torch")
    Q, D, q, d, dl, qh, dh, m = random_case(dim, fmt)
    owner = (np.arange(dl.size) % B).astype(np.int32)
    (dq, dqs), (dd, dds), d_l = device_pair(torch, q), device_pair(torch, d), cuda(torch, dl)
    gq, gqs = codec.quantize_mx_device(cuda(torch, Q.transpose(2, 1, 0)), "mxfp8")
    gd, gds = codec.quantize_mx_device(cuda(torch, D.T), fmt)
    for got, want, what in ((gq, dq, "query values"), (gqs, dqs, "query scales"), (gd, dd, "passage values"), (gds, dds, "passage scales")):
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), "device quantiser == numpy quantiser: " + what)
    pairs = codec.maxsim_batch_device(dq, dd, d_l, d_scale=dds, q_scale=dqs).cpu().numpy().T
    same(codec.maxsim_batch_device(dq, dd, d_l, owner=cuda(torch, owner), d_scale=dds, q_scale=dqs).cpu().numpy(),
         pairs[np.arange(dl.size), owner], "owned == its column of all pairs")
    same(codec.maxsim_batch_device(cuda(torch, Q.transpose(2, 1, 0)), dd, d_l, d_scale=dds).cpu().numpy().T, pairs, "fp32 d_Q == the pair")
    same(codec.maxsim_batch(q, d, dl, dtype=fmt), pairs, "host call, pairs == device call")
    same(codec.maxsim_batch(Q, D, dl, owner, dtype=fmt), pairs[np.arange(dl.size), owner], "host call, floats, owned")
    # |score - float64| <= 2 dim u sum_t |q_t| max_r |d_r| + T u sum_t |m_t|, on the decoded operands
    off = np.concatenate([[0], np.cumsum(dl)])
    dmax = np.array([np.linalg.norm(dh[:, a:z], axis=0).max() for a, z in zip(off[:-1], off[1:])])
    bound = 2 * dim * U * np.linalg.norm(qh, axis=0).sum(axis=0)[None, :] * dmax[:, None] + 33 * U * np.abs(m).sum(axis=1).T
    ratio = np.abs(pairs.astype(np.float64) - m.sum(axis=1).T) / bound
    print(f"dim {dim} {fmt}: largest error / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_device_quantiser_equals_numpy_on_edge_blocks(fmt):
    """what random data never holds: every E4M3 half-way point (all E2M1 ones among them), saturation, exact powers of two as amax,
    an all-zero block, -0, fp32 subnormals (the exponent clamp: the device must not flush them)"""
    torch = pytest.importorskip("torch")
    ties = [(1 + (m + 0.5) / 8) * 2.0 ** e for e in range(-7, 9) for m in range(8)] + [(m + 0.5) * 2.0 ** -9 for m in range(8)]
    X = np.zeros((64, 8), np.float32)
    X[:, :5].T.flat[:len(ties)] = ties                                          # five embeddings of half-way points, 496 -> 448 among them
    X[:8, 5], X[32:34, 5] = [6, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5], [7.9, -6.5]
    X[:3, 6], X[32:34, 6] = [2.0 ** 20, 2.0 ** 11 + 2.0 ** 9, -0.0], [2.0 ** -3, 1.25 * 2.0 ** -5]
    X[:2, 7] = [1e-40, -3e-41]                                                  # its second block: all zero
    X = np.asfortranarray(X)
    gv, gs = codec.quantize_mx_device(cuda(torch, X.T), fmt)
    v, s = codec.quantize_mx(X, fmt)
    np.testing.assert_array_equal(gv.cpu().numpy().T, v)
    np.testing.assert_array_equal(gs.cpu().numpy().T, s)


def test_device_route_clamps_bad_doclens_and_owners_and_replays_in_a_graph():
    torch = pytest.importorskip("torch")
    Q, D, q, d, dl, qh, dh, m = random_case(128, "mxfp4")
    N = dl.size
    (dq, dqs), (dd, dds) = device_pair(torch, q), device_pair(torch, d)
    call = lambda l, **kw: codec.maxsim_batch_device(dq, dd, cuda(torch, l), d_scale=dds, q_scale=dqs, **kw).cpu().numpy()   # noqa: E731
    clean = call(dl).T
    longer = np.concatenate([dl[:-1], [dl[-1] + 40, 7, -5, 3]])            # the last passage runs past n_D; three more hold nothing
    got = call(longer).T
    same(got[:N], clean, "passages with readable rows")
    assert np.all(np.isneginf(got[N:]))
    neg = dl.copy(); neg[2] = -dl[2]                                        # every later passage shifts
    got = call(neg).T
    same(got[:2], clean[:2], "before the negative doclen")
    assert np.all(np.isneginf(got[2]))
    short = codec.maxsim_batch_device(dq, dd[:100], cuda(torch, dl), d_scale=dds[:100], q_scale=dqs).cpu().numpy().T   # n_D < sum(doclens)
    same(short[:4], clean[:4], "passages wholly below n_D")                 # rows 0..48; the fifth passage is cut at row 100
    assert np.all(np.isneginf(short[5]))
    owner = (np.arange(N) % B).astype(np.int32)
    bad, want = owner.copy(), clean[np.arange(N), owner]
    bad[[0, 3]] = [-1, B]; want[[0, 3]] = -np.inf
    same(call(dl, owner=cuda(torch, bad)), want, "owners outside the batch")
    d_Q, d_l, d_o = cuda(torch, Q.transpose(2, 1, 0)), cuda(torch, dl), cuda(torch, owner)   # fp32 queries: the quantiser is captured too
    out = torch.empty(N, dtype=torch.float32, device="cuda")
    work = torch.empty(int(clb.lib().clb_maxsim_batch_mx_work_bytes(N, B, 33, 128)), dtype=torch.uint8, device="cuda")
    run = lambda: codec.maxsim_batch_device(d_Q, dd, d_l, owner=d_o, out=out, work=work, d_scale=dds)   # noqa: E731
    run()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for rep in range(3):
        out.fill_(0)
        graph.replay()
        same(out.cpu().numpy(), clean[np.arange(N), owner], f"replay {rep}")
