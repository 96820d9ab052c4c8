"""Dense MaxSim on fp16 / bf16 embeddings (codec.maxsim_batch(dtype=) / maxsim_batch_device on 16-bit tensors) against float64
numpy on the rounded operands, within the derived bound of DESIGN 4.2a; and bit for bit against itself across forms and routes."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

pytestmark = pytest.mark.gpu

# a passage boundary on every edge of a tile's 16 rows, a wave's 32 and a work-group's 64- / 128-row step, passages longer
# than a step, a run of one-row passages
EDGES = [1, 15, 16, 17, 31, 32, 33, 49, 300, 64, 5] + [1] * 20 + [2, 63, 65, 127, 128, 129]
SHAPES = [(128, 1, 1, "edges"), (128, 17, 3, "many"), (128, 32, 33, "edges"), (128, 33, 3, "edges"), (128, 128, 5, "edges"),
          (64, 32, 3, "many"), (8, 17, 1, "many"), (40, 16, 3, "edges"), (768, 16, 3, "edges")]
DTYPES = ["float16", "bfloat16"]
CASES = [(dtype,) + shape for dtype in DTYPES for shape in SHAPES]


def doclens_of(kind):
    if kind == "edges":
        return np.array(EDGES, dtype=np.int64)
    # above 2048 passages a work-group owns several: tiles straddle passages and owners
    return np.concatenate([EDGES, np.random.default_rng(3).integers(1, 24, size=4200 - len(EDGES))]).astype(np.int64)


def unit(rng, *shape):
    x = rng.standard_normal(shape).astype(np.float32)
    x = x / np.linalg.norm(x, axis=0, keepdims=True)
    x[np.abs(x) < 2.0 ** -14] = 0                        # no fp16 subnormals
    return np.asfortranarray(x)


def bits16(x, dtype):
    return x.astype(np.float16).view(np.uint16) if dtype == "float16" else codec.to_bfloat16_bits(x)


def widen(h, dtype):
    return (h.view(np.float16) if dtype == "float16" else (h.astype(np.uint32) << 16).view(np.float32)).astype(np.float64)


def reference(Q, D, dl, dtype):
    """(ref, tol), both (N, B): float64 on the rounded operands, and 2 dim u sum_t |q_t| max_r |d_r| + T u sum_t |m_t|"""
    (dim, T, _), U = Q.shape, 2.0 ** -23
    Qr, Dr, first = widen(bits16(Q, dtype), dtype), widen(bits16(D, dtype), dtype), np.concatenate([[0], np.cumsum(dl)[:-1]])
    m = np.maximum.reduceat(np.einsum("dtb,dn->btn", Qr, Dr), first, axis=2)                    # (B, T, N)
    d_max = np.maximum.reduceat(np.linalg.norm(Dr, axis=0), first)
    tol = 2 * dim * U * np.outer(d_max, np.linalg.norm(Qr, axis=0).sum(0)) + T * U * np.abs(m).sum(1).T
    return m.sum(1).T, tol


_cases = {}


def case(dtype, dim, T, B, kind):
    """(Q, D, doclens, ref, tol, owner, all-pairs result of the host route), computed once per case"""
    key = (dtype, dim, T, B, kind)
    if key not in _cases:
        rng = np.random.default_rng(dim * 1000 + T * 10 + B)
        dl = doclens_of(kind)
        Q, D = unit(rng, dim, T, B), unit(rng, dim, int(dl.sum()))
        owner = np.random.default_rng(5).integers(0, B, size=dl.size).astype(np.int32)        # out of order
        if B >= 3:
            owner[owner == 1] = 2                                                              # query 1 owns nothing
        _cases[key] = (Q, D, dl) + reference(Q, D, dl, dtype) + (owner, codec.maxsim_batch(Q, D, dl, dtype=dtype))
    return _cases[key]


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), what)          # bit for bit; shapes included


def on_device(torch, dtype, Q, D, dl, owner):
    """(fp32 queries, pre-rounded queries, 16-bit embeddings, doclens, owners) as the device route takes them"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                             # noqa: E731
    h = lambda a: t(bits16(a, dtype).view(np.int16)).view(getattr(torch, dtype))               # noqa: E731
    return t(Q.transpose(2, 1, 0)), h(Q.transpose(2, 1, 0)), h(D.T), t(dl), t(owner)


@pytest.mark.parametrize("dtype,dim,T,B,kind", CASES)
def test_both_forms_within_the_bound_of_float64(dtype, dim, T, B, kind):
    Q, D, dl, ref, tol, owner, pairs = case(dtype, dim, T, B, kind)
    rows = np.arange(dl.size)
    owned = codec.maxsim_batch(Q, D, dl, owner, dtype=dtype)
    for what, got, want, bound in (("all pairs", pairs, ref, tol), ("owned", owned, ref[rows, owner], tol[rows, owner])):
        ratio = np.abs(got - want) / bound
        print(f"{dtype} {(dim, T, B, kind)} {what}: largest error / tol = {ratio.max():.4f}")
        assert got.shape == want.shape and ratio.max() <= 1.0, (what, int(ratio.argmax()), ratio.max())


@pytest.mark.parametrize("dtype,dim,T,B,kind", CASES)
def test_forms_query_types_and_routes_give_the_same_bits(dtype, dim, T, B, kind):
    torch = pytest.importorskip("torch")
    Q, D, dl, _, _, owner, pairs = case(dtype, dim, T, B, kind)
    same(codec.maxsim_batch(Q, D, dl, owner, dtype=dtype), pairs[np.arange(dl.size), owner], "owned = its entries of all pairs")
    d_Q, d_Qh, d_D, d_l, d_o = on_device(torch, dtype, Q, D, dl, owner)
    same(codec.maxsim_batch_device(d_Q, d_D, d_l).cpu().numpy().T, pairs, "device route, fp32 queries")
    same(codec.maxsim_batch_device(d_Qh, d_D, d_l).cpu().numpy().T, pairs, "device route, pre-rounded queries")
    same(codec.maxsim_batch_device(d_Q, d_D, d_l, owner=d_o).cpu().numpy(), pairs[np.arange(dl.size), owner], "device route, owned")


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_route_clamps_bad_doclens_and_owners(dtype):
    """A valid D buffer, bad doclens and owners: -Inf for the passages concerned, the clean call's bits for the others."""
    torch = pytest.importorskip("torch")
    Q, D, dl, _, _, owner, pairs = case(dtype, 128, 17, 3, "many")
    d_Q, _, d_D, _, _ = on_device(torch, dtype, Q, D, dl, owner)
    t = lambda a: torch.from_numpy(a).cuda()                                                   # noqa: E731
    N = dl.size
    longer = np.concatenate([dl[:-1], [dl[-1] + 40, 7, -5, 3]])          # the last passage runs past n_D; three more hold nothing
    got = codec.maxsim_batch_device(d_Q, d_D, t(longer)).cpu().numpy().T
    same(got[:N], pairs, "passages with readable rows")
    assert np.all(np.isneginf(got[N:]))
    k = 100                                                               # a negative doclen in the middle: every later passage shifts
    neg = dl.copy(); neg[k] = -dl[k]
    got = codec.maxsim_batch_device(d_Q, d_D, t(neg)).cpu().numpy().T
    same(got[:k], pairs[:k], "before the negative doclen")
    assert np.all(np.isneginf(got[k]))
    bad, want = owner.copy(), pairs[np.arange(N), owner]
    bad[[0, 7, N - 1]] = -1; bad[[3, 2500]] = 3
    want[[0, 7, N - 1, 3, 2500]] = -np.inf
    same(codec.maxsim_batch_device(d_Q, d_D, t(dl), owner=t(bad)).cpu().numpy(), want, "owners outside the batch")
    with pytest.raises(clb.ArgumentError):
        codec.maxsim_batch_device(d_Q, d_D, t(dl), work=torch.empty(8, dtype=torch.uint8, device=d_Q.device))


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_after_refilling_in_place(dtype):
    torch = pytest.importorskip("torch")
    Q, D, dl, _, _, owner, _ = case(dtype, 128, 17, 3, "many")
    N = dl.size
    q, _, d, l, own = on_device(torch, dtype, Q, D, dl, owner)                                 # fp32 queries: the rounding launch is captured too
    out = torch.empty(N, dtype=torch.float32, device=q.device)
    work = torch.empty(int(clb.lib().clb_maxsim_batch_half_work_bytes(N, 3, 17, 128)), dtype=torch.uint8, device=q.device)
    call = lambda: codec.maxsim_batch_device(q, d, l, owner=own, out=out, work=work)           # noqa: E731
    call()                                                                                     # (the kernels are loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    Q2, D2 = unit(np.random.default_rng(11), 128, 17, 3), unit(np.random.default_rng(12), 128, int(dl.sum()))
    dl2, own2 = dl[::-1].copy(), ((np.arange(N) * 7 + 1) % 3).astype(np.int32)
    want = codec.maxsim_batch(Q2, D2, dl2, own2, dtype=dtype)
    q2, _, d2, l2, o2 = on_device(torch, dtype, Q2, D2, dl2, own2)
    q.copy_(q2); d.copy_(d2); l.copy_(l2); own.copy_(o2)
    for rep in range(3):
        out.fill_(0)
        graph.replay()
        same(out.cpu().numpy(), want, f"replay {rep}")
    same(call().cpu().numpy(), want, "eager")
