"""Dense MaxSim on int8 embeddings (codec.maxsim_batch(dtype="int8") / maxsim_batch_device on int8 tensors) and the quantiser
(codec.quantize_rows / quantize_rows_device) against a numpy restatement of their definition (include/colbert_hip.h): bit for
bit, no tolerance -- the integer dots are exact."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

pytestmark = pytest.mark.gpu

# a tile's 16 rows and a wave's 64 straddle passages, one passage is longer than a work-group's 256-row step; above 2048 passages
# a work-group owns two, and 2101 is no multiple of that
DOCLENS = np.concatenate([[1, 15, 16, 17, 33, 300], np.random.default_rng(3).integers(1, 6, size=2095)]).astype(np.int64)
N = DOCLENS.size
B = 3
OWNER = np.concatenate([np.repeat(np.arange(B), 350)[:N // 2], np.arange(N - N // 2) % B]).astype(np.int32)    # runs, then alternating
CASES = [(dim, T) for dim in (16, 80, 128, 1024) for T in (1, 17, 32, 33)]


def reference(q8, qs, d8, ds, dl):
    """(N, B): exact int64 dots, one float32 multiply by the row's scale, the maximum per passage, the scaled ordered sum"""
    (dim, T, nb), first = q8.shape, np.concatenate([[0], np.cumsum(dl)[:-1]])
    i = q8.reshape(dim, T * nb, order="F").T.astype(np.int64) @ d8.astype(np.int64)              # (T nb, n), row = t + T b
    m = np.maximum.reduceat(ds.astype(np.float32)[None, :] * i.astype(np.float32), first, axis=1)  # float(i) is exact: |i| <= 2^24
    m = m.reshape(nb, T, dl.size)
    acc = np.zeros((nb, dl.size), np.float32)
    for t in range(T):
        acc = acc + qs[t, :, None].astype(np.float32) * m[:, t, :]
    return acc.T


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), what)          # bit for bit; shapes included


_cases = {}


def case(dim, T):
    """(Q, D, (q8, qs), (d8, ds), ref): float operands, their host quantisation and the reference, computed once per shape"""
    if (dim, T) not in _cases:
        rng = np.random.default_rng(1000 * dim + T)
        Q, D = rng.standard_normal((dim, T, B), dtype=np.float32), rng.standard_normal((dim, int(DOCLENS.sum())), dtype=np.float32)
        q, d = codec.quantize_rows(Q), codec.quantize_rows(D)
        _cases[(dim, T)] = (np.asfortranarray(Q), np.asfortranarray(D), q, d, reference(*q, *d, DOCLENS))
    return _cases[(dim, T)]


def on_device(torch, Q, q, d):
    """(fp32 queries, int8 queries, their scales, int8 embeddings, their scales, doclens, owners) as the device route takes them"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                             # noqa: E731
    return t(Q.transpose(2, 1, 0)), t(q[0].transpose(2, 1, 0)), t(q[1].T), t(d[0].T), t(d[1]), t(DOCLENS), t(OWNER)


@pytest.mark.parametrize("dim,T", CASES)
def test_forms_and_routes_equal_the_restatement(dim, T):
    torch = pytest.importorskip("torch")
    Q, D, q, d, ref = case(dim, T)
    rows = np.arange(N)
    same(codec.maxsim_batch(Q, D, DOCLENS, dtype="int8"), ref, "host route, quantised in the call")
    same(codec.maxsim_batch(q, d, DOCLENS, OWNER), ref[rows, OWNER], "host route, int8 pairs, owned = its entries of all pairs")
    d_Q, d_q8, d_qs, d_d8, d_ds, d_l, d_o = on_device(torch, Q, q, d)
    same(codec.maxsim_batch_device(d_Q, d_d8, d_l, d_scale=d_ds).cpu().numpy().T, ref, "device route, fp32 queries")
    same(codec.maxsim_batch_device(d_q8, d_d8, d_l, d_scale=d_ds, q_scale=d_qs).cpu().numpy().T, ref, "device route, int8 queries")
    g8, gs = codec.quantize_rows_device(d_Q)
    same(codec.maxsim_batch_device(g8, d_d8, d_l, owner=d_o, d_scale=d_ds, q_scale=gs).cpu().numpy(), ref[rows, OWNER],
         "device route, owned, queries quantised first")


def test_the_largest_accumulator_is_exact():
    """dim 1024, every value +-127, and a row of -128 against a token of -128: i = 2^24"""
    rng = np.random.default_rng(9)
    q8 = np.asfortranarray(rng.choice(np.array([-127, 127], np.int8), size=(1024, 17, B)))
    d8 = np.asfortranarray(rng.choice(np.array([-127, 127], np.int8), size=(1024, 40)))
    q8[:, 0, 1] = -128; d8[:, 20] = -128
    qs, ds = rng.uniform(0.5, 2, size=(17, B)).astype(np.float32), rng.uniform(0.5, 2, size=40).astype(np.float32)
    dl = np.array([17, 16, 7], np.int64)
    ref = reference(q8, qs, d8, ds, dl)
    assert q8[:, 0, 1].astype(np.int64) @ d8[:, 20].astype(np.int64) == 2 ** 24
    same(codec.maxsim_batch((q8, qs), (d8, ds), dl), ref)


def test_device_route_clamps_bad_doclens_and_owners():
    """A valid D buffer, bad doclens and owners: -Inf for the passages concerned, the clean call's bits for the others; a query
    scale of 0 does not turn -Inf into NaN."""
    torch = pytest.importorskip("torch")
    Q, D, q, d, ref = case(128, 17)
    _, d_q8, d_qs, d_d8, d_ds, _, _ = on_device(torch, Q, q, d)
    t = lambda a: torch.from_numpy(a).cuda()                                                   # noqa: E731
    call = lambda dl, **kw: codec.maxsim_batch_device(d_q8, d_d8, t(dl), d_scale=d_ds, q_scale=kw.pop("qs", d_qs), **kw).cpu().numpy()  # noqa: E731
    longer = np.concatenate([DOCLENS[:-1], [DOCLENS[-1] + 40, 7, -5, 3]])   # the last passage runs past n_D; three more hold nothing
    got = call(longer).T
    same(got[:N], ref, "passages with readable rows")
    assert np.all(np.isneginf(got[N:]))
    k = 100                                                                # a negative doclen in the middle: every later passage shifts
    neg = DOCLENS.copy(); neg[k] = -DOCLENS[k]
    got = call(neg).T
    same(got[:k], ref[:k], "before the negative doclen")
    assert np.all(np.isneginf(got[k]))
    bad, want = OWNER.copy(), ref[np.arange(N), OWNER]
    bad[[0, 7, N - 1]] = -1; bad[[3, 1500]] = B
    want[[0, 7, N - 1, 3, 1500]] = -np.inf
    same(call(DOCLENS, owner=t(bad)), want, "owners outside the batch")
    zero_qs = d_qs.clone(); zero_qs[0] = 0
    got = call(longer, qs=zero_qs).T
    assert np.all(got[:N, 0] == 0) and np.all(np.isneginf(got[N:]))
    with pytest.raises(clb.ArgumentError):
        codec.maxsim_batch_device(d_q8, d_d8, t(DOCLENS), d_scale=d_ds, q_scale=d_qs, work=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        codec.maxsim_batch_device(d_q8, d_d8, t(DOCLENS), d_scale=d_ds)                        # int8 queries without scales


def test_graph_replay_after_refilling_in_place():
    torch = pytest.importorskip("torch")
    Q, D, q, d, ref = case(128, 17)
    d_Q, _, _, d_d8, d_ds, d_l, d_o = on_device(torch, Q, q, d)                                # fp32 queries: the quantiser is captured too
    out = torch.empty(N, dtype=torch.float32, device="cuda")
    work = torch.empty(int(clb.lib().clb_maxsim_batch_i8_work_bytes(N, B, 17, 128)), dtype=torch.uint8, device="cuda")
    call = lambda: codec.maxsim_batch_device(d_Q, d_d8, d_l, owner=d_o, out=out, work=work, d_scale=d_ds)   # noqa: E731
    call()                                                                                     # (the kernels are loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    Q2, D2, q2, d2, ref2 = case(128, 32)                                                       # other values, same D shape
    d_Q.copy_(torch.from_numpy(np.ascontiguousarray(Q2.transpose(2, 1, 0)[:, :17])).cuda())
    d_d8.copy_(torch.from_numpy(np.ascontiguousarray(d2[0].T)).cuda()); d_ds.copy_(torch.from_numpy(d2[1]).cuda())
    want = codec.maxsim_batch((q2[0][:, :17], q2[1][:17]), d2, DOCLENS, OWNER)
    for rep in range(3):
        out.fill_(0)
        graph.replay()
        same(out.cpu().numpy(), want, f"replay {rep}")
    same(call().cpu().numpy(), want, "eager")


@pytest.mark.parametrize("dim,n", [(16, 1), (16, 70), (1024, 1), (1024, 70), (80, 5)])
def test_quantize_rows_device_equals_quantize_rows(dim, n):
    torch = pytest.importorskip("torch")
    X = np.random.default_rng(dim + n).standard_normal((dim, n)).astype(np.float32)
    if n > 2:
        X[:, 1] = 0                                                                            # an all-zero row
        X[:, 2] = np.resize(np.array([127, 0.5, 1.5, 2.5, -0.5, -2.5, 63.5, -126.5], np.float32), dim)   # s = 1: x / s on ties
    X8, s = codec.quantize_rows(X)
    g8, gs = codec.quantize_rows_device(torch.from_numpy(np.ascontiguousarray(X.T)).cuda())
    same(gs.cpu().numpy(), s, "scales")
    np.testing.assert_array_equal(g8.cpu().numpy().T, X8)
    assert n <= 2 or (not X8[:, 1].any() and X8[:8, 2].tolist() == [127, 0, 2, 2, 0, -2, 64, -126])
