"""Dense MaxSim of un-indexed passages for a query batch (codec.maxsim_batch / maxsim_batch_device /
BertEncoder.score_passages) against the CPU oracle's maxsim called per query on the same arrays: the same bits."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

pytestmark = pytest.mark.gpu

# a passage boundary on every edge of a wave's 16 rows and of a work-group's 64-row (dim > 512: 32-row) step, one passage
# longer than several steps, a run of one-row passages
EDGES = [1, 15, 16, 17, 31, 32, 33, 49, 300, 64, 5] + [1] * 20 + [2, 63, 65]


def doclens_of(kind):
    if kind == "edges":
        return np.array(EDGES, dtype=np.int64)
    # above 2048 passages a work-group owns several: tiles straddle passages and owners
    return np.concatenate([EDGES, np.random.default_rng(3).integers(1, 24, size=4200 - len(EDGES))]).astype(np.int64)


def unit(rng, *shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return np.asfortranarray(x / np.linalg.norm(x, axis=0, keepdims=True))


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


_cases = {}


def case(oracle, dim, T, B, kind):
    """(Q, D, doclens, ref (N, B)): the oracle's maxsim per query, computed once per shape"""
    key = (dim, T, B, kind)
    if key not in _cases:
        rng = np.random.default_rng(dim * 1000 + T * 10 + B)
        dl = doclens_of(kind)
        Q, D = unit(rng, dim, T, B), unit(rng, dim, int(dl.sum()))
        ref = np.stack([oracle.maxsim(Q[:, :, q], D, np.arange(1, dl.size + 1), dl) for q in range(B)], axis=1)
        _cases[key] = (Q, D, dl, ref)
    return _cases[key]


SHAPES = [(128, 1, 1, "edges"), (128, 16, 3, "edges"), (128, 17, 3, "many"), (128, 32, 33, "edges"), (128, 32, 3, "many"),
          (128, 33, 3, "edges"), (128, 128, 33, "edges"), (64, 32, 3, "many"), (8, 17, 1, "many"), (768, 16, 3, "edges"),
          (12, 17, 3, "edges")]


@pytest.mark.parametrize("dim,T,B,kind", SHAPES)
def test_both_forms_equal_the_oracle(oracle, dim, T, B, kind):
    Q, D, dl, ref = case(oracle, dim, T, B, kind)
    N = dl.size
    pairs = codec.maxsim_batch(Q, D, dl)
    same(pairs, ref, "all pairs")
    rng = np.random.default_rng(5)
    owner = rng.integers(0, B, size=N).astype(np.int32)               # out of order
    if B >= 3:
        owner[owner == 1] = 2                                         # query 1 owns nothing
    same(codec.maxsim_batch(Q, D, dl, owner), ref[np.arange(N), owner], "owned")
    for q in sorted({0, B // 2, B - 1}):                              # one query owns everything: a column of the all-pairs result
        same(codec.maxsim_batch(Q, D, dl, np.full(N, q, np.int32)), pairs[:, q], f"owner = {q} everywhere")


@pytest.fixture(scope="module")
def on_device(oracle):
    torch = pytest.importorskip("torch")
    Q, D, dl, ref = case(oracle, 128, 32, 3, "many")
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    return torch, t, t(Q.transpose(2, 1, 0)), t(D.T), dl, ref


def test_device_route_equals_the_host_route(on_device):
    torch, t, d_Q, d_D, dl, ref = on_device
    owner = (np.arange(dl.size) % 3).astype(np.int32)
    same(codec.maxsim_batch_device(d_Q, d_D, t(dl)).cpu().numpy().T, ref, "all pairs")
    same(codec.maxsim_batch_device(d_Q, d_D, t(dl), owner=t(owner)).cpu().numpy(), ref[np.arange(dl.size), owner], "owned")
    with pytest.raises(clb.ArgumentError):
        codec.maxsim_batch_device(d_Q, d_D, t(dl), work=torch.empty(8, dtype=torch.uint8, device=d_Q.device))
    assert codec.maxsim_batch_device(d_Q, d_D, t(dl[:0])).shape == (3, 0)


def test_device_route_clamps_bad_doclens_and_owners(on_device):
    """The no-fault contract with a valid D buffer: rows at or past n_D are never read, a negative doclen is 0, an owner
    outside the batch reads no query -- -Inf for the passages concerned, the oracle's bits for the others."""
    torch, t, d_Q, d_D, dl, ref = on_device
    N = dl.size
    longer = np.concatenate([dl[:-1], [dl[-1] + 40, 7, -5, 3]])          # the last passage runs past n_D; three more hold nothing
    got = codec.maxsim_batch_device(d_Q, d_D, t(longer)).cpu().numpy().T
    same(got[:N], ref, "passages with readable rows")
    assert np.all(np.isneginf(got[N:]))
    k = 100                                                               # a negative doclen in the middle: every later passage shifts by dl[k]
    neg = dl.copy(); neg[k] = -dl[k]
    got = codec.maxsim_batch_device(d_Q, d_D, t(neg)).cpu().numpy().T
    same(got[:k], ref[:k], "before the negative doclen")
    assert np.all(np.isneginf(got[k]))
    owner = (np.arange(N) % 3).astype(np.int32)
    want = ref[np.arange(N), owner]
    owner[[0, 7, N - 1]] = -1; owner[[3, 2500]] = 3
    want[[0, 7, N - 1, 3, 2500]] = -np.inf
    same(codec.maxsim_batch_device(d_Q, d_D, t(dl), owner=t(owner)).cpu().numpy(), want, "owners outside the batch")


def test_graph_replay_after_refilling_in_place(oracle, on_device):
    torch, t, d_Q, d_D, dl, ref = on_device
    N = dl.size
    q, d, l = d_Q.clone(), d_D.clone(), t(dl)
    own = t((np.arange(N) % 3).astype(np.int32))
    out = torch.empty(N, dtype=torch.float32, device=q.device)
    work = torch.empty(int(clb.lib().clb_maxsim_batch_work_bytes(N, 3, 32)), dtype=torch.uint8, device=q.device)
    call = lambda: codec.maxsim_batch_device(q, d, l, owner=own, out=out, work=work)      # noqa: E731
    side = torch.cuda.Stream(q.device)
    side.wait_stream(torch.cuda.current_stream(q.device))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(q.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    # other queries, other embeddings, the doclens reversed, other owners -- in the captured tensors
    Q2, D2 = unit(np.random.default_rng(11), 128, 32, 3), unit(np.random.default_rng(12), 128, int(dl.sum()))
    dl2 = dl[::-1].copy()
    own2 = ((np.arange(N) * 7 + 1) % 3).astype(np.int32)
    want = np.stack([oracle.maxsim(Q2[:, :, j], D2, np.arange(1, N + 1), dl2) for j in range(3)], axis=1)[np.arange(N), own2]
    q.copy_(t(Q2.transpose(2, 1, 0))); d.copy_(t(D2.T)); l.copy_(t(dl2)); own.copy_(t(own2))
    for rep in range(3):
        out.fill_(0)
        graph.replay()
        same(out.cpu().numpy(), want, f"replay {rep}")
    same(call().cpu().numpy(), want, "eager")


def test_score_passages_scores_what_it_encoded(oracle, tmp_path):
    from colbert_jl_amd import tokenization
    from colbert_jl_amd.encoder import pack_weights
    from tests.test_encoder import VOCAB, _random_bert, _state
    torch, cfg, bert, linear = _random_bert(hidden=64, layers=2, heads=4, inter=128, vocab=len(VOCAB), max_pos=64, dim=128, seed=5)
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = tokenization.WordPieceTokenizer(str(tmp_path / "vocab.txt"))
    config = clb.ColBERTConfig(doc_maxlen=24, query_maxlen=12, index_bsize=4)
    enc = clb.BertEncoder(pack_weights(_state(bert, linear), cfg.to_dict(), 128), cfg.to_dict(), dim=128, tokenizer=tok, config=config)
    queries = ["what is col bert", "hello world", "a test of the tokenizer"]
    passages = [[], ["this is a longer passage with many words."],
                ["hello world!", "a", "the tokenizer", "this is a test", "many words with a longer passage, hello"]]
    scores, Q, D, dl = enc.score_passages(queries, passages, return_embeddings=True)
    assert [s.size for s in scores] == [0, 1, 5] and Q.shape == (128, 12, 3) and D.shape == (128, dl.sum()) and dl.size == 6
    e_D, e_dl = enc.encode_passages([p for ps in passages for p in ps])
    assert np.array_equal(dl, e_dl) and np.allclose(D, e_D, atol=1e-5)      # (the batch a passage travels in moves its last bits)
    off = 0
    for j, s in enumerate(scores):
        if s.size:
            lo, hi = dl[:off].sum(), dl[:off + s.size].sum()
            same(s, oracle.maxsim(Q[:, :, j], D[:, lo:hi], np.arange(1, s.size + 1), dl[off:off + s.size]), f"query {j}")
        off += s.size
    for got, want in zip(enc.score_passages(queries, passages), scores):
        same(got, want)
    enc.close()
