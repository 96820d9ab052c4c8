"""Appending passages to a resident index (Searcher.add_compressed / add_embeddings, clb_searcher_append): after an append the
handle must be indistinguishable from a fresh handle made from the concatenated index.  Every case builds a head Searcher
from the first P passages of a synthetic index (ivf = build_ivf of the head's codes), appends the rest and compares with the
CPU oracle searching the full index -- pids and candidate counts exact, fp32 scores bit-identical -- and, for what the oracle
does not have (eps, tau, the re-score count, the bound constants, the gather statistic), with a fresh Searcher of the full
index."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests.test_gpu_filtered_search import assert_result, assert_same_f32, check_filtered, random_allowed
from tests.util_filter import filtered_ranking

pytestmark = pytest.mark.gpu


def n_emb_of(idx, P):
    return int(idx["doclens"][:P].sum())


def head_index(idx, P):
    """the first P passages of idx as an index of their own, ivf = _build_ivf of their codes"""
    n = n_emb_of(idx, P)
    h = dict(idx)
    h["codes"], h["residuals"], h["doclens"] = idx["codes"][:n], np.asfortranarray(idx["residuals"][:, :n]), idx["doclens"][:P]
    h["ivf"], h["ivf_lengths"] = synthetic.build_ivf(h["codes"], idx["ivf_lengths"].size)
    return h


def tail(idx, P, P2=None):
    """(codes, residuals, doclens) of passages P+1 .. P2 (default: the last)"""
    a, b = n_emb_of(idx, P), (n_emb_of(idx, P2) if P2 is not None else idx["codes"].size)
    return idx["codes"][a:b], np.asfortranarray(idx["residuals"][:, a:b]), idx["doclens"][P:P2]


class Reference:
    """The oracle's full ranking of every query of one index, computed once (tests/util_filter.filtered_ranking with no
    filter: the oracle's own retrieve -> gather -> decompress -> maxsim -> stable sort); where one of the first three
    queries has k candidates its first k are also checked against oracle.search itself."""

    def __init__(self, oracle, idx, Qs, nprobe=2):
        self.oracle, self.idx, self.Qs, self.nprobe = oracle, idx, Qs, nprobe
        self.rank = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe) for j in range(Qs.shape[2])]
        self.checked = set()

    def ranking(self, j, k):
        rp, rs = self.rank[j]
        if rp.size >= k and j < 3 and (j, k) not in self.checked:
            op, os_, on = self.oracle.search(self.idx, self.Qs[:, :, j], self.nprobe, k)
            assert on == rp.size and np.array_equal(op, rp[:k])
            assert_same_f32(os_, rs[:k], "composed ranking against oracle.search")
            self.checked.add((j, k))
        return self.rank[j]


def check_search(s, ref, ks, pid_offset=0, modes=(0, 1), gather_forms=(-1,), singles=3):
    """retrieve, single queries and one batch of all queries of `ref`, in every mode (and gather form), against the oracle"""
    Qs, nq = ref.Qs, ref.Qs.shape[2]
    emb2pid = ref.oracle.build_emb2pid(np.ascontiguousarray(ref.idx["doclens"], dtype=np.int64))
    for j in range(min(2, nq)):
        want = ref.oracle.retrieve(ref.idx["ivf"], ref.idx["ivf_lengths"], ref.idx["centroids"], emb2pid, ref.nprobe, Qs[:, :, j])
        assert np.array_equal(s.retrieve(Qs[:, :, j], nprobe=ref.nprobe), want + pid_offset), f"retrieve q={j}"
    auto = s.pass1_gather[0]
    try:
        for mode in modes:
            try:
                s.set_mode(mode)
            except clb.Unsupported:
                assert mode == 1
                continue
            for form in gather_forms:
                s.set_pass1_gather(form if form < 0 else (auto if form == 0 else 1 - auto))
                for k in ks:
                    for j in range(min(singles, nq)):
                        p, sc, n = s.search_batch(Qs[:, :, j:j + 1], k, nprobe=ref.nprobe, pad_short=True)
                        assert_result(p[:, 0], sc[:, 0], n[0], ref.ranking(j, k), k, f"single mode={mode} form={form} k={k} q={j}", pid_offset)
                    bp, bs, bn = s.search_batch(Qs, k, nprobe=ref.nprobe, pad_short=True)
                    for j in range(nq):
                        assert_result(bp[:, j], bs[:, j], bn[j], ref.ranking(j, k), k, f"batch mode={mode} form={form} k={k} q={j}", pid_offset)
    finally:
        s.set_pass1_gather(-1)


def check_like_fresh(s, idx, Qs, k, pid_offset=0, nprobe=2):
    """what the oracle does not compute, against a fresh Searcher of the full index, bit for bit"""
    fresh = clb.Searcher(index=idx, pid_offset=pid_offset)
    try:
        assert (s.num_docs, s.num_embeddings) == (fresh.num_docs, fresh.num_embeddings) == (idx["doclens"].size, idx["codes"].size)
        assert s.pass1_gather == fresh.pass1_gather
        assert np.array_equal(s.bound_consts.view(np.uint32), fresh.bound_consts.view(np.uint32)), (s.bound_consts, fresh.bound_consts)
        try:
            fresh.set_mode(1)
        except clb.Unsupported:         # no approximate pass for this shape: debug_scores does not apply
            return
        for mode in (0, 1):
            fresh.set_mode(mode); s.set_mode(mode)
            for j in range(min(2, Qs.shape[2])):
                a, b = s.debug_scores(Qs[:, :, j], k, nprobe=nprobe), fresh.debug_scores(Qs[:, :, j], k, nprobe=nprobe)
                what = f"debug_scores mode={mode} q={j}"
                assert a["n_rescore"] == b["n_rescore"], (what, a["n_rescore"], b["n_rescore"])
                assert np.array_equal(a["pids"], b["pids"]), what
                for name in ("eps", "tau"):
                    assert np.float32(a[name]).view(np.uint32) == np.float32(b[name]).view(np.uint32), (what, name, a[name], b[name])
                assert_same_f32(a["approx"], b["approx"], what + " approx")
                assert_same_f32(a["exact"], b["exact"], what + " exact")
    finally:
        fresh.close()


@pytest.fixture(scope="module")
def small(oracle):
    idx = synthetic.make_index(0, 300, K=64)
    Qs = synthetic.make_queries(idx, 1000, 9)
    return idx, Qs, Reference(oracle, idx, Qs)


def longest_in_tail_split(idx):
    """a split with the longest passage behind it (and not the only one there): max_doclen grows with the append"""
    p = int(np.argmax(idx["doclens"]))              # 0-based passage
    assert p >= 2 and idx["doclens"][p] > idx["doclens"][:p - 1].max()
    return p - 1


@pytest.mark.parametrize("split", ["299", "150", "1", "longest_in_tail"])
def test_append_small_splits(oracle, small, split):
    """300 passages, K = 64, exact and two-pass: one passage appended, half, all but one (tail far larger than the head, most
    centroids' first-ever entries in the tail), and a split that puts the longest passage into the tail."""
    idx, Qs, ref = small
    P = longest_in_tail_split(idx) if split == "longest_in_tail" else int(split)
    s = clb.Searcher(index=head_index(idx, P))
    try:
        assert s.generation == 0
        new = s.add_compressed(*tail(idx, P))
        assert new == range(P + 1, 301) and s.generation == 1
        check_search(s, ref, ks=(10,))
        # nprobe = 2 probes all 64 lists of this index; with one probe per token a query sees a part of them
        check_search(s, Reference(oracle, idx, Qs[:, :8, :], nprobe=1), ks=(10,), singles=1)
        check_like_fresh(s, idx, Qs, 10)
    finally:
        s.close()


def test_three_successive_appends_equal_one(small):
    idx, Qs, ref = small
    s = clb.Searcher(index=head_index(idx, 1))
    try:
        for a, b in ((1, 101), (101, 201), (201, 300)):
            assert s.add_compressed(*tail(idx, a, b)) == range(a + 1, b + 1)
        assert s.generation == 3
        assert s.add_compressed(np.zeros(0, np.uint32), np.zeros((32, 0), np.uint8, order="F"), np.zeros(0, np.int64)) == range(301, 301)
        assert s.generation == 3                    # an empty append changes nothing
        check_search(s, ref, ks=(10,))
        check_like_fresh(s, idx, Qs, 10)
    finally:
        s.close()


def test_workspaces_are_sized_again_after_an_append(oracle, small):
    """Search on the head first -- every workspace slot 0 buffer (bitmap words, candidate capacity from the head's list
    lengths, max_doclen) is then sized for 30 passages -- append ten times as many, search again."""
    idx, Qs, ref = small
    P = 30
    head = head_index(idx, P)
    s = clb.Searcher(index=head)
    try:
        check_search(s, Reference(oracle, head, Qs), ks=(10,))
        s.add_compressed(*tail(idx, P))
        check_search(s, ref, ks=(10,))
    finally:
        s.close()


@pytest.mark.parametrize("route", ["nbits4", "dim64", "pid_offset", "device_arrays"])
def test_append_other_kernel_routes(oracle, small, route):
    """nbits = 4 at dim 128 (the tuned exact path: its per-passage code order is applied to the new rows alone), dim = 64
    (the general path: no reordering, no tables), a passage shard (pid_offset = 1000), and clb_searcher_append_device."""
    import torch
    kw = {"nbits4": dict(nbits=4), "dim64": dict(dim=64, nbits=2)}.get(route, {})
    if kw:
        idx = synthetic.make_index(0, 300, K=64, **kw)
        Qs = synthetic.make_queries(idx, 1000, 9)
        ref = Reference(oracle, idx, Qs)
    else:
        idx, Qs, ref = small
    off = 1000 if route == "pid_offset" else 0
    P = 150
    s = clb.Searcher(index=head_index(idx, P), pid_offset=off)
    try:
        co, re, dl = tail(idx, P)
        if route == "device_arrays":
            dev = torch.device("cuda", 0)
            d_co = torch.from_numpy(co.view(np.int32).copy()).to(dev)
            d_re = torch.from_numpy(np.ascontiguousarray(re.T)).to(dev)
            keep = (d_co.clone(), d_re.clone())
            new = s.add_compressed(d_co, d_re, dl)
            assert torch.equal(d_co, keep[0]) and torch.equal(d_re, keep[1])       # the caller's arrays are not written
        else:
            new = s.add_compressed(co, re, dl)
        assert new == range(off + P + 1, off + 301)
        check_search(s, ref, ks=(10,), pid_offset=off)
        check_like_fresh(s, idx, Qs, 10, pid_offset=off)
    finally:
        s.close()


def test_append_medium_both_gather_forms(oracle):
    """20 000 passages, K = 2048, 2 000 appended to 18 000, k = 1000 and 10, exact and two-pass with either gather form."""
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 9)
    ref = Reference(oracle, idx, Qs)
    s = clb.Searcher(index=head_index(idx, 18_000))
    try:
        assert s.add_compressed(*tail(idx, 18_000)) == range(18_001, 20_001)
        check_search(s, ref, ks=(1000, 10), gather_forms=(0, 1), singles=2)
        check_like_fresh(s, idx, Qs, 1000)
    finally:
        s.close()


def test_filters_across_an_append(oracle, small):
    """A filter made before the append is refused with the documented error and the next unfiltered search is right; filters
    made afterwards over old and new pids match the composed oracle in both scopes."""
    idx, Qs, ref = small
    P = 150
    s = clb.Searcher(index=head_index(idx, P))
    try:
        old = s.make_filter(pids=np.arange(1, P + 1, 2))
        s.add_compressed(*tail(idx, P))
        with pytest.raises(clb.ArgumentError, match="filter made before an append; make another"):
            s.search_batch(Qs, 10, filters=old)
        with pytest.raises(clb.ArgumentError, match="filter made before an append; make another"):
            s.search_embeddings(Qs[:, :, 0], 10, filter=old, scope="all")
        old.close()
        check_search(s, ref, ks=(10,), modes=(1,), singles=1)
        allowed = [np.union1d(random_allowed(300, 0.3, 70 + j), [1, P, P + 1, 300]) for j in range(3)]
        for scope in ("candidates", "all"):
            check_filtered(oracle, s, idx, Qs[:, :, :3], allowed, scope, ks=(10,))
    finally:
        s.close()


def test_rejected_appends_leave_the_handle_usable(oracle, small):
    """A code of K + 1 (CLB_EDOMAIN, found on the device) and a doclens sum that is off by one (CLB_EDIMENSION): the
    generation and the counts are unchanged and the head still answers as its own oracle says; the append then succeeds."""
    idx, Qs, ref = small
    P = 150
    head = head_index(idx, P)
    s = clb.Searcher(index=head)
    try:
        href = Reference(oracle, head, Qs)
        check_search(s, href, ks=(10,), modes=(1,), singles=1)
        co, re, dl = tail(idx, P)
        bad = co.copy(); bad[bad.size // 2] = 65
        with pytest.raises(clb.DomainError):
            s.add_compressed(bad, re, dl)
        dl1 = dl.copy(); dl1[-1] += 1
        with pytest.raises(clb.DimensionMismatch):
            s.add_compressed(co, re, dl1)
        dl2 = dl.copy(); dl2[0] = -dl2[0]
        with pytest.raises(clb.ColBERTError):
            s.add_compressed(co, re, dl2)
        assert s.generation == 0 and (s.num_docs, s.num_embeddings) == (P, head["codes"].size)
        check_search(s, href, ks=(10,))
        s.add_compressed(co, re, dl)
        assert s.generation == 1
        check_search(s, ref, ks=(10,), modes=(1,), singles=1)
    finally:
        s.close()


def test_synced_bound_constants_are_never_lowered(small):
    """A handle whose bound constants were raised (a shard of a group) keeps the element-wise maximum of the old constants
    and the grown index's own."""
    idx, Qs, ref = small
    s = clb.Searcher(index=head_index(idx, 150))
    fresh = clb.Searcher(index=idx)
    try:
        raised = s.bound_consts * np.array([1, 1, 4, 1, 1, 1], np.float32)
        s.raise_bound_consts(raised)
        s.add_compressed(*tail(idx, 150))
        assert np.array_equal(s.bound_consts, np.maximum(raised, fresh.bound_consts))
        check_search(s, ref, ks=(10,), modes=(1,), singles=1)
    finally:
        s.close(); fresh.close()


def test_raised_bound_constants_read_back_as_the_maximum_and_switch_the_centroid_products(small):
    """raise_bound_consts(x) with x below the old value in some fields and above it in others: the constants read back are
    maximum(old, x), and the handle now counts as a shard of a group -- batches of 16+ queries default to the score table
    from one fp16 product (centroid_products 3 -> 1; the measured fp16 error of the centroids is what it was)."""
    idx, _, _ = small
    s = clb.Searcher(index=idx)
    try:
        old = s.bound_consts
        n, dc = s.centroid_products
        assert n == 3 and dc > 0 and (old > 0).all(), (n, dc, old)
        x = old * np.array([2, 0.5, 1, 0.25, 3, 0.5], np.float32)
        s.raise_bound_consts(x)
        assert np.array_equal(s.bound_consts, np.maximum(old, x))
        assert s.centroid_products == (1, dc)
    finally:
        s.close()


def test_add_embeddings_equals_add_compressed_of_the_oracle_codec(oracle, small):
    """50 passages of Gaussian-mixture embeddings compressed with the index's own centroids and cutoffs on the device, against
    oracle.compress of the same columns appended as codes and residuals."""
    idx, Qs, _ = small
    embs, dl = synthetic.make_embeddings(11, 50)
    co, re = oracle.compress(idx["centroids"], idx["bucket_cutoffs"], 128, 2, embs)
    full = dict(idx)
    full["codes"] = np.concatenate([idx["codes"], co]); full["doclens"] = np.concatenate([idx["doclens"], dl])
    full["residuals"] = np.asfortranarray(np.concatenate([idx["residuals"], re], axis=1))
    full["ivf"], full["ivf_lengths"] = synthetic.build_ivf(full["codes"], 64)
    # queries that land on the new passages too
    Qn = np.asfortranarray(np.concatenate([Qs[:, :, :3], synthetic.make_queries(full, 5, 6)], axis=2))
    ref = Reference(oracle, full, Qn)
    a, b = clb.Searcher(index=idx), clb.Searcher(index=idx)
    try:
        assert a.add_embeddings(embs, dl) == range(301, 351)
        assert b.add_compressed(co, re, dl) == range(301, 351)
        check_search(a, ref, ks=(10,))
        for j in range(3):
            x, y = a.debug_scores(Qn[:, :, 3 + j], 10), b.debug_scores(Qn[:, :, 3 + j], 10)
            assert np.array_equal(x["pids"], y["pids"]) and x["eps"] == y["eps"] and x["tau"] == y["tau"]
            assert_same_f32(x["exact"], y["exact"], "add_embeddings against add_compressed")
        noc = dict(idx); del noc["bucket_cutoffs"]
        c = clb.Searcher(index=noc)
        with pytest.raises(clb.ColBERTError, match="bucket_cutoffs"):
            c.add_embeddings(embs, dl)
        with pytest.raises(clb.ColBERTError, match="encoder"):
            c.add_passages(["hello world"])
        c.close()
    finally:
        a.close(); b.close()


def test_text_search_graph_is_captured_again_after_an_append(small, tmp_path):
    """TextSearch(graph=True) with a tiny random-weight encoder: one query, an append, the same query -- the session must
    notice the searcher's new generation, size and capture again, and answer as a fresh session on a fresh searcher of the
    full index does (the stale graph holds freed addresses and is never replayed)."""
    from colbert_jl_amd import tokenization
    from colbert_jl_amd.encoder import pack_weights
    from tests.test_encoder import VOCAB, _random_bert, _state
    idx, _, _ = small
    torch, cfg, bert, linear = _random_bert(hidden=64, layers=2, heads=4, inter=128, vocab=len(VOCAB), max_pos=64, dim=128, seed=5)
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = tokenization.WordPieceTokenizer(str(tmp_path / "vocab.txt"))
    config = clb.ColBERTConfig(doc_maxlen=24, query_maxlen=12, index_bsize=4, nbits=2)
    enc = clb.BertEncoder(pack_weights(_state(bert, linear), cfg.to_dict(), 128), cfg.to_dict(), dim=128, tokenizer=tok, config=config)
    s = clb.Searcher(index=head_index(idx, 150), encoder=enc, config=config)
    fresh = clb.Searcher(index=idx, encoder=enc, config=config)
    try:
        queries = ["hello world", "this is a test of the tokenizer"]
        ts = s.text_search(5, graph=True)
        before = [ts(q) for q in queries]
        assert ts.generation == 0 and ts.graph is not None
        stale = ts.graph
        s.add_compressed(*tail(idx, 150))
        got = [ts(q) for q in queries]
        assert ts.generation == 1 and ts.graph is not None and ts.graph is not stale
        want_ts = fresh.text_search(5, graph=True)
        for q, g, b in zip(queries, got, before):
            w = want_ts(q)
            assert np.array_equal(g[0], w[0]), q
            assert_same_f32(g[1], w[1], q)
            assert g[1][0] >= b[1][0]           # more passages: the best score cannot fall
        ts.close(); want_ts.close()
    finally:
        s.close(); fresh.close(); enc.close()
