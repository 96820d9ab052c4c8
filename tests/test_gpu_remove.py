"""Removing passages from a resident index (Searcher.remove_passages, clb_searcher_remove): after a removal the handle must be
indistinguishable from a fresh handle made from the reduced index -- the same index with the removed passages' columns
deleted, their doclens set to 0 (pids are stable) and ivf = build_ivf of the codes that are left.  Every case compares with
the CPU oracle searching the reduced index -- pids and candidate counts exact, fp32 scores bit-identical, exact and two-pass
-- and, for what the oracle does not have (eps, tau, the re-score count, the bound constants, the gather statistic), with a
fresh Searcher of the reduced index."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import storage, synthetic
from tests.test_append_cpu import write_index
from tests.test_gpu_append import Reference, check_like_fresh, check_search, head_index, tail
from tests.test_gpu_filtered_search import assert_same_f32, check_filtered, random_allowed
from tests.test_remove_cpu import emptying_set, reduced_index

pytestmark = pytest.mark.gpu


def check_reduced(oracle, s, idx, Qs, removed, k=10, pid_offset=0, **kw):
    """s, a handle on idx that `removed` (local 1-based pids) were removed from, against the oracle and a fresh handle on the
    reduced index; -> the reduced index"""
    red, _ = reduced_index(idx, removed)
    check_search(s, Reference(oracle, red, Qs), ks=(k,), pid_offset=pid_offset, **kw)
    check_like_fresh(s, red, Qs, k, pid_offset=pid_offset)
    assert s.num_docs == idx["doclens"].size and s.num_embeddings == red["codes"].size
    assert s.num_embeddings == int(clb.lib().clb_searcher_num_embeddings(s._h))
    return red


@pytest.fixture(scope="module")
def small(oracle):
    idx = synthetic.make_index(0, 300, K=64)
    Qs = synthetic.make_queries(idx, 1000, 9)
    return idx, Qs, Reference(oracle, idx, Qs)


def test_remove_the_top_ranked_passage_of_every_query(oracle, small):
    idx, Qs, ref = small
    top = np.unique([ref.ranking(j, 10)[0][0] for j in range(Qs.shape[2])])
    for j in range(Qs.shape[2]):
        assert np.isin(ref.ranking(j, 10)[0][:10], top).any()        # every old top-10 holds a removed pid: the answers must change
    s = clb.Searcher(index=idx)
    fresh = clb.Searcher(index=reduced_index(idx, top)[0])
    try:
        assert s.remove_passages(top) == top.size and s.generation == 1
        # before any search of either: the resident index takes what a fresh handle's takes
        assert s.device_bytes == fresh.device_bytes
        p, _, _ = s.search_batch(Qs, 10, pad_short=True)
        assert not np.isin(p, top).any()
        check_reduced(oracle, s, idx, Qs, top)
    finally:
        s.close(); fresh.close()


@pytest.mark.parametrize("which", ["first", "last", "longest"])
def test_remove_a_boundary_passage(oracle, small, which):
    """passage 1 alone, passage 300 alone, the longest passage (max_doclen shrinks as a fresh handle's does)"""
    idx, Qs, _ = small
    pid = {"first": 1, "last": 300, "longest": int(np.argmax(idx["doclens"])) + 1}[which]
    if which == "longest":
        assert np.count_nonzero(idx["doclens"] == idx["doclens"].max()) == 1
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages([pid]) == 1
        check_reduced(oracle, s, idx, Qs, [pid])
    finally:
        s.close()


@pytest.mark.parametrize("which", ["every_other", "all_but_one", "empties_a_list"])
def test_bulk_removals(oracle, small, which):
    idx, Qs, _ = small
    if which == "empties_a_list":
        removed, c = emptying_set(idx)
        assert idx["ivf_lengths"][c] > 0 and reduced_index(idx, removed)[0]["ivf_lengths"][c] == 0
    else:
        removed = {"every_other": np.arange(1, 301, 2), "all_but_one": np.delete(np.arange(1, 301), 122)}[which]
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages(removed) == removed.size
        check_reduced(oracle, s, idx, Qs, removed)
    finally:
        s.close()


def test_pid_lists_duplicates_order_repeats_and_empty(oracle, small):
    idx, Qs, _ = small
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages(np.zeros(0, np.int64)) == 0 and s.generation == 0          # n = 0
        assert s.remove_passages([250, 7, 250, 300, 7, 7, 1, 64, 33, 32]) == 7 and s.generation == 1
        removed = [1, 7, 32, 33, 64, 250, 300]
        red = check_reduced(oracle, s, idx, Qs, removed)
        # the same pids again: nothing to remove, nothing changes
        assert s.remove_passages([7, 300]) == 0 and s.generation == 1
        assert s.remove_passages(np.zeros(0, np.int64)) == 0 and s.generation == 1
        assert s.num_embeddings == red["codes"].size
        # one already empty passage beside one that is not
        assert s.remove_passages([7, 8]) == 1 and s.generation == 2
        check_reduced(oracle, s, idx, Qs, removed + [8], modes=(1,), singles=1)
    finally:
        s.close()


def test_three_successive_removals_equal_one_of_the_union(oracle, small):
    idx, Qs, _ = small
    parts = [np.arange(1, 301, 7), np.arange(100, 140), np.array([300, 299, 2])]
    s = clb.Searcher(index=idx)
    try:
        done = np.zeros(0, np.int64)
        for part in parts:
            assert s.remove_passages(part) == np.setdiff1d(part, done).size      # the second part names five of the first again
            done = np.union1d(done, part)
        assert s.generation == 3
        check_reduced(oracle, s, idx, Qs, np.unique(np.concatenate(parts)))
    finally:
        s.close()


def removed_then_appended(idx):
    """[1-150 | 150 empty passages | passages 151-300 again, as 301-450], ivf = build_ivf of its codes"""
    a = int(idx["doclens"][:150].sum())
    r = dict(idx)
    r["codes"] = np.concatenate([idx["codes"][:a], idx["codes"][a:]])
    r["residuals"] = np.asfortranarray(idx["residuals"])
    r["doclens"] = np.concatenate([idx["doclens"][:150], np.zeros(150, np.int64), idx["doclens"][150:]])
    r["ivf"], r["ivf_lengths"] = synthetic.build_ivf(r["codes"], idx["ivf_lengths"].size)
    return r


def test_remove_then_append_the_same_passages(oracle, small):
    idx, Qs, _ = small
    want = removed_then_appended(idx)
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages(np.arange(151, 301)) == 150
        assert s.add_compressed(*tail(idx, 150)) == range(301, 451)
        assert s.generation == 2
        check_search(s, Reference(oracle, want, Qs), ks=(10,))
        check_like_fresh(s, want, Qs, 10)
    finally:
        s.close()


def test_append_then_remove_some_of_the_appended(oracle, small):
    idx, Qs, _ = small
    s = clb.Searcher(index=head_index(idx, 150))
    try:
        s.add_compressed(*tail(idx, 150))
        removed = np.array([151, 300, 222, 10, 150, 223])
        assert s.remove_passages(removed) == 6 and s.generation == 2
        check_reduced(oracle, s, idx, Qs, removed)
    finally:
        s.close()


@pytest.mark.parametrize("route", ["nbits4", "dim64", "dim24_nbits8", "dim8_nbits1", "pid_offset"])
def test_remove_other_kernel_routes(oracle, small, route):
    """nbits = 4 at dim 128 (64-byte rows: four 16-byte pieces), dim = 64 (the general path: no tables, the caller's row
    order), the general path's other row sizes (24 bytes: copied as 4-byte pieces; 1 byte: as bytes), a passage shard
    (pid_offset = 1000: pids carry the offset, one without it is out of bounds)."""
    kw = {"nbits4": dict(nbits=4), "dim64": dict(dim=64, nbits=2), "dim24_nbits8": dict(dim=24, nbits=8),
          "dim8_nbits1": dict(dim=8, nbits=1)}.get(route, {})
    if kw:
        idx = synthetic.make_index(0, 300, K=64, **kw)
        Qs = synthetic.make_queries(idx, 1000, 9)
    else:
        idx, Qs, _ = small
    off = 1000 if route == "pid_offset" else 0
    removed = np.concatenate([np.arange(2, 300, 3), [1, 300]])
    s = clb.Searcher(index=idx, pid_offset=off)
    try:
        if off:
            with pytest.raises(clb.BoundsError):
                s.remove_passages(removed)
            assert s.generation == 0 and s.num_embeddings == idx["codes"].size
        assert s.remove_passages(removed + off) == removed.size
        check_reduced(oracle, s, idx, Qs, removed, pid_offset=off)
    finally:
        s.close()


def test_rejected_removals_leave_the_handle_usable(small):
    idx, Qs, ref = small
    l = clb.lib()
    s = clb.Searcher(index=idx)
    try:
        for bad in ([5, 0], [301, 5], [-3]):
            with pytest.raises(clb.BoundsError, match="outside 1..300"):
                s.remove_passages(bad)
        n = C.c_int64(9)
        assert l.clb_searcher_remove(s._h, None, C.c_int64(2), C.byref(n)) == 4 and n.value == 0
        one = np.array([5], np.int64)
        assert l.clb_searcher_remove(s._h, one.ctypes.data_as(C.c_void_p), C.c_int64(-1), None) == 4
        assert s.generation == 0 and (s.num_docs, s.num_embeddings) == (300, idx["codes"].size)
        assert s.num_embeddings == int(l.clb_searcher_num_embeddings(s._h))
        check_search(s, ref, ks=(10,))
        check_like_fresh(s, idx, Qs, 10)
    finally:
        s.close()


def test_filters_across_a_removal(oracle, small):
    """A filter made BEFORE the removal over removed and kept pids is still accepted and gives, in both scopes, exactly what a
    fresh Searcher of the reduced index gives with a filter of the same pids -- in scope "all" too, where the set names empty
    passages: they hold nothing to score and are no candidates; filters made afterwards match the composed oracle."""
    idx, Qs, _ = small
    removed = np.arange(1, 301, 3)
    red, _ = reduced_index(idx, removed)
    alloweds = [np.union1d(random_allowed(300, 0.3, 40 + j), [1, 2, 3, 4, 299, 300]) for j in range(3)]
    for a in alloweds:
        assert np.isin(a, removed).any() and not np.isin(a, removed).all()
    s = clb.Searcher(index=idx)
    fresh = clb.Searcher(index=red)
    try:
        before = [s.make_filter(pids=a) for a in alloweds]
        same = [fresh.make_filter(pids=a) for a in alloweds]
        assert s.remove_passages(removed) == removed.size
        Q3 = np.asfortranarray(Qs[:, :, :3])
        for scope in ("candidates", "all"):
            for mode in (0, 1):
                s.set_mode(mode); fresh.set_mode(mode)
                got, want = s.search_batch(Q3, 10, filters=before, scope=scope), fresh.search_batch(Q3, 10, filters=same, scope=scope)
                what = f"scope={scope} mode={mode}"
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), what
                assert_same_f32(got[1], want[1], what)
                p, sc = s.search_embeddings(Q3[:, :, 0], 10, filter=before[0], scope=scope)
                assert np.array_equal(p, want[0][:, 0]), what
                assert_same_f32(sc, want[1][:, 0], what)
            assert not np.isin(got[0], removed).any()        # an empty passage is no candidate, in either scope
            if scope == "all":                                 # ... so the candidates are the set's passages that hold embeddings
                assert [int(n) for n in got[2]] == [np.setdiff1d(a, removed).size for a in alloweds]
        for f in before + same:
            f.close()
        check_filtered(oracle, s, red, Q3, alloweds, "candidates", ks=(10,))
    finally:
        s.close(); fresh.close()


def test_workspaces_are_sized_again_after_a_removal(oracle, small):
    """Search first -- every buffer of workspace slot 0 is sized for the whole index -- remove most of it, search again."""
    idx, Qs, ref = small
    s = clb.Searcher(index=idx)
    try:
        check_search(s, ref, ks=(10,))
        removed = np.arange(31, 301)
        assert s.remove_passages(removed) == 270
        check_reduced(oracle, s, idx, Qs, removed)
    finally:
        s.close()


def test_synced_bound_constants_are_never_lowered_by_a_removal(oracle, small):
    idx, Qs, _ = small
    removed = np.arange(1, 301, 2)
    red, _ = reduced_index(idx, removed)
    s = clb.Searcher(index=idx)
    fresh = clb.Searcher(index=red)
    try:
        raised = s.bound_consts * np.array([1, 1, 4, 1, 1, 1], np.float32)
        s.raise_bound_consts(raised)
        before = s.bound_consts
        assert s.remove_passages(removed) == removed.size
        assert np.all(s.bound_consts >= before)
        assert np.array_equal(s.bound_consts, np.maximum(before, fresh.bound_consts))
        check_search(s, Reference(oracle, red, Qs), ks=(10,), modes=(1,), singles=1)
    finally:
        s.close(); fresh.close()


def test_text_search_graph_is_captured_again_after_a_removal(small, tmp_path):
    """TextSearch(graph=True) with a tiny random-weight encoder: one query, a removal, the same query -- the session must
    notice the searcher's new generation, size and capture again, and answer as a fresh session on a fresh searcher of the
    reduced index does (the stale graph holds freed addresses and is never replayed)."""
    from colbert_jl_amd import tokenization
    from colbert_jl_amd.encoder import pack_weights
    from tests.test_encoder import VOCAB, _random_bert, _state
    idx, _, _ = small
    torch, cfg, bert, linear = _random_bert(hidden=64, layers=2, heads=4, inter=128, vocab=len(VOCAB), max_pos=64, dim=128, seed=5)
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = tokenization.WordPieceTokenizer(str(tmp_path / "vocab.txt"))
    config = clb.ColBERTConfig(doc_maxlen=24, query_maxlen=12, index_bsize=4, nbits=2)
    enc = clb.BertEncoder(pack_weights(_state(bert, linear), cfg.to_dict(), 128), cfg.to_dict(), dim=128, tokenizer=tok, config=config)
    s = clb.Searcher(index=idx, encoder=enc, config=config)
    try:
        queries = ["hello world", "this is a test of the tokenizer"]
        ts = s.text_search(5, graph=True)
        before = [ts(q) for q in queries]
        assert ts.generation == 0 and ts.graph is not None
        stale = ts.graph
        removed = np.unique(np.concatenate([b[0][:2] for b in before]))         # the two best passages of either query
        fresh = clb.Searcher(index=reduced_index(idx, removed)[0], encoder=enc, config=config)
        try:
            assert s.remove_passages(removed) == removed.size
            got = [ts(q) for q in queries]
            assert ts.generation == 1 and ts.graph is not None and ts.graph is not stale
            want_ts = fresh.text_search(5, graph=True)
            for q, g, b in zip(queries, got, before):
                w = want_ts(q)
                assert np.array_equal(g[0], w[0]), q
                assert_same_f32(g[1], w[1], q)
                assert not np.isin(g[0], removed).any() and g[1][0] <= b[1][0]   # fewer passages: the best score cannot rise
            ts.close(); want_ts.close()
        finally:
            fresh.close()
    finally:
        s.close(); enc.close()


def test_remove_medium_both_gather_forms(oracle):
    """20 000 passages, K = 2048, 2 000 random passages removed, k = 1000 and 10, exact and two-pass with either gather form."""
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 9)
    removed = np.random.default_rng(17).choice(20_000, 2_000, replace=False) + 1
    red, _ = reduced_index(idx, removed)
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages(removed) == 2_000
        check_search(s, Reference(oracle, red, Qs), ks=(1000, 10), gather_forms=(0, 1), singles=2)
        check_like_fresh(s, red, Qs, 1000)
        assert s.num_docs == 20_000 and s.num_embeddings == red["codes"].size
    finally:
        s.close()


def test_persisted_removal_reopens_as_the_live_searcher(oracle, small, tmp_path):
    idx, Qs, _ = small
    path = str(tmp_path / "index")
    write_index(path, idx, 150)
    storage.append_chunk(path, *[np.asarray(a) for a in tail(idx, 150)])
    removed = np.array([150, 151, 9, 290])
    s = clb.Searcher(path)
    try:
        assert s.remove_passages(removed, persist=True) == 4
        again = clb.Searcher(path)
        try:
            assert (again.num_docs, again.num_embeddings) == (s.num_docs, s.num_embeddings)
            a, b = s.search_batch(Qs, 10, pad_short=True), again.search_batch(Qs, 10, pad_short=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
            assert_same_f32(a[1], b[1], "reopened against live")
        finally:
            again.close()
        check_reduced(oracle, s, idx, Qs, removed, modes=(1,), singles=1)
        got = storage.load_index(path)
        assert np.all(got["doclens"][removed - 1] == 0)
    finally:
        s.close()
