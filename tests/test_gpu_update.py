"""Replacing passages of a resident index in place (Searcher.update_compressed / update_embeddings, clb_searcher_update): after
an update the handle must be indistinguishable from a fresh handle made from the updated index -- the same index with the named
passages' columns replaced, their doclens set (pids are stable) and ivf = build_ivf of the spliced codes
(tests/test_update_cpu.updated_index).  Every case compares with the CPU oracle searching that index -- pids and candidate
counts exact, fp32 scores bit-identical, exact and two-pass -- and, for what the oracle does not have (eps, tau, the re-score
count, the bound constants, the gather statistic), with a fresh Searcher of it."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import storage, synthetic
from tests.test_append_cpu import write_index
from tests.test_gpu_append import Reference, check_like_fresh, check_search, tail
from tests.test_gpu_filtered_search import assert_same_f32, check_filtered, random_allowed
from tests.test_remove_cpu import emptying_set, reduced_index
from tests.test_update_cpu import content_of, updated_index

pytestmark = pytest.mark.gpu


def check_updated(oracle, s, want, Qs, k=10, pid_offset=0, nprobe=2, **kw):
    """s against the oracle and a fresh handle on `want`, the index it should hold now"""
    check_search(s, Reference(oracle, want, Qs, nprobe=nprobe), ks=(k,), pid_offset=pid_offset, **kw)
    check_like_fresh(s, want, Qs, k, pid_offset=pid_offset, nprobe=nprobe)
    assert s.num_docs == want["doclens"].size and s.num_embeddings == want["codes"].size
    assert s.num_embeddings == int(clb.lib().clb_searcher_num_embeddings(s._h))


def joined(idx, donors):
    """the columns of the passages `donors` as the content of ONE passage"""
    co, re, dl = content_of(idx, donors)
    return co, re, np.array([dl.sum()], np.int64)


def state(s, Qs, k=10):
    """what two handles of the same index agree on, bit for bit"""
    out = [s.num_docs, s.num_embeddings, s.pass1_gather, s.bound_consts.tobytes()]
    for mode in (0, 1):
        s.set_mode(mode)
        p, sc, n = s.search_batch(Qs, k, pad_short=True)
        out += [p.tobytes(), sc.tobytes(), n.tobytes()]
    return out


@pytest.fixture(scope="module")
def small(oracle):
    idx = synthetic.make_index(0, 300, K=64)
    Qs = synthetic.make_queries(idx, 1000, 9)
    return idx, Qs, Reference(oracle, idx, Qs)


def test_replace_the_top_ranked_passage_of_every_query_by_low_ranked_content(oracle, small):
    idx, Qs, ref = small
    top = np.unique([ref.ranking(j, 10)[0][0] for j in range(Qs.shape[2])])
    last = np.unique(np.concatenate([ref.ranking(j, 10)[0][-3:] for j in range(Qs.shape[2])]))
    donors = np.setdiff1d(last, top)[:top.size]
    assert donors.size == top.size
    args = (top, *content_of(idx, donors))
    want = updated_index(idx, *args)
    s = clb.Searcher(index=idx)
    fresh = clb.Searcher(index=want)
    try:
        assert s.update_compressed(*args) == top.size and s.generation == 1
        # before any search of either: the resident index takes what a fresh handle's takes
        assert s.device_bytes == fresh.device_bytes
        after = s.search_batch(Qs, 10, pad_short=True)
        for j in range(Qs.shape[2]):            # every old top-10 held a replaced passage: every answer changed
            old_p, old_s = ref.ranking(j, 10)
            assert not (np.array_equal(old_p[:10], after[0][:, j]) and np.array_equal(old_s[:10], after[1][:, j])), j
        check_updated(oracle, s, want, Qs)
    finally:
        s.close(); fresh.close()


@pytest.mark.parametrize("which", ["first", "last", "longest_shrinks", "longer_than_any"])
def test_replace_a_boundary_passage(oracle, small, which):
    """passage 1 alone, passage 300 alone, the unique longest passage by the shortest (max_doclen shrinks as a fresh handle's
    does), a passage by one longer than any other (max_doclen grows)"""
    idx, Qs, _ = small
    longest, shortest = int(np.argmax(idx["doclens"])) + 1, int(np.argmin(idx["doclens"])) + 1
    assert np.count_nonzero(idx["doclens"] == idx["doclens"].max()) == 1
    pid, content = {"first": (1, content_of(idx, [150])), "last": (300, content_of(idx, [150])),
                    "longest_shrinks": (longest, content_of(idx, [shortest])),
                    "longer_than_any": (17, joined(idx, [longest, shortest]))}[which]
    want = updated_index(idx, [pid], *content)
    if which == "longest_shrinks":
        assert want["doclens"].max() < idx["doclens"].max()
    if which == "longer_than_any":
        assert pid != longest and want["doclens"][pid - 1] > idx["doclens"].max()
    s = clb.Searcher(index=idx)
    try:
        assert s.update_compressed([pid], *content) == 1
        check_updated(oracle, s, want, Qs)
    finally:
        s.close()


def test_new_length_zero_equals_remove_passages(oracle, small):
    idx, Qs, _ = small
    pids = np.array([290, 3, 151, 150, 77])
    rows = idx["residuals"].shape[0]
    a, b = clb.Searcher(index=idx), clb.Searcher(index=idx)
    try:
        assert a.update_compressed(pids, np.zeros(0, np.uint32), np.zeros((rows, 0), np.uint8, order="F"), np.zeros(5, np.int64)) == 5
        assert b.remove_passages(pids) == 5
        assert state(a, Qs) == state(b, Qs)
        check_updated(oracle, a, reduced_index(idx, pids)[0], Qs)
        # naming them again with length 0: nothing had or has embeddings
        assert a.update_compressed(pids, np.zeros(0, np.uint32), np.zeros((rows, 0), np.uint8, order="F"), np.zeros(5, np.int64)) == 0
        assert a.generation == 1
    finally:
        a.close(); b.close()


def test_refill_a_passage_that_a_removal_emptied(oracle, small):
    idx, Qs, _ = small
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages([5, 6, 300]) == 3
        args = ([300, 5], *content_of(idx, [300, 44]))          # 300 gets its own content back, 5 another's; 6 stays empty
        assert s.update_compressed(*args) == 2 and s.generation == 2
        check_updated(oracle, s, updated_index(reduced_index(idx, [5, 6, 300])[0], *args), Qs)
    finally:
        s.close()


def test_replace_all_passages(oracle, small):
    """every passage gets the content of the passage 7 behind it (mod 300): no old row is kept"""
    idx, Qs, _ = small
    pids = np.arange(1, 301)
    args = (pids, *content_of(idx, (pids + 6) % 300 + 1))
    s = clb.Searcher(index=idx)
    try:
        assert s.update_compressed(*args) == 300
        check_updated(oracle, s, updated_index(idx, *args), Qs)
    finally:
        s.close()


def test_replace_by_identical_content(oracle, small):
    idx, Qs, ref = small
    pids = np.array([1, 64, 65, 299, 300])
    s = clb.Searcher(index=idx)
    try:
        before = state(s, Qs)
        assert s.update_compressed(pids, *content_of(idx, pids)) == 5 and s.generation == 1
        assert state(s, Qs) == before
        check_search(s, ref, ks=(10,), modes=(1,), singles=1)
    finally:
        s.close()


def test_pid_order_does_not_matter(oracle, small):
    idx, Qs, _ = small
    pids = np.array([2, 64, 65, 128, 150, 151, 299])
    donors = np.array([201, 202, 203, 204, 205, 206, 207])
    states = []
    for order in (np.arange(7), np.arange(7)[::-1], np.random.default_rng(3).permutation(7)):
        s = clb.Searcher(index=idx)
        try:
            assert s.update_compressed(pids[order], *content_of(idx, donors[order])) == 7
            states.append(state(s, Qs))
            if len(states) == 3:
                check_updated(oracle, s, updated_index(idx, pids, *content_of(idx, donors)), Qs)
        finally:
            s.close()
    assert states[0] == states[1] == states[2]


def test_rejected_updates_leave_the_handle_usable(small):
    idx, Qs, ref = small
    l = clb.lib()
    s = clb.Searcher(index=idx)
    try:
        co, re, dl = content_of(idx, [10, 11])
        with pytest.raises(clb.ArgumentError, match="pid 5 is named twice"):
            s.update_compressed([5, 5], co, re, dl)
        for bad in ([5, 0], [301, 5], [-3, 5]):
            with pytest.raises(clb.BoundsError, match="outside 1..300"):
                s.update_compressed(bad, co, re, dl)
        for code in (0, 65):
            wrong = co.copy(); wrong[wrong.size // 2] = code
            with pytest.raises(clb.DomainError):
                s.update_compressed([5, 6], wrong, re, dl)
        dl1 = dl.copy(); dl1[-1] += 1
        with pytest.raises(clb.DimensionMismatch):
            s.update_compressed([5, 6], co, re, dl1)
        dl2 = dl.copy(); dl2[0] = -dl2[0]
        with pytest.raises(clb.ArgumentError):
            s.update_compressed([5, 6], co, re, dl2)
        n = C.c_int64(9)
        assert l.clb_searcher_update(s._h, C.c_int64(2), None, None, C.c_int64(0), None, None, C.byref(n)) == 4 and n.value == 0
        assert l.clb_searcher_update(s._h, C.c_int64(-1), None, None, C.c_int64(0), None, None, None) == 4
        # n = 0 does nothing
        rows = idx["residuals"].shape[0]
        assert s.update_compressed(np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros((rows, 0), np.uint8, order="F"), np.zeros(0, np.int64)) == 0
        assert s.generation == 0 and (s.num_docs, s.num_embeddings) == (300, idx["codes"].size)
        check_search(s, ref, ks=(10,))
        check_like_fresh(s, idx, Qs, 10)
    finally:
        s.close()


def test_an_update_that_empties_a_list_and_one_that_fills_it_again(oracle, small):
    idx, Qs, _ = small
    pids, c = emptying_set(idx)
    # replacement rows whose codes avoid centroid c: the other passages' rows that are not of c, dealt out 30 to a passage
    emb2pid = np.repeat(np.arange(1, 301), idx["doclens"])
    free = np.nonzero(~np.isin(emb2pid, pids) & (idx["codes"].astype(np.int64) != c + 1))[0][:30 * pids.size]
    args = (pids, idx["codes"][free], np.asfortranarray(idx["residuals"][:, free]), np.full(pids.size, 30, np.int64))
    emptied = updated_index(idx, *args)
    assert idx["ivf_lengths"][c] > 0 and emptied["ivf_lengths"][c] == 0
    s = clb.Searcher(index=idx)
    try:
        assert s.update_compressed(*args) == pids.size
        check_updated(oracle, s, emptied, Qs)
        back = (pids[:2], *content_of(idx, pids[:2]))           # their old content: list c holds entries again
        filled = updated_index(emptied, *back)
        assert filled["ivf_lengths"][c] > 0
        assert s.update_compressed(*back) == 2
        check_updated(oracle, s, filled, Qs, modes=(1,), singles=1)
    finally:
        s.close()


def test_a_handle_with_lists_in_the_callers_order(oracle, small):
    """every list permuted internally: the handle keeps the caller's order for the kept entries and puts the new ones behind
    them; results do not depend on the order inside a list"""
    idx, Qs, _ = small
    rng = np.random.default_rng(62)
    ivf = idx["ivf"].copy()
    off = np.concatenate([[0], np.cumsum(idx["ivf_lengths"])])
    for c in range(64):
        ivf[off[c]:off[c + 1]] = rng.permutation(ivf[off[c]:off[c + 1]])
    pids = np.array([300, 1, 64, 150, 151, 77])
    co, re, dl = content_of(idx, [9, 8, 7, 6, 5, 4])
    cut = int(dl[:5].sum())
    args = (pids, co[:cut], np.asfortranarray(re[:, :cut]), np.append(dl[:5], 0))       # 77 is emptied
    want = updated_index(idx, *args)
    s = clb.Searcher(index=dict(idx, ivf=ivf))
    try:
        assert s.update_compressed(*args) == 6
        check_search(s, Reference(oracle, want, Qs), ks=(10,))
        assert s.num_embeddings == want["codes"].size
    finally:
        s.close()


def test_three_successive_updates_equal_one_of_the_union(oracle, small):
    """later content wins: passage 120 is named by all three"""
    idx, Qs, _ = small
    parts = [(np.arange(100, 140), np.arange(1, 41)), (np.array([120, 300, 1]), np.array([50, 51, 52])),
             (np.array([2, 120]), np.array([60, 61]))]
    final = {}
    s, one = clb.Searcher(index=idx), clb.Searcher(index=idx)
    try:
        for pids, donors in parts:
            assert s.update_compressed(pids, *content_of(idx, donors)) == pids.size
            final.update(zip(pids.tolist(), donors.tolist()))
        assert s.generation == 3
        pids = np.array(sorted(final))
        donors = np.array([final[p] for p in pids])
        assert one.update_compressed(pids, *content_of(idx, donors)) == pids.size
        assert state(s, Qs) == state(one, Qs)
        check_updated(oracle, s, updated_index(idx, pids, *content_of(idx, donors)), Qs)
    finally:
        s.close(); one.close()


def test_update_append_remove_update(oracle, small):
    idx, Qs, _ = small
    head = 250
    n = int(idx["doclens"][:head].sum())
    model = dict(idx, codes=idx["codes"][:n], residuals=np.asfortranarray(idx["residuals"][:, :n]), doclens=idx["doclens"][:head])
    model["ivf"], model["ivf_lengths"] = synthetic.build_ivf(model["codes"], 64)
    s = clb.Searcher(index=model)
    try:
        a1 = (np.array([250, 1, 100]), *content_of(idx, [260, 261, 262]))
        assert s.update_compressed(*a1) == 3
        model = updated_index(model, *a1)
        check_updated(oracle, s, model, Qs, modes=(1,), singles=1)
        assert s.add_compressed(*tail(idx, head)) == range(251, 301)
        co, re, dl = tail(idx, head)
        model = dict(model, codes=np.concatenate([model["codes"], co]), doclens=np.concatenate([model["doclens"], dl]),
                     residuals=np.asfortranarray(np.concatenate([model["residuals"], re], axis=1)))
        model["ivf"], model["ivf_lengths"] = synthetic.build_ivf(model["codes"], 64)
        check_updated(oracle, s, model, Qs, modes=(1,), singles=1)
        removed = np.array([1, 251, 300, 17])
        assert s.remove_passages(removed) == 4
        model = reduced_index(model, removed)[0]
        check_updated(oracle, s, model, Qs, modes=(1,), singles=1)
        a2 = (np.array([300, 17, 299, 2]), *content_of(idx, [1, 2, 3, 4]))       # two emptied passages, two live ones
        assert s.update_compressed(*a2) == 4 and s.generation == 4
        model = updated_index(model, *a2)
        check_updated(oracle, s, model, Qs)
    finally:
        s.close()


def test_filters_made_before_an_update_stay_valid(oracle, small):
    idx, Qs, _ = small
    pids = np.arange(1, 301, 3)
    co, re, dl = content_of(idx, (pids + 100) % 300 + 1)
    dl = dl.copy()
    keep = np.ones(co.size, bool)
    off = np.concatenate([[0], np.cumsum(dl)])
    for i in range(0, pids.size, 4):            # every fourth named passage is emptied
        keep[off[i]:off[i + 1]] = False
        dl[i] = 0
    args = (pids, co[keep], np.asfortranarray(re[:, keep]), dl)
    want = updated_index(idx, *args)
    alloweds = [np.union1d(random_allowed(300, 0.3, 40 + j), [1, 2, 3, 4, 299, 300]) for j in range(3)]
    s = clb.Searcher(index=idx)
    fresh = clb.Searcher(index=want)
    try:
        before = [s.make_filter(pids=a) for a in alloweds]
        same = [fresh.make_filter(pids=a) for a in alloweds]
        assert s.update_compressed(*args) == pids.size
        Q3 = np.asfortranarray(Qs[:, :, :3])
        for scope in ("candidates", "all"):
            for mode in (0, 1):
                s.set_mode(mode); fresh.set_mode(mode)
                got, exp = s.search_batch(Q3, 10, filters=before, scope=scope), fresh.search_batch(Q3, 10, filters=same, scope=scope)
                what = f"scope={scope} mode={mode}"
                assert np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[2]), what
                assert_same_f32(got[1], exp[1], what)
        for f in before + same:
            f.close()
        check_filtered(oracle, s, want, Q3, alloweds, "candidates", ks=(10,))
    finally:
        s.close(); fresh.close()


def test_device_tensors_through_update_device(oracle, small):
    import torch
    idx, Qs, _ = small
    pids = np.array([300, 7, 150])
    co, re, dl = content_of(idx, [20, 21, 22])
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(co.view(np.int32).copy()).to(dev)
    d_re = torch.from_numpy(np.ascontiguousarray(re.T)).to(dev)
    keep = (d_co.clone(), d_re.clone())
    s = clb.Searcher(index=idx)
    try:
        assert s.update_compressed(pids, d_co, d_re, dl) == 3
        assert torch.equal(d_co, keep[0]) and torch.equal(d_re, keep[1])       # the caller's arrays are not written
        check_updated(oracle, s, updated_index(idx, pids, co, re, dl), Qs)
    finally:
        s.close()


def test_update_embeddings_equals_update_compressed_of_the_oracle_codec(oracle, small):
    idx, Qs, _ = small
    embs, dl = synthetic.make_embeddings(11, 50)
    co, re = oracle.compress(idx["centroids"], idx["bucket_cutoffs"], 128, 2, embs)
    pids = np.arange(5, 300, 5)[:50]
    want = updated_index(idx, pids, co, re, dl)
    Qn = np.asfortranarray(np.concatenate([Qs[:, :, :3], synthetic.make_queries(want, 5, 6)], axis=2))
    a, b = clb.Searcher(index=idx), clb.Searcher(index=idx)
    try:
        assert a.update_embeddings(pids, embs, dl) == 50
        assert b.update_compressed(pids, co, re, dl) == 50
        assert state(a, Qn) == state(b, Qn)
        check_search(a, Reference(oracle, want, Qn), ks=(10,))
        noc = dict(idx); del noc["bucket_cutoffs"]
        c = clb.Searcher(index=noc)
        with pytest.raises(clb.ColBERTError, match="bucket_cutoffs"):
            c.update_embeddings(pids, embs, dl)
        with pytest.raises(clb.ColBERTError, match="encoder"):
            c.update_passages([1], ["hello world"])
        c.close()
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("route", ["nbits1", "nbits4", "dim64", "dim24_nbits8", "general_case_4", "pid_offset"])
def test_update_other_kernel_routes(oracle, small, route):
    """dim 128 with nbits 1 and 4 (16- and 64-byte rows: one and four 16-byte pieces), the general path (no tables, the
    caller's row order) with 16-byte rows, 24-byte rows (copied as 4-byte pieces) and row 4 of tests/util_general.CASES (dim
    136: 34-byte rows, copied as bytes), and a passage shard (pid_offset = 1000: pids carry the offset)."""
    from tests.util_general import CASE_K, case_inputs
    kw = {"nbits1": dict(nbits=1), "nbits4": dict(nbits=4), "dim64": dict(dim=64, nbits=2), "dim24_nbits8": dict(dim=24, nbits=8)}.get(route)
    k, nprobe = 10, 2
    if kw:
        idx = synthetic.make_index(0, 300, K=64, **kw)
        Qs = synthetic.make_queries(idx, 1000, 9)
    elif route == "general_case_4":
        idx, Qs, nprobe = case_inputs(4)
        k = CASE_K
    else:
        idx, Qs, _ = small
    n_docs = idx["doclens"].size
    off = 1000 if route == "pid_offset" else 0
    pids = np.concatenate([np.arange(2, n_docs, 3), [1, n_docs]])
    co, re, dl = content_of(idx, (pids + 100) % n_docs + 1)
    keep = np.ones(co.size, bool)
    o = np.concatenate([[0], np.cumsum(dl)])
    dl = dl.copy()
    for i in range(0, pids.size, 5):            # every fifth named passage is emptied
        keep[o[i]:o[i + 1]] = False
        dl[i] = 0
    args = (co[keep], np.asfortranarray(re[:, keep]), dl)
    s = clb.Searcher(index=idx, pid_offset=off)
    try:
        if off:
            with pytest.raises(clb.BoundsError):
                s.update_compressed(pids, *args)
            assert s.generation == 0 and s.num_embeddings == idx["codes"].size
        assert s.update_compressed(pids + off, *args) == pids.size
        check_updated(oracle, s, updated_index(idx, pids, *args), Qs, k=k, pid_offset=off, nprobe=nprobe)
    finally:
        s.close()


def test_workspaces_are_sized_again_after_an_update(oracle, small):
    """Search first -- every buffer of workspace slot 0 is sized for the index as it is -- then make every tenth passage four
    times as long, search again."""
    idx, Qs, ref = small
    pids = np.arange(10, 301, 10)
    parts = [joined(idx, [p, p + 1 if p < 300 else 1, p - 1, p - 2]) for p in pids]
    args = (pids, np.concatenate([x[0] for x in parts]), np.asfortranarray(np.concatenate([x[1] for x in parts], axis=1)),
            np.concatenate([x[2] for x in parts]))
    s = clb.Searcher(index=idx)
    try:
        check_search(s, ref, ks=(10,))
        assert s.update_compressed(*args) == pids.size
        check_updated(oracle, s, updated_index(idx, *args), Qs)
    finally:
        s.close()


def test_text_search_graph_is_captured_again_after_an_update(small, tmp_path):
    """TextSearch(graph=True) with a tiny random-weight encoder: one query, an update, the same query -- the session must
    notice the searcher's new generation, size and capture again, and answer as a fresh session on a fresh searcher of the
    updated index does (the stale graph holds freed addresses and is never replayed)."""
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
        pids = np.unique(np.concatenate([b[0][:2] for b in before]))         # the two best passages of either query
        donors = np.setdiff1d(np.arange(1, 301), np.concatenate([b[0] for b in before]))[:pids.size]
        args = (pids, *content_of(idx, donors))
        fresh = clb.Searcher(index=updated_index(idx, *args), encoder=enc, config=config)
        try:
            assert s.update_compressed(*args) == pids.size
            got = [ts(q) for q in queries]
            assert ts.generation == 1 and ts.graph is not None and ts.graph is not stale
            want_ts = fresh.text_search(5, graph=True)
            for q, g in zip(queries, got):
                w = want_ts(q)
                assert np.array_equal(g[0], w[0]), q
                assert_same_f32(g[1], w[1], q)
            ts.close(); want_ts.close()
        finally:
            fresh.close()
    finally:
        s.close(); enc.close()


def test_persisted_update_reopens_as_the_live_searcher(oracle, small, tmp_path):
    idx, Qs, _ = small
    path = str(tmp_path / "index")
    write_index(path, idx, 150)
    storage.append_chunk(path, *[np.asarray(a) for a in tail(idx, 150)])
    args = (np.array([150, 151, 9, 290]), *content_of(idx, [1, 2, 3, 4]))
    s = clb.Searcher(path)
    try:
        assert s.update_compressed(*args, persist=True) == 4
        again = clb.Searcher(path)
        try:
            assert (again.num_docs, again.num_embeddings) == (s.num_docs, s.num_embeddings)
            assert state(s, Qs) == state(again, Qs)
        finally:
            again.close()
        check_updated(oracle, s, updated_index(idx, *args), Qs, modes=(1,), singles=1)
    finally:
        s.close()
