"""Re-rank given passages on the GPU (`candidates=`).  The reference of a ranked result is the CPU oracle composed by
tests/util_filter.filtered_ranking(..., scope="all") on the list with its empty passages taken out; of the list scores,
the oracle's MaxSim of each listed pid (the scores of that same ranking, looked up by pid); of the compositions, the same
handle's make_filter(pids) + scope="all" call.  Bar: the project's own -- pids and counts exact, fp32 bits identical, pid 0 /
-Inf padding.  No tolerance is involved anywhere."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd.searcher import search_request
from tests import util_general as ug
from tests.test_gpu_filtered_search import assert_result, assert_same_f32, bits
from tests.test_gpu_grouped_search import modes_of
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index
from tests.util_filter import filtered_ranking
from tests.util_group import random_lens
from tests.util_prior import boost

pytestmark = pytest.mark.gpu


def messy_list(n_docs, length, seed):
    """`length` pids of 1..n_docs, unsorted, with duplicates (from 2 entries on: the first entry again at the end)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, n_docs + 1, size=length).astype(np.int64)
    if length >= 2:
        a[-1] = a[0]
    if length >= 30:
        a[length // 2:length // 2 + 5] = a[3:8]
    return a


def list_ranking(oracle, idx, Q, pids):
    """the full ranking of query Q over the listed passages (1-based local pids) that hold embeddings"""
    pids = np.asarray(pids, dtype=np.int64).reshape(-1)
    live = pids[idx["doclens"][pids - 1] > 0] if pids.size else pids
    return filtered_ranking(oracle, idx, Q, 2, live, "all")


def scores_at(ranking, pids, pid_offset=0):
    """the list scores a ranking implies: its score of every listed pid at the pid's position, -Inf for a pid it does not hold"""
    by_pid = dict(zip((ranking[0] + pid_offset).tolist(), ranking[1].tolist()))
    return np.array([by_pid.get(int(p), -np.inf) for p in np.asarray(pids).reshape(-1)], dtype=np.float32)


def as_block(lists, L=None):
    """ragged lists as the pair form (pids (L, B), lens [B]), the padding filled with a pid that must never be read as one"""
    lens = np.array([len(c) for c in lists], np.int64)
    L = max(1, int(lens.max())) if L is None else L
    block = np.full((L, len(lists)), 1, np.int64)
    for b, c in enumerate(lists):
        block[:len(c), b] = c
    return block, lens


# ---- 1. modes and batch sizes -------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 37, 1000, 5000)


@pytest.fixture(scope="module")
def medium(oracle):
    """20 000 passages, K = 2048 (the fixture of the filter tests); five (query, list) cases of the lengths above, their
    rankings computed once"""
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 3)
    lists = [messy_list(20_000, n, 700 + i) for i, n in enumerate(LENGTHS)]
    for c in lists[2:]:
        assert np.unique(c).size < c.size and np.any(np.diff(c) < 0)               # duplicates, unsorted
    rankings = [list_ranking(oracle, idx, Qs[:, :, i % 3], c) for i, c in enumerate(lists)]
    assert [r[0].size for r in rankings[:2]] == [0, 1] and rankings[4][0].size > 4000
    return idx, Qs, lists, rankings


@pytest.fixture(scope="module")
def medium_searcher(medium):
    s = clb.Searcher(index=medium[0])
    yield s
    s.close()


def case_batch(Qs, lists, rankings, B, first=0):
    """B queries cycling through the five cases from case `first` on (case i is query i % 3 with list i)"""
    cases = [(first + j) % len(lists) for j in range(B)]
    Qb = np.asfortranarray(np.stack([Qs[:, :, c % 3] for c in cases], axis=2))
    return Qb, [lists[c] for c in cases], [rankings[c] for c in cases]


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["exact", "two_pass", "other_gather", "rows8"])
def test_listed_search_modes_and_batch_sizes(medium, medium_searcher, mode):
    """Lists of 0, 1, 37, 1 000 and 5 000 pids; k = 10 and 1 000 (above the list length for some queries); B = 1, 9 and 18;
    ragged lists and the pair form."""
    idx, Qs, lists, rankings = medium
    s = medium_searcher
    auto_form = s.pass1_gather[0]
    try:
        s.set_mode(min(mode, 1))
        s.set_pass1_gather(1 - auto_form if mode == 2 else -1)
        s.set_score_rows(1 if mode == 3 else 0)
        for k in (10, 1000):
            for B in ((18,) if mode == 3 else (1, 9, 18)):        # (8-bit rows: batches of 16+)
                for first in (range(len(lists)) if B == 1 else (0,)):
                    Qb, lb, rb = case_batch(Qs, lists, rankings, B, first)
                    cands = lb if (B // 9 + k // 1000) % 2 else as_block(lb)
                    bp, bs, bn = s.search_batch(Qb, k, candidates=cands)
                    for j in range(B):
                        assert_result(bp[:, j], bs[:, j], bn[j], rb[j], k, f"mode={mode} k={k} B={B} first={first} q={j}")
        # one query at a time through the one-query calls
        p, sc = s.search_embeddings(Qs[:, :, 0], 10, candidates=lists[3])
        assert_result(p, sc, s.last_num_candidates, rankings[3], 10, f"search_embeddings mode={mode}")
        p, sc = clb.search(s, Qs[:, :, 0], 10, candidates=lists[3])
        assert_result(p, sc, s.last_num_candidates, rankings[3], 10, f"clb.search mode={mode}")
    finally:
        s.set_score_rows(0)
        s.set_pass1_gather(-1)
        s.set_mode(1)


# ---- 2. every passage, thrice -------------------------------------------------------------------------------------------------
def test_every_passage_thrice(oracle):
    idx = synthetic.make_index(seed=21, n_docs=300, K=16)
    Qs = synthetic.make_queries(idx, 22, 3)
    every = np.random.default_rng(5).permutation(np.tile(np.arange(1, 301, dtype=np.int64), 3))
    whole = [list_ranking(oracle, idx, Qs[:, :, j], np.arange(1, 301)) for j in range(3)]
    n_live = int(np.count_nonzero(idx["doclens"] > 0))
    assert all(r[0].size == n_live for r in whole)
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            for k in (7, 300, 400):
                bp, bs, bn = s.search_batch(Qs, k, candidates=[every] * 3)
                assert np.all(bn == n_live)
                for j in range(3):
                    assert_result(bp[:, j], bs[:, j], bn[j], whole[j], k, f"thrice mode={mode} k={k} q={j}")
    finally:
        s.close()


# ---- 3. list scores -----------------------------------------------------------------------------------------------------------
def test_list_scores(medium, medium_searcher):
    idx, Qs, lists, rankings = medium
    s = medium_searcher
    Qb, lb, rb = case_batch(Qs, lists, rankings, 9)
    want = [scores_at(rb[j], lb[j]) for j in range(9)]
    got = {}
    try:
        for mode in (0, 1):
            s.set_mode(mode)
            bp, bs, bn, ls = s.search_batch(Qb, 10, candidates=lb, return_candidate_scores=True)
            assert s.mode == mode                                  # the exact-pass route leaves the handle's mode alone
            assert isinstance(ls, list) and [a.size for a in ls] == [c.size for c in lb]
            for j in range(9):
                assert_result(bp[:, j], bs[:, j], bn[j], rb[j], 10, f"with list scores mode={mode} q={j}")
                assert_same_f32(ls[j], want[j], f"list scores mode={mode} q={j}")      # equal to the oracle per position ...
                assert ls[j].size < 2 or bits(ls[j][-1:]) == bits(ls[j][:1])           # ... and equal for duplicates
                top = {int(p): x for p, x in zip(bp[:, j], bs[:, j]) if p}
                for p, x in zip(lb[j], ls[j]):                                         # the bits the ranked output reports
                    assert int(p) not in top or bits([x]) == bits([top[int(p)]])
            got[mode] = ls
        for j in range(9):                                         # the same bits on a mode-0 and a mode-1 handle
            assert np.array_equal(bits(got[0][j]), bits(got[1][j])), j
        # the pair form with a stride above every length: -Inf at the positions past the length
        block, lens = as_block(lb, L=5003)
        bp, bs, bn, ls = s.search_batch(Qb, 10, candidates=(block, lens), return_candidate_scores=True)
        assert ls.shape == (5003, 9) and ls.dtype == np.float32
        for j in range(9):
            assert_same_f32(ls[:lens[j], j], want[j], f"pair form q={j}")
            assert np.all(np.isneginf(ls[lens[j]:, j])), j
        # a grouping or a cursor does not change them: they are passage scores
        with s.make_grouping(group_lens=random_lens(20_000, 1, 9, 77)) as g:
            for kw in (dict(grouping=g), dict(grouping=g, per_group=3),
                       dict(after=(np.array([r[1][min(5, r[1].size - 1)] if r[1].size else np.inf for r in rb], np.float32),
                                   np.zeros(9, np.int64)))):
                for mode in (0, 1):
                    s.set_mode(mode)
                    ls = s.search_batch(Qb, 10, candidates=lb, return_candidate_scores=True, **kw)[3]
                    for j in range(9):
                        assert_same_f32(ls[j], want[j], f"list scores with {sorted(kw)} mode={mode} q={j}")
        # with a prior the score is E
        values = np.random.default_rng(9).normal(0, 2, 20_000).astype(np.float32)
        with s.make_prior(values) as pr:
            for mode in (0, 1):
                s.set_mode(mode)
                bp, bs, bn, ls = s.search_batch(Qb, 10, candidates=lb, return_candidate_scores=True, prior=pr, prior_weight=0.75)
                for j in range(9):
                    E = boost(want[j], values[lb[j] - 1], 0.75) if lb[j].size else want[j]
                    assert_same_f32(ls[j], E, f"list scores with a prior mode={mode} q={j}")
        # one query: the third result of the one-query calls
        p, sc, one = s.search_embeddings(Qs[:, :, 0], 10, candidates=lists[3], return_candidate_scores=True)
        assert_same_f32(one, scores_at(rankings[3], lists[3]), "search_embeddings")
    finally:
        s.set_mode(1)


# ---- 4. index changes ---------------------------------------------------------------------------------------------------------
def test_lists_after_remove_and_update(oracle):
    """Listed removed pids are no candidates (their list score is -Inf), an updated passage scores by its new content, and
    lists made of old pids still work: the pids never move."""
    idx = synthetic.make_index(0, 300, K=64)
    Qs = synthetic.make_queries(idx, 1000, 9)
    lists = [messy_list(300, n, 40 + j) for j, n in enumerate((0, 3, 50, 120, 299, 300, 300, 20, 77))]
    removed = np.unique(np.concatenate([lists[2][:10], lists[4][5:40], [300, 1]]))
    keep = np.setdiff1d(np.arange(1, 301), removed)
    upd = (keep[[3, 100]], *content_of(idx, keep[[50, 7]]))
    want, _ = reduced_index(idx, removed)
    want = updated_index(want, *upd)
    lists[3][:2] = upd[0]
    lists[7] = np.concatenate([removed[:6], removed[:6]])                    # nothing but removed passages, twice
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages(removed) == removed.size
        assert s.update_compressed(*upd) == 2
        rankings = [list_ranking(oracle, want, Qs[:, :, j], lists[j]) for j in range(9)]
        assert rankings[7][0].size == 0 and not np.isin(removed, np.concatenate([r[0] for r in rankings])).any()
        for mode in modes_of(s):
            for k in (5, 300):
                bp, bs, bn, ls = s.search_batch(Qs, k, candidates=lists, return_candidate_scores=True)
                bp2, bs2, bn2 = s.search_batch(Qs, k, candidates=lists)
                assert np.array_equal(bp, bp2) and np.array_equal(bits(bs), bits(bs2)) and np.array_equal(bn, bn2)
                for j in range(9):
                    assert_result(bp[:, j], bs[:, j], bn[j], rankings[j], k, f"changed index mode={mode} k={k} q={j}")
                    assert_same_f32(ls[j], scores_at(rankings[j], lists[j]), f"changed index list scores mode={mode} q={j}")
                    assert np.all(np.isneginf(ls[j][np.isin(lists[j], removed)])), j
    finally:
        s.close()


# ---- 5. a shard handle ----------------------------------------------------------------------------------------------------------
def test_a_shard_handle_with_a_pid_offset(oracle):
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=1, n_docs=300, K=64)
    B, k, off = 4, 30, 1000
    Qs = synthetic.make_queries(idx, 2, B)
    local = [messy_list(300, n, 60 + j) for j, n in enumerate((40, 0, 300, 7))]
    rankings = [list_ranking(oracle, idx, Qs[:, :, j], local[j]) for j in range(B)]
    s = clb.Searcher(index=idx, pid_offset=off)
    try:
        for mode in modes_of(s):
            bp, bs, bn, ls = s.search_batch(Qs, k, candidates=[c + off for c in local], return_candidate_scores=True)
            for j in range(B):
                assert_result(bp[:, j], bs[:, j], bn[j], rankings[j], k, f"global pids mode={mode} q={j}", pid_offset=off)
                assert_same_f32(ls[j], scores_at(rankings[j], local[j]), f"global pids, list scores q={j}")
        # another shard's pids (and what is no pid at all): BoundsError on the host route, skipped on the device route
        foreign = np.array([5, off, off + 301, 0, -3, 2 ** 62, -2 ** 63], np.int64)
        mixed = [np.concatenate([c[:len(c) // 2] + off, foreign, c[len(c) // 2:] + off]) for c in local]
        with pytest.raises(clb.BoundsError, match=r"candidate list of query 0, position 20: pid 5 outside 1001\.\.1300"):
            s.search_batch(Qs, k, candidates=mixed)
        block, lens = as_block(mixed)
        d_p, d_n = torch.from_numpy(np.ascontiguousarray(block.T)).cuda(), torch.from_numpy(lens).cuda()
        d_sc = torch.zeros(block.T.shape, dtype=torch.float32, device="cuda")
        Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
        for mode in modes_of(s):
            run = DeviceSearch(s, 32, B, k, 2)
            for scores in (None, d_sc):
                run(Qdev, candidates=(d_p, d_n), candidate_scores=scores)
                torch.cuda.synchronize()
                gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
                for j in range(B):
                    assert_result(gp[j], gs[j], gn[j], rankings[j], k, f"device route mode={mode} q={j}", pid_offset=off)
            ls = d_sc.cpu().numpy()
            for j in range(B):
                assert_same_f32(ls[j, :lens[j]], scores_at(rankings[j], mixed[j], off), f"device list scores mode={mode} q={j}")
                assert np.all(np.isneginf(ls[j, lens[j]:]))
    finally:
        s.close()


# ---- 6. compositions ----------------------------------------------------------------------------------------------------------
def test_compositions_equal_the_scope_all_filter_call(medium, medium_searcher):
    """grouping, per_group = 3, a prior, and paging with after=next_cursor(...): each bit-identical to the same handle's
    make_filter(pids) + scope="all" call, which the filter, grouping, prior and cursor tests hold against the oracle."""
    idx, Qs, lists, rankings = medium
    s = medium_searcher
    Qb, lb, rb = case_batch(Qs, lists, rankings, 9)
    filters = [s.make_filter(pids=c) for c in lb]
    values = np.random.default_rng(10).normal(0, 3, 20_000).astype(np.float32)

    def same(a, b, what):
        assert np.array_equal(a[0], b[0]), what
        assert np.array_equal(bits(a[1]), bits(b[1])), what
        assert np.array_equal(a[2], b[2]), what
    try:
        with s.make_grouping(group_lens=random_lens(20_000, 1, 9, 78)) as g, s.make_prior(values) as pr:
            for mode in (0, 1):
                s.set_mode(mode)
                for k in (10, 1000):
                    for name, kw in (("plain", {}), ("grouping", dict(grouping=g)), ("per_group", dict(grouping=g, per_group=3)),
                                     ("prior", dict(prior=pr, prior_weight=-0.5)),
                                     ("prior and grouping", dict(prior=pr, prior_weight=2.0, grouping=g))):
                        same(s.search_batch(Qb, k, candidates=lb, **kw), s.search_batch(Qb, k, filters=filters, scope="all", **kw),
                             f"{name} mode={mode} k={k}")
                # paging through the 1 000-pid list (and its neighbours) in pages of 64
                cursor, seen, pages = None, [[] for _ in range(9)], 0
                while True:
                    kw = {} if cursor is None else dict(after=cursor)
                    page = s.search_batch(Qb, 64, candidates=lb, **kw)
                    same(page, s.search_batch(Qb, 64, filters=filters, scope="all", **(kw or dict(after=(np.full(9, np.inf, np.float32),
                                                                                                           np.zeros(9, np.int64))))),
                         f"page {pages} mode={mode}")
                    pages += 1
                    for j in range(9):
                        seen[j] += page[0][page[0][:, j] != 0, j].tolist()
                    if not page[0].any():
                        break
                    cursor = clb.next_cursor(page[0], page[1])
                assert pages == -(-rb[4][0].size // 64) + 1
                for j in range(9):                                  # the concatenated pages are the full ranking
                    assert seen[j] == rb[j][0].tolist(), (mode, j)
    finally:
        for f in filters:
            f.close()
        s.set_mode(1)


# ---- 7. other shapes ----------------------------------------------------------------------------------------------------------
def check_shape(oracle, idx, Qs, nprobe, what):
    n_docs = idx["doclens"].size
    lists = [messy_list(n_docs, n, 90 + j) for j, n in enumerate((n_docs // 2, 0, 45))]
    rankings = [list_ranking(oracle, idx, Qs[:, :, j], lists[j]) for j in range(3)]
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            for k in (11, n_docs):
                bp, bs, bn = s.search_batch(Qs, k, nprobe=nprobe, candidates=lists)
                for j in range(3):
                    assert_result(bp[:, j], bs[:, j], bn[j], rankings[j], k, f"{what} mode={mode} k={k} q={j}")
            ls = s.search_batch(Qs, 11, nprobe=nprobe, candidates=lists, return_candidate_scores=True)[3]
            for j in range(3):
                assert_same_f32(ls[j], scores_at(rankings[j], lists[j]), f"{what} list scores mode={mode} q={j}")
    finally:
        s.close()


def test_lists_on_other_shapes(oracle):
    idx = synthetic.make_index(seed=41, n_docs=2000, K=256, nbits=4)              # nbits = 4 on the tuned exact path
    check_shape(oracle, idx, synthetic.make_queries(idx, 42, 3), 2, "nbits 4")
    idx = synthetic.make_index(seed=23, n_docs=3000, K=256)                       # T = 40: no two-pass, whatever the mode
    check_shape(oracle, idx, synthetic.make_queries(idx, 24, 3, T=40), 2, "T=40")


@pytest.mark.parametrize("case,route", [(9, "loop_mfma"), (8, "batched32")])
def test_lists_on_the_general_path(oracle, case, route):
    assert ug.CASES[case][4] == route
    idx, Qs, nprobe = ug.case_inputs(case)
    check_shape(oracle, idx, np.asfortranarray(Qs), nprobe, route)


# ---- 8. across the sub-batch boundary -----------------------------------------------------------------------------------------
def test_seventy_queries_on_the_host_route(oracle):
    idx = synthetic.make_index(seed=23, n_docs=6000, K=256)
    B = 70
    Qs = synthetic.make_queries(idx, 31, B)
    rng = np.random.default_rng(8)
    lists = [messy_list(6000, int(n), 200 + j) for j, n in enumerate(rng.integers(0, 200, B))]
    lists[63], lists[64] = messy_list(6000, 199, 1), messy_list(6000, 0, 2)
    rankings = [list_ranking(oracle, idx, Qs[:, :, j], lists[j]) for j in range(B)]
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            bp, bs, bn, ls = s.search_batch(Qs, 20, candidates=lists, return_candidate_scores=True)
            bp2, bs2, bn2 = s.search_batch(Qs, 20, candidates=as_block(lists))
            assert np.array_equal(bp, bp2) and np.array_equal(bits(bs), bits(bs2)) and np.array_equal(bn, bn2)
            for j in range(B):
                assert_result(bp[:, j], bs[:, j], bn[j], rankings[j], 20, f"B=70 mode={mode} q={j}")
                assert_same_f32(ls[j], scores_at(rankings[j], lists[j]), f"B=70 list scores mode={mode} q={j}")
    finally:
        s.close()


# ---- 9. device route and graph ------------------------------------------------------------------------------------------------
def test_device_route_and_replays_with_the_lists_overwritten(oracle):
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=256)
    k, B, L = 10, 4, 600
    Qs = synthetic.make_queries(idx, 31, B)
    Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
    rounds = [[messy_list(6000, n, 300 + 10 * r + j) for j, n in enumerate(ns)]
              for r, ns in enumerate(((600, 5, 130, 64), (1, 600, 0, 77), (300, 300, 300, 300), (0, 2, 599, 40)))]
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            for with_scores in (False, True):
                run = DeviceSearch(s, 32, B, k, 2)
                block, lens = as_block(rounds[0], L=L)
                d_p, d_n = torch.from_numpy(np.ascontiguousarray(block.T)).cuda(), torch.from_numpy(lens).cuda()
                d_sc = torch.zeros((B, L), dtype=torch.float32, device="cuda") if with_scores else None

                def check(lists, what):
                    torch.cuda.synchronize()
                    gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
                    host = s.search_batch(Qs, k, candidates=lists, return_candidate_scores=True)     # the host route
                    assert np.array_equal(gp.T, host[0]) and np.array_equal(bits(gs.T), bits(host[1])), what
                    assert np.array_equal(gn, host[2]), what
                    for j in range(B):
                        assert_result(gp[j], gs[j], gn[j], list_ranking(oracle, idx, Qs[:, :, j], lists[j]), k, f"{what} q={j}")
                    if with_scores:
                        ls = d_sc.cpu().numpy()
                        for j in range(B):
                            assert np.array_equal(bits(ls[j, :len(lists[j])]), bits(host[3][j])), (what, j)
                            assert np.all(np.isneginf(ls[j, len(lists[j]):])), (what, j)

                run(Qdev, candidates=(d_p, d_n), candidate_scores=d_sc)                   # eager
                check(rounds[0], f"eager mode={mode} scores={with_scores}")
                graph = run.capture(Qdev, candidates=(d_p, d_n), candidate_scores=d_sc)   # captured once
                nbytes = s.device_bytes
                for r in (1, 2, 3):                                # the list tensors overwritten in place, lengths included
                    block, lens = as_block(rounds[r], L=L)
                    d_p.copy_(torch.from_numpy(np.ascontiguousarray(block.T)))
                    d_n.copy_(torch.from_numpy(lens))
                    graph = run.replay(graph, Qdev, candidates=(d_p, d_n), candidate_scores=d_sc)
                    check(rounds[r], f"replay {r} mode={mode} scores={with_scores}")
                    assert s.device_bytes == nbytes
                # lengths the host would refuse: clamped to 0..L on the device
                d_n.copy_(torch.tensor([-5, L + 100, 3, 0]))
                graph.replay()
                clamped = [rounds[3][0][:0], as_block(rounds[3], L=L)[0][:, 1], rounds[3][2][:3], rounds[3][3][:0]]
                check(clamped, f"clamped lengths mode={mode} scores={with_scores}")
        # the tensors are checked like the cursor tensors: dtype, device, contiguity, shape
        run = DeviceSearch(s, 32, B, k, 2)
        good_p, good_n = torch.zeros((B, L), dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
        for bad in ((good_p.int(), good_n), (good_p, good_n.int()), (good_p.cpu(), good_n), (good_p.t(), good_n),
                    (good_p[:, ::2], good_n), (good_p[:3], good_n), (good_p, good_n[:3]), (good_p.view(-1), good_n), (good_p,)):
            with pytest.raises(clb.ArgumentError, match="candidates must be a pair of contiguous tensors"):
                run(Qdev, candidates=bad)
        for bad in (torch.zeros((B, L), dtype=torch.float64, device="cuda"), torch.zeros((B, L + 1), device="cuda"),
                    torch.zeros((B, L)), np.zeros((B, L), np.float32)):
            with pytest.raises(clb.ArgumentError, match="candidate_scores must be a contiguous float32"):
                run(Qdev, candidates=(good_p, good_n), candidate_scores=bad)
    finally:
        s.close()


# ---- 10. refusals on a live handle --------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(medium, medium_searcher):
    idx, Qs, lists, _ = medium
    s = medium_searcher
    three = [lists[2], lists[3], lists[1]]
    with s.make_filter(pids=[1, 2, 3]) as f:
        with pytest.raises(clb.Unsupported, match=r"candidates= together with filter\(s\)="):
            s.search_batch(Qs, 10, candidates=three, filters=[None, f, None])
        # ... and the library's own refusal, past the Python builder
        req = search_request(s, 3, candidates=three)
        req.filters = (C.c_void_p * 3)(None, f._h, None)
        out_p, out_s, n = np.zeros((10, 3), np.int64, order="F"), np.zeros((10, 3), np.float32, order="F"), np.zeros(3, np.int64)
        q = np.asfortranarray(Qs)
        rc = clb.lib().clb_search_batch_request(s._h, q.ctypes.data, 32, 3, 2, 10, req, out_p.ctypes.data, out_s.ctypes.data,
                                                n.ctypes.data)
        assert rc == clb.Unsupported.code and b"candidate lists together with filters" in clb.lib().clb_last_error()
    bad = [c.copy() for c in three]
    bad[1][2] = 20_001
    with pytest.raises(clb.BoundsError, match=r"candidate list of query 1, position 2: pid 20001 outside 1\.\.20000"):
        s.search_batch(Qs, 10, candidates=bad)
    bad[1][2] = 0
    with pytest.raises(clb.BoundsError, match=r"candidate list of query 1, position 2: pid 0 outside"):
        s.search_batch(Qs, 10, candidates=bad)
    # past the length nothing is looked at
    block, lens = as_block(three)
    block[lens[0]:, 0] = -7
    p1 = s.search_batch(Qs, 10, candidates=(block, lens))
    p2 = s.search_batch(Qs, 10, candidates=three)
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(bits(p1[1]), bits(p2[1]))
    with pytest.raises(clb.BoundsError, match="nprobe"):               # nprobe is validated, though otherwise unused
        s.search_batch(Qs, 10, nprobe=2049, candidates=three)
