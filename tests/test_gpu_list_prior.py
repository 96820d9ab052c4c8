"""Re-rank with first-stage scores on the GPU (`candidate_priors=`).  The reference of a ranked result is
tests/util_prior.boosted_ranking over tests/test_gpu_rerank.list_ranking (the CPU oracle's MaxSim of the listed passages that
hold embeddings) with the dense vector that holds, for every listed passage, the value at its FIRST occurrence in the list
and 0 elsewhere; the second reference is the same handle's one-query call with make_prior(dense) + candidates=[list].
Bar: pids and counts exact, fp32 bits identical, pid 0 / -Inf padding.  No tolerance is involved anywhere."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import util_general as ug
from tests.test_gpu_filtered_search import assert_result, assert_same_f32, bits
from tests.test_gpu_grouped_search import modes_of
from tests.test_gpu_rerank import LENGTHS, as_block, case_batch, list_ranking, messy_list, scores_at
from tests.util_group import collapse, ids_from_lens, random_lens
from tests.util_prior import boosted_ranking

pytestmark = pytest.mark.gpu


def dense_of(n_docs, pids, values, last=False):
    """the dense prior a list and its values stand for: values at the FIRST occurrence of every listed local pid (`last`: at
    the last, the mapping the feature must NOT implement), 0 elsewhere"""
    pids, values = np.asarray(pids, np.int64).reshape(-1), np.asarray(values, np.float32).reshape(-1)
    assert pids.size == values.size
    if last:
        pids, values = pids[::-1], values[::-1]
    u, first = np.unique(pids, return_index=True)
    dense = np.zeros(n_docs, np.float32)
    dense[u - 1] = values[first]
    return dense


def boosted(ranking, n_docs, pids, values, weight, group_ids=None):
    """the reference ranking of a list with list priors (with `group_ids`: its collapse)"""
    if ranking[0].size == 0:
        return ranking
    r = boosted_ranking(ranking, dense_of(n_docs, pids, values), weight)
    return r if group_ids is None else collapse(r, group_ids)


def value_block(values, L=None):
    """ragged values as the (L, B) block of the pair form, the padding filled with NaN: it must never be read as a value"""
    L = max(1, max(len(v) for v in values)) if L is None else L
    block = np.full((L, len(values)), np.nan, np.float32)
    for b, v in enumerate(values):
        block[:len(v), b] = v
    return block


# the value regimes: name -> (values of a list of n entries, weight)
REGIMES = {
    "tiny": (lambda rng, n: rng.normal(0, 1e-3, n), 1.0),
    "comparable": (lambda rng, n: rng.normal(0, 0.5, n), 1.0),
    "dominating": (lambda rng, n: rng.uniform(0, 1e3, n), 1.0),
    # the levels swallow every MaxSim score (ulp(2^30) = 128): the candidates of a level tie exactly and rank by pid
    "levels": (lambda rng, n: rng.integers(0, 4, n), float(2 ** 30)),
    "negative weight": (lambda rng, n: rng.normal(0, 0.5, n), -1.5),
    "all-zero": (lambda rng, n: np.zeros(n), 1.0),
    "weight 0": (lambda rng, n: rng.normal(0, 0.5, n), 0.0),
}


@pytest.fixture(scope="module")
def medium(oracle):
    """the 20 000-passage, K = 2048 fixture of tests/test_gpu_rerank.py with its five (query, list) cases, their rankings
    computed once; per regime the values of every list and the boosted rankings"""
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 3)
    lists = [messy_list(20_000, n, 700 + i) for i, n in enumerate(LENGTHS)]
    rankings = [list_ranking(oracle, idx, Qs[:, :, i % 3], c) for i, c in enumerate(lists)]
    values, refs = {}, {}
    for r, (name, (draw, w)) in enumerate(REGIMES.items()):
        rng = np.random.default_rng(900 + r)
        values[name] = [np.asarray(draw(rng, c.size), np.float32) for c in lists]
        refs[name] = [boosted(rankings[i], 20_000, lists[i], values[name][i], w) for i in range(len(lists))]
    # every regime does on the reference what it is for
    e10, top = rankings[3][0][:10], lambda name, i, n=10: refs[name][i][0][:n]
    assert not np.array_equal(top("comparable", 3), e10) and not np.array_equal(top("comparable", 4), rankings[4][0][:10])
    for i in (3, 4):                # dominating: the order follows the values -- the top 10 by E lie in the top tenth by value
        d = dense_of(20_000, lists[i], values["dominating"][i])
        cand = rankings[i][0]
        best = cand[np.argsort(-d[cand - 1], kind="stable")][:cand.size // 10]
        assert np.isin(top("dominating", i), best).all() and not np.array_equal(top("dominating", i), rankings[i][0][:10])
    lv = refs["levels"]             # levels: runs of exactly tied E across rank k = 10 and k = 1 000, in pid order
    assert lv[3][1][9] == lv[3][1][10] and lv[3][0][9] < lv[3][0][10]
    assert lv[4][1][999] == lv[4][1][1000] and lv[4][0][999] < lv[4][0][1000]
    for name in ("all-zero", "weight 0"):                      # the bits of the ranking without list priors
        for i in range(len(lists)):
            assert np.array_equal(refs[name][i][0], rankings[i][0]) and np.array_equal(bits(refs[name][i][1]), bits(rankings[i][1]))
    assert not np.array_equal(refs["negative weight"][3][0][:10], e10)
    return idx, Qs, lists, rankings, values, refs


@pytest.fixture(scope="module")
def medium_searcher(medium):
    s = clb.Searcher(index=medium[0])
    yield s
    s.close()


def batch_of(medium, regime, B, first=0):
    idx, Qs, lists, rankings, values, refs = medium
    Qb, lb, rb = case_batch(Qs, lists, refs[regime], B, first)
    _, vb, plain = case_batch(Qs, values[regime], rankings, B, first)
    return Qb, lb, vb, rb, plain, REGIMES[regime][1]


# ---- 1. modes and sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["exact", "two_pass", "other_gather", "rows8"])
def test_list_priors_modes_sizes_and_value_regimes(medium, medium_searcher, mode):
    """Lists of 0, 1, 37, 1 000 and 5 000 messy pids; k = 10 and 1 000; B = 1, 9 and 18; ragged values and the pair form;
    every value regime.  All-zero values and weight 0 also equal the call without list priors, bit for bit."""
    s = medium_searcher
    auto_form = s.pass1_gather[0]
    try:
        s.set_mode(min(mode, 1))
        s.set_pass1_gather(1 - auto_form if mode == 2 else -1)
        s.set_score_rows(1 if mode == 3 else 0)
        for regime in REGIMES:
            for k in (10, 1000):
                for B in ((18,) if mode == 3 else (1, 9, 18)):        # (8-bit rows: batches of 16+)
                    for first in (range(len(LENGTHS)) if B == 1 else (0,)):
                        Qb, lb, vb, rb, plain, w = batch_of(medium, regime, B, first)
                        ragged = (B // 9 + k // 1000) % 2
                        kw = dict(candidates=lb, candidate_priors=vb) if ragged else \
                            dict(candidates=as_block(lb), candidate_priors=value_block(vb))
                        bp, bs, bn = s.search_batch(Qb, k, prior_weight=w, **kw)
                        for j in range(B):
                            assert_result(bp[:, j], bs[:, j], bn[j], rb[j], k, f"{regime} mode={mode} k={k} B={B} first={first} q={j}")
                        if regime in ("all-zero", "weight 0"):
                            pp, ps, pn = s.search_batch(Qb, k, candidates=lb)
                            assert np.array_equal(bp, pp) and np.array_equal(bits(bs), bits(ps)) and np.array_equal(bn, pn), (regime, k, B)
        # one query at a time through the one-query calls
        idx, Qs, lists, rankings, values, refs = medium
        for call in (s.search_embeddings, lambda *a, **kw: clb.search(s, *a, **kw)):
            p, sc = call(Qs[:, :, 0], 10, candidates=lists[3], candidate_priors=values["negative weight"][3], prior_weight=-1.5)
            assert_result(p, sc, s.last_num_candidates, refs["negative weight"][3], 10, f"one query mode={mode}")
    finally:
        s.set_score_rows(0)
        s.set_pass1_gather(-1)
        s.set_mode(1)


# ---- 2. first occurrence wins -----------------------------------------------------------------------------------------------
def test_the_first_occurrence_of_a_duplicate_wins(oracle, medium, medium_searcher):
    """Duplicates with different values, inside one 256-position block of the slot-map kernel and across blocks -- with the
    lower position in the EARLIER block and the other occurrences up to ten blocks later, and the other way round in list
    order of the pid's neighbours, so no launch order of the blocks can give the right answer by accident."""
    idx, Qs = medium[0], medium[1]
    s = medium_searcher
    rng = np.random.default_rng(77)
    base = rng.choice(np.arange(1, 20_001), size=1200, replace=False).astype(np.int64)
    c = np.concatenate([base, base[:600][::-1], base[100:300], base[1100:1200]])      # 2 100 positions, 9 blocks
    c[5], c[7] = c[6], c[6]                                                           # ... and three in a row
    v = rng.normal(0, 2.0, c.size).astype(np.float32)
    pos = {}
    for i, p in enumerate(c.tolist()):
        pos.setdefault(p, []).append(i)
    assert any(len(x) >= 2 and x[0] // 256 == x[1] // 256 for x in pos.values())           # within one block
    assert sum(len(x) >= 2 and x[0] // 256 < x[-1] // 256 for x in pos.values()) > 500       # across blocks
    assert all(v[x[0]] != v[x[-1]] for x in pos.values() if len(x) >= 2)                   # different values
    base_rank = list_ranking(oracle, idx, Qs[:, :, 1], c)
    want = boosted_ranking(base_rank, dense_of(20_000, c, v), 1.0)
    wrong = boosted_ranking(base_rank, dense_of(20_000, c, v, last=True), 1.0)
    assert not np.array_equal(want[0][:50], wrong[0][:50])         # "last wins" is another ranking: no passing by accident
    Q1 = np.asfortranarray(Qs[:, :, 1:2])
    try:
        for mode in (0, 1):
            s.set_mode(mode)
            for k in (50, 1000):
                bp, bs, bn, ls = s.search_batch(Q1, k, candidates=[c], candidate_priors=[v], return_candidate_scores=True)
                assert_result(bp[:, 0], bs[:, 0], bn[0], want, k, f"first wins mode={mode} k={k}")
                assert_same_f32(ls[0], scores_at(want, c), f"first wins, candidate scores mode={mode}")
                bp, bs, bn = s.search_batch(Q1, k, candidates=[c], candidate_priors=[v])
                assert_result(bp[:, 0], bs[:, 0], bn[0], want, k, f"first wins, ranked only, mode={mode} k={k}")
    finally:
        s.set_mode(1)


# ---- 3. equivalence with a resident prior -----------------------------------------------------------------------------------
def test_a_row_equals_the_one_query_call_with_a_resident_prior(medium, medium_searcher):
    s = medium_searcher
    Qb, lb, vb, rb, plain, w = batch_of(medium, "negative weight", 9)
    try:
        for mode in (0, 1):
            s.set_mode(mode)
            for k in (10, 1000):
                bp, bs, bn = s.search_batch(Qb, k, candidates=lb, candidate_priors=vb, prior_weight=w)
                for j in range(9):
                    with s.make_prior(dense_of(20_000, lb[j], vb[j])) as pr:
                        op, os_, on = s.search_batch(np.asfortranarray(Qb[:, :, j:j + 1]), k, candidates=[lb[j]], prior=pr, prior_weight=w)
                    assert np.array_equal(bp[:, j], op[:, 0]) and np.array_equal(bits(bs[:, j]), bits(os_[:, 0])) and bn[j] == on[0], (mode, k, j)
    finally:
        s.set_mode(1)


# ---- 4. candidate scores ----------------------------------------------------------------------------------------------------
def test_candidate_scores_are_E_at_every_input_position(medium, medium_searcher):
    s = medium_searcher
    got = {}
    try:
        for regime in ("comparable", "levels"):
            Qb, lb, vb, rb, plain, w = batch_of(medium, regime, 9)
            want = [scores_at(rb[j], lb[j]) for j in range(9)]
            for mode in (0, 1):
                s.set_mode(mode)
                bp, bs, bn, ls = s.search_batch(Qb, 10, candidates=lb, candidate_priors=vb, prior_weight=w, return_candidate_scores=True)
                assert s.mode == mode
                for j in range(9):
                    assert_result(bp[:, j], bs[:, j], bn[j], rb[j], 10, f"{regime} with candidate scores mode={mode} q={j}")
                    assert_same_f32(ls[j], want[j], f"{regime} candidate scores mode={mode} q={j}")
                    assert ls[j].size < 2 or bits(ls[j][-1:]) == bits(ls[j][:1])            # every occurrence of a duplicate
                got[regime, mode] = ls
            for j in range(9):                                                          # unchanged by mode
                assert np.array_equal(bits(got[regime, 0][j]), bits(got[regime, 1][j])), (regime, j)
        # the pair form with a stride above every length: -Inf past the length, the NaN padding of the values never read
        Qb, lb, vb, rb, plain, w = batch_of(medium, "comparable", 9)
        block, lens = as_block(lb, L=5003)
        bp, bs, bn, ls = s.search_batch(Qb, 10, candidates=(block, lens), candidate_priors=value_block(vb, L=5003),
                                        return_candidate_scores=True)
        for j in range(9):
            assert_same_f32(ls[:lens[j], j], scores_at(rb[j], lb[j]), f"pair form q={j}")
            assert np.all(np.isneginf(ls[lens[j]:, j])), j
    finally:
        s.set_mode(1)


# ---- 5. with a grouping -----------------------------------------------------------------------------------------------------
def test_list_priors_with_a_grouping(medium, medium_searcher):
    """documents of 1 to 6 passages: the result is the collapse of the boosted ranking -- a document is represented by its
    candidate with the largest E"""
    idx, Qs, lists, rankings, values, refs = medium
    s = medium_searcher
    gids = ids_from_lens(random_lens(20_000, 1, 6, 79))
    try:
        with s.make_grouping(group_ids=gids) as g:
            for regime in ("comparable", "dominating", "levels"):
                Qb, lb, vb, rb, plain, w = batch_of(medium, regime, 9)
                want = [collapse(r, gids) for r in rb]
                assert any(a[0].size < b[0].size for a, b in zip(want, rb))                   # the collapse removed something
                for mode in (0, 1):
                    s.set_mode(mode)
                    for k in (10, 1000):
                        for kw in (dict(grouping=g), dict(grouping=g, per_group=1)):
                            bp, bs, bn = s.search_batch(Qb, k, candidates=lb, candidate_priors=vb, prior_weight=w, **kw)
                            bp, bs = bp.reshape(k, 9), bs.reshape(k, 9)
                            for j in range(9):
                                assert_result(bp[:, j], bs[:, j], bn[j], want[j], k, f"grouped {regime} mode={mode} k={k} q={j}")
    finally:
        s.set_mode(1)


# ---- 6. the general-shape path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["dim64-batched", "dim768-per-query"])
def test_list_priors_on_the_general_path(oracle, shape):
    """300 passages, every passage listed thrice with three distinct values: topk_of's boost, batched and one query at a time"""
    if shape == "dim64-batched":
        idx = synthetic.make_index(seed=531, n_docs=300, K=32, dim=64, nbits=4, doclen_mean=20, doclen_std=12)
        Qs, nprobe = synthetic.make_queries(idx, 631, 3, T=24), 2
        assert ug.expected_route(64, 4, 24) == "batched32"
    else:
        assert ug.CASES[10][4] == "loop_mfma" and ug.CASES[10][5] == 300
        idx, Qs, nprobe = ug.case_inputs(10)
    Qs = np.asfortranarray(Qs)
    rng = np.random.default_rng(6)
    every = rng.permutation(np.tile(np.arange(1, 301, dtype=np.int64), 3))
    vals = [rng.normal(0, 1.0, 900).astype(np.float32) for _ in range(3)]
    base = [list_ranking(oracle, idx, Qs[:, :, j], every) for j in range(3)]
    want = [boosted(base[j], 300, every, vals[j], 0.75) for j in range(3)]
    assert all(not np.array_equal(want[j][0], base[j][0]) for j in range(3))
    s = clb.Searcher(index=idx)
    try:
        for k in (7, 300):
            bp, bs, bn, ls = s.search_batch(Qs, k, nprobe=nprobe, candidates=[every] * 3, candidate_priors=vals, prior_weight=0.75,
                                            return_candidate_scores=True)
            for j in range(3):
                assert_result(bp[:, j], bs[:, j], bn[j], want[j], k, f"{shape} k={k} q={j}")
                assert_same_f32(ls[j], scores_at(want[j], every), f"{shape} candidate scores q={j}")
    finally:
        s.close()


# ---- 7. a shard handle ------------------------------------------------------------------------------------------------------
def test_a_shard_handle_with_a_pid_offset_and_removed_passages(oracle):
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    from tests.test_remove_cpu import reduced_index
    idx = synthetic.make_index(seed=1, n_docs=300, K=64)
    B, k, off = 4, 30, 1000
    Qs = synthetic.make_queries(idx, 2, B)
    rng = np.random.default_rng(12)
    local = [messy_list(300, n, 60 + j) for j, n in enumerate((40, 0, 300, 7))]
    vals = [rng.normal(0, 1.0, c.size).astype(np.float32) for c in local]
    base = [list_ranking(oracle, idx, Qs[:, :, j], local[j]) for j in range(B)]
    want = [boosted(base[j], 300, local[j], vals[j], 2.0) for j in range(B)]
    s = clb.Searcher(index=idx, pid_offset=off)
    try:
        for mode in modes_of(s):
            bp, bs, bn = s.search_batch(Qs, k, candidates=[c + off for c in local], candidate_priors=vals, prior_weight=2.0)
            for j in range(B):
                assert_result(bp[:, j], bs[:, j], bn[j], want[j], k, f"global pids mode={mode} q={j}", pid_offset=off)
        # another shard's pids with large values beside them: BoundsError on the host route, skipped with their values on the device
        foreign, fv = np.array([5, off, off + 301, 0, -3, 2 ** 62, -2 ** 63], np.int64), np.full(7, 1e6, np.float32)
        mixed = [np.concatenate([c[:len(c) // 2] + off, foreign, c[len(c) // 2:] + off]) for c in local]
        mixed_v = [np.concatenate([v[:len(v) // 2], fv, v[len(v) // 2:]]) for v in vals]
        with pytest.raises(clb.BoundsError, match=r"candidate list of query 0, position 20: pid 5 outside 1001\.\.1300"):
            s.search_batch(Qs, k, candidates=mixed, candidate_priors=mixed_v, prior_weight=2.0)
        block, lens = as_block(mixed)
        d_p, d_n = torch.from_numpy(np.ascontiguousarray(block.T)).cuda(), torch.from_numpy(lens).cuda()
        d_v = torch.from_numpy(np.ascontiguousarray(value_block(mixed_v).T)).cuda()
        d_sc = torch.zeros(block.T.shape, dtype=torch.float32, device="cuda")
        Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
        for mode in modes_of(s):
            run = DeviceSearch(s, 32, B, k, 2)
            for scores in (None, d_sc):
                run(Qdev, candidates=(d_p, d_n), candidate_scores=scores, candidate_priors=d_v, prior_weight=2.0)
                torch.cuda.synchronize()
                gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
                for j in range(B):
                    assert_result(gp[j], gs[j], gn[j], want[j], k, f"device route mode={mode} q={j}", pid_offset=off)
            ls = d_sc.cpu().numpy()
            for j in range(B):
                assert_same_f32(ls[j, :lens[j]], scores_at(want[j], mixed[j], off), f"device candidate scores mode={mode} q={j}")
        # an emptied listed passage with a large value is no candidate
        removed = np.unique(np.concatenate([local[0][:6], local[2][10:40]]))
        assert s.remove_passages(removed + off) == removed.size
        left, _ = reduced_index(idx, removed)
        big = [np.where(np.isin(c, removed), np.float32(1e6), v).astype(np.float32) for c, v in zip(local, vals)]
        want = [boosted(list_ranking(oracle, left, Qs[:, :, j], local[j]), 300, local[j], big[j], 2.0) for j in range(B)]
        assert not np.isin(removed, np.concatenate([r[0] for r in want])).any()
        for mode in modes_of(s):
            bp, bs, bn, ls = s.search_batch(Qs, k, candidates=[c + off for c in local], candidate_priors=big, prior_weight=2.0,
                                            return_candidate_scores=True)
            for j in range(B):
                assert_result(bp[:, j], bs[:, j], bn[j], want[j], k, f"after remove mode={mode} q={j}", pid_offset=off)
                assert np.all(np.isneginf(ls[j][np.isin(local[j], removed)])), j
    finally:
        s.close()


# ---- 8. the device route ----------------------------------------------------------------------------------------------------
def test_device_route_eager_graph_and_values_the_host_would_refuse(oracle):
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=256)
    k, B, L, w = 10, 4, 600, 0.5
    Qs = synthetic.make_queries(idx, 31, B)
    Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
    rng = np.random.default_rng(13)
    rounds = [[messy_list(6000, n, 300 + 10 * r + j) for j, n in enumerate(ns)]
              for r, ns in enumerate(((600, 5, 130, 64), (1, 600, 0, 77), (300, 300, 300, 300)))]
    vrounds = [[rng.normal(0, 0.5, c.size).astype(np.float32) for c in lists] for lists in rounds]
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            for with_scores in (False, True):
                run = DeviceSearch(s, 32, B, k, 2)
                block, lens = as_block(rounds[0], L=L)
                d_p, d_n = torch.from_numpy(np.ascontiguousarray(block.T)).cuda(), torch.from_numpy(lens).cuda()
                d_v = torch.from_numpy(np.ascontiguousarray(value_block(vrounds[0], L=L).T)).cuda()
                d_sc = torch.zeros((B, L), dtype=torch.float32, device="cuda") if with_scores else None
                kw = dict(candidates=(d_p, d_n), candidate_scores=d_sc, candidate_priors=d_v, prior_weight=w)

                def check(lists, vals, what, weight=w):
                    torch.cuda.synchronize()
                    gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
                    host = s.search_batch(Qs, k, candidates=lists, candidate_priors=vals, prior_weight=weight,
                                          return_candidate_scores=True)                                # the host route
                    assert np.array_equal(gp.T, host[0]) and np.array_equal(bits(gs.T), bits(host[1])), what
                    assert np.array_equal(gn, host[2]), what
                    for j in range(B):
                        ref = boosted(list_ranking(oracle, idx, Qs[:, :, j], lists[j]), 6000, lists[j], vals[j], weight)
                        assert_result(gp[j], gs[j], gn[j], ref, k, f"{what} q={j}")
                    if with_scores:
                        ls = d_sc.cpu().numpy()
                        for j in range(B):
                            assert np.array_equal(bits(ls[j, :len(lists[j])]), bits(host[3][j])), (what, j)
                            assert np.all(np.isneginf(ls[j, len(lists[j]):])), (what, j)

                run(Qdev, **kw)                                                            # eager
                check(rounds[0], vrounds[0], f"eager mode={mode} scores={with_scores}")
                graph = run.capture(Qdev, **kw)                                            # captured once
                nbytes = s.device_bytes
                for r in (1, 2):                       # pids, lengths and values overwritten in place
                    block, lens = as_block(rounds[r], L=L)
                    d_p.copy_(torch.from_numpy(np.ascontiguousarray(block.T)))
                    d_n.copy_(torch.from_numpy(lens))
                    d_v.copy_(torch.from_numpy(np.ascontiguousarray(value_block(vrounds[r], L=L).T)))
                    graph = run.replay(graph, Qdev, **kw)
                    check(rounds[r], vrounds[r], f"replay {r} mode={mode} scores={with_scores}")
                    assert s.device_bytes == nbytes                                        # the replayed call allocated nothing
        # what the host route refuses counts as 0 on the device: NaN, +-Inf, and a product with the weight that overflows
        run = DeviceSearch(s, 32, B, k, 2)
        lists, big_w = rounds[2], 4.0
        bad = [v.copy() for v in vrounds[2]]
        bad[0][[0, 17, 299]] = [np.nan, np.inf, -np.inf]
        bad[1][[3, 4]] = [1e38, -3e38]                                  # finite, but 4 * 1e38 is not
        bad[3][:] = np.nan
        zeroed = [np.where(np.isfinite(v) & (np.abs(v) < 8e37), v, np.float32(0)).astype(np.float32) for v in bad]
        assert sum(int(np.count_nonzero(a != b)) for a, b in zip(bad, zeroed)) == 5 + 300
        block, lens = as_block(lists, L=L)
        d_p, d_n = torch.from_numpy(np.ascontiguousarray(block.T)).cuda(), torch.from_numpy(lens).cuda()
        d_v = torch.from_numpy(np.ascontiguousarray(value_block(bad, L=L).T)).cuda()
        with_scores, d_sc = True, torch.zeros((B, L), dtype=torch.float32, device="cuda")
        with pytest.raises(clb.ArgumentError, match="the candidate prior of query 0, position 0 is not a finite number"):
            s.search_batch(Qs, k, candidates=lists, candidate_priors=bad, prior_weight=big_w)
        for mode in modes_of(s):
            run(Qdev, candidates=(d_p, d_n), candidate_scores=d_sc, candidate_priors=d_v, prior_weight=big_w)
            check(lists, zeroed, f"refused values mode={mode}", big_w)
        # the tensor is checked like the other list tensors: dtype, device, contiguity, shape
        good_p, good_n = torch.zeros((B, L), dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
        for wrong in (torch.zeros((B, L), dtype=torch.float64, device="cuda"), torch.zeros((B, L + 1), device="cuda"),
                      torch.zeros((B, L)), torch.zeros((L, B), device="cuda").t(), np.zeros((B, L), np.float32)):
            with pytest.raises(clb.ArgumentError, match="candidate_priors must be a contiguous float32"):
                run(Qdev, candidates=(good_p, good_n), candidate_priors=wrong)
    finally:
        s.close()


def test_seventy_queries_read_their_own_rows(oracle):
    """sub-batches above 64 queries read their own rows of the value block, on both routes"""
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=256)
    B, k = 70, 20
    Qs = synthetic.make_queries(idx, 31, B)
    rng = np.random.default_rng(8)
    lists = [messy_list(6000, int(n), 200 + j) for j, n in enumerate(rng.integers(0, 200, B))]
    lists[63], lists[64] = messy_list(6000, 199, 1), messy_list(6000, 150, 2)
    vals = [rng.normal(0, 0.5, c.size).astype(np.float32) for c in lists]
    want = [boosted(list_ranking(oracle, idx, Qs[:, :, j], lists[j]), 6000, lists[j], vals[j], 1.0) for j in range(B)]
    s = clb.Searcher(index=idx)
    try:
        block, lens = as_block(lists)
        d_p, d_n = torch.from_numpy(np.ascontiguousarray(block.T)).cuda(), torch.from_numpy(lens).cuda()
        d_v = torch.from_numpy(np.ascontiguousarray(value_block(vals).T)).cuda()
        Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
        for mode in modes_of(s):
            bp, bs, bn = s.search_batch(Qs, k, candidates=lists, candidate_priors=vals)
            run = DeviceSearch(s, 32, B, k, 2)
            run(Qdev, candidates=(d_p, d_n), candidate_priors=d_v)
            torch.cuda.synchronize()
            gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
            for j in range(B):
                assert_result(bp[:, j], bs[:, j], bn[j], want[j], k, f"B=70 host mode={mode} q={j}")
                assert_result(gp[j], gs[j], gn[j], want[j], k, f"B=70 device mode={mode} q={j}")
    finally:
        s.close()


# ---- 9. refusals on a live handle -------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(medium, medium_searcher):
    idx, Qs, lists, rankings, values, refs = medium
    s = medium_searcher
    three, v3 = [lists[2], lists[3], lists[1]], [values["comparable"][i] for i in (2, 3, 1)]
    kw = dict(candidates=three, candidate_priors=v3)
    with s.make_prior(np.zeros(20_000, np.float32)) as pr, s.make_grouping(group_lens=random_lens(20_000, 1, 6, 80)) as g:
        with pytest.raises(clb.Unsupported, match="candidate_priors together with prior"):
            s.search_batch(Qs, 10, prior=pr, **kw)
        with pytest.raises(clb.Unsupported, match="per_group together with candidate_priors"):
            s.search_batch(Qs, 10, grouping=g, per_group=2, **kw)
        with pytest.raises(clb.Unsupported, match="after together with candidate_priors"):
            s.search_batch(Qs, 10, after=(np.full(3, np.inf, np.float32), np.zeros(3, np.int64)), **kw)
        # ... and the library's own refusals, past the Python builder
        from colbert_jl_amd.searcher import search_request
        q = np.asfortranarray(Qs)
        out_p, out_s, n = np.zeros((2, 10, 3), np.int64, order="F"), np.zeros((2, 10, 3), np.float32, order="F"), np.zeros(3, np.int64)
        cs, cp = np.full(3, np.inf, np.float32), np.zeros(3, np.int64)
        for fields, message in ((dict(prior=pr._h), b"list priors together with a prior are not supported"),
                                (dict(grouping=g._h, per_group=2), b"per_group together with list priors"),
                                (dict(after_scores=cs.ctypes.data, after_pids=cp.ctypes.data), b"cursors together with list priors")):
            req = search_request(s, 3, **kw)
            for name, value in fields.items():
                setattr(req, name, value)
            rc = clb.lib().clb_search_batch_request(s._h, q.ctypes.data, 32, 3, 2, 10, req, out_p.ctypes.data, out_s.ctypes.data,
                                                    n.ctypes.data)
            assert rc == clb.Unsupported.code and message in clb.lib().clb_last_error(), message
    # the values are checked against their own lists, the weight against the largest listed |value|
    with pytest.raises(clb.ArgumentError, match="query 1 hold 999 values for a list of 1000 pids"):
        s.search_batch(Qs, 10, candidates=three, candidate_priors=[v3[0], v3[1][:-1], v3[2]])
    with pytest.raises(clb.ArgumentError, match="is not below FLT_MAX"):
        s.search_batch(Qs, 10, prior_weight=1e38, candidates=three, candidate_priors=[v3[0], v3[1] * 100, v3[2]])


# ---- 10. no change without list priors --------------------------------------------------------------------------------------
def test_calls_without_list_priors_launch_what_they_launched(medium, medium_searcher):
    """The plain call, the listed call and the listed entry with list_prior == NULL report the launch counts of the calls that
    never heard of the keyword; a call WITH list priors reports more, so the counts can tell."""
    idx, Qs, lists, rankings, values, refs = medium
    s = medium_searcher
    Qb, lb, vb, rb, plain, w = batch_of(medium, "comparable", 9)
    block, lens = as_block(lb)
    pids, L = np.ascontiguousarray(block.T), block.shape[0]
    vals = np.ascontiguousarray(value_block(vb).T)
    out_p, out_s, n = np.zeros((9, 10), np.int64), np.zeros((9, 10), np.float32), np.zeros(9, np.int64)
    p = lambda a: a.ctypes.data
    l = clb.lib()

    def counts(call):
        s.profile_read()
        call()
        return {name: v["launches"] for name, v in s.profile_read().items()}

    def listed_entry():
        assert l.clb_search_batch_listed(s._h, p(Qb), 32, 9, 2, 10, p(pids), p(lens), L, None, p(out_p), p(out_s), p(n)) == 0

    def listed_prior_entry(values):
        def call():
            assert l.clb_search_batch_listed_prior(s._h, p(Qb), 32, 9, 2, 10, p(pids), p(lens), L, None if values is None else p(values),
                                                   C.c_float(1.0), None, p(out_p), p(out_s), p(n)) == 0
        return call
    s.profile_enable(True)
    try:
        for mode in (0, 1):
            s.set_mode(mode)
            plain_counts = counts(lambda: s.search_batch(Qb, 10))
            listed_counts = counts(listed_entry)
            assert counts(lambda: s.search_batch(Qb, 10, candidate_priors=None, prior_weight=3.0)) == plain_counts, mode
            assert counts(lambda: s.search_batch(Qb, 10, candidates=lb)) == listed_counts, mode
            assert counts(lambda: s.search_batch(Qb, 10, candidates=lb, candidate_priors=None)) == listed_counts, mode
            assert counts(listed_prior_entry(None)) == listed_counts, mode
            ref_p, ref_s = out_p.copy(), out_s.copy()
            listed_entry()
            assert np.array_equal(ref_p, out_p) and np.array_equal(bits(ref_s), bits(out_s))       # ... and the same result
            with_priors = counts(listed_prior_entry(vals))
            assert with_priors != listed_counts and sum(with_priors.values()) > sum(listed_counts.values()), mode
            for j in range(9):
                assert_result(out_p[j], out_s[j], n[j], rb[j], 10, f"the named entry mode={mode} q={j}")
    finally:
        s.profile_enable(False)
        s.set_mode(1)
