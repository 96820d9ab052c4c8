"""Hits of a grouped search (`per_group=m`) on the GPU against tests/util_group_hits.hits_reference over the oracle's full
stable ranking of the query's (filtered) candidates: the first k distinct groups, of each its first m occurrences.  Every
comparison: pids equal, fp32 score bits equal, n_cand (the candidate groups) equal, pid 0 / -Inf padding."""
import ctypes as C
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import util_general as ug
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import bits, random_allowed
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index
from tests.util_filter import filtered_ranking
from tests.util_group import collapse, ids_from_lens, random_lens
from tests.util_group_hits import assert_hits, hits_reference

pytestmark = pytest.mark.gpu


def modes_of(s, modes=(0, 1)):
    """set_mode over the modes the handle has (two-pass: dim 128, nbits 2 only)"""
    for mode in modes:
        try:
            s.set_mode(mode)
        except clb.Unsupported:
            continue
        yield mode


def check_hits(s, g, gids, rankings, Qb, k, m, what, nprobe=2, filters=None, scope="candidates", pid_offset=0, queries=None):
    """one batch call with per_group=m against the reference over `rankings` (the full (filtered) rankings of Qb's queries)"""
    bp, bs, bn = s.search_batch(Qb, k, nprobe=nprobe, pad_short=True, filters=filters, scope=scope, grouping=g, per_group=m)
    assert bp.shape == (m, k, Qb.shape[2]) and bp.flags.f_contiguous and bs.flags.f_contiguous
    for j in (range(Qb.shape[2]) if queries is None else queries):
        assert_hits(bp[:, :, j], bs[:, :, j], bn[j], rankings[j], gids, k, m, f"{what} k={k} m={m} q={j}", pid_offset)
    return bp, bs, bn


@pytest.fixture(scope="module")
def medium(oracle):
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 9)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]


# ---- 1. basic parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["singletons", "lens4", "random_1_40", "one_group"])
def test_hits_basic_parity(oracle, medium, grouping):
    """20 000 passages, B = 9, m = 1, 2, 3, 16 and k = 1, 10, 100, 1000, exact and two-pass with either gather form."""
    idx, Qs, rankings = medium
    n_docs = 20_000
    lens = {"singletons": np.ones(n_docs, np.int64), "lens4": np.full(n_docs // 4, 4), "random_1_40": random_lens(n_docs, 1, 40, 5),
            "one_group": np.array([n_docs])}[grouping]
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        g = s.make_grouping(group_lens=lens)
        auto_form = s.pass1_gather[0]
        for mode in modes_of(s):
            for form in ((-1, 1 - auto_form) if mode == 1 else (-1,)):
                s.set_pass1_gather(form)
                for k in (1, 10, 100, 1000):
                    grouped = s.search_batch(Qs, k, pad_short=True, grouping=g)
                    for m in (1, 2, 3, 16):
                        what = f"{grouping} mode={mode} form={form}"
                        bp, bs, bn = check_hits(s, g, gids, rankings, Qs, k, m, what)
                        # entry 0 of every group is the grouped search, bit for bit (m = 1: all of it)
                        assert np.array_equal(bp[0], grouped[0]) and np.array_equal(bits(bs[0]), bits(grouped[1])), what
                        assert np.array_equal(bn, grouped[2]), what
                        if grouping == "singletons":           # row 0 is the ungrouped search, the other rows are padding
                            up, us, un = s.search_batch(Qs, k, pad_short=True)
                            assert np.array_equal(bp[0], up) and np.array_equal(bits(bs[0]), bits(us)) and np.array_equal(bn, un)
                            assert np.all(bp[1:] == 0) and np.all(np.isneginf(bs[1:]))
                    if grouping == "one_group" and k == 1:     # the 16 hits of the only group: the ungrouped top-16
                        up, us, _ = s.search_batch(Qs, 16, pad_short=True)
                        assert np.array_equal(bp[:, 0, :], up) and np.array_equal(bits(bs[:, 0, :]), bits(us))
            s.set_pass1_gather(-1)
        # one query through the single-query calls: (m, k)
        p, sc = s.search_embeddings(Qs[:, :, 0], 10 if grouping != "one_group" else 1, grouping=g, per_group=3)
        k1 = p.shape[1]
        assert_hits(p, sc, s.last_num_candidates, rankings[0], gids, k1, 3, f"{grouping} search_embeddings")
        p2, sc2 = clb.search(s, Qs[:, :, 0], k1, grouping=g, per_group=3)
        assert np.array_equal(p, p2) and np.array_equal(bits(sc), bits(sc2))
        g.close()
    finally:
        s.close()


# ---- 2. one document holds many of the best passages ------------------------------------------------------------------------
def test_hits_on_a_dominated_collection(oracle):
    """6 000 passages in 120 groups of 50; a group is five base passages, each ten times: ten-fold exact score ties inside
    every group, which the lower pid must win."""
    base = synthetic.make_index(seed=71, n_docs=600, K=256)
    p = np.arange(6000)
    donors = 5 * (p // 50) + (p % 50) % 5 + 1
    co, re, dl = content_of(base, donors)
    idx = dict(base, codes=co, residuals=re, doclens=dl)
    idx["ivf"], idx["ivf_lengths"] = synthetic.build_ivf(co, 256)
    Qs = synthetic.make_queries(idx, 72, 4)
    k = 100
    gids = ids_from_lens([50] * 120)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(4)]
    rp, rs, _ = hits_reference(rankings[0], gids, k, 16)       # the precondition: ties among the hits of one group
    assert np.any((rs[1:, :] == rs[:-1, :]) & (rp[1:, :] > 0)) and np.all((rp[1:, :] > rp[:-1, :]) | (rs[1:, :] < rs[:-1, :]) | (rp[1:, :] == 0))
    s = clb.Searcher(index=idx)
    try:
        with s.make_grouping(group_ids=gids) as g:
            for mode in modes_of(s):
                for m in (5, 16):
                    check_hits(s, g, gids, rankings, Qs, k, m, f"dominated mode={mode}")
    finally:
        s.close()


# ---- 3. runs that end on the edges of the new kernels -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    idx = synthetic.make_index(seed=81, n_docs=40_000, doclen_mean=3, doclen_std=1, K=512)
    assert idx["doclens"].min() >= 1                           # every passage is a candidate: slot i is passage i + 1
    Qs = synthetic.make_queries(idx, 82, 3)
    everything = np.arange(1, 40_001)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 2, everything, "all") for j in range(3)]


def edge_groupings():
    """Group lengths over 40 000 slots whose runs end exactly at the given slots (the entry BEFORE a boundary in `cuts` is the
    last of its run), short random runs elsewhere.  The edges are those of the two kernels the hits add:
      * the m-th best of every run (group_extend_kernel) walks all candidates in the tiles of the collapse: a thread owns 8
        entries, a wave 512, a tile 8192; the last tile (from slot 32 768) spreads its 7232 entries over the threads again;
      * its ordered compaction gives thread t the slots [40 t, 40 t + 40) of the 40 000: thread edges at multiples of 40,
        wave edges at multiples of 2560;
      * the hits of a result (group_hits_kernel) are read by one wave, the first 64 entries of the run in registers and the
        rest in strides of 64: runs of 63, 64, 65, 127, 128 and 129 entries (in the exact mode a run of the grouping is a
        run of that kernel), and a run of 5000."""
    def from_cuts(cuts, seed):
        rng = np.random.default_rng(seed)
        cuts = sorted(set(cuts) | {40_000})
        lens, at = [], 0
        for c in cuts:
            while c - at > 5000:                               # fill with short runs up to the next forced boundary
                n = int(rng.integers(1, 30))
                lens.append(n); at += n
            if c > at:
                lens.append(c - at); at = c
        return np.asarray(lens, np.int64)
    wave_runs = [63, 64, 65, 127, 128, 129]
    wave_cuts = list(np.cumsum([100] + wave_runs)) + list(20_000 + np.cumsum([0] + wave_runs))
    return {"run_of_5000": from_cuts([17_000, 22_000], 1),
            "extend_thread_wave": from_cuts([7, 8, 9, 504, 511, 512, 513, 520], 2),
            "extend_tiles": from_cuts([8184, 8191, 8192, 8193, 16_384, 24_577, 32_767, 32_768, 32_769, 39_999], 3),
            "compaction_edges": from_cuts([39, 40, 41, 2559, 2560, 2561, 5120, 39_960], 4),
            "hits_wave_strides": from_cuts(wave_cuts, 5),
            "whole_tiles": np.array([8192, 8192, 1, 8191, 15_424], np.int64)}


@pytest.mark.parametrize("name", list(edge_groupings()))
def test_hits_with_runs_on_every_edge(oracle, wide, name):
    """40 000 candidates per query (a scope "all" filter over every pid), m = 16; one and sixteen work-groups per query in
    the selection whose threshold the extension reads."""
    idx, Qs, rankings = wide
    lens = edge_groupings()[name]
    assert int(lens.sum()) == 40_000
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(mask=np.ones(40_000, bool)) as f, s.make_grouping(group_lens=lens) as g:
            for wide_sel in (0, 1):
                s.set_wide_select(wide_sel)
                for mode in modes_of(s, (1, 0) if wide_sel == 0 else (1,)):
                    for k in (5, 300):
                        _, _, bn = check_hits(s, g, gids, rankings, Qs, k, 16, f"{name} wide={wide_sel} mode={mode}", filters=f,
                                              scope="all")
                        assert np.all(bn == lens.size)
    finally:
        s.close()


# ---- 4. filters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("selectivity", [0.5, 0.02])
def test_hits_with_filters(oracle, medium, scope, selectivity):
    """per-query filters (two filtered queries and an unfiltered one); at selectivity 0.02 most groups keep one passage"""
    idx, Qs, _ = medium
    Q3 = np.asfortranarray(Qs[:, :, :3])
    alloweds = [random_allowed(20_000, selectivity, 300 + j) for j in range(2)] + [None]
    rankings = [filtered_ranking(oracle, idx, Q3[:, :, j], 2, alloweds[j], scope) for j in range(3)]
    lens = random_lens(20_000, 1, 9, 6)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        filters = [None if a is None else s.make_filter(pids=a) for a in alloweds]
        with s.make_grouping(group_ids=gids * 2 + 11) as g:    # any non-decreasing ids
            for mode in modes_of(s):
                for k, m in ((10, 2), (10, 16), (1000, 3)):
                    check_hits(s, g, gids, rankings, Q3, k, m, f"{scope} sel={selectivity} mode={mode}", filters=filters, scope=scope)
                p, sc = s.search_embeddings(Q3[:, :, 0], 10, filter=filters[0], scope=scope, grouping=g, per_group=4)
                assert_hits(p, sc, s.last_num_candidates, rankings[0], gids, 10, 4, "single query")
        for f in filters:
            if f is not None:
                f.close()
    finally:
        s.close()


def test_a_filter_that_leaves_a_winner_short_and_fewer_than_k_groups(oracle, medium):
    """Ten groups of four allowed, three of them cut to one or two passages: k = 25 is a short result (padded columns), the
    cut groups are short columns (padded rows) -- never an error through the padded calls, CLB_EBOUNDS from the C call that
    did not ask for padding, as for the grouped search."""
    idx, Qs, _ = medium
    gids = ids_from_lens(np.full(5000, 4))
    allowed = np.setdiff1d(np.arange(4001, 4041), [4002, 4003, 4004, 4010, 4011, 4039])
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(pids=allowed) as f, s.make_grouping(group_ids=gids) as g:
            for mode in modes_of(s):
                for scope in ("all", "candidates"):
                    r = filtered_ranking(oracle, idx, Qs[:, :, 0], 2, allowed, scope)
                    for m in (2, 4, 16):
                        p, sc = clb.search(s, Qs[:, :, 0], 25, filter=f, scope=scope, grouping=g, per_group=m)
                        assert_hits(p, sc, s.last_num_candidates, r, gids, 25, m, f"short {scope} mode={mode} m={m}")
                        bp, bs, bn = s.search_batch(Qs, 25, filters=f, scope=scope, grouping=g, pad_short=True, per_group=m)
                        assert_hits(bp[:, :, 0], bs[:, :, 0], bn[0], r, gids, 25, m, f"short batch {scope} mode={mode} m={m}")
                    if scope == "all":                         # the preconditions, from the reference: a short result ...
                        rp, _, rn = hits_reference(r, gids, 25, 2)
                        assert rn == 10 and np.all(p[:, 10:] == 0) and np.all(np.isneginf(sc[:, 10:]))
                        assert np.any((rp[0] > 0) & (rp[1] == 0))      # ... and a winner with fewer than two passages
                q = np.asfortranarray(Qs[:, :, :1])
                op, os_, nc = np.zeros(50, np.int64), np.zeros(50, np.float32), np.zeros(1, np.int64)
                ptr = lambda a: a.ctypes.data_as(C.c_void_p)
                rc = clb.lib().clb_search_batch_grouped_hits(s._h, ptr(q), 32, 1, 2, 25, (C.c_void_p * 1)(f._h.value), 1, g._h, 2, 0,
                                                             ptr(op), ptr(os_), ptr(nc))
                assert rc == clb.BoundsError.code and b"10 candidate groups" in clb.lib().clb_last_error()
    finally:
        s.close()


# ---- 5. sub-batches -------------------------------------------------------------------------------------------------------
def test_hits_sub_batches(oracle, medium):
    """B = 70: two sub-batches of the single call, one grouping and one per_group for both."""
    idx, _, _ = medium
    Qs = synthetic.make_queries(idx, 70, 70)
    checked = (0, 1, 63, 64, 69)
    rankings = {j: filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in checked}
    lens = random_lens(20_000, 1, 12, 7)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        with s.make_grouping(group_lens=lens) as g:
            for mode in modes_of(s):
                check_hits(s, g, gids, rankings, Qs, 200, 3, f"B=70 mode={mode}", queries=checked)
    finally:
        s.close()


# ---- 6. general shapes and the other code widths -----------------------------------------------------------------------------
GENERAL = [(64, 2, 20, "batched32"), (136, 4, 20, "batched64"), (128, 2, 150, "loop_mfma"), (128, 2, 513, "scalar")]


def test_the_general_cases_take_all_four_routes():
    assert [ug.expected_route(d, nb, T) for d, nb, T, _ in GENERAL] == [r for *_, r in GENERAL]
    assert {r for *_, r in GENERAL} == set(ug.ROUTES)


@pytest.mark.parametrize("dim,nbits,T,route", GENERAL)
def test_hits_general_shapes(oracle, dim, nbits, T, route):
    if T > 128:
        idx = synthetic.make_index(seed=43, n_docs=900 if T > 512 else 3000, K=128, doclen_mean=24, doclen_std=6)
    else:
        idx = synthetic.make_index(seed=41 + dim + nbits, n_docs=900, K=96, dim=dim, nbits=nbits, doclen_mean=30, doclen_std=12)
    n_docs = idx["doclens"].size
    Qs = synthetic.make_queries(idx, 42, 3, T=T)
    lens = random_lens(n_docs, 1, 7, 8)
    gids = ids_from_lens(lens)
    allowed = random_allowed(n_docs, 0.4, 7)
    s = clb.Searcher(index=idx)
    try:
        with s.make_grouping(group_lens=lens) as g, s.make_filter(pids=allowed) as f:
            plain = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)]
            check_hits(s, g, gids, plain, Qs, 40, 3, route)
            filt = [filtered_ranking(oracle, idx, Qs[:, :, j], 2, allowed, "all") for j in range(3)]
            check_hits(s, g, gids, filt, Qs, 7, 16, f"{route} all", filters=f, scope="all")
    finally:
        s.close()


@pytest.mark.parametrize("nbits", [1, 4])
def test_hits_other_code_widths(oracle, nbits):
    """nbits 1 and 4 at dim 128: the tuned path in its single-pass form"""
    idx = synthetic.make_index(seed=51 + nbits, n_docs=3000, K=256, nbits=nbits)
    Qs = synthetic.make_queries(idx, 52, 9)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]
    lens = random_lens(3000, 1, 10, 9)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        with s.make_grouping(group_lens=lens) as g:
            for k, m in ((1, 16), (50, 2), (600, 5)):
                check_hits(s, g, gids, rankings, Qs, k, m, f"nbits={nbits}")
                check_hits(s, g, gids, rankings, np.asfortranarray(Qs[:, :, :1]), k, m, f"nbits={nbits} B=1", queries=[0])
    finally:
        s.close()


# ---- 7. after remove and update ----------------------------------------------------------------------------------------------
def test_hits_after_remove_and_update_but_not_after_an_append(oracle):
    full = synthetic.make_index(0, 330, K=64)
    idx = head_index(full, 300)
    Qs = synthetic.make_queries(idx, 1000, 9)
    lens = random_lens(300, 2, 12, 10)
    gids = ids_from_lens(lens)
    before = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]
    top = collapse(before[0], gids)
    removed = np.array([top[0][0]])                            # query 0's best passage goes: its group keeps the others
    low = before[0][0][-1]                                     # query 0's worst candidate gets the content of its best
    assert gids[low - 1] != gids[top[0][0] - 1]
    want, _ = reduced_index(idx, removed)
    upd = ([low], *content_of(idx, [top[0][0]]))
    want = updated_index(want, *upd)
    s = clb.Searcher(index=idx)
    try:
        g = s.make_grouping(group_ids=gids)
        assert s.remove_passages(removed) == 1
        assert s.update_compressed(*upd) == 1
        after = [filtered_ranking(oracle, want, Qs[:, :, j], 2) for j in range(9)]
        assert hits_reference(after[0], gids, 1, 2)[0][0, 0] == low
        for mode in modes_of(s):
            for k, m in ((1, 2), (10, 3), (40, 16)):
                check_hits(s, g, gids, after, Qs, k, m, f"after remove + update mode={mode}")
        assert s.add_compressed(*tail(full, 300)) == range(301, 331)
        with pytest.raises(clb.ArgumentError, match="grouping made before an append; make another"):
            s.search_batch(Qs, 10, grouping=g, per_group=2)
        g.close()
    finally:
        s.close()


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------
def test_captured_graph_replays_the_hits(oracle):
    """The device-slot entry point with per_group captured as a HIP graph over a static query buffer: every replay with new
    queries equals the stream call and the reference."""
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=1024)
    k, m = 60, 3
    a = [random_allowed(6000, 0.5, 1), random_allowed(6000, 0.02, 2)]
    lens = random_lens(6000, 1, 15, 11)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    f = [s.make_filter(pids=x) for x in a]
    g = s.make_grouping(group_lens=lens)
    try:
        for B, filtered in ((1, False), (17, False), (17, True)):
            Qs = synthetic.make_queries(idx, 31, 2 * B)
            Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
            run = DeviceSearch(s, 32, B, k, 2)
            order = [(j % 3) if j % 3 < 2 else None for j in range(B)]
            fb = [None if o is None else f[o] for o in order] if filtered else None
            q_static = Qdev[:B].clone()
            graph = run.capture(q_static, fb, "candidates", g, m)
            for it in range(2):
                q_static.copy_(Qdev[it * B:(it + 1) * B])
                graph = run.replay(graph, q_static, fb, "candidates", g, m)
                torch.cuda.synchronize()
                gp, gs, gn = run.hit_p.cpu().numpy().copy(), run.hit_s.cpu().numpy().copy(), run.ncand.cpu().numpy().copy()
                assert gp.shape == (B, k, m)
                run.hit_p.zero_(); run.hit_s.zero_()
                hp, hs = run(Qdev[it * B:(it + 1) * B], fb, "candidates", g, m)
                torch.cuda.synchronize()
                assert np.array_equal(gp, hp.cpu().numpy()) and np.array_equal(gn, run.ncand.cpu().numpy())
                assert np.array_equal(bits(gs), bits(hs.cpu().numpy()))
                for j in range(0, B, 4):
                    allowed = a[order[j]] if filtered and order[j] is not None else None
                    r = filtered_ranking(oracle, idx, Qs[:, :, it * B + j], 2, allowed, "candidates")
                    assert_hits(gp[j].T, gs[j].T, gn[j], r, gids, k, m, f"graph B={B} filtered={filtered} it={it} q={j}")
            del graph
    finally:
        g.close()
        for x in f:
            x.close()
        s.close()


# ---- 9. contracts -----------------------------------------------------------------------------------------------------------
def test_per_group_contracts_on_a_live_searcher(oracle):
    idx = synthetic.make_index(seed=1, n_docs=300, K=64)
    Qs = synthetic.make_queries(idx, 2, 2)
    off = 1000
    ids = ids_from_lens([100, 150, 50])
    s = clb.Searcher(index=idx, pid_offset=off)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    try:
        with s.make_grouping(group_ids=ids) as g:
            for bad in (0, 17):
                with pytest.raises(clb.ArgumentError, match="per_group must be 1..16"):
                    s.search_batch(Qs, 3, grouping=g, per_group=bad)
                op, os_, nc = np.zeros(3 * 17, np.int64), np.zeros(3 * 17, np.float32), np.zeros(1, np.int64)
                q = np.asfortranarray(Qs[:, :, :1])
                assert clb.lib().clb_search_batch_grouped_hits(s._h, ptr(q), 32, 1, 2, 3, None, 0, g._h, bad, 1, ptr(op), ptr(os_),
                                                               ptr(nc)) == clb.ArgumentError.code
            with pytest.raises(clb.ArgumentError, match="needs grouping="):
                s.search_batch(Qs, 3, per_group=2)
            op, os_, nc = np.zeros(6, np.int64), np.zeros(6, np.float32), np.zeros(1, np.int64)
            q = np.asfortranarray(Qs[:, :, :1])
            assert clb.lib().clb_search_batch_grouped_hits(s._h, ptr(q), 32, 1, 2, 3, None, 0, None, 2, 1, ptr(op), ptr(os_),
                                                           ptr(nc)) == clb.ArgumentError.code
            ranking = filtered_ranking(oracle, idx, Qs[:, :, 0], 2)
            check_hits(s, g, ids, [ranking] * 2, np.asfortranarray(Qs[:, :, [0, 0]]), 3, 4, "pid_offset", pid_offset=off)
        with clb.ShardedSearcher([clb.Searcher(index=idx)]) as group, group.make_grouping(group_ids=ids) as sg:
            with pytest.raises(clb.Unsupported, match="per_group"):
                group.search_batch(Qs, 2, grouping=sg, per_group=2)
            with pytest.raises(clb.Unsupported, match="per_group"):
                group.search_embeddings(Qs[:, :, 0], 2, grouping=sg, per_group=1)
            p, _, _ = group.search_batch(Qs, 2, grouping=sg, pad_short=True)       # ... and searches on without it
            assert p.shape == (2, 2)
    finally:
        s.close()


# ---- 10. random configurations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("COLBERT_TEST_FUZZ_SEEDS", "8"))))
def test_hits_random_configurations(oracle, seed):
    """Randomly drawn shapes (corpus, centroids, nbits, passage lengths, query length, batch, k, nprobe, per_group), a random
    non-decreasing grouping and an optional filter."""
    rng = np.random.default_rng(8000 + seed)
    n_docs = int(rng.integers(40, 6000))
    K = int(2 ** rng.integers(3, 11))
    nbits = int(rng.choice([1, 2, 2, 2, 4]))
    idx = synthetic.make_index(seed=8100 + seed, n_docs=n_docs, K=K, nbits=nbits, doclen_mean=float(rng.integers(4, 120)),
                               doclen_std=float(rng.integers(0, 40)), topical=bool(rng.integers(0, 2)))
    T = int(rng.choice([1, 3, 17, 32, 32, 32, 33, 48]))
    B = int(rng.integers(1, 10))
    Qs = synthetic.make_queries(idx, 8200 + seed, B, T=T)
    k = int(min(n_docs, rng.choice([1, 10, 100, 1000, n_docs])))
    m = int(rng.integers(1, 17))
    nprobe = int(min(K, rng.choice([1, 2, 2, 3, 8])))
    lens = random_lens(n_docs, 1, int(rng.choice([1, 2, 8, 50, n_docs])), 8300 + seed)
    gids = np.cumsum(np.concatenate([[int(rng.integers(-5, 5))], rng.integers(1, 4, size=lens.size - 1)]))      # the caller's ids
    gids = np.repeat(gids, lens)
    scope = str(rng.choice(["candidates", "all"]))
    allowed = None if rng.integers(0, 2) == 0 else random_allowed(n_docs, float(rng.choice([1.0, 0.5, 0.1, 0.01])), 8400 + seed)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe, allowed, scope) for j in range(B)]
    s = clb.Searcher(index=idx)
    try:
        f = None if allowed is None else s.make_filter(pids=allowed)
        with s.make_grouping(group_ids=gids) as g:
            for mode in modes_of(s):
                check_hits(s, g, gids, rankings, Qs, k, m, f"seed={seed} mode={mode}", nprobe=nprobe, filters=f, scope=scope)
        if f is not None:
            f.close()
    finally:
        s.close()


# ---- 11. the extended list really runs, and is not "list everything" -----------------------------------------------------------
def test_the_extended_list_runs_and_stays_inside_the_listed_groups(oracle, medium):
    """Groups of 4, k = 10, two-pass mode.  Precondition, from the oracle's ranking and the eps the device reports: some winning
    group's second-best candidate scores below S_k - 4 eps - 0.05 exactly (S_k = the 10th group's score; the 0.05 covers the
    coarse tau of the selection), so the list of the grouped search cannot hold it and the second hits can only come from the
    extension.  Then, on the re-scored passages of the batch: the extension adds some (grouped < hits(m = 2)), every added
    passage shares a group of 4 with a listed one (hits(m = 2) <= 4 grouped), and one hit per group adds none."""
    idx, Qs, rankings = medium
    k = 10
    gids = ids_from_lens(np.full(5000, 4))
    s = clb.Searcher(index=idx)
    try:
        s.set_mode(1)
        with s.make_grouping(group_ids=gids) as g:
            eps = max(float(s.debug_scores(Qs[:, :, j], k, 2)["eps"]) for j in range(3))
            assert np.isfinite(eps) and eps > 0
            found = 0
            for j in range(3):
                rp, rs, _ = hits_reference(rankings[j], gids, k, 2)
                s_k = rs[0, k - 1]
                second = rs[1, :][rp[1, :] > 0]
                found += int(np.count_nonzero(second < s_k - 4 * eps - 0.05))
            print(f"eps {eps:.4f}; winners of queries 0-2 whose second hit lies below S_k - 4 eps - 0.05: {found}")
            assert found > 0
            s.profile_enable(True, counters=True)
            counts = {}
            for name, kw in (("grouped", {}), ("m1", {"per_group": 1}), ("m2", {"per_group": 2})):
                s.search_batch(Qs, k, pad_short=True, grouping=g, **kw)
                counts[name] = s.last_batch_stats()["rescored_docs"]
            s.profile_enable(False)
            print(f"re-scored passages of 9 queries: {counts}")
            assert counts["grouped"] < counts["m2"] <= 4 * counts["grouped"]
            assert counts["m1"] == counts["grouped"]
            check_hits(s, g, gids, rankings, Qs, k, 2, "extended list")
    finally:
        s.close()
