"""Grouped search on the GPU against tests/util_group.grouped_reference: the oracle's full stable ranking of the query's
(filtered) candidates with the first occurrence of every group kept.  Every comparison: pids equal, fp32 score bits equal,
n_cand (the number of candidate groups) equal, short results padded with pid 0 / -Inf."""
import ctypes as C
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import util_general as ug
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import assert_result, assert_same_f32, bits, random_allowed
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index
from tests.util_filter import filtered_ranking
from tests.util_group import collapse, ids_from_lens, random_lens

pytestmark = pytest.mark.gpu


def modes_of(s, modes=(0, 1)):
    """set_mode over the modes the handle has (two-pass: dim 128, nbits 2 only)"""
    for mode in modes:
        try:
            s.set_mode(mode)
        except clb.Unsupported:
            continue
        yield mode


def check_batch(s, g, gids, rankings, Qb, k, what, nprobe=2, filters=None, scope="candidates", pid_offset=0, queries=None):
    """one grouped batch call against the collapse of `rankings` (the full (filtered) rankings of Qb's queries)"""
    bp, bs, bn = s.search_batch(Qb, k, nprobe=nprobe, pad_short=True, filters=filters, scope=scope, grouping=g)
    for j in (range(Qb.shape[2]) if queries is None else queries):
        assert_result(bp[:, j], bs[:, j], bn[j], collapse(rankings[j], gids), k, f"{what} k={k} q={j}", pid_offset)
    return bp, bs, bn


@pytest.fixture(scope="module")
def medium(oracle):
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 9)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]


# ---- 1. basic parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["singletons", "lens4", "random_1_40", "one_group"])
def test_grouped_search_basic_parity(oracle, medium, grouping):
    """20 000 passages, B = 9, k = 1, 10, 100, 1000, exact and two-pass with either gather form."""
    idx, Qs, rankings = medium
    n_docs = 20_000
    lens = {"singletons": np.ones(n_docs, np.int64), "lens4": np.full(n_docs // 4, 4), "random_1_40": random_lens(n_docs, 1, 40, 5),
            "one_group": np.array([n_docs])}[grouping]
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        g = s.make_grouping(group_lens=lens)
        assert g.count == lens.size == clb.lib().clb_grouping_count(g._h)
        auto_form = s.pass1_gather[0]
        for mode in modes_of(s):
            for form in ((-1, 1 - auto_form) if mode == 1 else (-1,)):
                s.set_pass1_gather(form)
                for k in (1, 10, 100, 1000):
                    bp, bs, bn = check_batch(s, g, gids, rankings, Qs, k, f"{grouping} mode={mode} form={form}")
                    if grouping == "singletons":               # ... which is the ungrouped search, bit for bit
                        up, us, un = s.search_batch(Qs, k, pad_short=True)
                        assert np.array_equal(bp, up) and np.array_equal(bn, un) and np.array_equal(bits(bs), bits(us))
                    if grouping == "one_group":
                        assert np.all(bn == 1) and (k == 1 or np.all(bp[1:] == 0))
                    assert np.array_equal(np.sort(g.groups_of(bp[:min(k, bn[0]), 0])),
                                          np.unique(g.groups_of(bp[:min(k, bn[0]), 0])))      # every group once
            s.set_pass1_gather(-1)
        if grouping == "one_group":                            # k = 1 answers, k = 2 is short
            p, sc = s.search_embeddings(Qs[:, :, 0], 1, grouping=g)
            assert p[0] == rankings[0][0][0] and s.last_num_candidates == 1
            with pytest.raises(clb.BoundsError, match="candidate groups"):
                s.search_embeddings(Qs[:, :, 0], 2, grouping=g)
            with pytest.raises(clb.BoundsError):
                s.search_batch(Qs, 2, grouping=g)
        g.close()
    finally:
        s.close()


# ---- 2. one document holds many of the best passages ------------------------------------------------------------------------
def test_dominated_collection(oracle):
    """6 000 passages in 120 groups of 50; a group is five base passages, each ten times: the best passages of a query crowd
    into few groups, and a host-side collapse of an ungrouped top-4k would come out short."""
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
    for rp, _ in rankings:                                     # the precondition, from the oracle alone
        assert rp.size >= 4 * k and np.unique(gids[rp[:4 * k] - 1]).size < k
    s = clb.Searcher(index=idx)
    try:
        with s.make_grouping(group_ids=gids) as g:
            for mode in modes_of(s):
                check_batch(s, g, gids, rankings, Qs, k, f"dominated mode={mode}")
            assert s.mode == 1
            s.profile_enable(True, counters=True)
            s.search_batch(Qs, k, pad_short=True)
            plain = s.last_batch_stats()["rescored_docs"]
            s.search_batch(Qs, k, pad_short=True, grouping=g)
            grouped = s.last_batch_stats()["rescored_docs"]
            s.profile_enable(False)
            print(f"dominated collection: re-scored passages of 4 queries, ungrouped {plain}, grouped {grouped}")
            assert grouped > plain
    finally:
        s.close()


# ---- 3. runs across chunk and tile boundaries -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    idx = synthetic.make_index(seed=81, n_docs=40_000, doclen_mean=3, doclen_std=1, K=512)
    assert idx["doclens"].min() >= 1                           # every passage is a candidate: slot i is passage i + 1
    Qs = synthetic.make_queries(idx, 82, 3)
    everything = np.arange(1, 40_001)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 2, everything, "all") for j in range(3)]


def boundary_groupings():
    """group lengths over 40 000 slots whose runs end exactly at the given slots (the entry BEFORE a boundary in `cuts` is
    the last of its run), short random runs elsewhere"""
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
    return {"run_of_5000": from_cuts([17_000, 22_000], 1),                                  # spans most of a tile
            "ends_1023_1024": from_cuts([1016, 1023, 1024, 1025, 1032], 2),                 # thread-chunk and wave edges
            "ends_tile": from_cuts([8184, 8191, 8192, 8193, 16_384, 24_577], 3),            # tile edges, a run ending ON the edge
            "ends_32768": from_cuts([32_760, 32_767, 32_768, 32_769, 39_999], 4),
            "long_runs": np.array([8192, 8192, 1, 8191, 15_424], np.int64)}                 # whole tiles, a run over two tiles


@pytest.mark.parametrize("name", list(boundary_groupings()))
def test_runs_across_chunk_and_tile_boundaries(oracle, wide, name):
    """40 000 candidates per query (a scope "all" filter over every pid): several tiles of the collapse, with runs cut at
    and around its thread, wave and tile edges; one and sixteen work-groups per query in the selection."""
    idx, Qs, rankings = wide
    lens = boundary_groupings()[name]
    assert int(lens.sum()) == 40_000
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(mask=np.ones(40_000, bool)) as f, s.make_grouping(group_lens=lens) as g:
            assert g.count == lens.size
            for wide_sel in (0, 1):
                s.set_wide_select(wide_sel)
                for mode in modes_of(s):
                    for k in (5, 1000):
                        _, _, bn = check_batch(s, g, gids, rankings, Qs, k, f"{name} wide={wide_sel} mode={mode}", filters=f,
                                               scope="all")
                        assert np.all(bn == lens.size)
    finally:
        s.close()


# ---- 4. filters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("selectivity", [0.5, 0.02])
def test_grouped_search_with_filters(oracle, medium, scope, selectivity):
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
                for k in (10, 1000):
                    check_batch(s, g, gids, rankings, Q3, k, f"{scope} sel={selectivity} mode={mode}", filters=filters, scope=scope)
                p, sc = s.search_embeddings(Q3[:, :, 0], 10, filter=filters[0], scope=scope, grouping=g)
                assert_result(p, sc, s.last_num_candidates, collapse(rankings[0], gids), 10, "single query")
                assert np.array_equal(g.groups_of(p), 2 * gids[p - 1] + 11)
        for f in filters:
            if f is not None:
                f.close()
    finally:
        s.close()


def test_a_filter_that_leaves_fewer_than_k_groups(oracle, medium):
    """The short result: (0, -Inf) padding through the Python calls (a filtered search never raises), CLB_EBOUNDS from the
    C call when the caller did not ask for padding, BoundsError from `search` where the ungrouped call raises it."""
    idx, Qs, rankings = medium
    gids = ids_from_lens(np.full(5000, 4))
    allowed = np.arange(4001, 4041)                            # ten groups
    r = filtered_ranking(oracle, idx, Qs[:, :, 0], 2, allowed, "all")
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(pids=allowed) as f, s.make_grouping(group_ids=gids) as g:
            for mode in modes_of(s):
                for scope, rank in (("all", r), ("candidates", filtered_ranking(oracle, idx, Qs[:, :, 0], 2, allowed, "candidates"))):
                    p, sc = clb.search(s, Qs[:, :, 0], 25, filter=f, scope=scope, grouping=g)
                    assert_result(p, sc, s.last_num_candidates, collapse(rank, gids), 25, f"short {scope} mode={mode}")
                    bp, bs, bn = s.search_batch(Qs, 25, filters=f, scope=scope, grouping=g, pad_short=True)
                    assert_result(bp[:, 0], bs[:, 0], bn[0], collapse(rank, gids), 25, f"short batch {scope} mode={mode}")
                assert s.last_num_candidates <= 10
                q = np.asfortranarray(Qs[:, :, :1])
                op, os_, nc = np.zeros(25, np.int64), np.zeros(25, np.float32), np.zeros(1, np.int64)
                ptr = lambda a: a.ctypes.data_as(C.c_void_p)
                rc = clb.lib().clb_search_batch_grouped(s._h, ptr(q), 32, 1, 2, 25, (C.c_void_p * 1)(f._h.value), 1, g._h, 0, ptr(op),
                                                        ptr(os_), ptr(nc))
                assert rc == clb.BoundsError.code and b"10 candidate groups" in clb.lib().clb_last_error()
                # no filter, more groups asked for than the candidates hold: the ungrouped call raises here, so does this one
                n_groups = collapse(rankings[0], gids)[0].size
                with pytest.raises(clb.BoundsError):
                    clb.search(s, Qs[:, :, 0], n_groups + 1, grouping=g)
                p, sc = clb.search(s, Qs[:, :, 0], n_groups, grouping=g)
                assert_result(p, sc, s.last_num_candidates, collapse(rankings[0], gids), n_groups, f"all groups mode={mode}")
    finally:
        s.close()


# ---- 5. sub-batches -------------------------------------------------------------------------------------------------------
def test_grouped_sub_batches(oracle, medium):
    """B = 1, 64, 65 and 70: one grouping for every sub-batch of 64 queries."""
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
                for B in (1, 64, 65, 70):
                    check_batch(s, g, gids, rankings, np.asfortranarray(Qs[:, :, :B]), 200, f"B={B} mode={mode}",
                                queries=[j for j in checked if j < B])
    finally:
        s.close()


# ---- 6. general shapes and the other code widths -----------------------------------------------------------------------------
GENERAL = [(64, 2, 20, "batched32"), (128, 8, 20, "batched32"), (136, 4, 20, "batched64"), (128, 2, 150, "loop_mfma"),
           (128, 2, 513, "scalar")]


def test_the_general_cases_take_all_four_routes():
    assert [ug.expected_route(d, nb, T) for d, nb, T, _ in GENERAL] == [r for *_, r in GENERAL]
    assert {r for *_, r in GENERAL} == set(ug.ROUTES)


@pytest.mark.parametrize("dim,nbits,T,route", GENERAL)
def test_grouped_search_general_shapes(oracle, dim, nbits, T, route):
    assert ug.expected_route(dim, nbits, T) == route
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
            for nprobe in (2, 5):
                plain = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe) for j in range(3)]
                check_batch(s, g, gids, plain, Qs, 40, f"{route} nprobe={nprobe}", nprobe=nprobe)
                for scope in ("candidates", "all"):
                    filt = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe, allowed, scope) for j in range(3)]
                    check_batch(s, g, gids, filt, Qs, 7, f"{route} {scope} nprobe={nprobe}", nprobe=nprobe, filters=f, scope=scope)
    finally:
        s.close()


@pytest.mark.parametrize("nbits", [1, 4])
def test_grouped_search_other_code_widths(oracle, nbits):
    """nbits 1 and 4 at dim 128: the tuned path in its single-pass form"""
    idx = synthetic.make_index(seed=51 + nbits, n_docs=3000, K=256, nbits=nbits)
    Qs = synthetic.make_queries(idx, 52, 9)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]
    lens = random_lens(3000, 1, 10, 9)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        with s.make_grouping(group_lens=lens) as g:
            for k in (1, 50, 600):
                check_batch(s, g, gids, rankings, Qs, k, f"nbits={nbits}")
                check_batch(s, g, gids, rankings, np.asfortranarray(Qs[:, :, :1]), k, f"nbits={nbits} B=1", queries=[0])
    finally:
        s.close()


# ---- 7. after remove and update ----------------------------------------------------------------------------------------------
def test_a_grouping_outlives_remove_and_update_but_not_an_append(oracle):
    full = synthetic.make_index(0, 330, K=64)
    idx = head_index(full, 300)
    Qs = synthetic.make_queries(idx, 1000, 9)
    lens = random_lens(300, 2, 12, 10)
    gids = ids_from_lens(lens)
    before = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]
    top = collapse(before[0], gids)
    gone_group = gids[top[0][0] - 1]                           # query 0's best group: all of its passages go ...
    removed = np.concatenate([np.nonzero(gids == gone_group)[0] + 1, [top[0][1]]])      # ... and the best passage of its second
    low = before[0][0][-1]                                     # query 0's worst candidate becomes its group's best
    assert low not in removed and gids[low - 1] not in (gone_group, gids[top[0][1] - 1])
    want, _ = reduced_index(idx, removed)
    upd = ([low], *content_of(idx, [top[0][0]]))
    want = updated_index(want, *upd)
    s = clb.Searcher(index=idx)
    try:
        g = s.make_grouping(group_ids=gids)
        assert s.remove_passages(removed) == removed.size
        assert s.update_compressed(*upd) == 1
        after = [filtered_ranking(oracle, want, Qs[:, :, j], 2) for j in range(9)]
        now = collapse(after[0], gids)
        assert gone_group not in gids[now[0] - 1] and now[0][0] == low         # the group is gone; the updated passage leads
        for mode in modes_of(s):
            for k in (1, 10, 40):
                check_batch(s, g, gids, after, Qs, k, f"after remove + update mode={mode}")
        assert s.add_compressed(*tail(full, 300)) == range(301, 331)
        with pytest.raises(clb.ArgumentError, match="grouping made before an append; make another"):
            s.search_batch(Qs, 10, grouping=g)
        g.close()
        grown = dict(want)
        co, re, dl = tail(full, 300)
        grown["codes"] = np.concatenate([want["codes"], co]); grown["residuals"] = np.asfortranarray(np.concatenate([want["residuals"], re], axis=1))
        grown["doclens"] = np.concatenate([want["doclens"], dl])
        grown["ivf"], grown["ivf_lengths"] = synthetic.build_ivf(grown["codes"], 64)
        gids2 = np.concatenate([gids, np.repeat(np.arange(gids[-1] + 1, gids[-1] + 11), 3)])
        with s.make_grouping(group_ids=gids2) as g2:
            assert g2.count == lens.size + 10
            ranks2 = [filtered_ranking(oracle, grown, Qs[:, :, j], 2) for j in range(9)]
            for mode in modes_of(s):
                check_batch(s, g2, gids2, ranks2, Qs, 10, f"after the append mode={mode}")
    finally:
        s.close()


# ---- 8. contracts on a live searcher -------------------------------------------------------------------------------------------
def test_grouping_contracts_on_a_live_searcher(oracle):
    l = clb.lib()
    i64 = C.c_int64
    idx = synthetic.make_index(seed=1, n_docs=300, K=64)
    Qs = synthetic.make_queries(idx, 2, 2)
    off = 1000
    s, other = clb.Searcher(index=idx, pid_offset=off), clb.Searcher(index=idx)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(0xdead0)
    ids = ids_from_lens([100, 150, 50])
    try:
        bad = ids.copy(); bad[200] = 0                         # the ids decrease at local passage 201
        assert l.clb_grouping_create(s._h, p(bad), i64(300), C.byref(h)) == 4 and h.value is None
        assert f"decrease at passage {off + 201} ".encode() in l.clb_last_error()
        with pytest.raises(clb.ArgumentError, match="non-decreasing"):
            s.make_grouping(group_ids=bad)
        for n in (299, 301, 0):                                # wrong length
            assert l.clb_grouping_create(s._h, p(ids), i64(n), C.byref(h)) == 4 and b"one group id per passage" in l.clb_last_error()
        with pytest.raises(clb.ArgumentError):
            s.make_grouping(group_ids=ids[:-1])
        assert l.clb_grouping_create(s._h, None, i64(300), C.byref(h)) == 4
        assert l.clb_grouping_create(s._h, p(ids), i64(300), None) == 4
        g, foreign = s.make_grouping(group_ids=ids * 7), other.make_grouping(group_ids=ids)
        assert g.count == 3 == l.clb_grouping_count(g._h)
        with pytest.raises(clb.ArgumentError, match="another searcher"):
            s.search_batch(Qs, 2, grouping=foreign)
        ranking = filtered_ranking(oracle, idx, Qs[:, :, 0], 2)
        bp, bs, bn = check_batch(s, g, ids, [ranking] * 2, np.asfortranarray(Qs[:, :, [0, 0]]), 3, "pid_offset", pid_offset=off)
        assert np.array_equal(g.groups_of(bp[:bn[0], 0]), 7 * ids[bp[:bn[0], 0] - off - 1])      # the caller's own ids
        with pytest.raises(clb.BoundsError):
            g.groups_of([off])
        g.close()
        g.close()                                              # closing twice is fine
        with pytest.raises(clb.ColBERTError, match="open PassageGrouping"):
            s.search_batch(Qs, 2, grouping=g)
        other.close()
        foreign.close()                                        # after its searcher: just frees
        up, us, un = s.search_batch(Qs, 5, pad_short=True)     # ... and the handle still searches ungrouped
        rp, rs, rn = oracle.search(idx, Qs[:, :, 0], nprobe=2, k=5)
        assert un[0] == rn and np.array_equal(up[:, 0], rp + off)
        assert_same_f32(us[:, 0], rs, "ungrouped after grouped")
    finally:
        s.close()


# ---- 9. graph capture -----------------------------------------------------------------------------------------------------
def test_captured_graph_replays_the_grouped_search(oracle):
    """The device-slot entry point captured as a HIP graph over a static query buffer, with and without per-query filters:
    every replay equals the direct call and the reference."""
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=1024)
    k = 60
    a = [random_allowed(6000, 0.5, 1), random_allowed(6000, 0.02, 2)]
    lens = random_lens(6000, 1, 15, 11)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    f = [s.make_filter(pids=x) for x in a]
    g = s.make_grouping(group_lens=lens)
    try:
        for B, scope, filtered in ((1, "candidates", False), (17, "candidates", False), (1, "candidates", True), (17, "candidates", True),
                                   (17, "all", True)):
            Qs = synthetic.make_queries(idx, 31, 2 * B)
            Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
            run = DeviceSearch(s, 32, B, k, 2)
            order = [(j % 3) if j % 3 < 2 else None for j in range(B)]
            fb = [None if o is None else f[o] for o in order] if filtered else None
            q_static = Qdev[:B].clone()
            graph = run.capture(q_static, fb, scope, g)
            for it in range(2):
                q_static.copy_(Qdev[it * B:(it + 1) * B])
                graph.replay()
                torch.cuda.synchronize()
                gp, gs, gn = run.out_p.cpu().numpy().copy(), run.out_s.cpu().numpy().copy(), run.ncand.cpu().numpy().copy()
                run(Qdev[it * B:(it + 1) * B], fb, scope, g)
                torch.cuda.synchronize()
                assert np.array_equal(gp, run.out_p.cpu().numpy()) and np.array_equal(gn, run.ncand.cpu().numpy())
                assert np.array_equal(bits(gs), bits(run.out_s.cpu().numpy()))
                for j in range(0, B, 4):
                    allowed = a[order[j]] if filtered and order[j] is not None else None
                    r = filtered_ranking(oracle, idx, Qs[:, :, it * B + j], 2, allowed, scope)
                    assert_result(gp[j], gs[j], gn[j], collapse(r, gids), k, f"graph B={B} {scope} filtered={filtered} it={it} q={j}")
            del graph
    finally:
        g.close()
        for x in f:
            x.close()
        s.close()


# ---- 10. random configurations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("COLBERT_TEST_FUZZ_SEEDS", "8"))))
def test_grouped_search_random_configurations(oracle, seed):
    """Randomly drawn shapes (corpus, centroids, nbits, passage lengths, query length, batch, k, nprobe), a random
    non-decreasing grouping and an optional filter."""
    rng = np.random.default_rng(7000 + seed)
    n_docs = int(rng.integers(40, 6000))
    K = int(2 ** rng.integers(3, 11))
    nbits = int(rng.choice([1, 2, 2, 2, 4]))
    idx = synthetic.make_index(seed=7100 + seed, n_docs=n_docs, K=K, nbits=nbits, doclen_mean=float(rng.integers(4, 120)),
                               doclen_std=float(rng.integers(0, 40)), topical=bool(rng.integers(0, 2)))
    T = int(rng.choice([1, 3, 17, 32, 32, 32, 33, 48]))
    B = int(rng.integers(1, 10))
    Qs = synthetic.make_queries(idx, 7200 + seed, B, T=T)
    k = int(min(n_docs, rng.choice([1, 10, 100, 1000, n_docs])))
    nprobe = int(min(K, rng.choice([1, 2, 2, 3, 8])))
    lens = random_lens(n_docs, 1, int(rng.choice([1, 2, 8, 50, n_docs])), 7300 + seed)
    gids = np.cumsum(np.concatenate([[int(rng.integers(-5, 5))], rng.integers(1, 4, size=lens.size - 1)]))      # the caller's ids
    gids = np.repeat(gids, lens)
    scope = str(rng.choice(["candidates", "all"]))
    allowed = None if rng.integers(0, 2) == 0 else random_allowed(n_docs, float(rng.choice([1.0, 0.5, 0.1, 0.01])), 7400 + seed)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe, allowed, scope) for j in range(B)]
    s = clb.Searcher(index=idx)
    try:
        f = None if allowed is None else s.make_filter(pids=allowed)
        with s.make_grouping(group_ids=gids) as g:
            assert g.count == lens.size
            for mode in modes_of(s):
                bp, _, bn = check_batch(s, g, gids, rankings, Qs, k, f"seed={seed} mode={mode}", nprobe=nprobe, filters=f, scope=scope)
                assert np.array_equal(g.groups_of(bp[:min(k, bn[0]), 0]), gids[bp[:min(k, bn[0]), 0] - 1])
        if f is not None:
            f.close()
    finally:
        s.close()
