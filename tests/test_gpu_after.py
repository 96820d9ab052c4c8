"""Search after a cursor on the GPU against tests/util_after: the oracle's full ranking of the query's (filtered) candidates
cut on the host behind the cursor.  Every comparison: pids equal, fp32 score bits equal, pid 0 / -Inf past the last member,
n_cand that of the full ranking.  No tolerance is involved anywhere."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import util_general as ug
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import bits, random_allowed
from tests.test_gpu_grouped_search import modes_of
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index
from tests.util_after import after_ranking, assert_page
from tests.util_filter import filtered_ranking

pytestmark = pytest.mark.gpu

N_MEDIUM = 20_000
NO_CURSOR, FINISHED = (np.inf, 0), (-np.inf, 0)


def cursor_at(ranking, rank, pid_offset=0):
    """the cursor whose page starts at `rank` (0-based) of the ranking: the member before it; rank 0: none"""
    rp, rs = ranking
    if rank <= 0:
        return NO_CURSOR
    r = min(rank, rp.size)
    return (rs[r - 1], int(rp[r - 1]) + pid_offset)


def arrays(cursors):
    return (np.array([c[0] for c in cursors], np.float32), np.array([c[1] for c in cursors], np.int64))


def check_pages(s, Qb, k, cursors, rankings, what, nprobe=2, filters=None, scope="candidates", pid_offset=0):
    """one batch call with one cursor per query against the cut rankings; returns the result"""
    bp, bs, bn = s.search_batch(Qb, k, nprobe=nprobe, filters=filters, scope=scope, after=arrays(cursors))
    for j, cur in enumerate(cursors):
        assert_page(bp[:, j], bs[:, j], bn[j], rankings[j], cur, k, f"{what} k={k} q={j}", pid_offset)
    return bp, bs, bn


def page_to_the_end(s, Qb, k, rankings, what, nprobe=2, filters=None, scope="candidates", pid_offset=0, max_pages=10 ** 6):
    """pages of k from no cursor until every query's page is padding alone (or max_pages); returns the concatenated pids per
    query and the number of calls"""
    B = Qb.shape[2]
    cursors, seen, calls = [NO_CURSOR] * B, [[] for _ in range(B)], 0
    while calls < max_pages:
        bp, bs, _ = check_pages(s, Qb, k, cursors, rankings, f"{what} page {calls}", nprobe, filters, scope, pid_offset)
        calls += 1
        for j in range(B):
            seen[j] += bp[bp[:, j] != 0, j].tolist()
        if not bp.any():
            break
        cs, cp = clb.next_cursor(bp, bs)
        cursors = list(zip(cs, cp.tolist()))
    return seen, calls


@pytest.fixture(scope="module")
def medium(oracle):
    idx = synthetic.make_index(seed=3, n_docs=N_MEDIUM, K=2048)
    Qs = synthetic.make_queries(idx, 4, 9)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]


@pytest.fixture(scope="module")
def medium_searcher(medium):
    s = clb.Searcher(index=medium[0])
    yield s
    s.close()


# ---- 1. paging to the end -----------------------------------------------------------------------------------------------------
def test_paging_to_the_end_of_a_tiny_index(oracle):
    """300 passages, pages of 7 until the empty page: the concatenation is the full ranking.  Covers fewer than k sure
    candidates, the short last page and the empty page."""
    idx = synthetic.make_index(seed=21, n_docs=300, K=16)
    Qs = synthetic.make_queries(idx, 22, 3)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)]
    sizes = [r[0].size for r in rankings]
    assert all(100 <= n <= 300 for n in sizes), sizes
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            seen, calls = page_to_the_end(s, Qs, 7, rankings, f"tiny mode={mode}")
            for j in range(3):
                assert seen[j] == rankings[j][0].tolist(), (mode, j)
            assert calls == max(-(-n // 7) + 1 for n in sizes)         # ceil(n / 7) pages and the empty one
            for j in range(3):                                          # ... per query, one at a time
                Q1 = np.asfortranarray(Qs[:, :, j:j + 1])
                _, c1 = page_to_the_end(s, Q1, 7, rankings[j:j + 1], f"tiny mode={mode} q={j} alone")
                assert c1 == -(-sizes[j] // 7) + 1
    finally:
        s.close()


# ---- 2. parity ----------------------------------------------------------------------------------------------------------------
def medium_cursors(rankings):
    ns = [r[0].size for r in rankings]
    ranks = [0, 1, 10, 999, 1000, 5000, ns[6] - 3, ns[7]]
    return [cursor_at(rankings[j], ranks[j]) for j in range(8)] + [FINISHED]


def test_after_parity(oracle, medium, medium_searcher):
    """20 000 passages, one batch with the cursors at ranks 0 (+Inf), 1, 10, 999, 1000, 5000, n - 3, n and -Inf; k = 1, 10,
    100, 1000; exact and two-pass, either gather form, one and sixteen work-groups per query in the selection."""
    idx, Qs, rankings = medium
    s = medium_searcher
    assert rankings[5][0].size > 5000
    cursors = medium_cursors(rankings)
    auto_form = s.pass1_gather[0]
    for mode in modes_of(s):
        for form in ((-1, 1 - auto_form) if mode == 1 else (-1,)):
            s.set_pass1_gather(form)
            for wide in ((0, 1) if mode == 1 else (-1,)):
                s.set_wide_select(wide)
                for k in (1, 10, 100, 1000):
                    bp, bs, bn = check_pages(s, Qs, k, cursors, rankings, f"mode={mode} form={form} wide={wide}")
                    up, us, un = s.search_batch(Qs, k, pad_short=True)           # no cursor: the plain call, bit for bit
                    assert np.array_equal(bp[:, 0], up[:, 0]) and np.array_equal(bits(bs[:, 0]), bits(us[:, 0]))
                    assert np.array_equal(bn, un)
                    assert not bp[:, 8].any() and not bp[:, 7].any()             # -Inf and one past the end: empty pages
        s.set_pass1_gather(-1)
        s.set_wide_select(-1)
    assert s.mode == 1
    # every query without a cursor: the plain call for the whole batch
    bp, bs, bn = s.search_batch(Qs, 100, after=(np.full(9, np.inf, np.float32), np.zeros(9, np.int64)))
    up, us, un = s.search_batch(Qs, 100, pad_short=True)
    assert np.array_equal(bp, up) and np.array_equal(bits(bs), bits(us)) and np.array_equal(bn, un)
    with pytest.raises(clb.ArgumentError, match="NaN"):
        s.search_batch(Qs, 10, after=(np.full(9, np.nan, np.float32), np.zeros(9, np.int64)))
    # a short page never raises, with or without a cursor in the call
    n0 = rankings[0][0].size
    got = s.search_embeddings(Qs[:, :, 0], n0 + 5, after=NO_CURSOR)
    assert_page(got[0], got[1], s.last_num_candidates, rankings[0], NO_CURSOR, n0 + 5, "short, no cursor")


# ---- 3. cursors that are not results ------------------------------------------------------------------------------------------
def test_cursors_that_are_not_results(oracle, medium, medium_searcher):
    idx, Qs, rankings = medium
    s = medium_searcher
    rp, rs = rankings[0]
    assert rs[500] > rs[501] and rs[299] > rs[300] > rs[301]
    member_s, member_p = rs[300], int(rp[300])
    cursors = [(np.float32(0.5 * (float(rs[500]) + float(rs[501]))), 0), (member_s, 0), (member_s, member_p - 1),
               (member_s, 2 ** 62), (np.nextafter(member_s, np.float32(np.inf)), 0), (np.nextafter(member_s, np.float32(-np.inf)), 0),
               (member_s, member_p)]
    starts = [501, 300, 300, 301, 300, 301, 301]                # the rank each page starts at, from the oracle's ranking
    for cur, st in zip(cursors, starts):
        assert after_ranking(rankings[0], *cur)[0][0] == rp[st], (cur, st)
    Qb = np.asfortranarray(np.repeat(Qs[:, :, :1], len(cursors), axis=2))
    for mode in modes_of(s):
        for k in (10, 1000):
            check_pages(s, Qb, k, cursors, [rankings[0]] * len(cursors), f"not results mode={mode}")
        got = s.search_embeddings(Qs[:, :, 0], 10, after=cursors[0])
        assert_page(got[0], got[1], s.last_num_candidates, rankings[0], cursors[0], 10, f"single query mode={mode}")
        got = clb.search(s, Qs[:, :, 0], 10, after=cursors[3])
        assert_page(got[0], got[1], s.last_num_candidates, rankings[0], cursors[3], 10, f"module search mode={mode}")


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------
def index_with_copies(idx, pids, copies):
    """`idx` with the passages `pids` (1-based) appended `copies` more times each, the IVF rebuilt from the codes"""
    off = np.concatenate([[0], np.cumsum(idx["doclens"])])
    rows = np.concatenate([np.arange(off[p - 1], off[p]) for _ in range(copies) for p in pids])
    out = dict(idx)
    out["codes"] = np.concatenate([idx["codes"], idx["codes"][rows]])
    out["residuals"] = np.asfortranarray(np.concatenate([idx["residuals"], idx["residuals"][:, rows]], axis=1))
    out["doclens"] = np.concatenate([idx["doclens"], np.tile(idx["doclens"][np.asarray(pids) - 1], copies)])
    out["ivf"], out["ivf_lengths"] = synthetic.build_ivf(out["codes"], idx["ivf_lengths"].size)
    return out


def test_pages_cross_runs_of_exactly_tied_scores(oracle):
    base = synthetic.make_index(seed=31, n_docs=400, K=16)
    Qs = synthetic.make_queries(base, 32, 3)
    first = filtered_ranking(oracle, base, Qs[:, :, 0], 2)
    idx = index_with_copies(base, np.sort(first[0][:50]), 3)     # query 0's 50 best passages, four times each
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)]
    runs = []
    for rp, rs in rankings:                                      # the precondition, from the oracle alone
        starts = [i for i in range(rs.size - 3) if rs[i] == rs[i + 3] and (i == 0 or rs[i - 1] != rs[i])]
        assert len(starts) >= 20, len(starts)
        assert all(np.all(np.diff(rp[i:i + 4]) > 0) for i in starts)             # ties rank by ascending pid
        runs.append(starts)
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            seen, _ = page_to_the_end(s, Qs, 3, rankings, f"ties mode={mode}", max_pages=40)      # 3 never divides a run of 4
            for j in range(3):
                assert seen[j] == rankings[j][0][:len(seen[j])].tolist() and len(seen[j]) >= 117
            for i in runs[0][:6]:                                # the cursor at every position of a run, and on both sides of it
                rp, rs = rankings[0]
                cursors = [(rs[i], 0), (rs[i], 2 ** 40)] + [(rs[i + m], int(rp[i + m])) for m in range(4)]
                Qb = np.asfortranarray(np.repeat(Qs[:, :, :1], len(cursors), axis=2))
                check_pages(s, Qb, 3, cursors, [rankings[0]] * len(cursors), f"inside a run mode={mode}")
    finally:
        s.close()


# ---- 5. filters ---------------------------------------------------------------------------------------------------------------
def test_after_with_filters(oracle, medium, medium_searcher):
    idx, Qs, plain = medium
    s = medium_searcher
    Q3 = np.asfortranarray(Qs[:, :, :3])
    ten = random_allowed(N_MEDIUM, 0.10, 300)
    two_k = np.sort(np.random.default_rng(301).choice(N_MEDIUM, 2000, replace=False) + 1)
    with s.make_filter(pids=ten) as f10, s.make_filter(pids=two_k) as f2k, s.make_filter(pids=np.arange(1, N_MEDIUM + 1)) as fall:
        for scope, f, allowed in (("candidates", f10, ten), ("all", f2k, two_k)):
            ranks = [filtered_ranking(oracle, idx, Q3[:, :, j], 2, allowed, scope) for j in range(3)]
            cursors = [cursor_at(ranks[0], 0), cursor_at(ranks[1], 50), cursor_at(ranks[2], ranks[2][0].size)]
            for mode in modes_of(s):
                for k in (10, 1000):
                    check_pages(s, Q3, k, cursors, ranks, f"filter {scope} mode={mode}", filters=f, scope=scope)
        # per-query filters with None entries, per-query cursors
        mixed = [filtered_ranking(oracle, idx, Q3[:, :, 0], 2, ten), plain[1], filtered_ranking(oracle, idx, Q3[:, :, 2], 2, ten)]
        cursors = [cursor_at(mixed[0], 50), cursor_at(mixed[1], 1000), NO_CURSOR]
        for mode in modes_of(s):
            check_pages(s, Q3, 100, cursors, mixed, f"mixed filters mode={mode}", filters=[f10, None, f10])
        # every passage as the candidate set, k above the one-work-group top-k: the full-sort route
        everything = filtered_ranking(oracle, idx, Q3[:, :, 0], 2, np.arange(1, N_MEDIUM + 1), "all")
        assert everything[0].size == N_MEDIUM
        Q1 = np.asfortranarray(Q3[:, :, :1])
        for mode in modes_of(s):
            check_pages(s, Q1, 16_400, [cursor_at(everything, 1000)], [everything], f"full sort mode={mode}", filters=fall,
                        scope="all")
            check_pages(s, Q1, 16_400, [cursor_at(everything, 10_000)], [everything], f"full sort, short mode={mode}", filters=fall,
                        scope="all")


# ---- 6. the cut moved and pruned ----------------------------------------------------------------------------------------------
def test_the_cut_moves_with_the_cursor_and_prunes(oracle, medium, medium_searcher):
    """Two-pass mode, one query: a deep page re-scores about a page's worth of passages, none of them certainly before the
    cursor.  An implementation that keeps the old cut and filters afterwards returns deep pages short."""
    idx, Qs, rankings = medium
    s = medium_searcher
    rp, rs = rankings[0]
    n = rp.size
    assert n > 6000
    Q1 = np.asfortranarray(Qs[:, :, :1])
    s.set_mode(1)
    assert s.mode == 1
    dbg = s.debug_scores(Qs[:, :, 0], 100)
    approx, eps = dbg["approx"], np.float32(dbg["eps"])
    assert approx.size == n and np.isfinite(eps)

    def rescored(rank, k):
        cur = cursor_at(rankings[0], rank)
        s.profile_enable(True, counters=True)
        check_pages(s, Q1, k, [cur], rankings[:1], f"cut at rank {rank}")
        st = s.last_batch_stats()
        s.profile_enable(False)
        not_passed = int(np.count_nonzero(approx <= np.float32(cur[0]) + np.float32(2) * eps))
        print(f"cursor at rank {rank}, k={k}: re-scored {st['rescored_docs']} of {st['cand_docs']} candidates; "
              f"{not_passed} have approx <= s* + 2 eps")
        return st, not_passed

    st, _ = rescored(1000, 100)
    assert st["cand_docs"] == n and 100 <= st["rescored_docs"] < st["cand_docs"]
    st, not_passed = rescored(5000, 100)
    assert not_passed < st["cand_docs"] - 1000                 # the precondition, from debug_scores alone
    assert 100 <= st["rescored_docs"] <= not_passed            # passed candidates are not re-scored
    st, not_passed = rescored(n - 3, 100)                      # fewer than k sure: still nothing passed is re-scored
    assert not_passed < st["cand_docs"] - 1000
    assert 3 <= st["rescored_docs"] <= not_passed


# ---- 7. general shapes --------------------------------------------------------------------------------------------------------
def three_pages(s, Qs, k, rankings, what, nprobe=2):
    seen, calls = page_to_the_end(s, Qs, k, rankings, what, nprobe=nprobe, max_pages=3)
    assert calls == 3
    for j in range(Qs.shape[2]):
        assert seen[j] == rankings[j][0][:3 * k].tolist(), (what, j)


def test_after_on_other_shapes(oracle):
    # nbits = 4 on the tuned exact path
    idx = synthetic.make_index(seed=41, n_docs=2000, K=256, nbits=4)
    Qs = synthetic.make_queries(idx, 42, 3)
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            three_pages(s, Qs, 25, [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)], f"nbits 4 mode={mode}")
    finally:
        s.close()
    # T = 40 on the tuned path: no two-pass, whatever the mode
    idx = synthetic.make_index(seed=23, n_docs=3000, K=256)
    Qs = synthetic.make_queries(idx, 24, 3, T=40)
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            three_pages(s, Qs, 25, [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)], f"T=40 mode={mode}")
    finally:
        s.close()


@pytest.mark.parametrize("case,route", [(9, "loop_mfma"), (8, "batched32")])
def test_after_on_the_general_path(oracle, case, route):
    assert ug.CASES[case][4] == route
    idx, Qs, nprobe = ug.case_inputs(case)
    Qs = np.asfortranarray(Qs)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe) for j in range(3)]
    s = clb.Searcher(index=idx)
    try:
        three_pages(s, Qs, 11, rankings, route, nprobe=nprobe)
        cursors = [cursor_at(rankings[0], rankings[0][0].size - 2), FINISHED, NO_CURSOR]
        check_pages(s, Qs, ug.CASE_K, cursors, rankings, f"{route} ends", nprobe=nprobe)
    finally:
        s.close()


# ---- 8. device route and graph ------------------------------------------------------------------------------------------------
def test_device_route_and_paging_under_a_captured_graph(oracle):
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    full = synthetic.make_index(seed=23, n_docs=6030, K=256)
    idx = head_index(full, 6000)
    k, B = 10, 4
    Qs = synthetic.make_queries(idx, 31, B)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(B)]
    Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
    s = clb.Searcher(index=idx)
    try:
        for mode in modes_of(s):
            run = DeviceSearch(s, 32, B, k, 2)
            cursors = [cursor_at(rankings[j], r) for j, r in enumerate((0, 5, 700, rankings[3][0].size - 4))]
            cs, cp = arrays(cursors)
            d_s, d_p = torch.from_numpy(cs).cuda(), torch.from_numpy(cp).cuda()
            run(Qdev, after=(d_s, d_p))                        # eager
            torch.cuda.synchronize()
            gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
            hp, hs, hn = s.search_batch(Qs, k, after=(cs, cp))                     # the host route
            assert np.array_equal(gp.T, hp) and np.array_equal(bits(gs.T), bits(hs)) and np.array_equal(gn, hn)
            for j in range(B):
                assert_page(gp[j], gs[j], gn[j], rankings[j], cursors[j], k, f"eager mode={mode} q={j}")
            d_s.fill_(float("nan"))                            # nothing can be raised here: empty pages
            run(Qdev, after=(d_s, d_p))
            torch.cuda.synchronize()
            assert not run.out_p.cpu().numpy().any() and np.all(np.isneginf(run.out_s.cpu().numpy()))
            # capture once, then page by copying the last output row into the cursor tensors
            d_s.fill_(float("inf")); d_p.zero_()
            graph = run.capture(Qdev, after=(d_s, d_p))
            cursors = [NO_CURSOR] * B
            for page in range(5):
                graph.replay()
                torch.cuda.synchronize()
                gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
                for j in range(B):
                    assert_page(gp[j], gs[j], gn[j], rankings[j], cursors[j], k, f"graph mode={mode} page={page} q={j}")
                    assert np.array_equal(gp[j], rankings[j][0][page * k:(page + 1) * k])
                d_s.copy_(run.out_s[:, k - 1]); d_p.copy_(run.out_p[:, k - 1])
                cursors = list(zip(gs[:, k - 1], gp[:, k - 1].tolist()))
            for bad in ((d_s.double(), d_p), (d_s, d_p.int()), (d_s.cpu(), d_p), (d_s, d_p.cpu()), (d_s[:2], d_p), (d_s,)):
                with pytest.raises(clb.ArgumentError, match="after must be a pair"):
                    run(Qdev, after=bad)
            with pytest.raises(clb.Unsupported, match="after together with grouping"):
                with s.make_grouping(group_lens=[s.num_docs]) as g:
                    run(Qdev, grouping=g, after=(d_s, d_p))
        # after an append the graph is stale and replay captures again
        s.set_mode(0)
        run = DeviceSearch(s, 32, B, k, 2)
        d_s, d_p = torch.full((B,), float("inf"), device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
        graph = run.capture(Qdev, after=(d_s, d_p))
        assert not run.graph_is_stale()
        assert s.add_compressed(*tail(full, 6000)) == range(6001, 6031)
        assert run.graph_is_stale()
        grown = [filtered_ranking(oracle, full, Qs[:, :, j], 2) for j in range(B)]
        cursors = [cursor_at(grown[j], 20) for j in range(B)]
        cs, cp = arrays(cursors)
        d_s.copy_(torch.from_numpy(cs)); d_p.copy_(torch.from_numpy(cp))
        graph = run.replay(graph, Qdev, after=(d_s, d_p))
        torch.cuda.synchronize()
        assert not run.graph_is_stale()
        gp, gs, gn = run.out_p.cpu().numpy(), run.out_s.cpu().numpy(), run.ncand.cpu().numpy()
        for j in range(B):
            assert_page(gp[j], gs[j], gn[j], grown[j], cursors[j], k, f"after the append q={j}")
        del graph
    finally:
        s.close()


# ---- 9. index changes ---------------------------------------------------------------------------------------------------------
def test_after_on_a_changed_index_and_with_a_pid_offset(oracle):
    idx = synthetic.make_index(0, 600, K=256)
    Qs = synthetic.make_queries(idx, 1000, 3)
    before = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)]
    removed = before[0][0][[0, 7, 8]]
    low = int(before[0][0][-1])                                # query 0's worst passage gets the content of its best
    want, _ = reduced_index(idx, removed)
    upd = ([low], *content_of(idx, [int(before[0][0][1])]))
    want = updated_index(want, *upd)
    s = clb.Searcher(index=idx)
    try:
        assert s.remove_passages(removed) == 3
        assert s.update_compressed(*upd) == 1
        after = [filtered_ranking(oracle, want, Qs[:, :, j], 2) for j in range(3)]
        assert not np.array_equal(after[0][0][:10], before[0][0][:10])
        for mode in modes_of(s):
            three_pages(s, Qs, 7, after, f"changed index mode={mode}")
            check_pages(s, Qs, 20, [cursor_at(after[j], after[j][0].size - 5) for j in range(3)], after, f"changed, last page mode={mode}")
    finally:
        s.close()
    # a shard of a larger collection: cursors hold GLOBAL pids
    sh = synthetic.make_index(seed=2024, n_docs=4000, K=256, n_blocks=8, blocks=range(4, 6))
    off = int(sh["pid_offset"])
    assert off == 2000
    Qs = synthetic.make_queries(sh, 5, 3)
    rankings = [filtered_ranking(oracle, sh, Qs[:, :, j], 2) for j in range(3)]
    s = clb.Searcher(index=sh, pid_offset=off)
    try:
        for mode in modes_of(s):
            seen, _ = page_to_the_end(s, Qs, 9, rankings, f"pid_offset mode={mode}", pid_offset=off, max_pages=4)
            for j in range(3):
                assert seen[j] == (rankings[j][0][:36] + off).tolist()
            rp, rs = rankings[0]
            cursors = [(rs[40], 0), (rs[40], int(rp[40]) + off), (rs[40], int(rp[40]))]      # the last one is a LOCAL pid: before the member
            Qb = np.asfortranarray(np.repeat(Qs[:, :, :1], 3, axis=2))
            bp, _, _ = check_pages(s, Qb, 9, cursors, [rankings[0]] * 3, f"global pids mode={mode}", pid_offset=off)
            assert bp[0, 0] == rp[40] + off and bp[0, 1] == rp[41] + off and bp[0, 2] == rp[40] + off
    finally:
        s.close()
