"""Search with a score prior on the GPU against tests/util_prior: the oracle's full ranking of the query's (filtered)
candidates re-ranked by E = fl32(e + fl32(weight * value)), the lower pid first among equal E, and collapsed for grouped calls.
Every comparison: pids equal, fp32 score bits equal, n_cand equal, short results padded with pid 0 / -Inf."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import util_general as ug
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import assert_result, bits, random_allowed
from tests.test_gpu_grouped_search import modes_of
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index
from tests.util_filter import filtered_ranking
from tests.util_group import collapse, ids_from_lens, random_lens
from tests.util_prior import boosted_ranking

pytestmark = pytest.mark.gpu

N_MEDIUM = 20_000


def check_batch(s, p, values, rankings, Qb, k, what, weight=1.0, nprobe=2, filters=None, scope="candidates", grouping=None,
                gids=None, pid_offset=0, queries=None):
    """one batch call with prior `p` (host values `values`) against the boosted `rankings` (the full unboosted (filtered)
    rankings of Qb's queries), collapsed by `gids` for a grouped call"""
    bp, bs, bn = s.search_batch(Qb, k, nprobe=nprobe, pad_short=True, filters=filters, scope=scope, grouping=grouping, prior=p,
                                prior_weight=weight)
    for j in (range(Qb.shape[2]) if queries is None else queries):
        want = boosted_ranking(rankings[j], values, weight)
        if gids is not None:
            want = collapse(want, gids)
        assert_result(bp[:, j], bs[:, j], bn[j], want, k, f"{what} k={k} w={weight} q={j}", pid_offset)
    return bp, bs, bn


@pytest.fixture(scope="module")
def medium(oracle):
    idx = synthetic.make_index(seed=3, n_docs=N_MEDIUM, K=2048)
    Qs = synthetic.make_queries(idx, 4, 9)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]


def medium_prior(name):
    rng = np.random.default_rng(18)
    return {"zeros": np.zeros(N_MEDIUM, np.float32),
            "normal": rng.normal(0.0, 0.5, N_MEDIUM).astype(np.float32),
            "recency": np.linspace(0.0, 2.0, N_MEDIUM).astype(np.float32),              # monotone over the pids
            "negative": (-0.1 - rng.random(N_MEDIUM)).astype(np.float32),
            "two_to_16": (2.0 ** 16 * rng.integers(0, 32, N_MEDIUM)).astype(np.float32)}[name]


# ---- 1. parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeros", "normal", "recency", "negative", "two_to_16"])
def test_prior_parity(oracle, medium, name):
    """20 000 passages, B = 9, k = 1, 10, 100, 1000; exact and two-pass, either gather form, one and sixteen work-groups per
    query in the selection."""
    idx, Qs, rankings = medium
    values = medium_prior(name)
    if name == "normal":                                       # the precondition, from the oracle alone: the prior re-ranks
        for k in (10, 100, 1000):
            for r in rankings:
                assert not np.array_equal(np.sort(r[0][:k]), np.sort(boosted_ranking(r, values)[0][:k]))
    s = clb.Searcher(index=idx)
    try:
        with s.make_prior(values) as p:
            assert len(p) == N_MEDIUM and p.max_abs == float(np.abs(values).max()) == clb.lib().clb_prior_max_abs(p._h)
            auto_form = s.pass1_gather[0]
            for mode in modes_of(s):
                for form in ((-1, 1 - auto_form) if mode == 1 else (-1,)):
                    s.set_pass1_gather(form)
                    for wide in ((0, 1) if mode == 1 else (-1,)):
                        s.set_wide_select(wide)
                        for k in (1, 10, 100, 1000):
                            bp, bs, bn = check_batch(s, p, values, rankings, Qs, k, f"{name} mode={mode} form={form} wide={wide}")
                            if name == "zeros":                # ... which is the search without a prior, bit for bit
                                up, us, un = s.search_batch(Qs, k, pad_short=True)
                                assert np.array_equal(bp, up) and np.array_equal(bn, un) and np.array_equal(bits(bs), bits(us))
                s.set_pass1_gather(-1)
                s.set_wide_select(-1)
            assert s.mode == 1
            if name == "two_to_16":
                eps = max(s.debug_scores(Qs[:, :, j], 10)["eps"] for j in range(9))
                top = [boosted_ranking(r, values)[1] for r in rankings]
                print(f"two_to_16: eps {eps}, ulp(M) {np.spacing(np.float32(p.max_abs))}")
                assert np.spacing(np.float32(top[0][0])) > eps                     # ulp(M) above eps ...
                for k in (100, 1000):                                              # ... and exact ties across the k-th place
                    assert sum(1 for t in top if t[k - 1] == t[k]) >= 5
            else:                                              # small priors: the cut really pruned
                s.profile_enable(True, counters=True)
                s.search_batch(Qs, 100, pad_short=True, prior=p)
                st = s.last_batch_stats()
                s.profile_enable(False)
                print(f"{name}: re-scored {st['rescored_docs']} of {st['cand_docs']} candidates (9 queries, k = 100)")
                assert 9 * 100 <= st["rescored_docs"] < st["cand_docs"]
    finally:
        s.close()


# ---- 2. the cut moves ---------------------------------------------------------------------------------------------------------
def test_the_cut_moves_with_the_prior(oracle, medium):
    """A passage at unboosted rank >= 5000 receives just enough to land inside the top 10, the unboosted rank-1 passage is
    pushed out of the top 100: re-sorting the plain top 1000 on the host cannot give this answer."""
    idx, Qs, rankings = medium
    rp, rs = rankings[0]
    assert rp.size > 6000
    low, first = int(rp[5500]), int(rp[0])
    values = np.zeros(N_MEDIUM, np.float32)
    values[low - 1] = np.float32(rs[4] - rs[5500]) + np.float32(0.25)           # above the unboosted rank 5
    values[first - 1] = -(np.float32(rs[0] - rs[150]) + np.float32(0.25))       # below the unboosted rank 151
    want = boosted_ranking(rankings[0], values)
    assert low in want[0][:10] and first not in want[0][:100]
    # the reason for this test, from the oracle alone: the host re-sort of the plain top 1000 misses the lifted passage
    resorted = boosted_ranking((rp[:1000], rs[:1000]), values)
    assert low not in rp[:1000] and not np.array_equal(resorted[0][:10], want[0][:10])
    s = clb.Searcher(index=idx)
    try:
        with s.make_prior(values) as p:
            for mode in modes_of(s):
                for k in (10, 100, 1000):
                    bp, _, _ = check_batch(s, p, values, rankings, Qs, k, f"cut moves mode={mode}")
                    assert low in bp[:10, 0] and first not in bp[:min(k, 100), 0]
                got = s.search_embeddings(Qs[:, :, 0], 10, prior=p)
                assert_result(got[0], got[1], s.last_num_candidates, want, 10, f"single query mode={mode}")
    finally:
        s.close()


# ---- 3. weights -------------------------------------------------------------------------------------------------------------
def test_prior_weights_on_one_handle(oracle, medium):
    idx, Qs, rankings = medium
    values = medium_prior("normal")
    assert np.float32(1e-40) > 0 and (np.float32(1e-40) * values != 0).any()       # the products are denormal, not zero
    s = clb.Searcher(index=idx)
    try:
        with s.make_prior(values) as p:
            for mode in modes_of(s):
                for weight in (0.0, 0.25, -1.0, 3.0, 1e-40):
                    for k in (10, 1000):
                        check_batch(s, p, values, rankings, Qs, k, f"weights mode={mode}", weight=weight)
            with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
                s.search_batch(Qs, 10, prior=p, prior_weight=3e38)
            l, ptr = clb.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
            q = np.asfortranarray(Qs[:, :, :1])
            op, os_, nc = np.zeros(5, np.int64), np.zeros(5, np.float32), np.zeros(1, np.int64)
            assert l.clb_search_batch_prior(s._h, ptr(q), 32, 1, 2, 5, None, 0, None, p._h, 3e38, 1, ptr(op), ptr(os_), ptr(nc)) == 4
            assert b"not below FLT_MAX" in l.clb_last_error()
            assert l.clb_search_batch_prior(s._h, ptr(q), 32, 1, 2, 5, None, 0, None, p._h, float("nan"), 1, ptr(op), ptr(os_),
                                            ptr(nc)) == 4
            assert b"prior_weight must be finite" in l.clb_last_error()
    finally:
        s.close()


# ---- 4. composition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["candidates", "all"])
def test_prior_with_filters_and_groupings(oracle, medium, scope):
    idx, Qs, plain = medium
    Q3 = np.asfortranarray(Qs[:, :, :3])
    values = medium_prior("normal")
    alloweds = [random_allowed(N_MEDIUM, 0.5, 300), random_allowed(N_MEDIUM, 0.02, 301), None]
    filtered = [filtered_ranking(oracle, idx, Q3[:, :, j], 2, alloweds[j], scope) for j in range(3)]
    groupings = {"lens4": np.full(N_MEDIUM // 4, 4), "random_1_40": random_lens(N_MEDIUM, 1, 40, 5)}
    s = clb.Searcher(index=idx)
    try:
        filters = [None if a is None else s.make_filter(pids=a) for a in alloweds]
        with s.make_prior(values) as p:
            for mode in modes_of(s):
                for k in (10, 1000):
                    check_batch(s, p, values, filtered, Q3, k, f"filter {scope} mode={mode}", filters=filters, scope=scope)
                    for name, lens in groupings.items():
                        gids = ids_from_lens(lens)
                        with s.make_grouping(group_lens=lens) as g:
                            if scope == "candidates":
                                check_batch(s, p, values, plain, Q3, k, f"{name} mode={mode}", grouping=g, gids=gids)
                            check_batch(s, p, values, filtered, Q3, k, f"filter {scope} + {name} mode={mode}", weight=1.5,
                                        filters=filters, scope=scope, grouping=g, gids=gids)
        for f in filters:
            if f is not None:
                f.close()
    finally:
        s.close()


def test_prior_short_results_and_pid_offset(oracle):
    """a pid_offset handle; a filter that leaves fewer than k passages is padded, an unfiltered short result raises with the
    wording of the call without a prior"""
    idx = synthetic.make_index(seed=1, n_docs=600, K=256)
    Qs = synthetic.make_queries(idx, 2, 3)
    off = 1000
    values = np.random.default_rng(3).normal(0, 0.5, 600).astype(np.float32)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)]
    allowed = np.arange(101, 141)
    short = [filtered_ranking(oracle, idx, Qs[:, :, j], 2, allowed, "all") for j in range(3)]
    s = clb.Searcher(index=idx, pid_offset=off)
    try:
        with s.make_prior(values) as p, s.make_filter(pids=allowed + off) as f:
            for mode in modes_of(s):
                check_batch(s, p, values, rankings, Qs, 20, f"pid_offset mode={mode}", pid_offset=off)
                bp, bs, bn = check_batch(s, p, values, short, Qs, 60, f"short mode={mode}", filters=f, scope="all", pid_offset=off)
                assert np.all(bn == 40) and np.all(bp[40:] == 0) and np.all(np.isneginf(bs[40:]))
                n = rankings[0][0].size
                with pytest.raises(clb.BoundsError) as with_prior:
                    s.search_embeddings(Qs[:, :, 0], n + 1, prior=p)
                with pytest.raises(clb.BoundsError) as without:
                    s.search_batch(np.asfortranarray(Qs[:, :, :1]), n + 1)
                assert str(with_prior.value) == str(without.value) and f"{n} candidate passages" in str(without.value)
                got = s.search_embeddings(Qs[:, :, 0], n, prior=p)
                assert_result(got[0], got[1], s.last_num_candidates, boosted_ranking(rankings[0], values), n, "all candidates", off)
            with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
                with s.make_grouping(group_lens=[600]) as g:
                    s.search_batch(Qs, 5, grouping=g, per_group=2, prior=p)
    finally:
        s.close()


# ---- 5. lifetimes -------------------------------------------------------------------------------------------------------------
def test_a_prior_outlives_remove_and_update_but_not_an_append(oracle):
    import torch
    full = synthetic.make_index(0, 630, K=256)
    idx = head_index(full, 600)
    Qs = synthetic.make_queries(idx, 1000, 9)
    values = np.random.default_rng(8).normal(0, 0.5, 600).astype(np.float32)
    before = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(9)]
    top = boosted_ranking(before[0], values)[0]
    removed = top[:3]
    low = int(top[-1])                                         # query 0's worst passage gets the content of its best
    want, _ = reduced_index(idx, removed)
    upd = ([low], *content_of(idx, [int(top[0])]))
    want = updated_index(want, *upd)
    s, other = clb.Searcher(index=idx), clb.Searcher(index=idx)
    try:
        p = s.make_prior(values)
        pt = s.make_prior(torch.from_numpy(values).cuda())     # from a device tensor: the same prior
        assert pt.max_abs == p.max_abs and len(pt) == 600
        for bad_value in (np.nan, -np.inf):
            v = values.copy(); v[41] = bad_value
            for arg in (v, torch.from_numpy(v).cuda()):
                with pytest.raises(clb.ArgumentError, match="passage 42 is not a finite number"):
                    s.make_prior(arg)
        with pytest.raises(clb.ArgumentError, match="one value per passage"):
            s.make_prior(torch.zeros(599, device="cuda"))
        h = C.c_void_p(0xdead0)
        assert clb.lib().clb_prior_create(s._h, values.ctypes.data_as(C.c_void_p), C.c_int64(599), C.byref(h)) == 4 and h.value is None
        assert b"one value per passage" in clb.lib().clb_last_error()
        foreign = other.make_prior(values)
        with pytest.raises(clb.ArgumentError, match="another searcher"):
            s.search_batch(Qs, 5, prior=foreign)
        other.close()
        foreign.close()                                        # after its searcher: just frees
        for mode in modes_of(s):
            a = check_batch(s, p, values, before, Qs, 40, f"numpy mode={mode}", weight=0.5)
            b = check_batch(s, pt, values, before, Qs, 40, f"tensor mode={mode}", weight=0.5)
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
        pt.close()
        assert s.remove_passages(removed) == 3
        assert s.update_compressed(*upd) == 1
        after = [filtered_ranking(oracle, want, Qs[:, :, j], 2) for j in range(9)]
        fresh = clb.Searcher(index=want)
        try:
            with fresh.make_prior(values) as pf:
                for mode in modes_of(s):
                    fresh.set_mode(mode)
                    for k in (1, 10, 40):
                        got = check_batch(s, p, values, after, Qs, k, f"after remove + update mode={mode}")
                        ref = fresh.search_batch(Qs, k, pad_short=True, prior=pf)
                        assert all(np.array_equal(x, y) for x, y in zip(got, ref))
        finally:
            fresh.close()
        assert s.add_compressed(*tail(full, 600)) == range(601, 631)
        with pytest.raises(clb.ArgumentError, match="prior made before an append; make another"):
            s.search_batch(Qs, 10, prior=p)
        p.close()
        p.close()                                              # closing twice is fine
        with pytest.raises(clb.ColBERTError, match="open PassagePrior"):
            s.search_batch(Qs, 10, prior=p)
        grown = dict(want)
        co, re, dl = tail(full, 600)
        grown["codes"] = np.concatenate([want["codes"], co]); grown["residuals"] = np.asfortranarray(np.concatenate([want["residuals"], re], axis=1))
        grown["doclens"] = np.concatenate([want["doclens"], dl])
        grown["ivf"], grown["ivf_lengths"] = synthetic.build_ivf(grown["codes"], 256)
        values2 = np.concatenate([values, np.full(30, 1.5, np.float32)])
        with s.make_prior(values2) as p2:
            ranks2 = [filtered_ranking(oracle, grown, Qs[:, :, j], 2) for j in range(9)]
            for mode in modes_of(s):
                check_batch(s, p2, values2, ranks2, Qs, 10, f"after the append mode={mode}")
    finally:
        s.close()


# ---- 6. general shapes --------------------------------------------------------------------------------------------------------
GENERAL = [(8, "batched32"), (9, "loop_mfma"), (1, "scalar")]     # rows of tests/util_general.CASES, one per exact-path branch


@pytest.mark.parametrize("case,route", GENERAL)
def test_prior_general_shapes(oracle, case, route):
    assert ug.CASES[case][4] == route and {r for _, r in GENERAL} >= {"loop_mfma", "scalar"}
    idx, Qs, nprobe = ug.case_inputs(case)
    Qs = np.asfortranarray(Qs)
    n_docs = idx["doclens"].size
    values = np.random.default_rng(40 + case).normal(0, 0.5, n_docs).astype(np.float32)
    lens = random_lens(n_docs, 1, 7, 8)
    gids = ids_from_lens(lens)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe) for j in range(3)]
    s = clb.Searcher(index=idx)
    try:
        with s.make_prior(values) as p, s.make_grouping(group_lens=lens) as g:
            for k in (1, ug.CASE_K):
                check_batch(s, p, values, rankings, Qs, k, route, nprobe=nprobe)
                check_batch(s, p, values, rankings, Qs, k, f"{route} weight", weight=-0.75, nprobe=nprobe)
                check_batch(s, p, values, rankings, Qs, k, f"{route} grouped", nprobe=nprobe, grouping=g, gids=gids)
            one = np.asfortranarray(Qs[:, :, :1])
            check_batch(s, p, values, rankings, one, ug.CASE_K, f"{route} B=1", nprobe=nprobe, queries=[0])
    finally:
        s.close()


def test_prior_on_a_query_of_40_tokens(oracle):
    """dim 128, T = 40: the tuned kernels with no two-pass, whatever the mode"""
    idx = synthetic.make_index(seed=23, n_docs=3000, K=256)
    Qs = synthetic.make_queries(idx, 24, 3, T=40)
    values = np.random.default_rng(25).normal(0, 0.5, 3000).astype(np.float32)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(3)]
    s = clb.Searcher(index=idx)
    try:
        with s.make_prior(values) as p:
            for mode in modes_of(s):
                for k in (10, 1000):
                    check_batch(s, p, values, rankings, Qs, k, f"T=40 mode={mode}")
    finally:
        s.close()


# ---- 7. device slot and graph ---------------------------------------------------------------------------------------------------
def test_device_slot_and_captured_graph_with_a_prior(oracle):
    """DeviceSearch with a prior, eager and captured in a graph over a static query buffer and replayed twice, equals the host
    call and the reference; a second slot searches with another prior on another stream meanwhile."""
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=256)
    k, B, w = 60, 5, 0.75
    rng = np.random.default_rng(26)
    v1, v2 = rng.normal(0, 0.5, 6000).astype(np.float32), np.linspace(1.0, 0.0, 6000).astype(np.float32)
    lens = random_lens(6000, 1, 15, 11)
    gids = ids_from_lens(lens)
    Qs = synthetic.make_queries(idx, 31, 2 * B)
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], 2) for j in range(2 * B)]
    Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
    s = clb.Searcher(index=idx)
    p1, p2, g = s.make_prior(v1), s.make_prior(v2), s.make_grouping(group_lens=lens)
    try:
        for mode in modes_of(s):
            for grouping, ids in ((None, None), (g, gids)):
                run, run2 = DeviceSearch(s, 32, B, k, 2), DeviceSearch(s, 32, B, k, 2, slot=1)
                run2(Qdev[:B], grouping=grouping, prior=p2, prior_weight=2.0)       # sizes slot 1 before anything overlaps
                torch.cuda.synchronize()
                q_static = Qdev[:B].clone()
                graph = run.capture(q_static, None, "candidates", grouping, None, p1, w)
                side = torch.cuda.Stream()
                for it in range(2):
                    q_static.copy_(Qdev[it * B:(it + 1) * B])
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):              # the other slot, the other prior, at the same time
                        run2(Qdev[it * B:(it + 1) * B], grouping=grouping, prior=p2, prior_weight=2.0)
                    graph.replay()
                    torch.cuda.synchronize()
                    gp, gs, gn = run.out_p.cpu().numpy().copy(), run.out_s.cpu().numpy().copy(), run.ncand.cpu().numpy().copy()
                    run(Qdev[it * B:(it + 1) * B], grouping=grouping, prior=p1, prior_weight=w)          # eager
                    torch.cuda.synchronize()
                    assert np.array_equal(gp, run.out_p.cpu().numpy()) and np.array_equal(gn, run.ncand.cpu().numpy())
                    assert np.array_equal(bits(gs), bits(run.out_s.cpu().numpy()))
                    hp, hs, hn = s.search_batch(np.asfortranarray(Qs[:, :, it * B:(it + 1) * B]), k, pad_short=True, grouping=grouping,
                                                prior=p1, prior_weight=w)                              # the host call
                    assert np.array_equal(gp.T, hp) and np.array_equal(gn, hn) and np.array_equal(bits(gs.T), bits(hs))
                    o2p, o2s, o2n = run2.out_p.cpu().numpy(), run2.out_s.cpu().numpy(), run2.ncand.cpu().numpy()
                    for j in range(B):
                        want = boosted_ranking(rankings[it * B + j], v1, w)
                        want2 = boosted_ranking(rankings[it * B + j], v2, 2.0)
                        if ids is not None:
                            want, want2 = collapse(want, ids), collapse(want2, ids)
                        assert_result(gp[j], gs[j], gn[j], want, k, f"graph mode={mode} grouped={ids is not None} it={it} q={j}")
                        assert_result(o2p[j], o2s[j], o2n[j], want2, k, f"slot 1 mode={mode} grouped={ids is not None} it={it} q={j}")
                del graph
    finally:
        p1.close(); p2.close(); g.close()
        s.close()
