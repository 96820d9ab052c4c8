"""Selection, ranking and merging on negative, zero and sign-mixed scores: everything that ranks goes
through one float -> order-key mapping and one radix-select core, and until this file the suite had shown them positive MaxSim
scores only.  Three routes, each against the reference the feature already has:

  1. queries whose MaxSim scores are negative (`negated` on an index with shifted centroids), lie on both sides of zero
     (`straddle` on one-row passages), or are all +0.0 (`zero`) -- tests/util_selection.py says why the indexes differ, and
     tests/test_selection_model_cpu.py checks from the oracle alone that the inputs are what they claim;
  2. score priors that mirror a query's ranking below zero, lay a run of +0.0 across the k-th place, spread the boosted
     scores over forty exponents of both signs, or reach 1e38;
  3. raw records into the merge and threshold hooks.

Bar everywhere: pids equal, fp32 score bits equal, candidate counts equal.  Figures for profiles/selection_keys.md are printed
(pytest -s)."""
import itertools

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd.searcher import next_cursor
from tests import pass1_model as pm
from tests import selection_model as sm
from tests import util_selection as us
from tests.test_gpu_filtered_search import assert_result, assert_same_f32, random_allowed
from tests.test_gpu_group_hits import check_hits
from tests.test_gpu_grouped_search import check_batch as check_grouped
from tests.test_gpu_grouped_search import modes_of
from tests.test_gpu_parity import check_search
from tests.test_gpu_pass1_model import assert_inside, run_hook
from tests.test_gpu_prior import check_batch as check_prior
from tests.test_gpu_sharded_grouped import (as_lists, device_group_tau, device_grouped_merge, merge_case, numpy_group_tau,
                                            numpy_grouped_merge, shard_like_lists)
from tests.test_gpu_sharded_searcher import check_group
from tests.test_pass1_model_cpu import K as FRIENDLY_K
from tests.test_pass1_model_cpu import covering_query, friendly
from tests.util_after import assert_page
from tests.util_filter import filtered_ranking
from tests.util_group import collapse, ids_from_lens, random_lens

pytestmark = pytest.mark.gpu


def note(text):
    print(f"selection_keys: {text}")


def reset(s):
    s.set_wide_select(-1); s.set_pass1_gather(-1); s.set_score_rows(-1); s.set_centroid_products(-1)


def configurations(s, B):
    """(mode, wide, gather form, score rows, centroid products): the exact mode once; the two-pass mode with one and sixteen
    work-groups per query in the selection, both gather forms and -- in batches of 16+ queries, where they exist -- both row
    formats and both score-table products"""
    auto = s.pass1_gather[0]
    for mode in modes_of(s):
        if mode == 0:
            yield 0, -1, -1, -1, -1
            continue
        rows, products = ((0, 1), (1, 3)) if B >= 16 else ((0,), (-1,))
        yield from ((1,) + c for c in itertools.product((0, 1), (-1, 1 - auto), rows, products))


def run_matrix(s, Q9, ranks, ks, what, nprobe=2, batches=(9, 33)):
    try:
        for B in batches:
            Qb = us.tiled(Q9, B)
            for mode, wide, form, rows, products in configurations(s, B):
                s.set_wide_select(wide); s.set_pass1_gather(form); s.set_score_rows(rows); s.set_centroid_products(products)
                for k in ks:
                    bp, bs, bn = s.search_batch(Qb, k, nprobe=nprobe, pad_short=True)
                    for j in range(B):
                        assert_result(bp[:, j], bs[:, j], bn[j], ranks[j % Q9.shape[2]], k,
                                      f"{what} B={B} mode={mode} wide={wide} form={form} rows={rows} products={products} k={k} q={j}")
    finally:
        reset(s)


def note_pruning(s, Q, ks, what, nprobe=2):
    """The re-scored share of the candidates in the two-pass mode's default configuration.  Parity cannot see a threshold
    that is merely too low (everything is listed and the answer is still exact); this figure can.  Printed for
    profiles/selection_keys.md, with the two bounds that hold whatever the scores are."""
    try:
        s.set_mode(1)
    except clb.Unsupported:
        note(f"{what}: no two-pass mode on this handle, no re-scored share")
        return
    s.profile_enable(True, counters=True)
    try:
        for k in ks:
            _, _, bn = s.search_batch(Q, k, nprobe=nprobe, pad_short=True)
            st = s.last_batch_stats()
            note(f"{what} B={Q.shape[2]} k={k}: re-scored {st['rescored_docs']} of {st['cand_docs']} candidates "
                 f"({st['rescored_docs'] / max(st['cand_docs'], 1):.4f})")
            assert int(np.minimum(bn, k).sum()) <= st["rescored_docs"] <= st["cand_docs"] == int(bn.sum()), (what, k, st)
    finally:
        s.profile_enable(False)


# ---- route 1: queries ---------------------------------------------------------------------------------------------------------
MATRIX = [("medium_shifted", "negated", 32), ("medium_shifted", "negated", 4), ("medium_shifted", "one_hot_zero", 32),
          ("medium_shifted", "one_hot_zero", 4), ("medium_shifted", "zero", 32), ("medium", "zero", 4), ("short", "straddle", 32),
          ("short", "straddle", 4), ("medium", "negated", 32), ("medium", "straddle", 32), ("medium", "one_hot_zero", 32)]


@pytest.mark.parametrize("index_name,name,T", MATRIX)
def test_query_variants_in_every_configuration(oracle, index_name, name, T):
    """B = 9 and B = 33, k = 1, 10, 1000, every configuration of `configurations`.  On "medium" (the unshifted index) the scores
    of `negated` and `straddle` stay positive (tests/util_selection.py); they run there as well, as plain parity cases."""
    ranks = us.rankings(oracle, index_name, name, T)
    Q = us.queries(index_name, name, T)
    s = clb.Searcher(index=us.INDEXES[index_name]())
    try:
        run_matrix(s, Q, ranks, us.KS, f"{index_name} {name} T={T}")
        note_pruning(s, Q, us.KS, f"{index_name} {name} T={T}")
    finally:
        s.close()


@pytest.mark.parametrize("index_name,name", [("medium_shifted", "negated"), ("short", "straddle"), ("medium_shifted", "zero"),
                                             ("medium_shifted", "one_hot_zero")])
@pytest.mark.parametrize("wide", [0, 1])
def test_query_variants_through_check_search(oracle, index_name, name, wide):
    """tests/test_gpu_parity.check_search as it stands: single queries and the batch, both gather forms, both row formats"""
    Q = np.asfortranarray(us.queries(index_name, name)[:, :, :3])
    check_search(oracle, us.INDEXES[index_name](), Q, k=10, wide=wide)


@pytest.mark.parametrize("name", ["negated", "straddle", "zero"])
def test_more_candidates_than_a_work_group_keeps_in_registers(oracle, name):
    """40 000 candidates per query: strided ownership in topk_kernel and select_margin_kernel, the block-wise ordered compaction,
    1 024-slot segments in the wide chain; k = 5 000 lists more than the rank kernel takes, k = 17 000 is past the LDS sort"""
    ranks = us.rankings(oracle, "large", name, 32, us.LARGE_NPROBE)[:3]
    assert all(rp.size > 32_768 for rp, _ in ranks)            # from the oracle, before the device is touched
    if name == "negated":
        assert all(rs.max() < 0 for _, rs in ranks)
    Q = np.asfortranarray(us.queries("large", name)[:, :, :3])
    s = clb.Searcher(index=us.large_index())
    try:
        run_matrix(s, Q, ranks, (10, 5000, 17000), f"large {name}", nprobe=us.LARGE_NPROBE, batches=(3,))
        note_pruning(s, Q, (10, 5000, 17000), f"large {name}", nprobe=us.LARGE_NPROBE)
    finally:
        s.close()


def page_to_the_end(s, Q, ranks, k, what):
    B = Q.shape[2]
    cs, cp = np.full(B, np.inf, np.float32), np.zeros(B, np.int64)           # +Inf: no cursor, the first page
    longest = max(rp.size for rp, _ in ranks)
    for page in range(longest // k + 2):
        bp, bs, bn = s.search_batch(Q, k, after=(cs, cp))
        for j in range(B):
            assert_page(bp[:, j], bs[:, j], bn[j], ranks[j], (cs[j], cp[j]), k, f"{what} page={page} q={j}")
        if np.all(bp[0] == 0):
            return page
        cs, cp = next_cursor(bp, bs)
    raise AssertionError(f"{what}: no empty page after {longest // k + 2} pages")


@pytest.mark.parametrize("name", ["negated", "straddle"])
def test_a_cursor_pages_to_the_end_below_zero(oracle, name):
    ranks = us.rankings(oracle, "small", name)
    Q = us.queries("small", name)
    s = clb.Searcher(index=us.small_index())
    try:
        for mode in modes_of(s):
            pages = page_to_the_end(s, Q, ranks, 16, f"small {name} mode={mode}")
            assert pages >= 2
    finally:
        s.close()


@pytest.mark.parametrize("index_name,name", [("medium_shifted", "negated"), ("short", "straddle"), ("medium_shifted", "zero")])
def test_cursors_at_negative_scores_at_zero_and_between_candidates(oracle, index_name, name):
    ranks = us.rankings(oracle, index_name, name)
    Q = us.queries(index_name, name)
    B = Q.shape[2]
    cursors = {}
    at = lambda r: (np.array([rs[min(r, rs.size - 1)] for _, rs in ranks], np.float32),
                    np.array([rp[min(r, rp.size - 1)] for rp, _ in ranks], np.int64))
    for r in (0, 5, 500):
        cursors[f"rank {r}"] = at(r)                                           # negative for `negated`, +0.0 for `zero`
    cursors["plus zero, before every pid"] = (np.zeros(B, np.float32), np.zeros(B, np.int64))
    cursors["plus zero, past every pid"] = (np.zeros(B, np.float32), np.full(B, 1 << 40, np.int64))
    below = np.array([np.nextafter(rs[min(7, rs.size - 1)], np.float32(-np.inf)) for _, rs in ranks], np.float32)
    cursors["one ulp below rank 7"] = (below, np.zeros(B, np.int64))           # (mostly) no candidate's score
    cursors["one ulp below rank 7, past every pid"] = (below, np.full(B, 1 << 40, np.int64))
    if name == "negated":
        assert np.all(cursors["rank 5"][0] < 0)
    if name == "zero":
        assert np.all(cursors["rank 5"][0].view(np.uint32) == 0)
    assert sum(1 for (rp, rs), b in zip(ranks, below) if not np.any(rs == b)) * 2 >= B
    s = clb.Searcher(index=us.INDEXES[index_name]())
    try:
        for mode in modes_of(s):
            for what, (cs, cp) in cursors.items():
                for k in (10, 1000):
                    bp, bs, bn = s.search_batch(Q, k, after=(cs, cp))
                    for j in range(B):
                        assert_page(bp[:, j], bs[:, j], bn[j], ranks[j], (cs[j], cp[j]), k, f"{index_name} {name} mode={mode} {what} q={j}")
    finally:
        s.close()


@pytest.mark.parametrize("index_name,name", [("medium_shifted", "negated"), ("short", "straddle"), ("medium_shifted", "one_hot_zero")])
def test_filtered_grouped_and_per_group_calls(oracle, index_name, name):
    idx = us.INDEXES[index_name]()
    n_docs = idx["doclens"].size
    plain = us.rankings(oracle, index_name, name)[:3]
    Q3 = np.asfortranarray(us.queries(index_name, name)[:, :, :3])
    alloweds = [random_allowed(n_docs, 0.5, 300), random_allowed(n_docs, 0.02, 301), None]
    filtered = [filtered_ranking(oracle, idx, np.ascontiguousarray(Q3[:, :, j]), 2, alloweds[j]) for j in range(3)]
    lens = random_lens(n_docs, 1, 40, 5)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        filters = [None if a is None else s.make_filter(pids=a) for a in alloweds]
        with s.make_grouping(group_lens=lens) as g:
            for mode in modes_of(s):
                for k in (10, 1000):
                    what = f"{index_name} {name} mode={mode}"
                    bp, bs, bn = s.search_batch(Q3, k, filters=filters)
                    for j in range(3):
                        assert_result(bp[:, j], bs[:, j], bn[j], filtered[j], k, f"{what} filtered k={k} q={j}")
                    check_grouped(s, g, gids, plain, Q3, k, f"{what} grouped")
                    check_grouped(s, g, gids, filtered, Q3, k, f"{what} filtered + grouped", filters=filters)
                    check_hits(s, g, gids, plain, Q3, k, 3, f"{what} per_group")
                    check_hits(s, g, gids, filtered, Q3, k, 3, f"{what} filtered + per_group", filters=filters)
        for f in filters:
            if f is not None:
                f.close()
    finally:
        s.close()


@pytest.mark.parametrize("index_name,name", [("medium_shifted", "negated"), ("short", "straddle"), ("medium_shifted", "one_hot_zero")])
@pytest.mark.parametrize("world", [2, 4])
def test_a_shard_group(oracle, index_name, name, world):
    """both merge kernels and the published-threshold protocol: every shard's list and every threshold is negative, or the lists
    cross zero at different places"""
    idx = us.INDEXES[index_name]()
    ranks = us.rankings(oracle, index_name, name)
    Q = us.queries(index_name, name)
    lens = random_lens(idx["doclens"].size, 1, 40, 6)
    gids = ids_from_lens(lens)
    g = clb.ShardedSearcher.from_index(idx, world)
    try:
        for k in (10, 1000):
            check_group(g, Q, ranks, k, f"{index_name} {name} world={world} k={k}")
        with g.make_grouping(group_lens=lens) as gr:
            for proto in ("two_phase", "single"):
                for k in (10, 1000):
                    bp, bs, bn = g.search_batch(Q, k, 2, pad_short=True, grouping=gr, protocol=proto)
                    for j in range(Q.shape[2]):
                        assert_result(bp[:, j], bs[:, j], bn[j], collapse(ranks[j], gids), k,
                                      f"{index_name} {name} world={world} grouped protocol={proto} k={k} q={j}")
    finally:
        g.close()


@pytest.mark.parametrize("name", ["negated", "straddle", "zero", "one_hot_zero"])
def test_general_shape_index(oracle, name):
    """dim 64: the 64-bit sort keys of the generic path"""
    ranks = us.rankings(oracle, "general", name)
    if name == "negated":
        assert all(rs.max() < 0 for _, rs in ranks)
    Q = us.queries("general", name)
    lens = random_lens(600, 1, 7, 8)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=us.general_index())
    try:
        with s.make_grouping(group_lens=lens) as g:
            for mode in modes_of(s):
                for k in (1, 30, 600):
                    bp, bs, bn = s.search_batch(Q, k, pad_short=True)
                    for j in range(Q.shape[2]):
                        assert_result(bp[:, j], bs[:, j], bn[j], ranks[j], k, f"general {name} mode={mode} k={k} q={j}")
                    check_grouped(s, g, gids, ranks, Q, k, f"general {name} grouped mode={mode}")
    finally:
        s.close()


# ---- route 1, through the hook ----------------------------------------------------------------------------------------------
TOP = 10


def friendly_shifted():
    idx, base = friendly()
    return us.shifted(idx), us.shifted(base)


HOOK = [(name, nprobe, gather, rows) for name in ("negated", "straddle", "zero") for nprobe in (FRIENDLY_K, 2) for gather in (0, 1)
        for rows in ((0, 1) if nprobe == 2 else (0,))]


@pytest.mark.parametrize("name,nprobe,gather,rows", HOOK)
def test_hook_on_negative_and_zero_scores(name, nprobe, gather, rows):
    """the friendly index of tests/test_pass1_model_cpu.py with shifted centroids (every score of -Q is negative): the error
    against eps, tau against the approximate scores, the listed count in fp32, and the float64 interval of tests/pass1_model.py"""
    idx, base = friendly_shifted()
    o = pm.Operands(idx)
    Q1 = covering_query(idx) if nprobe == 2 else np.ascontiguousarray(synthetic.make_queries(base, 63, 1)[:, :, 0])
    Q = np.ascontiguousarray(us.variant(Q1[:, :, None], name)[:, :, 0])
    d = run_hook(idx, Q, nprobe, gather=gather, rows=rows, products=3 if rows else -1)
    a, e = d["approx"], d["exact"]
    what = f"hook {name} nprobe={nprobe} gather={gather} rows={rows}"
    assert a.size > 0 and np.isfinite(d["eps"]) and d["eps"] > 0
    if name == "negated":
        assert e.max() < 0 and a.max() < 0
    if name == "zero":
        assert np.all(e.view(np.uint32) == 0)
    err = float(np.abs(a.astype(np.float64) - e.astype(np.float64)).max())
    note(f"{what}: n = {a.size}, max |approx - exact| / eps = {err:.3e} / {d['eps']:.3e} = {err / d['eps']:.4f}")
    assert err <= d["eps"]
    tau, eps = np.float32(d["tau"]), np.float32(d["eps"])
    if a.size > TOP:
        kth = sm.from_order_key(np.array([sm.kth_largest_key(sm.order_key(a), TOP)], np.uint32))[0]
        assert tau.view(np.uint32) == kth.view(np.uint32), (what, tau, kth)
        assert sm.select_value(a, TOP).view(np.uint32) == tau.view(np.uint32)
        thr = np.float32(tau - np.float32(2.0) * eps)
        assert d["n_rescore"] == np.count_nonzero(~(a < thr)), (what, d["n_rescore"], np.count_nonzero(~(a < thr)))
    else:
        assert np.isneginf(tau) and d["n_rescore"] == a.size
    assert_inside(o, Q, d, what, products=3, rows8=bool(rows))


# ---- route 2: priors ----------------------------------------------------------------------------------------------------------
def prior_cases(name, oracle):
    """(label, values, weight, variant of the queries) of one kind of prior on the medium index"""
    n = us.N_MEDIUM
    r0 = us.rankings(oracle, "medium", "plain")[0]
    if name == "zero_run":
        return [(f"zero_run k={k}", us.prior_values("zero_run", r0, n, k), 1.0, "plain") for k in us.PRIOR_KS]
    if name == "octaves":
        z0 = us.rankings(oracle, "medium", "zero_first")[0]
        return [(f"octaves w={w}", us.prior_values("octaves", z0, n), w, "zero_first") for w in (1.0, -1.5)]
    return [(name, us.prior_values(name, r0, n), 1.0, "plain")]


@pytest.mark.parametrize("name", ["mirror", "zero_run", "octaves", "huge", "huge_low"])
def test_priors_that_reshape_the_score_distribution(oracle, name):
    """modes 0 and 1, one and sixteen work-groups per query, both gather forms, k = 1, 10, 100, 1000; after every two-pass call
    sum_b min(k, n_cand[b]) <= rescored_docs <= cand_docs (= B k <= ... when every query has k candidates)"""
    s = clb.Searcher(index=us.medium_index())
    try:
        auto = s.pass1_gather[0]
        for label, values, weight, variant in prior_cases(name, oracle):
            ranks = us.rankings(oracle, "medium", variant)
            Q = us.queries("medium", variant)
            with s.make_prior(values) as p:
                for mode in modes_of(s):
                    for form, wide in (itertools.product((-1, 1 - auto), (0, 1)) if mode == 1 else ((-1, -1),)):
                        s.set_pass1_gather(form); s.set_wide_select(wide)
                        s.profile_enable(mode == 1, counters=True)
                        for k in us.PRIOR_KS:
                            _, _, bn = check_prior(s, p, values, ranks, Q, k, f"{label} mode={mode} form={form} wide={wide}", weight=weight)
                            if mode == 1:
                                st = s.last_batch_stats()
                                if form == -1 and wide == 0:
                                    note(f"{label} k={k}: re-scored {st['rescored_docs']} of {st['cand_docs']} candidates "
                                         f"({st['rescored_docs'] / st['cand_docs']:.4f})")
                                assert int(np.minimum(bn, k).sum()) <= st["rescored_docs"] <= st["cand_docs"], (label, k, st)
                                assert st["cand_docs"] == int(bn.sum())
                                if name == "huge_low" and k == 1000:       # tau - 2 delta is -Inf: everything is listed
                                    assert st["rescored_docs"] == st["cand_docs"], (label, st)
                        s.profile_enable(False)
    finally:
        s.close()


def test_priors_compose_below_zero(oracle):
    """the mirror prior with a filter and with a grouping; on the 40 000-passage index; on the general-shape index.  (per_group
    takes no prior, and a shard group has no priors: nothing to run there.)"""
    n = us.N_MEDIUM
    ranks = us.rankings(oracle, "medium", "plain")[:3]
    Q3 = np.asfortranarray(us.queries("medium", "plain")[:, :, :3])
    values = us.prior_values("mirror", ranks[0], n)
    idx = us.medium_index()
    alloweds = [random_allowed(n, 0.5, 300), random_allowed(n, 0.02, 301), None]
    filtered = [filtered_ranking(oracle, idx, np.ascontiguousarray(Q3[:, :, j]), 2, alloweds[j]) for j in range(3)]
    lens = random_lens(n, 1, 40, 5)
    gids = ids_from_lens(lens)
    s = clb.Searcher(index=idx)
    try:
        filters = [None if a is None else s.make_filter(pids=a) for a in alloweds]
        with s.make_prior(values) as p, s.make_grouping(group_lens=lens) as g:
            for mode in modes_of(s):
                for k in (10, 1000):
                    check_prior(s, p, values, filtered, Q3, k, f"mirror filtered mode={mode}", filters=filters)
                    check_prior(s, p, values, ranks, Q3, k, f"mirror grouped mode={mode}", grouping=g, gids=gids)
            with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
                s.search_batch(Q3, 5, grouping=g, per_group=2, prior=p)
        for f in filters:
            if f is not None:
                f.close()
    finally:
        s.close()
    # ... and on negated queries: a NEGATIVE unboosted score boosted (there E = -e is positive)
    for index_name, variant, nprobe, ks in (("large", "plain", us.LARGE_NPROBE, (10, 5000)), ("general", "plain", 2, (1, 30)),
                                            ("medium_shifted", "negated", 2, (10, 1000))):
        idx = us.INDEXES[index_name]()
        ranks = us.rankings(oracle, index_name, variant, 32, nprobe)[:3]
        Q3 = np.asfortranarray(us.queries(index_name, variant)[:, :, :3])
        values = us.prior_values("mirror", ranks[0], idx["doclens"].size)
        s = clb.Searcher(index=idx)
        try:
            with s.make_prior(values) as p:
                for mode in modes_of(s):
                    for wide in ((0, 1) if mode == 1 else (-1,)):
                        s.set_wide_select(wide)
                        s.profile_enable(mode == 1, counters=True)
                        for k in ks:
                            _, _, bn = check_prior(s, p, values, ranks, Q3, k, f"mirror {index_name} mode={mode} wide={wide}", nprobe=nprobe)
                            if mode == 1:
                                st = s.last_batch_stats()
                                if wide == 0:
                                    note(f"mirror on {index_name} {variant} B=3 k={k}: re-scored {st['rescored_docs']} of "
                                         f"{st['cand_docs']} candidates ({st['rescored_docs'] / max(st['cand_docs'], 1):.4f})")
                                assert int(np.minimum(bn, k).sum()) <= st["rescored_docs"] <= st["cand_docs"], (index_name, k, st)
                        s.profile_enable(False)
        finally:
            s.close()


# ---- route 3: records into the merge and threshold hooks --------------------------------------------------------------------
def device_merge(P, S, k, packed):
    import torch
    from colbert_jl_amd.distributed import merge_gathered, merge_packed, packed_topk_bytes
    L, B, _ = P.shape
    dev = torch.device("cuda", 0)
    if packed:
        blocks = np.zeros((L, packed_topk_bytes(k, B)), np.uint8)
        for l in range(L):
            blocks[l, :B * k * 8] = np.ascontiguousarray(P[l], np.int64).view(np.uint8).reshape(-1)
            blocks[l, B * k * 8:B * k * 12] = np.ascontiguousarray(S[l], np.float32).view(np.uint8).reshape(-1)
        op, os_ = merge_packed(torch.from_numpy(blocks).to(dev), B, k)
    else:
        op, os_ = merge_gathered(torch.from_numpy(np.ascontiguousarray(P, np.int64)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(S, np.float32)).to(dev), k)
    torch.cuda.synchronize()
    return op.cpu().numpy(), os_.cpu().numpy()


SHAPES = [(L, k) for L in (1, 2, 7) for k in (1, 33, 1000)]


@pytest.mark.parametrize("kind", us.SCORE_KINDS)
def test_merge_of_lists_below_and_across_zero(kind):
    """n_lists = 1, 2, 7, k = 1, 33, 1000, B = 3: negative, sign-mixed and forty-exponent scores, subnormals, +-FLT_MAX, runs of
    +0.0 shared between the lists, -Inf padding of another length in every list; against the stable sort of the union"""
    rng = np.random.default_rng(11)
    for L, k in SHAPES:
        P, S = us.sorted_lists(rng, L, 3, k, kind)
        want_p, want_s = us.merged_reference(P, S, k)
        for packed in (False, True):
            got_p, got_s = device_merge(P, S, k, packed)
            assert np.array_equal(got_p, want_p), (kind, L, k, packed)
            assert_same_f32(got_s, want_s, f"merge {kind} L={L} k={k} packed={packed}")


def test_merge_of_lists_that_hold_both_zeros():
    """-0.0 ranks below +0.0 in the top-k kernels; the merge of two such lists is what one top k over the union returns: +0.0
    first, then by pid, no record lost and none twice"""
    mz, pz = np.float32(-0.0), np.float32(0.0)
    rng = np.random.default_rng(12)
    cases = [([[(5, pz), (1, mz)], [(3, pz), (2, mz)]], 4)]
    for L, k in ((2, 33), (7, 33), (7, 1000)):
        pool = rng.permutation(np.arange(1, L * k + 1))
        lists = []
        for l in range(L):
            m = int(rng.integers(1, k + 1))
            sc = rng.choice(np.array([1.0, pz, mz, -1.0], np.float32), m)
            lists.append(list(zip(pool[l * k:l * k + m].tolist(), sc)))
        cases.append((lists, k))
    for lists, k in cases:
        L = len(lists)
        P = np.zeros((L, 1, k), np.int64); S = np.full((L, 1, k), -np.inf, np.float32)
        for l, recs in enumerate(lists):
            p, sc = sm.rank_by_key([r[0] for r in recs], [r[1] for r in recs])       # sorted as the top-k kernels sort
            P[l, 0, :p.size], S[l, 0, :p.size] = p, sc
        live = P.reshape(-1) > 0
        want_p, want_s = sm.rank_by_key(P.reshape(-1)[live], S.reshape(-1)[live])
        n = min(k, want_p.size)
        for packed in (False, True):
            got_p, got_s = device_merge(P, S, k, packed)
            assert np.array_equal(got_p[0, :n], want_p[:n]), (L, k, packed, got_p[0, :8], want_p[:8])
            assert_same_f32(got_s[0, :n], want_s[:n], f"zeros L={L} k={k} packed={packed}")
            assert np.all(got_p[0, n:] == 0) and np.all(np.isneginf(got_s[0, n:]))
        # the grouped merge compares the same way: every record a group of its own
        G = np.where(P > 0, P, -1)
        ncl = np.count_nonzero(P > 0, axis=2).astype(np.int64)
        edges = np.full((L, 1, 2), -1, np.int64)
        for l in range(L):
            g_l = G[l, 0][G[l, 0] >= 0]
            edges[l, 0] = (g_l.min(), g_l.max())
        for packed in (False, True):
            got_p, got_s, got_n = device_grouped_merge(P, S, G, ncl, edges, k, packed)
            assert np.array_equal(got_p[0, :n], want_p[:n]) and got_n[0] == ncl.sum(), (L, k, packed)
            assert_same_f32(got_s[0, :n], want_s[:n], f"grouped zeros L={L} k={k} packed={packed}")


@pytest.mark.parametrize("kind", us.SCORE_KINDS)
def test_grouped_merge_and_group_threshold_below_and_across_zero(kind):
    rng = np.random.default_rng(13)
    for L, k in SHAPES:
        qs = [merge_case(rng, L, k, 0.8, 0.2 if L > 1 else 0.0) for _ in range(3)]
        qs = [([[(p, float(sc), g_) for (p, _, g_), sc in zip(recs, us.special_scores(rng, len(recs), kind))] for recs in q[0]],
               q[1], q[2]) for q in qs]
        arrs = [as_lists(q[0], k) for q in qs]
        P, S, G = (np.concatenate([a[i] for a in arrs], axis=1) for i in range(3))
        ncl = np.stack([q[1] for q in qs], axis=1); edges = np.stack([q[2] for q in qs], axis=1)
        want = numpy_grouped_merge(P, S, G, ncl, edges, k)
        for packed in (False, True):
            got = device_grouped_merge(P, S, G, ncl, edges, k, packed)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (kind, L, k, packed)
            assert_same_f32(got[1], want[1], f"grouped merge {kind} L={L} k={k} packed={packed}")
        recs = [shard_like_lists(rng, L, k, 0.5, 0.8) for _ in range(3)]
        top = np.stack([r[0] for r in recs], axis=1); gid = np.stack([r[1] for r in recs], axis=1)
        top[gid >= 0] = us.special_scores(rng, int(np.count_nonzero(gid >= 0)), kind)
        assert_same_f32(device_group_tau(top, gid), numpy_group_tau(top, gid, k), f"group tau {kind} S={L} k={k}")
