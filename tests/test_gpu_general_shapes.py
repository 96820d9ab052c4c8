"""The general-shape search path (csrc/generic_kernels.hpp, run_search_general / run_retrieve_general(_batched) in
csrc/search.hip) against the CPU oracle at every kernel and dispatch branch it has: identical pids and candidate counts,
fp32 scores bit for bit.  tests/util_general.expected_route says which kernels a shape reaches;
tests/test_general_shapes_cpu.py holds the oracle itself to a float64 restatement at the shapes of the case table.  Every
input is one the reference accepts."""
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import util_general as ug
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import assert_result
from tests.test_gpu_parity import assert_same_f32, check_search
from tests.test_remove_cpu import reduced_index
from tests.util_filter import filtered_ranking

pytestmark = pytest.mark.gpu

RAGGED = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 0, 1, 16, 1]


def marking_launches(s, run):
    """timed `mark_candidates` launches of run(): mark_and_compact is timed on the batched route only (one launch per
    sub-batch of 64 queries); the per-query loop of the other routes calls it untimed"""
    s.profile_enable(True)
    try:
        s.profile_read()
        out = run()
        return out, int(s.profile_read()["mark_candidates"]["launches"])
    finally:
        s.profile_enable(False)


def assert_route(idx, Qs, k, nprobe, route):
    """`route` is what expected_route gives for the shape, and the handle's profile rows agree as far as they can tell:
    batched or one query at a time (they cannot tell <32> from <64> nor the loop-form MFMA kernel from the scalar one)"""
    assert ug.expected_route(idx["dim"], idx["nbits"], Qs.shape[1]) == route
    s = clb.Searcher(index=idx)
    try:
        _, n = marking_launches(s, lambda: s.search_batch(Qs, k, nprobe=nprobe))
        assert n == (-(-Qs.shape[2] // 64) if route.startswith("batched") else 0), (route, n)
    finally:
        s.close()


def compare_batch(s, oracle, idx, Qs, k, nprobe, refs=None, what=""):
    """one search_batch call (or the single-query entry point at B = 1) on handle s, each query against its own oracle result"""
    B = Qs.shape[2]
    refs = refs or [oracle.search(idx, Qs[:, :, j], nprobe=nprobe, k=k) for j in range(B)]
    if B == 1:
        p, sc = s.search_embeddings(Qs[:, :, 0], k, nprobe=nprobe)
        got = [(p, sc, s.last_num_candidates)]
    else:
        bp, bs, bn = s.search_batch(Qs, k, nprobe=nprobe)
        got = [(bp[:, j], bs[:, j], bn[j]) for j in range(B)]
    for j, (p, sc, n) in enumerate(got):
        rp, rs, rn = refs[j]
        assert n == rn and np.array_equal(p, rp), (what, j, np.nonzero(p != rp)[0][:5])
        assert_same_f32(sc, rs, f"{what} q={j}")
    return refs


# ---- the case table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(ug.CASES)), ids=ug.CASE_IDS)
def test_general_case_table(oracle, case):
    idx, Qs, nprobe = ug.case_inputs(case)
    Qs = np.asfortranarray(Qs)
    route = ug.CASES[case][4]
    assert_route(idx, Qs, ug.CASE_K, nprobe, route)
    if ug.CASES[case][:3] in ((256, 8, 128), (256, 4, 64)):
        assert ug.lds_bytes(*ug.CASES[case][:3]) > 64 * 1024          # run_search_general: `if (lds > 64 * 1024)`
    check_search(oracle, idx, Qs, k=ug.CASE_K, nprobe=nprobe, modes=(0,))


# ---- ragged passages on every route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nbits,T,route", [(64, 2, 20, "batched32"), (136, 4, 20, "batched64"), (264, 2, 20, "loop_mfma"),
                                               (64, 8, 520, "scalar")])
def test_general_ragged_passages(oracle, dim, nbits, T, route):
    """Passages of 0, 1, 2, 15 ... 49 rows among 1 500 (row tails of the 16-row steps, the one-step-ahead code load, empty
    passages between candidates), nprobe = 8 so that most passages are candidates."""
    assert ug.expected_route(dim, nbits, T) == route
    base = synthetic.make_index(seed=71, n_docs=1500, K=64, dim=dim, nbits=nbits, doclen_mean=12, doclen_std=14)
    idx = ug.ragged_index(base, RAGGED, seed=72, reps=19)
    for v in set(RAGGED):
        assert np.count_nonzero(idx["doclens"] == v) >= 19
    Qs = synthetic.make_queries(base, 73, 3, T=T)
    fewest = min(oracle.search(idx, Qs[:, :, j], nprobe=8, k=1)[2] for j in range(3))
    assert fewest > 600, fewest
    check_search(oracle, idx, Qs, k=fewest, nprobe=8, modes=(0,))


# ---- batch sizes -------------------------------------------------------------------------------------------------------
def test_general_batch_sizes_around_the_sub_batch(oracle):
    """B = 1, 64, 65, 70 on the batched route: the (max(64, 2048 / B), B) grid and the split into sub-batches of 64"""
    idx = synthetic.make_index(seed=75, n_docs=600, K=64, dim=64, nbits=2, doclen_mean=20, doclen_std=12)
    Qs = synthetic.make_queries(idx, 76, 70, T=20)
    refs = [oracle.search(idx, Qs[:, :, j], nprobe=2, k=30) for j in range(70)]
    s = clb.Searcher(index=idx)
    try:
        for B in (1, 64, 65, 70):
            Qb = np.asfortranarray(Qs[:, :, :B])
            _, n = marking_launches(s, lambda: compare_batch(s, oracle, idx, Qb, 30, 2, refs[:B], f"B={B}"))
            assert n == -(-B // 64), (B, n)
    finally:
        s.close()


def test_general_batch_on_the_per_query_route(oracle):
    """B = 5 at dim 264: the per-query loop (slot b of cand / cand_hdr / ncand / scores, slot 0 of the selection)"""
    idx = synthetic.make_index(seed=77, n_docs=600, K=64, dim=264, nbits=2, doclen_mean=20, doclen_std=12)
    Qs = synthetic.make_queries(idx, 78, 5, T=20)
    s = clb.Searcher(index=idx)
    try:
        _, n = marking_launches(s, lambda: compare_batch(s, oracle, idx, Qs, 30, 2, what="dim 264 B=5"))
        assert n == 0
    finally:
        s.close()


# ---- large nprobe and k on a generic handle ----------------------------------------------------------------------------
def test_general_large_nprobe(oracle):
    idx = synthetic.make_index(seed=79, n_docs=900, K=96, dim=64, nbits=8, doclen_mean=20, doclen_std=12)
    check_search(oracle, idx, synthetic.make_queries(idx, 80, 3, T=20), k=50, nprobe=40, modes=(0,))


def test_general_large_k_and_full_sort(oracle):
    """dim 8 / nbits 1, 20 000 passages: k = 12 000 (the one-work-group top-k kernel), k = 17 000 (the full stable sort; with
    256 distinct rows per centroid the scores tie in long runs, which the sort has to keep in pid order), k = n_docs + 1"""
    idx = synthetic.make_index(seed=81, n_docs=20000, K=256, dim=8, nbits=1, doclen_mean=10, doclen_std=2)
    Qs = synthetic.make_queries(idx, 82, 2)
    check_search(oracle, idx, Qs, k=12000, nprobe=64, modes=(0,))
    check_search(oracle, idx, Qs, k=17000, nprobe=128, modes=(0,))
    s = clb.Searcher(index=idx)
    try:
        pids, scores = s.search_embeddings(Qs[:, :, 0], 20000, nprobe=256)
        rp, rs, rn = oracle.search(idx, Qs[:, :, 0], nprobe=256, k=20000)
        assert rn == 20000 and np.array_equal(pids, rp)
        assert_same_f32(scores, rs, "nprobe = K, k = n_docs")
        with pytest.raises(clb.BoundsError):
            s.search_embeddings(Qs[:, :, 0], 20001, nprobe=256)
    finally:
        s.close()


# ---- one generic handle, many shapes -----------------------------------------------------------------------------------
def test_general_mixed_shapes_on_one_handle(oracle):
    """The generic counterpart of test_search_mixed_shapes_on_one_handle: the workspace (Ttuned, cells, g_cells, sel, the
    scalar kernel's scratch) grows across the three routes a dim-64 handle has, in an order that visits each before and after
    the others; then the whole sequence again on the grown workspace."""
    idx = synthetic.make_index(seed=83, n_docs=3000, K=256, dim=64, nbits=8, doclen_mean=24, doclen_std=6)
    calls = [(150, 2, 1), (20, 4, 32), (600, 2, 2), (20, 2, 9), (150, 3, 2), (128, 9, 5)]          # (T, nprobe, B)
    assert [ug.expected_route(64, 8, c[0]) for c in calls] == ["loop_mfma", "batched32", "scalar", "batched32", "loop_mfma", "batched32"]
    Qs = [synthetic.make_queries(idx, 840 + i, B, T=T) for i, (T, _, B) in enumerate(calls)]
    refs = [None] * len(calls)
    s = clb.Searcher(index=idx)
    try:
        for rep in range(2):
            for i, (T, nprobe, B) in enumerate(calls):
                refs[i] = compare_batch(s, oracle, idx, Qs[i], 20, nprobe, refs[i], f"rep={rep} T={T} nprobe={nprobe} B={B}")
    finally:
        s.close()


# ---- retrieve ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nbits", [(24, 8), (256, 4), (768, 1)])
def test_general_retrieve(oracle, dim, nbits):
    """Searcher.retrieve on a generic handle: generic_cells_kernel + the stable sort whatever the dim; nprobe 1, 5 and K, and a
    query with two identical tokens (the same lists probed twice)"""
    K = 40
    idx = synthetic.make_index(seed=85 + dim, n_docs=600, K=K, dim=dim, nbits=nbits, doclen_mean=20, doclen_std=12)
    Qs = synthetic.make_queries(idx, 86, 2, T=20)
    Qs[:, 7, 1] = Qs[:, 3, 1]
    emb2pid = oracle.build_emb2pid(idx["doclens"])
    s = clb.Searcher(index=idx)
    try:
        for nprobe in (1, 5, K):
            for j in range(2):
                want = oracle.retrieve(idx["ivf"], idx["ivf_lengths"], idx["centroids"], emb2pid, nprobe, Qs[:, :, j])
                assert np.array_equal(s.retrieve(Qs[:, :, j], nprobe=nprobe), want), (nprobe, j)
            assert want.size == 600 or nprobe < K
    finally:
        s.close()


# ---- huge centroids: the IEEE-division branch of the fast kernel -------------------------------------------------------
@pytest.mark.parametrize("scale", [1.4e18, 4e18])
def test_general_huge_centroids(oracle, scale):
    """generic_score_mfma_fast_kernel divides by the reciprocal inside `den > 1e-18f && den < 1e18f` and by IEEE division
    outside.  den = the embedding's norm (+ FLT_EPSILON) = its centroid's norm at this scale (the bucket weights vanish next to
    it).  x 1.4e18: norms on both sides of 1e18, so both branches run inside one wave; x 4e18: every embedding divides."""
    base = synthetic.make_index(seed=87, n_docs=600, K=96, dim=64, nbits=8, doclen_mean=20, doclen_std=12)
    assert ug.expected_route(64, 8, 20) == "batched32"
    idx = dict(base, centroids=np.asfortranarray(base["centroids"] * np.float32(scale)))
    norms = np.linalg.norm(idx["centroids"].astype(np.float64), axis=0)[idx["codes"].astype(np.int64) - 1]
    if scale < 2e18:
        assert np.count_nonzero(norms < 0.97e18) > 1000 and np.count_nonzero(norms > 1.03e18) > 1000
    else:
        assert norms.min() > 2e18 and norms.max() ** 2 <= 1.6e37
    Qs = synthetic.make_queries(base, 88, 3, T=20)
    for j in range(3):
        assert np.all(np.isfinite(oracle.search(idx, Qs[:, :, j], nprobe=2, k=30)[1]))
    check_search(oracle, idx, Qs, k=30, modes=(0,))


# ---- filters on the per-query route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("dim,T,nprobe", [(64, 150, 2), (264, 20, 1)])
def test_general_filters_on_the_per_query_route(oracle, dim, T, nprobe, scope):
    """B = 3 with [f0, None, f1] where the queries run one at a time (mark_and_compact(..., b, 1, ...)): f0 keeps half of
    the passages, f1 fewer than k (a short, padded result)"""
    assert ug.expected_route(dim, 2, T) == "loop_mfma"
    idx = synthetic.make_index(seed=89, n_docs=900, K=64, dim=dim, nbits=2, doclen_mean=20, doclen_std=12)
    Qs = synthetic.make_queries(idx, 90, 3, T=T)
    k = 30
    rng = np.random.default_rng(91)
    allowed = [np.nonzero(rng.random(900) < 0.5)[0] + 1, None, np.sort(rng.choice(900, size=25, replace=False)) + 1]
    s = clb.Searcher(index=idx)
    filters = [None if a is None else s.make_filter(pids=a) for a in allowed]
    try:
        bp, bs, bn = s.search_batch(Qs, k, nprobe=nprobe, filters=filters, scope=scope)
        for j in range(3):
            ranking = filtered_ranking(oracle, idx, Qs[:, :, j], nprobe, allowed[j], scope)
            assert_result(bp[:, j], bs[:, j], bn[j], ranking, k, f"dim={dim} T={T} scope={scope} q={j}")
        assert bn[0] >= k and bn[1] >= k and 0 < bn[2] < k
        assert bn[2] == 25 or scope == "candidates"
    finally:
        for f in filters:
            if f is not None:
                f.close()
        s.close()


# ---- append, then the scalar kernel ------------------------------------------------------------------------------------
def test_general_append_a_longer_passage_then_long_queries(oracle):
    """The scalar kernel's scratch holds max_doclen rows per work-group: append a passage 50 rows longer than every resident
    one and search at T = 520 (scalar) and T = 20 (batched), then remove that passage and search at T = 520 again."""
    base = synthetic.make_index(seed=93, n_docs=300, K=64, dim=64, nbits=2, doclen_mean=20, doclen_std=6)
    longest = int(base["doclens"].max()) + 50
    full = ug.ragged_index(base, [longest], seed=96, reps=1)
    p = int(np.argmax(full["doclens"]))                                    # 0-based
    P = 150
    assert p >= P and full["doclens"][p] == longest and full["doclens"][:P].max() <= longest - 40
    Qlong, Qshort = synthetic.make_queries(base, 95, 2, T=520), synthetic.make_queries(base, 96, 3, T=20)
    assert ug.expected_route(64, 2, 520) == "scalar"
    s = clb.Searcher(index=head_index(full, P))
    try:
        compare_batch(s, oracle, head_index(full, P), Qlong[:, :, :1], 20, 2, what="head T=520")   # scratch sized for the head
        assert list(s.add_compressed(*tail(full, P))) == list(range(P + 1, 301))
        compare_batch(s, oracle, full, Qlong, 20, 2, what="appended T=520")
        compare_batch(s, oracle, full, Qshort, 20, 2, what="appended T=20")
        # the long passage is a candidate of the long queries, so the kernel did decompress its rows
        assert any(p + 1 in filtered_ranking(oracle, full, Qlong[:, :, j], 2)[0] for j in range(2))
        assert s.remove_passages([p + 1]) == 1
        red, _ = reduced_index(full, [p + 1])
        compare_batch(s, oracle, red, Qlong, 20, 2, what="removed T=520")
    finally:
        s.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("COLBERT_TEST_FUZZ_SEEDS", "10"))))
def test_general_search_random_configurations(oracle, seed):
    """Randomly drawn general shapes: dim, nbits, K, corpus size, passage lengths, query length, batch, nprobe, k, scaled
    queries (util_general.fuzz_configuration, which also lists the route of every default seed).  No dim 128 is drawn, so
    every configuration is a general shape."""
    c = ug.fuzz_configuration(seed)
    ug.expected_route(c["dim"], c["nbits"], c["T"])                # raises for a tuned shape
    idx = synthetic.make_index(seed=9100 + seed, n_docs=c["n_docs"], K=c["K"], dim=c["dim"], nbits=c["nbits"],
                               doclen_mean=c["mean"], doclen_std=c["std"], topical=c["topical"])
    Qs = synthetic.make_queries(idx, 9200 + seed, c["B"], T=c["T"])
    if c["scale"] != 1.0:
        Qs = np.asfortranarray(Qs * np.float32(c["scale"]))
    k, nprobe = c["k"], c["nprobe"]
    counts = [oracle.search(idx, Qs[:, :, j], nprobe=nprobe, k=1)[2] for j in range(c["B"])]
    fewest = min(counts)
    if k > fewest:                                                 # BoundsError first (searching.jl:127), then the largest k all can fill
        srch = clb.Searcher(index=idx)
        try:
            with pytest.raises(clb.BoundsError):
                srch.search_embeddings(Qs[:, :, int(np.argmin(counts))], k, nprobe=nprobe)
        finally:
            srch.close()
        k = fewest
    check_search(oracle, idx, Qs, k=k, nprobe=nprobe, modes=(0,))
