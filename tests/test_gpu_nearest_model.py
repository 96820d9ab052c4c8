"""The index build's nearest-centroid search (nearest_centroids<MODE>, csrc/codec.hip) through its test hook clb_debug_nearest,
against the float64 model tests/nearest_model.py: the group lists inside the model's interval, the margin that ships, the decision
invariant, and WHICH tier decided every point of inputs built to need a particular one (their properties are asserted without a
device in tests/test_nearest_model_cpu.py).  Codes always equal the CPU oracle's.  Every case runs both modes."""
import numpy as np
import pytest

from colbert_jl_amd import codec
from tests import nearest_model as nm

pytestmark = pytest.mark.gpu

MODES = (0, 1)


def run_and_check(oracle, C, X, mode, what, expect_x1=None, ties=True, **kw):
    """One hook call; codes = the oracle's, cn / dc / margin = the model's, lists as in (a), decisions as in (c)."""
    r = codec.debug_nearest(C, X, mode=mode, **kw)
    ref = nm.oracle_winners(oracle, C, X, mode)
    assert np.array_equal(r["codes"].astype(np.int64) - 1, ref), (what, mode, np.flatnonzero(r["codes"].astype(np.int64) - 1 != ref)[:10])
    if expect_x1 is not None:
        assert r["x1"] == expect_x1, (what, mode)
    assert r["cn"] == pytest.approx(nm.cn_of(C), rel=2e-5)
    assert r["dc"] == (pytest.approx(nm.dc_of(C), rel=1e-4) if r["x1"] else 0.0)
    model, upper = nm.margins(X, r["cn"], r["dc"])
    fin = np.isfinite(model)
    assert np.array_equal(np.isfinite(r["margin"]), fin)
    assert np.all(r["margin"][fin] <= upper[fin] * (1 + 1e-5)), (what, mode)        # a margin inflated by a stray factor fails here
    assert r["margin"][fin] == pytest.approx(model[fin], rel=1e-4), (what, mode)     # ... and one that lost a term here
    W = nm.scores(C, X, mode)
    r["worst"] = nm.check_lists(r["vals"], r["gids"], r["margin"], nm.group_maxima(W, C.shape[1]))
    assert np.all(r["tier"] <= nm.TIER_EXHAUSTIVE)
    assert np.all(r["tier"][~fin] != nm.TIER_LISTS)                 # no finite margin (a component beyond fp16): never the lists
    assert r["undecided1"] == np.count_nonzero(r["tier"] != nm.TIER_LISTS)
    assert r["tier2_points"] >= r["undecided2"] and np.count_nonzero(r["tier"] == nm.TIER_SECOND) == r["tier2_points"] - r["undecided2"]
    if ties:
        at = np.flatnonzero(r["tier"] == nm.TIER_LISTS)
        tied = dict(zip(at, nm.canonical_ties(oracle, C, X[:, at], mode, W[:, at])))
        assert all(tied[p][0] == ref[p] for p in at)
        nm.check_decisions(r["vals"], r["gids"], r["margin"], r["tier"], tied)
    print(f"{what} mode {mode}: worst |v - W| / (margin / 2) = {r['worst']:.3f}; undecided {r['undecided1']}, "
          f"second tier {r['tier2_points']} -> {r['undecided2']}, chunks {r['chunks']}, x1 {r['x1']}")
    return r


# ---- (a) + (c): lists, margin, decisions on the near-tie data ---------------------------------------------------------------------
@pytest.mark.parametrize("products", [1, 3])
@pytest.mark.parametrize("scale", [1.0, 50.0, 2.0e-3, 1.0e3])
def test_lists_lie_in_the_models_interval_and_the_margin_is_the_models(oracle, products, scale):
    """Every listed value within margin / 2 of the float64 group maximum, each half ordered, nothing better left out; the kernel's
    margin equals the model's formula and stays below it at the worst conversion error fp16 allows (dq = 2^-11 ||x||)."""
    C, X = nm.near_ties(scale)
    for mode in MODES:
        run_and_check(oracle, C, X, mode, f"near ties x{scale:g} products {products}", expect_x1=products == 1 and scale != 1.0e3,
                      products=products)


# ---- (b): coherent rounding ---------------------------------------------------------------------------------------------------------
def listed(r, p, c):
    g = int(nm.group_of(c))
    at = np.flatnonzero(r["gids"][p, g & 1] == g)
    return float(r["vals"][p, g & 1, at[0]]) if at.size else None


def check_coherent(oracle, C, X, a, b, mode, what):
    r = run_and_check(oracle, C, X, mode, what, expect_x1=True)
    assert np.array_equal(r["codes"].astype(np.int64) - 1, a)
    for p in range(X.shape[1]):
        va, vb = listed(r, p, a[p]), listed(r, p, b[p])
        assert vb is not None and (va is None or vb > va), (what, p, va, vb)       # the lists DO put b above a: not vacuous
        g1 = max(r["vals"][p, 0, 0], r["vals"][p, 1, 0])
        assert (va is not None and va >= g1 - r["margin"][p]) or r["tier"][p] != nm.TIER_LISTS, (what, p, va, g1, r["margin"][p])
    return r


@pytest.mark.parametrize("mode", MODES)
def test_coherent_rounding_of_the_points(oracle, mode):
    """Every component of x rounds against c_a and for c_b: the error of a's value is 0.87 of dq ||c_a||, the fp16 product puts b
    2.2e-3 ahead of a winner that leads by 3e-5 -- the dq cn term of the margin must bring a's group back."""
    C, X, a, b = nm.coherent_points()
    check_coherent(oracle, C, X, a, b, mode, "coherent points")


def test_coherent_rounding_of_the_points_with_large_norms(oracle):
    """MODE 1, centroid norms of 58: the accumulators start at -||c||^2 / 2 = -1 700 and the bias term of the margin matters"""
    C, X, a, b = nm.coherent_points(64.0)
    assert 30 < np.linalg.norm(C[:, a[0]].astype(np.float64)) < 60
    check_coherent(oracle, C, X, a, b, 1, "coherent points, norms x64")


@pytest.mark.parametrize("mode", MODES)
def test_coherent_rounding_of_the_centroids(oracle, mode):
    """The roles swapped: fp16-exact points, every component of c_a rounds down and of c_b up -- the error of a's value IS
    ||x|| ||c_a - fp16 c_a||, the xn dc term."""
    C, X, a, b = nm.coherent_centroids()
    check_coherent(oracle, C, X, a, b, mode, "coherent centroids")


# ---- (d): tiers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_well_spread_data_is_decided_from_the_first_lists(oracle, mode):
    C, X = nm.well_spread()
    r = run_and_check(oracle, C, X, mode, "well spread", expect_x1=True)
    assert r["undecided1"] == 0 and r["tier2_points"] == 0 and r["undecided2"] == 0 and r["chunks"] == 1
    assert np.all(r["tier"] == nm.TIER_LISTS)


@pytest.mark.parametrize("sitters", [1, 40, 64])
@pytest.mark.parametrize("mode", MODES)
def test_a_few_undecided_points_go_straight_to_the_exhaustive_scan(oracle, mode, sitters):
    C, X, sit, dup = nm.few_undecided(sitters)
    r = run_and_check(oracle, C, X, mode, f"{sitters} sitters", expect_x1=True)
    assert r["undecided1"] == sitters and r["tier2_points"] == 0 and r["undecided2"] == 0
    assert np.array_equal(np.flatnonzero(r["tier"] == nm.TIER_EXHAUSTIVE), sit) and np.all(np.delete(r["tier"], sit) == nm.TIER_LISTS)
    assert np.all(r["codes"][sit] == dup[0] + 1)                    # the first of the five copies


@pytest.mark.parametrize("mode", MODES)
def test_more_undecided_points_go_through_the_second_tier(oracle, mode):
    """80 undecided points: 50 near ties the three-product lists decide, 30 on a five-fold centroid that only the scan decides"""
    C, X, near, sit, info = nm.second_tier(mode)
    r = run_and_check(oracle, C, X, mode, "second tier", expect_x1=True)
    assert (r["undecided1"], r["tier2_points"], r["undecided2"]) == (near.size + sit.size, near.size + sit.size, sit.size)
    assert np.array_equal(r["tier"], nm.predict_tiers(C, X, mode))
    assert np.all(r["codes"][near] == info["slots"][0] + 1) and np.all(r["codes"][sit] == info["dup"][0] + 1)


@pytest.mark.parametrize("mode", MODES)
def test_three_products_when_asked_for_or_forced_by_the_centroids(oracle, mode):
    C, X, sit, dup = nm.few_undecided(40)
    r = run_and_check(oracle, C, X, mode, "three products asked for", expect_x1=False, products=3)
    assert r["dc"] == 0.0 and r["tier2_points"] == 0                 # no second tier behind three-product lists
    assert np.array_equal(np.flatnonzero(r["tier"] == nm.TIER_EXHAUSTIVE), sit)
    C = C.copy(); C[5, 77] = np.float32(7.0e4)
    r = run_and_check(oracle, C, X, mode, "a centroid component of 7e4", expect_x1=False)
    assert r["dc"] == 0.0 and r["tier2_points"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_a_point_beyond_the_fp16_range_is_scored_exactly(oracle, mode):
    C, X = nm.well_spread()
    X = X.copy(); X[9, 123] = np.float32(7.0e4); X[:, 500] *= np.float32(1.0e6)
    r = run_and_check(oracle, C, X, mode, "points beyond fp16", expect_x1=True)
    assert np.array_equal(np.flatnonzero(r["tier"] != nm.TIER_LISTS), [123, 500]) and np.all(np.isinf(r["margin"][[123, 500]]))
    assert np.all(r["tier"][[123, 500]] == nm.TIER_EXHAUSTIVE)


# ---- (e): chunks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_chunk_loop_offsets_and_second_tier_reuse(oracle, mode):
    """n = 2 * 4 096 + 37 with undecided points in every chunk, the tail included.  chunk_max = 4 096: 150 (second tier), 20 and 5
    (the direct scan).  Two chunks above 64 AND one below between them do not fit into two chunks and a tail, so the same input
    also runs at chunk_max = 1 024: 70 (second tier, its planes built), 10 (direct), 70 (second tier again, planes reused), ...
    Codes, tiers, lists and margins equal those of one chunk of the shipped size."""
    C, X, near, sit, info = nm.chunked(mode)
    n = X.shape[1]
    whole = run_and_check(oracle, C, X, mode, "chunks: shipped chunk_max", expect_x1=True, ties=False)
    assert whole["chunks"] == 1 and whole["tier2_points"] == near.size + sit.size and whole["undecided2"] == sit.size
    assert np.array_equal(whole["tier"], nm.predict_tiers(C, X, mode))
    und = np.sort(np.concatenate([near, sit]))
    for cm in (4096, 1024):
        r = codec.debug_nearest(C, X, mode=mode, chunk_max=cm)
        per = nm.undecided_per_chunk(n, cm, und)
        assert r["chunks"] == per.size == -(-n // cm)
        assert r["undecided1"] == per.sum() and r["tier2_points"] == per[per > nm.SECOND_TIER_ABOVE].sum()
        assert r["undecided2"] == sum(np.count_nonzero((sit >= e) & (sit < e + cm)) for e, k in zip(range(0, n, cm), per)
                                      if k > nm.SECOND_TIER_ABOVE)
        for key in ("codes", "tier", "vals", "gids", "margin"):
            assert np.array_equal(r[key], whole[key]), (cm, key)


# ---- (f): ring and tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 33, 64, 65, 96, 97, 128])
def test_ring_and_tile_edges(oracle, K):
    """1 to 4 centroid tiles through the three-buffer ring (a partial last tile at K = 33, 65, 97), point counts around the 32-point
    group, the 512-point work-group and a last group with one live row"""
    rng = np.random.default_rng(K)
    C = nm.unit(rng, K)
    for n in (1, 31, 32, 33, 511, 512, 513, 2049):
        X = nm.unit(rng, n)
        X[:, : min(n, K) : 3] = C[:, : min(n, K) : 3]
        for mode in MODES:
            r = run_and_check(oracle, C, X, mode, f"K {K} n {n}", expect_x1=True)
            assert r["chunks"] == 1


@pytest.mark.parametrize("K", [1, 2, 31])
def test_small_K_takes_the_fp32_mfma_kernel(oracle, K):
    rng = np.random.default_rng(100 + K)
    C = nm.unit(rng, K)
    for n in (1, 63, 64, 65):
        X = nm.unit(rng, n)
        for mode in MODES:
            r = codec.debug_nearest(C, X, mode=mode)
            assert np.array_equal(r["codes"].astype(np.int64) - 1, nm.oracle_winners(oracle, C, X, mode)), (K, n, mode)
            assert r["chunks"] == 0 and np.all(r["tier"] == 255) and np.all(r["gids"] == -1)      # no lists below 32 centroids


@pytest.mark.parametrize("K", [1100, 2080])
def test_sliced_exhaustive_scan(oracle, K):
    """40 points on a five-fold centroid: the scan deals the 35 (65) centroid tiles to 4 (8) work-groups per point tile, the
    last one with fewer tiles than the others"""
    C, X, sit, dup = nm.few_undecided(40, K=K, n=300, seed=K)
    for mode in MODES:
        r = run_and_check(oracle, C, X, mode, f"sliced scan K {K}", expect_x1=True)
        assert r["undecided1"] == 40 and r["tier2_points"] == 0 and np.all(r["codes"][sit] == dup[0] + 1)


# ---- (g): the scratch k-means keeps across its iterations ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_scratch_reuse_across_calls_with_moved_centroids(oracle, mode):
    """Call 1 uses the second tier (its bf16 planes of call 1's centroids stay in the scratch); call 2, same K, moved centroids, must
    equal a call on a fresh scratch bit for bit -- lists, margins, tiers and counts included.  The centroids move by one tile (32
    columns on, same halves): the same 80 points need the second tier again, and lists made from call 1's planes would name the
    groups the crafted centroids have left."""
    C1, X, near, sit, info = nm.second_tier(mode)
    C2 = np.asfortranarray(np.roll(C1, 32, axis=1))
    fresh = run_and_check(oracle, C2, X, mode, "moved centroids, fresh scratch", expect_x1=True, ties=False)
    assert (fresh["tier2_points"], fresh["undecided2"]) == (near.size + sit.size, sit.size)
    assert np.all(fresh["codes"][near] == (info["slots"][0] + 32) % C1.shape[1] + 1)
    with codec.NearestScratch() as scratch:
        first = codec.debug_nearest(C1, X, mode=mode, scratch=scratch)
        assert first["tier2_points"] == near.size + sit.size
        again = codec.debug_nearest(C2, X, mode=mode, scratch=scratch)
    for key, v in fresh.items():
        if key != "worst":
            assert np.array_equal(again[key], v), key
