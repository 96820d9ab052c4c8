"""tests/nearest_model.py against the CPU oracle, and the property each crafted input of tests/test_gpu_nearest_model.py is built
for -- gap sizes, which points must and must not overflow their lists, nothing in between -- so that what the device test asserts
about tiers and counts rests on the reference alone.  No device."""
import numpy as np
import pytest

from tests import nearest_model as nm


oracle_codes = nm.oracle_winners


def assert_model_is_the_oracle(orc, C, X, what):
    for mode in (0, 1):
        assert np.array_equal(nm.winners(nm.scores(C, X, mode)), oracle_codes(orc, C, X, mode)), (what, mode)


def test_group_map():
    """gid = 2 tile + h holds 32 tile + (s & 3) + 8 (s >> 2) + 4 h: every centroid in exactly one group, 16 per full group"""
    for K in (1, 31, 32, 33, 97, 2080):
        seen = np.concatenate([nm.group_members(g, K) for g in range(nm.n_groups(K))])
        assert np.array_equal(np.sort(seen), np.arange(K))
        for g in range(nm.n_groups(K)):
            mem = nm.group_members(g, K)
            assert np.all(nm.group_of(mem) == g) and (len(mem) == 16 or 32 * (g >> 1) + 32 > K)
    assert list(nm.group_members(5, 1000)) == [68, 69, 70, 71, 76, 77, 78, 79, 84, 85, 86, 87, 92, 93, 94, 95]


def test_margin_constants():
    """the formula at unit vectors: three products 2.5 * 7.4e-5 + 1.2e-5; one product adds both conversion terms, the
    accumulation and the bias term; the single-product arm is the larger one as soon as dc > 0 is of fp16 size"""
    assert nm.margin_of(1.0, 0.0, 1.0, 0.0) == pytest.approx(2.5 * 7.4e-5 + 1.2e-5, rel=1e-12)
    m1 = nm.margin_of(1.0, 3e-4, 1.0, 2e-4)
    assert m1 == pytest.approx(2.5 * (1.001 * (3e-4 * 1.0005 + 2e-4) + 384 * 2.0 ** -24) + 1.2e-5 + 1.6e-5, rel=1e-12)
    assert nm.margin_of(1.0, 0.0, 1.0, 1e-30) == pytest.approx(2.5 * 7.4e-5 + 1.2e-5 + 1.6e-5, rel=1e-12)    # the max of the two arms
    x = np.full((128, 1), 7.0e4)
    assert np.isinf(nm.margins(x, 1.0, 1e-4)[0][0]) and np.isfinite(nm.margins(x, 1.0, 0.0)[0][0])
    assert nm.dc_of(np.full((128, 2), 7.0e4)) == np.inf and nm.dc_of(np.ones((128, 2))) == 1e-30


@pytest.mark.parametrize("K", [32, 33, 97, 512])
def test_the_list_check_accepts_exact_lists_and_rejects_wrong_ones(K):
    """check_lists itself: the lists of an error-free kernel pass with ratio ~0; a value off by more than margin / 2, a list out of
    order, a group of the other half, a repeated group and a better group left out are each refused"""
    rng = np.random.default_rng(K)
    C, X = nm.unit(rng, K), nm.unit(rng, 70)
    G = nm.group_maxima(nm.scores(C, X, 0), K)
    vals, gids = nm.ideal_lists(G)
    margin = np.full(70, 2e-4, dtype=np.float32)
    assert nm.check_lists(vals, gids, margin, G) < 1e-3            # (fp32 storage of the values)
    p, h = 3, 0

    def refused(v, g):
        with pytest.raises(AssertionError):
            nm.check_lists(v, g, margin, G)

    v = vals.copy(); v[p, h, 0] += 1.5e-4; refused(v, gids)                                  # value outside margin / 2
    if K >= 97:                                                    # (needs two live entries per half)
        v, g = vals.copy(), gids.copy()
        v[p, h, :2] = v[p, h, 1::-1]; g[p, h, :2] = g[p, h, 1::-1]; refused(v, g)           # ascending
        g = gids.copy(); g[p, h, 1] = g[p, h, 0]; refused(vals, g)                           # the same group twice
    g = gids.copy(); g[p, h, 0] = gids[p, 1, 0]; refused(vals, g)                            # a group of the other half
    if K == 512:                                                   # the best group replaced by the fifth: an unlisted one above the list
        fifth = 2 * int(np.argsort(-G[0::2, p])[4])
        v, g = vals.copy(), gids.copy()
        v[p, h, :3] = vals[p, h, 1:]; g[p, h, :3] = gids[p, h, 1:]; v[p, h, 3] = G[fifth, p]; g[p, h, 3] = fifth
        refused(v, g)
    if K == 33:                                                    # an open slot although a group of the half is not listed
        v, g = vals.copy(), gids.copy()
        assert g[p, 0, 1] != nm.EMPTY and g[p, 0, 2] == nm.EMPTY
        v[p, 0, 1] = -np.inf; g[p, 0, 1] = nm.EMPTY; refused(v, g)
    margin[p] = np.inf                                             # a point without a finite margin is not judged
    v = vals.copy(); v[p, h, 0] += 1.0
    nm.check_lists(v, gids, margin, G)


@pytest.mark.parametrize("scale", [1.0, 50.0, 2.0e-3, 1.0e3])
def test_near_ties_model_against_oracle(oracle, scale):
    """Gaps down to 1e-7 lie below what the canonical fp32 chain resolves, so float64 and the oracle may name different winners
    there -- only there: where they differ the float64 scores are within twice the chain's 128 * 2^-24 ||x|| ||c|| (MODE 1: plus
    the two roundings of the distance) of each other."""
    C, X = nm.near_ties(scale)
    for mode in (0, 1):
        W = nm.scores(C, X, mode)
        mine, ref = nm.winners(W), oracle_codes(oracle, C, X, mode)
        xn = np.linalg.norm(X.astype(np.float64), axis=0)
        cn = np.linalg.norm(C.astype(np.float64), axis=0).max()
        tol = 2 * (128 * nm.U * xn * cn + (2 * nm.U * (xn + cn) ** 2 if mode else 0.0))
        p = np.flatnonzero(mine != ref)
        assert p.size < 0.2 * X.shape[1]
        assert np.all(W[mine[p], p] - W[ref[p], p] <= tol[p]), (scale, mode)
        # ... and the oracle's winner is among the centroids canonical_ties finds (the device test's decision invariant uses them)
        sub = np.arange(0, X.shape[1], 25)
        tied = nm.canonical_ties(oracle, C, X[:, sub], mode, W[:, sub])
        assert all(t[0] == ref[q] for t, q in zip(tied, sub)), (scale, mode)


def coherent_facts(C, X, a, b, mode):
    C64, X64 = C.astype(np.float64), X.astype(np.float64)
    W = nm.scores(C64, X64, mode)
    W16 = nm.scores(nm.f16(C64), nm.f16(X64), 0)                   # the product of the rounded operands ...
    if mode == 1:
        W16 = W16 - 0.5 * np.sum(C64 * C64, axis=0)[:, None]       # ... started at the bias of the UNROUNDED centroid
    p = np.arange(X.shape[1])
    return W, W[a, p] - W[b, p], W16[a, p] - W16[b, p], np.abs(W16[a, p] - W[a, p])


@pytest.mark.parametrize("scale,modes", [(1.0, (0, 1)), (64.0, (1,))])
def test_coherent_points_are_what_they_claim(oracle, scale, modes):
    C, X, a, b = nm.coherent_points(scale)
    assert np.all(nm.group_of(a) != nm.group_of(b))
    assert nm.dc_of(C) == 1e-30                                    # every centroid fp16-exact: the dq cn term stands alone
    norms = np.linalg.norm(C.astype(np.float64), axis=0)
    assert norms.max() == pytest.approx(0.91 * scale, rel=0.01)
    xn, dq, _ = nm.point_norms(X)
    m, _ = nm.margins(X, nm.cn_of(C), nm.dc_of(C))
    for mode in modes:
        W, gap, gap16, err_a = coherent_facts(C, X, a, b, mode)
        assert np.array_equal(nm.winners(W), a) and np.array_equal(oracle_codes(oracle, C, X, mode), a)
        assert np.all(gap > 0) and np.all(gap16 < 0) and np.all(gap < -gap16)          # a wins; fp16 puts b first, by more
        assert np.all(gap == pytest.approx(3.0e-5 * scale * scale, rel=0.02))
        assert np.all(err_a >= 0.85 * (dq / 1.001) * norms[a]) and np.all(err_a <= 0.5 * m)   # the bound nearly attained, and kept
        assert np.all(-gap16 < m)                                  # so a's group stays inside the margin: decided, and decided right
        drop = 2.0 * nm.EPS_SAFETY * 384 * nm.U * xn * nm.cn_of(C) + nm.slack_of(xn, nm.cn_of(C), 1e-30)
        assert np.all(-gap16 > 2 * drop)                           # a margin WITHOUT the dq cn term leaves a's group out
    assert_model_is_the_oracle(oracle, C, X, "coherent points") if scale == 1.0 else None


def test_coherent_centroids_are_what_they_claim(oracle):
    C, X, a, b = nm.coherent_centroids()
    assert np.all(nm.group_of(a) != nm.group_of(b))
    xn, dq, _ = nm.point_norms(X)
    assert np.all(dq == 0)                                         # the points are fp16-exact: the xn dc term stands alone
    cn, dc = nm.cn_of(C), nm.dc_of(C)
    m, _ = nm.margins(X, cn, dc)
    for mode in (0, 1):
        W, gap, gap16, err_a = coherent_facts(C, X, a, b, mode)
        assert np.array_equal(nm.winners(W), a) and np.array_equal(oracle_codes(oracle, C, X, mode), a)
        assert np.all(gap > 0) and np.all(gap16 < 0) and np.all(gap < -gap16)
        dca = np.linalg.norm((C - nm.f16(C).astype(np.float32)).astype(np.float64), axis=0)[a]
        assert np.all(err_a >= 0.99 * (xn / 1.001) * dca) and np.all(err_a <= 0.5 * m)
        assert np.all(-gap16 < m)
        drop = 2.0 * nm.EPS_SAFETY * 384 * nm.U * xn * cn + nm.slack_of(xn, cn, dc)
        assert np.all(-gap16 > 2 * drop)                           # a margin without the xn dc term leaves a's group out


def group_gap(C, X, mode):
    G = np.sort(nm.group_maxima(nm.scores(C, X, mode), C.shape[1]), axis=0)
    return G[-1] - G[-2]


def test_well_spread_is_well_spread(oracle):
    C, X = nm.well_spread()
    assert 0 < nm.dc_of(C) < 1e-3
    for mode in (0, 1):
        assert group_gap(C, X, mode).min() > 0.25
        assert np.all(nm.predict_tiers(C, X, mode) == nm.TIER_LISTS)
    assert_model_is_the_oracle(oracle, C, X, "well spread")


@pytest.mark.parametrize("sitters,kw", [(1, {}), (40, {}), (64, {}), (40, dict(K=1100, n=300, seed=1100)),
                                        (40, dict(K=2080, n=300, seed=2080))])
def test_few_undecided_input(oracle, sitters, kw):
    C, X, sit, dup = nm.few_undecided(sitters, **kw)
    assert len(set((dup // 32).tolist())) == 5 and np.all(nm.group_of(dup) % 2 == 0) and sit.size == sitters <= nm.SECOND_TIER_ABOVE
    others = np.setdiff1d(np.arange(X.shape[1]), sit)
    for mode in (0, 1):
        W = nm.scores(C, X, mode)
        assert np.all(nm.winners(W)[sit] == dup[0])
        assert np.all(W[dup][:, sit] == W[dup[0], sit])            # five groups with the same maximum, exactly
        assert group_gap(C, X[:, others], mode).min() > 0.25
        tier = nm.predict_tiers(C, X, mode)                        # (as if the second tier ran: it does not, below 65 points)
        assert np.all(tier[sit] == nm.TIER_EXHAUSTIVE) and np.all(tier[others] == nm.TIER_LISTS)
    assert_model_is_the_oracle(oracle, C, X, "few undecided")


def check_second_tier_input(orc, C, X, near, sit, info, mode):
    lo, hi = info["zone"]
    assert 0 < lo < info["gap"] <= hi, info
    assert np.all(nm.group_of(info["slots"]) % 2 == 0) and len(set(nm.group_of(info["slots"]).tolist())) == 4
    assert np.all(nm.point_norms(X[:, near])[1] == 0)              # the near-tie points are fp16-exact
    assert np.unique(X[:, near], axis=1).shape[1] == near.size     # and all different
    tier = nm.predict_tiers(C, X, mode)
    assert np.all(tier >= 0)                                       # nobody in the grey zone
    assert np.array_equal(np.flatnonzero(tier == nm.TIER_SECOND), near)
    assert np.array_equal(np.flatnonzero(tier == nm.TIER_EXHAUSTIVE), sit)
    win = nm.winners(nm.scores(C, X, mode))
    assert np.all(win[near] == info["slots"][0]) and np.all(win[sit] == info["dup"][0])
    assert np.array_equal(win, oracle_codes(orc, C, X, mode))
    return tier


@pytest.mark.parametrize("mode", [0, 1])
def test_second_tier_input(oracle, mode):
    C, X, near, sit, info = nm.second_tier(mode)
    check_second_tier_input(oracle, C, X, near, sit, info, mode)
    assert near.size + sit.size > nm.SECOND_TIER_ABOVE and 0 < sit.size < near.size + sit.size


@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_input(oracle, mode):
    C, X, near, sit, info = nm.chunked(mode)
    n = X.shape[1]
    assert n == 2 * 4096 + 37
    check_second_tier_input(oracle, C, X, near, sit, info, mode)
    und = np.sort(np.concatenate([near, sit]))
    assert list(nm.undecided_per_chunk(n, 4096, und)) == [150, 20, 5]            # second tier, the direct scan twice
    per = nm.undecided_per_chunk(n, 1024, und)
    assert list(per[:3]) == [70, 10, 70] and per[-1] == 5 and per.sum() == 175   # second tier, direct scan, second tier AGAIN
    # a near tie only ever shares a chunk with more than 64 undecided points: its tier is the same at every chunk size
    for cm in (1024, 4096, n):
        per = nm.undecided_per_chunk(n, cm, und)
        assert np.all(per[near // cm] > nm.SECOND_TIER_ABOVE)


def test_hook_is_declared_exported_and_checks_its_arguments_without_a_device():
    import ctypes as C
    import colbert_jl_amd as clb
    l = clb.lib()
    for name in ("clb_debug_nearest", "clb_debug_nearest_scratch_create", "clb_debug_nearest_scratch_destroy"):
        assert name in clb.declared_symbols() and hasattr(l, name), name
    x = np.zeros(128 * 64, dtype=np.float32)
    p, i64 = C.c_void_p(x.ctypes.data), C.c_int64
    ok = dict(mode=0, products=-1, chunk_max=1 << 22, K=64, n=1)
    for bad in (dict(mode=2), dict(products=2), dict(chunk_max=0), dict(K=0), dict(n=0)):
        a = {**ok, **bad}
        assert l.clb_debug_nearest(0, a["mode"], a["products"], i64(a["chunk_max"]), p, i64(a["K"]), p, i64(a["n"]), None, p, p, p, p, p) == 4, bad
    assert l.clb_debug_nearest(0, 0, -1, i64(1 << 22), p, i64(64), p, i64(1), None, p, p, p, p, None) == 4          # a null output
    assert l.clb_debug_nearest_scratch_create(0, None) == 4 and l.clb_debug_nearest_scratch_destroy(None) == 0
