"""The selection model (tests/selection_model.py) against itself, and the inputs of tests/test_gpu_selection_keys.py against
the oracle: every input really puts in front of the kernels what its name says, and ranking it with a wrong key (the float's
bits taken as unsigned; the sign dropped) changes a top k the GPU tests compare -- so those tests would fail for such a
kernel.  No kernel code runs here."""
import numpy as np
import pytest

from tests import selection_model as sm
from tests import util_selection as us
from tests.util_prior import boosted_ranking

WRONG_KEYS = (sm.wrong_key_unsigned_bits, sm.wrong_key_magnitude)


def every_class():
    """float32 values of every sign / exponent class, ascending: -Inf, -FLT_MAX .. the negative subnormals, -0.0, +0.0, the
    positive subnormals .. FLT_MAX, +Inf; three mantissas per exponent"""
    mant = np.array([0, 1, 0x7fffff], np.uint32)
    pos = (np.arange(0, 255, dtype=np.uint32)[:, None] << np.uint32(23) | mant[None, :]).reshape(-1)
    pos = np.concatenate([pos, np.array([0x7f800000], np.uint32)])             # +0.0, subnormals, normals, +Inf
    neg = (pos | sm.SIGN)[::-1]
    return np.concatenate([neg, pos]).view(np.float32)


# ---- the model --------------------------------------------------------------------------------------------------------------
def test_keys_are_monotone_over_every_class_and_invert_bit_for_bit():
    x = every_class()
    assert np.isneginf(x[0]) and np.isposinf(x[-1]) and x.size == 2 * (255 * 3 + 1)
    assert np.all(x[1:] >= x[:-1])
    key = sm.order_key(x)
    assert key.dtype == np.uint32 and np.all(key[1:] > key[:-1])               # strictly: the two zeros differ
    mz, pz = sm.order_key(np.array([-0.0, 0.0], np.float32))
    assert mz == 0x7fffffff and pz == 0x80000000                               # -0.0 the lower key
    assert np.array_equal(sm.from_order_key(key).view(np.uint32), x.view(np.uint32))
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    ok = ~np.isnan(f)
    assert np.array_equal(sm.from_order_key(sm.order_key(f)).view(np.uint32), bits)
    a, b = f[ok][:-1], f[ok][1:]
    ne = a != b
    assert np.array_equal((a < b)[ne], (sm.order_key(a) < sm.order_key(b))[ne])
    # the two wrong keys are wrong: each misorders a pair the right key orders
    for wrong in WRONG_KEYS:
        assert wrong(np.float32([-2.0]))[0] > wrong(np.float32([-1.0]))[0]


def test_schedule_reads_every_bit_below_the_highest_differing_one_in_at_most_four_digits():
    for top in range(32):
        for diff in {1 << top, (1 << (top + 1)) - 1, (1 << top) | 1}:
            sched = sm.digit_schedule(diff)
            assert 1 <= len(sched) <= 4
            assert sched[0][0] + sched[0][1] == top + 1 and sched[-1][0] == 0
            assert all(1 <= w <= 8 for _, w in sched)
            assert all(a[0] == b[0] + b[1] for a, b in zip(sched, sched[1:]))          # contiguous, no bit twice
    assert sm.digit_schedule(0x80000000) == [(24, 8), (16, 8), (8, 8), (0, 8)]         # keys of both signs: four full digits
    assert sm.digit_schedule(0x00012345) == [(9, 8), (1, 8), (0, 1)]
    assert sm.digit_schedule(0x5) == [(0, 3)]


@pytest.mark.parametrize("kind", ["positive", "negative", "both_signs", "zeros_and_negatives", "all_equal"])
def test_coarse_value_is_a_lower_bound_inside_the_kth_bin(kind):
    rng = np.random.default_rng(5)
    x = {"positive": rng.uniform(2, 4, 3000), "negative": -rng.uniform(2, 40, 3000),
         "both_signs": rng.choice([-1.0, 1.0], 3000) * np.exp2(rng.uniform(-20, 20, 3000)),
         "zeros_and_negatives": np.concatenate([np.zeros(50), -rng.uniform(0, 1e-3, 2950)]),
         "all_equal": np.full(3000, -0.375)}[kind].astype(np.float32)
    keys = sm.order_key(x)
    n_digits = 0 if kind == "all_equal" else len(sm.digit_schedule(int(keys.min()) ^ int(keys.max())))
    assert n_digits == {"both_signs": 4, "zeros_and_negatives": 4, "all_equal": 0}.get(kind, n_digits)
    for k in (1, 2, 10, 1000, 3000):
        kth = np.sort(x)[::-1][k - 1]
        assert sm.select_value(x, k).view(np.uint32) == kth.view(np.uint32)
        prev = None
        for limit in (1, 2, 3, 4):
            v = sm.select_value(x, k, limit)
            assert not np.isnan(v) and v <= kth
            assert prev is None or v >= prev                                       # more digits: never a lower edge
            assert np.count_nonzero(x >= v) >= k
            if limit >= n_digits:
                assert v.view(np.uint32) == kth.view(np.uint32)
            prev = v
    if kind == "zeros_and_negatives":      # the bin of +0.0 has no float below it with the sign bit clear: the edge is +0.0 itself
        assert sm.select_value(x, 10, 2).view(np.uint32) == 0


def test_the_float_comparison_gives_two_records_one_place_when_a_list_holds_both_zeros():
    """two shard results as the top-k kernels sort them (+0.0 before -0.0): ranked by the float comparison two records land on
    one place and one place stays empty; ranked by the order key every record has a place of its own, +0.0 first"""
    mz, pz = np.float32(-0.0), np.float32(0.0)
    lists = [[(5, pz), (1, mz)], [(3, pz), (2, mz)]]
    by_float = [r[0] for r in sm.rank_merge(lists, 4, sm.before_by_float)]
    assert sorted(by_float) != [0, 1, 2, 3]
    by_key = sm.rank_merge(lists, 4, sm.before_by_key)
    assert [r[0] for r in by_key] == [0, 1, 2, 3] and [r[1] for r in by_key] == [3, 5, 1, 2]
    want = sm.rank_by_key([5, 1, 3, 2], [pz, mz, pz, mz])
    assert want[0].tolist() == [3, 5, 1, 2]


# ---- the inputs of the GPU tests, from the oracle alone -----------------------------------------------------------------------
def top_differs(ranking, k, wrong):
    rp, rs = ranking
    if rp.size <= k:
        return False
    return not np.array_equal(sm.rank_by_key(rp, rs, wrong)[0][:k], rp[:k])


def test_the_reference_ranks_by_the_order_key(oracle):
    for index_name, name in (("medium_shifted", "negated"), ("short", "straddle"), ("medium", "zero")):
        for rp, rs in us.rankings(oracle, index_name, name)[:3]:
            kp, ks = sm.rank_by_key(rp, rs)
            assert np.array_equal(kp, rp) and np.array_equal(ks.view(np.uint32), rs.view(np.uint32))


def test_negating_a_query_leaves_its_scores_positive_on_the_unshifted_index(oracle):
    """the reason for `shifted`: MaxSim's maximum over the rows of a passage finds a positive product for -Q as well"""
    for name in ("negated", "straddle"):
        for rp, rs in us.rankings(oracle, "medium", name)[:3]:
            assert rs.size > 1000 and rs.min() > 0


@pytest.mark.parametrize("T", [4, 32])
def test_negated_queries_have_negative_scores(oracle, T):
    r = us.rankings(oracle, "medium_shifted", "negated", T)
    for k in us.KS:
        assert sum(1 for rp, rs in r if rs.size >= k and rs[k - 1] < 0) * 2 >= len(r)
    assert all(rs.max() < 0 for _, rs in r)                    # in fact every score of every query
    for wrong in WRONG_KEYS:
        assert any(top_differs(x, k, wrong) for x in r for k in us.KS)
    one_hot = us.rankings(oracle, "medium_shifted", "one_hot_zero", T)
    assert all(rs.min() > 0 for _, rs in one_hot[0::3]) and all(rs.max() < 0 for _, rs in one_hot[2::3])
    assert all(np.all(rs.view(np.uint32) == 0) for _, rs in one_hot[1::3])
    for wrong in WRONG_KEYS:
        assert any(top_differs(x, k, wrong) for x in one_hot for k in us.KS)


@pytest.mark.parametrize("T", [4, 32])
def test_straddling_queries_have_candidates_on_both_sides_of_zero(oracle, T):
    r = us.rankings(oracle, "short", "straddle", T)
    assert all(rs[0] > 0 > rs[-1] for _, rs in r)
    # the k-th place lies below zero and the first above it: for a tested k, in at least a third of the queries
    assert sum(1 for _, rs in r if any(rs.size >= k and rs[0] > 0 > rs[k - 1] for k in us.KS)) * 3 >= len(r)
    e = np.concatenate([us.exponents(rs) for _, rs in r])
    assert e.max() - e.min() >= 8                              # many exponents: the first digit is not the mantissa's
    for wrong in WRONG_KEYS:
        assert any(top_differs(x, k, wrong) for x in r for k in us.KS)


def test_a_zero_query_scores_every_candidate_plus_zero(oracle):
    for index_name in ("medium", "medium_shifted"):
        for rp, rs in us.rankings(oracle, index_name, "zero"):
            assert rs.size > 10 and np.all(rs.view(np.uint32) == 0)
            assert np.all(np.diff(rp) > 0)                     # the expected result: pids ascending
            # all keys equal: neither wrong key can change this ranking, nothing here is sensitive to them
            assert all(not top_differs((rp, rs), k, wrong) for wrong in WRONG_KEYS for k in (1, 10))


def test_the_large_index_gives_more_candidates_than_one_work_group_caches(oracle):
    for name in ("negated", "straddle", "zero"):
        r = us.rankings(oracle, "large", name, 32, us.LARGE_NPROBE)[:3]
        assert all(rp.size > 32_768 for rp, _ in r)
        if name == "negated":
            assert all(rs.max() < 0 for _, rs in r)
            for wrong in WRONG_KEYS:
                assert all(top_differs(x, k, wrong) for x in r for k in (10, 5000, 17000))


def test_cursor_inputs(oracle):
    neg = us.rankings(oracle, "small", "negated")
    assert sum(1 for _, rs in neg if rs.size and rs.max() < 0) * 2 >= len(neg)
    strad = us.rankings(oracle, "small", "straddle")
    assert sum(1 for _, rs in strad if rs.size and rs[0] > 0 > rs[-1]) * 2 >= len(strad)


@pytest.fixture(scope="module")
def medium_plain(oracle):
    return us.rankings(oracle, "medium", "plain")


def test_prior_inputs(oracle, medium_plain):
    r0 = medium_plain[0]
    rp, rs = r0
    n = us.N_MEDIUM
    assert rs.min() > 0 and rp.size > 2 * max(us.PRIOR_KS)
    # mirror: E = -e bit for bit, the ranking reversed (ties aside), everything negative
    mp, mE = boosted_ranking(r0, us.prior_values("mirror", r0, n))
    assert mE.max() < 0 and np.array_equal(np.sort(mE.view(np.uint32)), np.sort((-rs).view(np.uint32)))
    assert mp[0] == rp[-1] and not set(mp[:1000]) & set(rp[:1000])
    # zero_run: positives, a run of +0.0 across rank k cut by pid, negatives
    for k in us.PRIOR_KS:
        zp, zE = boosted_ranking(r0, us.prior_values("zero_run", r0, n, k))
        assert zE[k - 1].view(np.uint32) == 0 and zE[k].view(np.uint32) == 0
        run = np.nonzero(zE == 0)[0]
        assert run[0] == k // 2 and run[-1] == 2 * k and np.all(zE[run].view(np.uint32) == 0)
        assert np.all(np.diff(zp[run]) > 0) and zE[:run[0]].min(initial=np.inf) > 0 and zE[run[-1] + 1:].max() < 0
        assert not np.array_equal(zp[run][:k - k // 2], rp[k // 2:k])          # the cut by pid is not the cut by MaxSim score
    # octaves: on the zero query E = w v exactly
    zero0 = us.rankings(oracle, "medium", "zero")[0]
    for w in (1.0, -1.5):
        op, oE = boosted_ranking(zero0, us.prior_values("octaves", zero0, n), w)
        assert np.ptp(us.exponents(oE[oE > 0])) >= 30 and np.ptp(us.exponents(oE[oE < 0])) >= 30
    # huge: the largest |E| is near FLT_MAX, and the unboosted best is now the worst
    hp, hE = boosted_ranking(r0, us.prior_values("huge", r0, n))
    assert hE[0] > 1e37 and hE[-1] < -1e37 and hp[-1] == rp[0] and np.all(np.isfinite(hE))
    # huge_low: for k = 1000 the k-th boosted score of EVERY query is one ulp above -FLT_MAX, for k <= 100 it is an ordinary one;
    # with M = |that value| the slack delta = 4 * 2^-24 * M (eps left out: it only adds) takes tau - 2 delta to -Inf in fp32
    low = us.prior_values("huge_low", r0, n)
    for r in medium_plain:
        _, lE = boosted_ranking(r, low)
        assert lE[999] == us.LOWEST and lE[99] > 0 and np.isfinite(lE).all()
    with np.errstate(over="ignore"):
        delta = np.float32(4) * np.float32(2.0 ** -24) * np.abs(us.LOWEST)
        assert delta.dtype == np.float32 and np.isneginf(us.LOWEST - np.float32(2) * delta)
        assert np.isfinite(np.float32(10) - np.float32(2) * delta)
    for name, kw, ranking in (("mirror", {}, r0), ("huge_low", {}, r0), ("zero_run", {"k": 10}, r0), ("zero_run", {"k": 1000}, r0), ("octaves", {}, zero0),
                              ("huge", {}, r0)):
        boosted = boosted_ranking(ranking, us.prior_values(name, ranking, n, **kw))
        for wrong in WRONG_KEYS:
            assert any(top_differs(boosted, k, wrong) for k in us.PRIOR_KS), (name, wrong.__name__)


def test_merge_records_are_sorted_and_hold_what_they_should():
    rng = np.random.default_rng(1)
    for kind in us.SCORE_KINDS:
        P, S = us.sorted_lists(rng, 7, 3, 33, kind)
        for l in range(7):
            for b in range(3):
                m = np.count_nonzero(P[l, b] > 0)
                assert np.all(P[l, b, m:] == 0) and np.all(np.isneginf(S[l, b, m:])) and not np.isnan(S[l, b]).any()
                kp, ks = sm.rank_by_key(P[l, b, :m], S[l, b, :m])
                assert np.array_equal(kp, P[l, b, :m])                             # sorted for the kernels' order as well
        live = S[P > 0]
        assert np.signbit(live).any() and not np.any((live == 0) & np.signbit(live))
        mp, ms = us.merged_reference(P, S, 33)
        for b in range(3):
            kp, ks = sm.rank_by_key(P[:, b][P[:, b] > 0], S[:, b][P[:, b] > 0])
            assert np.array_equal(kp[:33], mp[b][:kp.size]) and np.array_equal(ks[:33].view(np.uint32), ms[b][:ks.size].view(np.uint32))
    edges = us.special_scores(rng, 4000, "edges")
    assert {us.FLT_MAX, -us.FLT_MAX} <= set(edges.tolist()) and np.any((edges != 0) & (np.abs(edges) < 2.0 ** -126))
