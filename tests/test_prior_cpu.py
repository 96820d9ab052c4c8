"""Score priors, the part that needs no GPU: the reference helper of tests/util_prior.py against the unboosted references, a
host model of the boosted two-pass cut with its rounding slack (tests/prior_model.py) and its teeth, the C
ABI's new symbols with their argument checks, and the Python keywords."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import prior_model as pm
from tests.test_group_cpu import _NoDevice
from tests.util_filter import filtered_ranking, first_k
from tests.util_group import collapse, ids_from_lens, random_lens
from tests.util_prior import boost, boosted_ranking, prior_ranking, prior_reference

NEW_SYMBOLS = ("clb_prior_create", "clb_prior_create_device", "clb_prior_max_abs", "clb_prior_destroy", "clb_search_batch_prior",
               "clb_search_batch_prior_device_slot")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(oracle):
    idx = synthetic.make_index(seed=11, n_docs=400, K=64)
    Qs = synthetic.make_queries(idx, 12, 3)
    return idx, Qs


def test_a_zero_prior_and_a_zero_weight_change_nothing(oracle, small):
    idx, Qs = small
    rng = np.random.default_rng(1)
    zeros, some = np.zeros(400, np.float32), rng.normal(0, 0.5, 400).astype(np.float32)
    gids = ids_from_lens(random_lens(400, 1, 6, 2))
    allowed = np.nonzero(rng.random(400) < 0.5)[0] + 1
    for j in range(3):
        Q = Qs[:, :, j]
        for allow, scope in ((None, "candidates"), (allowed, "candidates"), (allowed, "all")):
            plain = filtered_ranking(oracle, idx, Q, 2, allow, scope)
            for values, weight in ((zeros, 1.0), (zeros, -3.5), (some, 0.0)):
                bp, bs = prior_ranking(oracle, idx, Q, 2, values, weight, allow, scope)
                assert np.array_equal(bp, plain[0]) and np.array_equal(bits(bs), bits(plain[1]))
                gp, gs = prior_ranking(oracle, idx, Q, 2, values, weight, allow, scope, group_ids=gids)
                cp, cs = collapse(plain, gids)
                assert np.array_equal(gp, cp) and np.array_equal(bits(gs), bits(cs))
        for k in (1, 10, 400):                                 # ... and without a filter that is oracle.search
            rp, rs, rn = oracle.search(idx, Q, nprobe=2, k=min(k, filtered_ranking(oracle, idx, Q, 2)[0].size))
            pp, ps, pn = prior_reference(oracle, idx, Q, 2, rp.size, some, 0.0)
            assert pn == rn and np.array_equal(pp, rp) and np.array_equal(bits(ps), bits(rs))


def test_the_reference_rounds_twice_and_breaks_ties_by_pid():
    # two roundings: equal to the explicit fp32 steps everywhere, and not the single rounding of the exact e + w v (an fma)
    rng = np.random.default_rng(5)
    e, v = rng.uniform(5, 30, 2000).astype(np.float32), rng.normal(0, 0.5, 2000).astype(np.float32)
    w = np.float32(0.3)
    two = boost(e, v, w)
    steps = np.array([np.float32(x + np.float32(w * y)) for x, y in zip(e, v)], np.float32)
    fused = (e.astype(np.float64) + np.float64(w) * v.astype(np.float64)).astype(np.float32)       # exact in float64, rounded once
    assert np.array_equal(bits(two), bits(steps)) and np.count_nonzero(bits(two) != bits(fused)) > 0
    # equal E: the lower pid first, whatever the order of the input ranking
    ranking = (np.array([7, 3, 5, 9]), np.array([2.0, 1.0, 3.0, 0.5], np.float32))
    values = np.zeros(9, np.float32); values[[6, 2, 4, 8]] = [1.0, 2.0, 0.0, 2.5]           # E = 3 for all four
    p, s = boosted_ranking(ranking, values)
    assert list(p) == [3, 5, 7, 9] and np.all(s == 3.0)
    pp, ps, n = first_k(boosted_ranking(ranking, values, 2.0), 6, pid_offset=100)
    assert n == 4 and list(pp) == [109, 103, 107, 105, 0, 0] and np.all(np.isneginf(ps[4:]))


# ---- the host model of the cut ------------------------------------------------------------------------------------------------
MODEL_CASES = [(seed, mag, eps, values, ties)
               for seed, (mag, eps) in enumerate([(0.0, 0.05), (1.0, 0.05), (2.0 ** 10, 0.05), (2.0 ** 20, 0.05), (2.0 ** 20, 0.01),
                                                  (2.0 ** 10, 0.001), (1.0, 0.5), (2.0 ** 20, 0.3)])
               for values, ties in (("uniform", 40), ("levels", 40), ("constant", 0))]


def test_the_model_cases_cover_what_the_issue_names():
    mags = {c[1] for c in MODEL_CASES}
    assert {0.0, 1.0, 2.0 ** 10, 2.0 ** 20} <= mags
    big = pm.make_case(3, 3000, 2.0 ** 20, 0.05, "constant")
    assert np.spacing(np.float32(np.abs(big["A"]).max())) > big["eps"]          # ulp(A) exceeds eps
    tied = pm.make_case(0, 3000, 1.0, 0.05, "uniform", ties=40)
    _, counts = np.unique(tied["A"], return_counts=True)
    assert np.count_nonzero(counts >= 8) >= 30                                  # blocks of exactly tied A


@pytest.mark.parametrize("seed,mag,eps,values,ties", MODEL_CASES)
def test_the_documented_slack_keeps_the_true_top_k(seed, mag, eps, values, ties):
    case = pm.make_case(100 + seed, 3000, mag, eps, values, ties)
    for k in (1, 10, 100):
        assert pm.misses(case, k) == [], (k, "float64 threshold")
        assert pm.misses(case, k, fp32_steps=True) == [], (k, "threshold in fp32 steps")
    short = pm.make_case(200 + seed, 60, mag, eps, values, 0)
    assert pm.listed(short, 100).all()                         # fewer than k candidates: everything is listed


def test_teeth_without_the_slack_the_cut_loses_a_passage():
    """the precondition of the slack: the same inputs with delta = 0 miss members of the true top k -- where ulp(A) exceeds
    eps, never where the prior is small"""
    lost = {}
    for seed, mag, eps, values, ties in MODEL_CASES:
        case = pm.make_case(100 + seed, 3000, mag, eps, values, ties)
        lost[(seed, values)] = sum(len(pm.misses(case, k, delta=0.0)) for k in (1, 10, 100))
        if mag <= 1.0:
            assert lost[(seed, values)] == 0, (seed, values)   # the cut of the search without a prior was never at fault
    assert sum(1 for n in lost.values() if n) >= 3, lost
    # a worked example: ulp = 1/8 at 2^20, eps = 0.01.  The passage with e just above a rounding boundary and a just below it
    # has E one ulp above A; two others hold the k = 2 places by A
    pi = np.full(3, 2.0 ** 20, np.float32)
    e = np.array([10.0625 + 0.004, 10.25, 10.0625 + 0.05], np.float32)         # E = 2^20 + {10.125, 10.25, 10.125}
    a = np.array([10.0625 - 0.004, 10.25, 10.0625 + 0.05], np.float32)         # A = 2^20 + {10.0,   10.25, 10.125}
    case = dict(e=e, a=a, pi=pi, A=a + pi, E=e + pi, eps=0.01)
    assert list(case["A"] - pi) == [10.0, 10.25, 10.125] and list(case["E"] - pi) == [10.125, 10.25, 10.125]
    assert list(pm.true_top(case, 2)) == [1, 0]                # pid breaks the tie of E: slot 0 is in the answer
    assert pm.misses(case, 2, delta=0.0) == [0] and pm.misses(case, 2) == [] and pm.misses(case, 2, fp32_steps=True) == []


# ---- the C ABI and the Python keywords ----------------------------------------------------------------------------------------
def test_prior_symbols_are_declared_and_exported():
    """Fails before score priors exist: the header declares and the library exports the six entry points."""
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    assert hasattr(clb, "PassagePrior")
    header = " ".join(open(clb._lib.HEADER).read().replace("*", " ").split())
    assert "prior made before an append; make another" in header and "never contracted into an fma" in header
    assert "prior == NULL launches exactly what clb_search_batch_grouped launches" in header


def test_prior_entry_points_check_their_arguments_first():
    """Null handles and null outputs are ArgumentError (4) before any device work; a null prior has max_abs 0 and may be
    destroyed; a weight that is not finite is refused before the searcher is looked at."""
    l = clb.lib()
    i64 = C.c_int64
    null, out, some = C.c_void_p(), C.c_void_p(0xdead0), C.c_void_p(0xdead0)
    v = np.zeros(3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for create in (l.clb_prior_create, l.clb_prior_create_device):
        out = C.c_void_p(0xdead0)
        assert create(null, p(v), i64(3), C.byref(out)) == 4
        assert b"null searcher" in l.clb_last_error() and out.value is None      # a failed create leaves no handle
        assert create(null, p(v), i64(3), None) == 4
    assert l.clb_prior_max_abs(null) == 0.0
    assert l.clb_prior_destroy(null) == 0
    q = np.zeros((128, 32, 1), np.float32, order="F")
    op, os_, nc = np.zeros(5, np.int64), np.zeros(5, np.float32), np.zeros(1, np.int64)
    assert l.clb_search_batch_prior(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, null, null, 1.0, 1, p(op), p(os_), p(nc)) == 4
    assert b"null searcher" in l.clb_last_error()
    assert l.clb_search_batch_prior_device_slot(null, 0, None, i64(32), i64(1), i64(2), i64(5), None, 0, null, null, 1.0, None, None,
                                                None, None) == 4
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert l.clb_search_batch_prior(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, null, some, bad, 1, p(op), p(os_),
                                        p(nc)) == 4
        assert b"prior_weight must be finite" in l.clb_last_error()
        assert l.clb_search_batch_prior_device_slot(null, 0, None, i64(32), i64(1), i64(2), i64(5), None, 0, null, some, bad, None,
                                                    None, None, None) == 4
        assert b"prior_weight must be finite" in l.clb_last_error()
    # without a prior the weight is not looked at: the searcher is
    assert l.clb_search_batch_prior(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, null, null, float("nan"), 1, p(op), p(os_),
                                    p(nc)) == 4
    assert b"null searcher" in l.clb_last_error()
    if l.clb_device_count() == 0:
        idx = synthetic.make_index(0, 20, K=8)
        with pytest.raises(clb.HipError):                      # CLB_EHIP: nothing is boosted or ranked on the host
            clb.Searcher(index=idx).make_prior(np.zeros(20, np.float32))


def test_make_prior_checks_its_values_on_the_host():
    s = _NoDevice()                                            # 100 passages, pid_offset 1000
    for wrong in (np.zeros(99), np.zeros(101), np.zeros((100, 1)), np.zeros(0)):
        with pytest.raises(clb.ArgumentError, match="one value per passage"):
            s.make_prior(wrong)
    for bad_value in (np.nan, np.inf, -np.inf, 1e39):          # 1e39 is not finite in fp32
        v = np.zeros(100)
        v[[7, 50]] = bad_value
        with pytest.raises(clb.ArgumentError, match="passage 1008 is not a finite number"):
            s.make_prior(v)


def fake_prior(s, max_abs):
    """a PassagePrior with a handle that is never handed to the library (the host checks raise first)"""
    return clb.PassagePrior(s, C.c_void_p(0xdead0), 100, max_abs)


def test_prior_keywords_are_validated_on_the_host():
    s = _NoDevice()
    Q = np.zeros((128, 32, 2), np.float32, order="F")
    g = clb.PassageGrouping(s, None, 2, ids_from_lens([60, 40]))
    p = fake_prior(s, 2.0)
    try:
        assert len(p) == 100 and p.max_abs == 2.0
        for bad in (float("nan"), float("inf"), -np.inf, 1e39, "1", None, True):
            with pytest.raises(clb.ArgumentError, match="prior_weight"):
                s.search_batch(Q, 5, prior=p, prior_weight=bad)
        with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
            s.search_batch(Q, 5, prior=p, prior_weight=2e38)                    # 2e38 * 2 overflows fp32
        with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
            s.search_embeddings(Q[:, :, 0], 5, prior=p, prior_weight=-2e38)
        for call in (lambda: s.search_batch(Q, 5, grouping=g, per_group=2, prior=p),
                     lambda: s.search_embeddings(Q[:, :, 0], 5, grouping=g, per_group=1, prior=p),
                     lambda: clb.search(s, Q[:, :, 0], 5, grouping=g, per_group=3, prior=p, prior_weight=0.5)):
            with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
                call()
        with pytest.raises(clb.ColBERTError, match="open PassageGrouping"):       # the (closed) grouping is looked at next
            s.search_batch(Q, 5, grouping=g, prior=p)
    finally:
        p._h = None                                            # never destroyed: it was never created
    with p:                                                    # a context manager; closing a closed prior is fine
        pass
    p.close()
    for call in (lambda: s.search_batch(Q, 5, prior=p), lambda: s.search_embeddings(Q[:, :, 0], 5, prior=p),
                 lambda: clb.search(s, Q[:, :, 0], 5, prior=p), lambda: s.search_batch(Q, 5, prior=np.zeros(100, np.float32))):
        with pytest.raises(clb.ColBERTError, match="open PassagePrior"):
            call()
