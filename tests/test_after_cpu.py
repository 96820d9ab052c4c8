"""Search after a cursor, the part that needs no GPU: a host model of the moved two-pass cut (DESIGN section 5;
tests/after_model.py) with its teeth, the reference helper of tests/util_after.py against a brute-force sort, the C ABI's new
symbols with their argument checks, and the Python keywords."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests import after_model as am
from tests.test_group_cpu import _NoDevice
from tests.test_prior_cpu import fake_prior
from tests.util_after import after_ranking, assert_page
from tests.util_filter import filtered_ranking
from tests.util_group import ids_from_lens

NEW_SYMBOLS = ("clb_search_batch_after", "clb_search_batch_after_device_slot")
F32 = np.float32


# ---- the host model of the cut ------------------------------------------------------------------------------------------------
MODEL_CASES = [(seed, n, eps, gap) for seed, (n, eps, gap) in enumerate([(3000, 0.05, None), (3000, 0.5, None), (400, 0.05, 0.04),
                                                                        (400, 0.3, 0.2), (60, 0.05, 0.01), (2000, 0.001, None)])]


def case_of(seed, n, eps, gap):
    return am.make_case(300 + seed, n, eps, gap, ties_a=min(12, n // 20), ties_e=min(12, n // 20))


def test_the_model_cases_cover_what_the_issue_names():
    case = case_of(0, 3000, 0.05, None)
    d = np.abs(case["a"].astype(np.float64) - case["e"]) / case["eps"]
    assert np.count_nonzero(d > 0.99) > 1500                                   # a pinned at e +- 0.999 eps
    for key in ("a", "e"):
        _, counts = np.unique(case[key], return_counts=True)
        assert np.count_nonzero(counts >= 6) >= 10, key                        # blocks of exactly tied a / exactly tied e
    cur = am.cursors(case)
    scores = np.array([c[0] for c in cur], np.float32)
    assert np.isposinf(scores).any() and np.isneginf(scores).any()
    assert (scores[np.isfinite(scores)] > case["e"].max()).any() and (scores[np.isfinite(scores)] < case["e"].min()).any()
    assert np.count_nonzero(np.isin(scores, case["e"])) >= 24                  # members' own scores
    assert np.count_nonzero(np.isfinite(scores) & ~np.isin(scores, case["e"])) >= 24
    tie_vals = [v for v, c in zip(*np.unique(case["e"], return_counts=True)) if c >= 6]
    assert sum(1 for s, p in cur if s == tie_vals[0]) >= 8                      # every pid position of a tie block, and both sides
    lo_hits = sum(1 for s, _ in cur if np.isfinite(s) and np.any(case["a"] == F32(F32(s) - F32(case["eps"]))))
    hi_hits = sum(1 for s, _ in cur if np.isfinite(s) and np.any(case["a"] == F32(F32(s) + F32(case["eps"]))))
    assert lo_hits >= 6 and hi_hits >= 6                                       # fl(s* -+ eps) lands exactly on a candidate's a


def test_the_steps_bracket_the_real_bounds():
    rng = np.random.default_rng(4)
    for s, eps in zip(rng.uniform(-40, 40, 4000).astype(np.float32), rng.uniform(1e-4, 1.0, 4000).astype(np.float32)):
        lo, hi = am.bounds(s, eps)
        assert float(lo) <= float(s) - float(eps) and float(hi) >= float(s) + float(eps)
        assert float(lo) >= float(s) - float(eps) - 2 * float(np.spacing(np.abs(F32(s - eps)))) - 1e-37
    assert am.step_down(F32(0)) == -am.FLT_MIN and am.step_up(F32(0)) == am.FLT_MIN and am.step_down(am.FLT_MIN) == -am.FLT_MIN
    assert am.step_down(F32(1)) == np.nextafter(F32(1), F32(0)) and am.step_up(F32(-1)) == np.nextafter(F32(-1), F32(0))
    assert am.step_down(F32(-1)) == np.nextafter(F32(-1), F32(-2)) and am.step_up(F32(1)) == np.nextafter(F32(1), F32(2))
    assert np.isneginf(am.step_down(F32(-np.inf))) and am.step_up(F32(-np.inf)) == -am.FLT_MAX
    assert np.isposinf(am.step_up(F32(np.inf))) and np.isneginf(am.step_down(-am.FLT_MAX))
    lo, hi = am.bounds(F32(-np.inf), F32(0.05))
    assert np.isneginf(lo) and hi == -am.FLT_MAX                               # nothing is sure, everything has passed


@pytest.mark.parametrize("seed,n,eps,gap", MODEL_CASES)
def test_the_moved_cut_keeps_the_true_next_k_and_lists_nothing_passed(seed, n, eps, gap):
    case = case_of(seed, n, eps, gap)
    a64, e64 = case["a"].astype(np.float64), case["e"].astype(np.float64)
    for s, p in am.cursors(case, seed):
        for k in (1, 7, 100):
            L, passed = am.listed(case, s, k)
            assert am.misses(case, s, p, k) == [], (s, p, k)
            assert not np.any(L & passed), (s, p, k)                           # no passed candidate is listed ...
            if np.isfinite(s):                                                 # ... and passed is everything above s* + eps, to two ulps
                hi = am.bounds(s, case["eps"])[1]
                assert np.array_equal(passed, case["a"] > hi)
                assert float(hi) <= float(s) + case["eps"] + 2.5 * float(np.spacing(np.abs(hi)))
                assert np.all(e64[passed] > float(s))                          # passed: certainly before the cursor
                assert not np.any(L & (a64 > float(s) + case["eps"] + 2.5 * float(np.spacing(np.abs(hi)))))
            if np.isposinf(s):                                                 # no cursor: nothing masked, the plain cut
                assert not passed.any()
            if np.isneginf(s):
                assert passed.all() and not L.any()
        few = am.listed(case, s, n + 1)[0]                                     # fewer than k sure: everything not passed
        assert np.array_equal(few, ~am.listed(case, s, n + 1)[1])


def test_teeth_the_kth_largest_below_the_cursor_loses_a_member():
    """the obvious rule -- tau = the k-th largest a among a <= s* -- counts candidates that turn out to lie BEFORE the cursor;
    on the same inputs the sure rule loses nothing"""
    lost = 0
    for seed, n, eps, gap in MODEL_CASES:
        case = case_of(seed, n, eps, gap)
        for s, p in am.cursors(case, seed):
            for k in (1, 7):
                assert am.misses(case, s, p, k) == []
                lost += len(am.misses(case, s, p, k, rule="below_cursor"))
    assert lost >= 3, lost
    # a worked example, eps = 0.1, cursor (10, 2), k = 2: pids 1 and 2 lie before the cursor (e > s*) with a <= s*; the
    # answer is pids 3 and 4, three eps further down
    case = dict(e=np.array([10.05, 10.05, 9.7, 9.69], np.float32), a=np.array([9.96, 9.96, 9.7, 9.69], np.float32), eps=0.1)
    assert list(am.true_next(case, 10.0, 2, 2)) == [2, 3]
    assert am.misses(case, 10.0, 2, 2, rule="below_cursor") == [2, 3] and am.misses(case, 10.0, 2, 2) == []


def boundary_case(round_up):
    """s* and eps with fl(s* - eps) above s* - eps (round_up) -- or fl(s* + eps) below s* + eps -- and a candidate ON that
    unstepped bound: the cursor's own passage (pid 1, e = s*) for lo, a passage with e = s* and a later pid for hi"""
    rng = np.random.default_rng(9)
    while True:
        s, eps = F32(rng.uniform(8, 16)), F32(rng.uniform(0.05, 0.1))
        lo, hi = am.bounds(s, eps, ulp_step=False)
        if round_up and float(lo) > float(s) - float(eps):
            # pid 1 = the cursor itself, a on lo; pid 2, the answer, 2.5 eps below the cursor with a at its lower end
            e2 = F32(s - F32(2.5) * eps)
            return dict(e=np.array([s, e2], np.float32), a=np.array([lo, F32(e2 - F32(0.9) * eps)], np.float32), eps=float(eps)), s, 1
        if not round_up and float(hi) < float(s) + float(eps):
            # pid 2 ties with the cursor (pid 1) and is the answer; its a sits on hi
            return dict(e=np.array([s, s], np.float32), a=np.array([s, hi], np.float32), eps=float(eps)), s, 1


def test_teeth_the_ulp_step_is_what_makes_the_bounds_hold_whatever_the_rounding():
    """lo and hi one step outside fl(s* -+ eps) satisfy lo <= s* - eps and hi >= s* + eps however the subtraction and the
    comparison round.  With the STRICT comparisons the kernels use (a < lo, a > hi) an fp32 a below the rounded-up fl(s* - eps)
    is below s* - eps as well (no fp32 number lies between them), so the unstepped bounds lose nothing there -- measured here,
    not only argued; with a candidate ON the unstepped bound and the comparison a <= lo / a >= hi they do lose the answer, and
    the stepped bounds do not, on the same inputs."""
    for round_up in (True, False):
        case, s, p = boundary_case(round_up)
        k = 1
        truth = list(am.true_next(case, s, p, k))
        assert truth == [1]
        assert am.misses(case, s, p, k) == [] and am.misses(case, s, p, k, strict=False) == []
        assert am.misses(case, s, p, k, ulp_step=False, strict=False) == [1], round_up
        assert am.misses(case, s, p, k, ulp_step=False) == []


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_pages_of_the_reference_concatenate_to_a_brute_force_sort(oracle):
    idx = synthetic.make_index(seed=21, n_docs=300, K=16)
    Qs = synthetic.make_queries(idx, 22, 3)
    for j in range(3):
        ranking = filtered_ranking(oracle, idx, Qs[:, :, j], 2)
        rp, rs = ranking
        brute = sorted(zip(rp.tolist(), rs.tolist()), key=lambda t: (-t[1], t[0]))
        assert [b[0] for b in brute] == rp.tolist()
        cursor, pages, seen = (np.inf, 0), 0, []
        while True:
            ap, as_ = after_ranking(ranking, *cursor)
            page_p, page_s = ap[:7], as_[:7]
            pages += 1
            gp = np.zeros(7, np.int64); gs = np.full(7, -np.inf, np.float32)
            gp[:page_p.size] = page_p; gs[:page_s.size] = page_s
            assert assert_page(gp, gs, rp.size, ranking, cursor, 7, "reference") == page_p.size
            if page_p.size == 0:
                break
            seen += page_p.tolist()
            cursor = clb.next_cursor(gp, gs)
        assert seen == rp.tolist() and pages == -(-rp.size // 7) + 1
        # cursors hold GLOBAL pids: with an offset the member at rank 4 itself lies past the local p*
        assert after_ranking(ranking, rs[4], rp[4], pid_offset=1000)[0].size == np.count_nonzero(rs <= rs[4])
        assert after_ranking(ranking, rs[4], rp[4] + 1000, pid_offset=1000)[0].tolist() == rp[5:].tolist()
        assert after_ranking(ranking, -np.inf, 0)[0].size == 0 and after_ranking(ranking, np.nan, 0)[0].size == 0


# ---- the C ABI and the Python keywords ----------------------------------------------------------------------------------------
def test_after_symbols_are_declared_and_exported():
    """Fails before the search after a cursor exists: the header declares and the library exports the two entry points."""
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    assert hasattr(clb, "next_cursor")
    header = " ".join(open(clb._lib.HEADER).read().replace("*", " ").split())
    assert "e(p) < s or (e(p) == s and pid(p) > p )" in header
    assert "the graph holds the ADDRESSES of the cursor arrays, not their values" in header


def test_after_entry_points_check_their_arguments_first():
    """A null handle, a null output, half a cursor and a NaN cursor are ArgumentError (4) before any device work."""
    l = clb.lib()
    i64 = C.c_int64
    null, some = C.c_void_p(), C.c_void_p(0xdead0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    q = np.zeros((128, 32, 2), np.float32, order="F")
    op, os_, nc = np.zeros(10, np.int64), np.zeros(10, np.float32), np.zeros(2, np.int64)
    cs, cp = np.array([np.inf, 3.0], np.float32), np.zeros(2, np.int64)
    host = lambda s, a_s, a_p, o_p=p(op), o_s=p(os_): l.clb_search_batch_after(s, p(q), i64(32), i64(2), i64(2), i64(5), None, 0, a_s,
                                                                                a_p, o_p, o_s, p(nc))
    dev = lambda s, a_s, a_p, o_p=some, o_s=some: l.clb_search_batch_after_device_slot(s, 0, some, i64(32), i64(2), i64(2), i64(5),
                                                                                       None, 0, a_s, a_p, o_p, o_s, None, None)
    for call in (host, dev):
        assert call(null, p(cs), p(cp)) == 4 and b"null searcher" in l.clb_last_error()
        assert call(null, None, None) == 4 and b"null searcher" in l.clb_last_error()
        assert call(some, p(cs), p(cp), None) == 4 and b"is null" in l.clb_last_error()
        assert call(some, p(cs), p(cp), some, None) == 4 and b"is null" in l.clb_last_error()
        assert call(some, p(cs), None) == 4 and b"both be given or both be null" in l.clb_last_error()
        assert call(some, None, p(cp)) == 4 and b"both be given or both be null" in l.clb_last_error()
    bad = np.array([1.0, np.nan], np.float32)
    assert host(some, p(bad), p(cp)) == 4 and b"the cursor score of query 1 is NaN" in l.clb_last_error()


def test_after_keywords_are_validated_on_the_host():
    s = _NoDevice()
    Q = np.zeros((128, 32, 2), np.float32, order="F")
    g = clb.PassageGrouping(s, None, 2, ids_from_lens([60, 40]))
    pr = fake_prior(s, 2.0)
    cur = (np.array([3.0, np.inf], np.float32), np.array([5, 0]))
    try:
        for kw, name in ((dict(grouping=g), "grouping"), (dict(grouping=g, per_group=2), "grouping"), (dict(prior=pr), "prior")):
            for call in (lambda: s.search_batch(Q, 5, after=cur, **kw), lambda: s.search_embeddings(Q[:, :, 0], 5, after=(3.0, 5), **kw),
                         lambda: clb.search(s, Q[:, :, 0], 5, after=(3.0, 5), **kw)):
                with pytest.raises(clb.Unsupported, match=f"after together with {name}"):
                    call()
        with pytest.raises(clb.Unsupported, match="after together with per_group"):
            s.search_batch(Q, 5, after=cur, per_group=2)
    finally:
        pr._h = None
    for bad in ((cur[0],), cur[0], (cur[0][:1], cur[1]), (cur[0], cur[1][:1]), (cur[0], np.array([1.5, 2.0])), ("x", cur[1]),
                (cur[0], np.array([1, 2 ** 63], np.uint64))):
        with pytest.raises(clb.ArgumentError, match="after|cursor"):
            s.search_batch(Q, 5, after=bad)
    with pytest.raises(clb.ArgumentError, match="the cursor score of query 1 is NaN"):
        s.search_batch(Q, 5, after=(np.array([1.0, np.nan]), cur[1]))
    with pytest.raises(clb.ArgumentError, match="pair"):
        s.search_embeddings(Q[:, :, 0], 5, after=3.0)
    with pytest.raises(clb.ArgumentError, match="NaN"):
        s.search_embeddings(Q[:, :, 0], 5, after=(float("nan"), 1))


def test_a_sharded_searcher_refuses_a_cursor():
    sh = object.__new__(clb.ShardedSearcher)
    Q = np.zeros((128, 32, 1), np.float32, order="F")
    for call in (lambda: sh.search_batch(Q, 5, after=(np.zeros(1, np.float32), np.zeros(1, np.int64))),
                 lambda: sh.search_embeddings(Q[:, :, 0], 5, after=(1.0, 1)), lambda: sh.search("q", 5, after=(1.0, 1)),
                 lambda: clb.search(sh, Q[:, :, 0], 5, after=(1.0, 1))):
        with pytest.raises(clb.Unsupported, match="after="):
            call()


def test_next_cursor_on_padded_and_unpadded_pages():
    p = np.array([[4, 9], [7, 2], [1, 0]], np.int64)                            # (k, B): query 1's last row is padding
    s = np.array([[3.0, 2.0], [2.5, 1.0], [2.5, -np.inf]], np.float32)
    cs, cp = clb.next_cursor(p, s)
    assert cs.dtype == np.float32 and cp.dtype == np.int64
    assert list(cp) == [1, 0] and cs[0] == 2.5 and np.isneginf(cs[1])
    assert clb.next_cursor(p[:, 0], s[:, 0]) == (np.float32(2.5), 1)
    fin = clb.next_cursor(p[:, 1], s[:, 1])
    assert fin == (float("-inf"), 0)
    assert clb.next_cursor(np.zeros((4, 2), np.int64), np.full((4, 2), -np.inf, np.float32))[0].tolist() == [-np.inf, -np.inf]
    with pytest.raises(clb.ColBERTError):
        clb.next_cursor(p, s[:2])
