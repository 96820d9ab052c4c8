"""Score priors across a shard group, without a GPU: the float64 model of the two-phase cut with the exchanged magnitude
(the threshold from the gathered tops, the slack from M = max_i M_i; tests/prior_model.py cut into shards),
the host logic of `ShardedSearcher.make_prior` and of the `prior=` / `prior_weight=` keywords on stub shards, and the new
symbols of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import sharded
from tests import prior_model as pm
from tests.test_prior_cpu import MODEL_CASES              # magnitudes 0 .. 2^20, uniform / levels / constant, tied blocks
from tests.test_sharded_searcher_cpu import SIZES, StubShard

NEW_SYMBOLS = ("clb_search_shard_phase1_prior_slot", "clb_search_shard_phase2_prior_slot", "clb_debug_prior_tau_device")
KS = (1, 10, 100)
WORLDS = (2, 4)


# ---- the float64 model -------------------------------------------------------------------------------------------------
def cuts(n, world):
    return [(n * i) // world for i in range(world + 1)]


def exchanged(case, k, world):
    """what the shards publish: (the gathered tops -- every shard's k largest A --, M_i of every shard)"""
    A = case["A"]
    c = cuts(A.size, world)
    tops = [np.sort(A[c[i]:c[i + 1]])[::-1][:k] for i in range(world)]
    M = [float(np.max(np.abs(A[c[i]:c[i + 1]].astype(np.float64)))) if c[i + 1] > c[i] else 0.0 for i in range(world)]
    return np.concatenate(tops), M


def listed_sharded(case, k, world, slack="max", fp32_steps=False):
    """The union of the per-shard lists {A >= tau - 2 delta - 2 eps}: tau the k-th largest gathered value (everything with fewer
    than k), delta = 4 u (M + eps) with M = max_i M_i ("max": what phase 2 forms), min_i M_i ("min"), every shard its own M_i
    ("own"), or delta = 0 ("zero")."""
    A, eps = case["A"], case["eps"]
    c = cuts(A.size, world)
    tops, M = exchanged(case, k, world)
    out = np.zeros(A.size, bool)
    for i in range(world):
        sl = slice(c[i], c[i + 1])
        if tops.size < k:
            out[sl] = True
            continue
        tau = np.sort(tops)[-k]
        m = {"max": max(M), "min": min(M), "own": M[i], "zero": None}[slack]
        delta = 0.0 if m is None else pm.documented_delta(m, eps)
        if fp32_steps:
            t_in = np.float32(tau) - np.float32(2.0) * np.float32(delta)
            thr = np.float32(t_in) - np.float32(2.0) * np.float32(eps)
            out[sl] = ~(A[sl] < thr)
        else:
            out[sl] = A[sl].astype(np.float64) >= float(tau) - 2.0 * delta - 2.0 * eps
    return out


def misses(case, k, world, **kw):
    L = listed_sharded(case, k, world, **kw)
    return [int(i) for i in pm.true_top(case, k) if not L[i]]


def one_sided(case, world, keep_from=1):
    """the case with the prior term |pi| on the shards from `keep_from` on and none before: magnitudes that differ between the
    shards, and the top of the ranking on the boosted ones"""
    c = cuts(case["A"].size, world)
    pi = np.abs(case["pi"])
    pi[:c[keep_from]] = 0.0
    out = dict(case, pi=pi, A=case["a"] + pi, E=case["e"] + pi)
    assert out["A"].dtype == np.float32 and out["E"].dtype == np.float32
    return out


def test_the_model_cases_cover_magnitudes_and_ties():
    assert {0.0, 1.0, 2.0 ** 10, 2.0 ** 20} <= {c[1] for c in MODEL_CASES}
    assert any(c[4] for c in MODEL_CASES)
    tied = pm.make_case(101, 3000, 1.0, 0.05, "uniform", ties=40)
    _, counts = np.unique(tied["A"], return_counts=True)
    assert np.count_nonzero(counts >= 8) >= 30
    big = pm.make_case(103, 3000, 2.0 ** 20, 0.05, "constant")
    assert np.spacing(np.float32(np.abs(big["A"]).max())) > big["eps"]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("seed,mag,eps,values,ties", MODEL_CASES)
def test_the_gathered_threshold_with_the_largest_magnitude_keeps_the_true_top_k(seed, mag, eps, values, ties, world):
    case = pm.make_case(100 + seed, 3000, mag, eps, values, ties)
    for c in (case, one_sided(case, world), one_sided(case, world, world - 1)):
        tops, M = exchanged(c, 100, world)
        # the k-th largest gathered value IS the k-th largest A over the union: every shard gave its k best
        assert np.sort(tops)[-100] == np.sort(c["A"])[-100]
        assert max(M) == float(np.max(np.abs(c["A"].astype(np.float64))))
        for k in KS:
            assert misses(c, k, world) == [], (k, "float64 threshold")
            assert misses(c, k, world, fp32_steps=True) == [], (k, "threshold in fp32 steps")
            # ... and it lists what the single handle's cut lists: same tau, same M
            assert np.array_equal(listed_sharded(c, k, world), pm.listed(c, k))
    short = pm.make_case(200 + seed, 60, mag, eps, values, 0)
    assert listed_sharded(short, 100, world).all()             # fewer than k candidates in the whole group: everything is listed


def test_teeth_no_slack_and_the_smallest_magnitude_lose_members():
    """On the inputs above: delta = 0 misses members of the true top k where ulp(A) exceeds eps, and so does a delta formed
    from the SMALLEST M_i once the shards' magnitudes differ (the prior on all shards but the first: min_i M_i is then a
    MaxSim score, ~30, and the slack it gives is nothing at 2^20).
    A shard cutting with its OWN M_i: counted below.  No loss was found at these sizes (24 cases, 2 and 4 shards, with and
    without the one-sided prior, k = 1, 10, 100) -- a member near the threshold has
    |A| within 2 eps + 2 delta of |tau|, so the shard that owns it has M_i >= |tau| minus that, and 4 u M_i falls short of the
    needed 3 u M + ... only where M_i and M straddle a power of two in just the wrong way.  The exchange of M is kept because
    the proof needs |tau| <= M and |A(p)| <= M with ONE M on every shard; a bound that holds 'nearly always' is not a bound."""
    lost_zero, lost_min, lost_own = {}, {}, {}
    for seed, mag, eps, values, ties in MODEL_CASES:
        case = pm.make_case(100 + seed, 3000, mag, eps, values, ties)
        for world in WORLDS:
            side = one_sided(case, world)
            key = (seed, values, world)
            # without a slack the sharded cut IS the single handle's cut without one: same tau, same lists
            for k in KS:
                assert misses(case, k, world, slack="zero") == pm.misses(case, k, delta=0.0)
            lost_zero[key] = sum(len(misses(c, k, world, slack="zero")) for c in (case, side) for k in KS)
            lost_min[key] = sum(len(misses(side, k, world, slack="min")) for k in KS)
            lost_own[key] = sum(len(misses(c, k, world, slack="own")) for c in (case, side) for k in KS)
            if mag <= 1.0:
                assert lost_zero[key] == 0 and lost_min[key] == 0          # the cut without a prior was never at fault
    for world in WORLDS:
        # at least the three cases the single handle's test counts (tests/test_prior_cpu.py), on every world
        assert sum(1 for key, n in lost_zero.items() if n and key[2] == world) >= 3, lost_zero
        assert sum(1 for key, n in lost_min.items() if n and key[2] == world) >= 1, lost_min
    assert sum(lost_own.values()) == 0, lost_own               # the counted evidence of the docstring: 48 cases x 2 x 3 k
    # a worked example, two shards of two candidates: ulp = 1/8 at 2^20, eps = 0.01.  Shard 0 holds MaxSim-sized A only
    # (M_0 ~ 10); on shard 1 the passage with e just above a rounding boundary and a just below it has E one ulp above A.
    pi = np.array([0.0, 0.0, 0.0, 2.0 ** 20, 2.0 ** 20, 2.0 ** 20], np.float32)
    e = np.array([9.0, 8.0, 7.0, 10.0625 + 0.004, 10.25, 10.0625 + 0.05], np.float32)
    a = np.array([9.0, 8.0, 7.0, 10.0625 - 0.004, 10.25, 10.0625 + 0.05], np.float32)
    case = dict(e=e, a=a, pi=pi, A=a + pi, E=e + pi, eps=0.01)
    assert cuts(6, 2) == [0, 3, 6]
    assert list(pm.true_top(case, 2)) == [4, 3]                # E: 2^20 + {10.125, 10.25, 10.125}; pid breaks the tie
    tops, M = exchanged(case, 2, 2)
    assert M[0] == 9.0 and M[1] > 2.0 ** 20
    assert misses(case, 2, 2, slack="zero") == [3] and misses(case, 2, 2, slack="min") == [3]
    assert misses(case, 2, 2) == [] and misses(case, 2, 2, fp32_steps=True) == []


# ---- host logic on stub shards -----------------------------------------------------------------------------------------
class PriorShard(StubShard):
    """A stub shard that records the values its make_prior is given."""

    class Part:
        def __init__(self, values):
            self.values, self.closed = np.array(values), False
            self.max_abs = float(np.max(np.abs(values))) if values.size else 0.0
            self._h = 1

        def close(self):
            self.closed = True

    def make_prior(self, values):
        assert values.dtype == np.float32 and values.size == self.num_docs and values.flags.c_contiguous
        self.part = self.Part(values)
        return self.part


def stub_group(first=0):
    off = first + np.concatenate([[0], np.cumsum(SIZES)])
    return clb.ShardedSearcher([PriorShard(int(off[i]), SIZES[i]) for i in range(len(SIZES))])


@pytest.mark.parametrize("first", (0, 40))
def test_values_are_cut_at_the_bounds(first):
    g = stub_group(first)
    n = g.num_docs
    v = np.random.default_rng(first).normal(0, 0.5, n)
    v[5] = -77.0                                               # the one passage of shard 1
    p = g.make_prior(v)
    assert isinstance(p, clb.ShardedPrior) and len(p) == n and len(p.parts) == len(SIZES)
    c = np.concatenate([[0], np.cumsum(SIZES)])
    for i, s in enumerate(g.shards):
        assert np.array_equal(s.part.values, v.astype(np.float32)[c[i]:c[i + 1]])
    assert p.max_abs == 77.0 and [x.max_abs for x in p.parts][1] == 77.0        # the maximum over ALL shards
    assert sharded.slice_prior(v, g._bounds)[1][2].size == SIZES[2]
    with p:
        pass
    assert p.closed and all(s.part.closed for s in g.shards)


def test_errors_name_the_global_pid_before_any_shard_is_called():
    g = stub_group(first=40)                                   # passages 41 .. 56; shard 2 holds 47 .. 53
    n = g.num_docs
    for bad_value in (np.nan, np.inf, -np.inf, 1e39):          # 1e39 is not finite in fp32
        v = np.zeros(n)
        v[[8, 12]] = bad_value                                 # on the third shard: global pid 40 + 8 + 1
        with pytest.raises(clb.ArgumentError, match="passage 49 is not a finite number"):
            g.make_prior(v)
    with pytest.raises(clb.ArgumentError, match=r"one value per passage.*15 values.*pid 56 has no value"):
        g.make_prior(np.zeros(n - 1))
    with pytest.raises(clb.ArgumentError, match=r"one value per passage.*17 values.*pid 57 is not a passage"):
        g.make_prior(np.zeros(n + 1))
    with pytest.raises(clb.ArgumentError, match="one value per passage"):
        g.make_prior(np.zeros((n, 1)))
    assert not any(hasattr(s, "part") for s in g.shards)


def test_the_weight_is_checked_against_the_groups_largest_value():
    g, other = stub_group(), stub_group()
    Q = np.zeros((128, 32, 2), np.float32, order="F")
    v = np.zeros(g.num_docs)
    v[0], v[15] = 1.0, 4.0                                     # shard 0: max 1; the last shard: max 4
    p = g.make_prior(v)
    assert p.parts[0].max_abs == 1.0 and p.max_abs == 4.0
    for call in (lambda w: g.search_batch(Q, 5, 2, prior=p, prior_weight=w),
                 lambda w: g.search_embeddings(Q[:, :, 0], 5, 2, prior=p, prior_weight=w),
                 lambda w: clb.search(g, Q[:, :, 0], 5, prior=p, prior_weight=w)):
        with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
            call(1e38)                                         # fine for shard 0 alone (1e38 * 1), not for the group (1e38 * 4)
        with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
            call(-1e38)
        for bad in (float("nan"), float("inf"), 1e39, "1", None, True):
            with pytest.raises(clb.ArgumentError, match="prior_weight"):
                call(bad)
    # keyword routing: per_group with a prior is the single handle's refusal, a cursor is refused before anything else
    with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
        g.search_batch(Q, 5, 2, prior=p, per_group=2)
    with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
        clb.search(g, Q[:, :, 0], 5, prior=p, per_group=2)
    with pytest.raises(clb.Unsupported, match="per_group=.*across a shard group"):
        g.search_batch(Q, 5, 2, per_group=2)
    with pytest.raises(clb.Unsupported, match="after=.*across a shard group"):
        g.search_batch(Q, 5, 2, prior="anything", prior_weight=float("nan"), after=(np.zeros(2), np.zeros(2)))
    with pytest.raises(clb.Unsupported, match="after=.*across a shard group"):
        clb.search(g, Q[:, :, 0], 5, prior=p, after=(np.zeros(1), np.zeros(1)))
    # a prior of another group, anything that is no ShardedPrior, a closed one
    theirs = other.make_prior(v)
    for bad in (theirs, "recency", p.parts[0], np.zeros(16, np.float32)):
        with pytest.raises(clb.ColBERTError, match="ShardedPrior of this shard group"):
            g.search_batch(Q, 5, 2, prior=bad)
        with pytest.raises(clb.ColBERTError, match="ShardedPrior of this shard group"):
            clb.search(g, Q[:, :, 0], 5, prior=bad)
    mine = g.make_prior(v)
    mine.close()
    with pytest.raises(clb.ColBERTError, match="open ShardedPrior"):
        g.search_batch(Q, 5, 2, prior=mine)
    # one made before an append
    g._bounds[-1] += 2
    with pytest.raises(clb.ArgumentError, match="prior made before an append; make another"):
        g.search_batch(Q, 5, 2, prior=p)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    assert hasattr(clb, "ShardedPrior") and hasattr(clb.ShardedSearcher, "make_prior")
    header = " ".join(open(clb._lib.HEADER).read().replace("*", " ").split())
    assert "Score priors across a shard group" in header and "M must be the maximum over ALL shards" in header


def test_new_entry_points_check_their_arguments_first():
    """Null handles and operands are ArgumentError (4) before any device work; a weight that is not finite is refused before
    the searcher is looked at."""
    l = clb.lib()
    null = C.c_void_p()
    x = C.c_void_p(0x1000)              # a non-null address that is never read: every call below is refused before it
    assert l.clb_search_shard_phase1_prior_slot(null, 0, None, 32, 1, 2, 4, None, 0, None, 0, x, 1.0, x, None, x, None) == 4
    assert b"null" in l.clb_last_error()
    assert l.clb_search_shard_phase2_prior_slot(null, 0, None, 32, 1, 2, 4, x, None, x, 2, None, 0, x, 1.0, x, x, None, x, None, None) == 4
    assert l.clb_search_shard_phase2_prior_slot(null, 0, None, 32, 1, 2, 4, x, None, x, 2, None, 0, null, 1.0, x, x, None, x, None, None) == 4
    assert b"prior is null" in l.clb_last_error()
    for bad in (float("nan"), float("inf")):
        assert l.clb_search_shard_phase1_prior_slot(null, 0, None, 32, 1, 2, 4, None, 0, None, 0, x, bad, x, None, x, None) == 4
        assert b"prior_weight must be finite" in l.clb_last_error()
        assert l.clb_search_shard_phase2_prior_slot(null, 0, None, 32, 1, 2, 4, x, None, x, 2, None, 0, x, bad, x, x, None, x, None, None) == 4
        assert b"prior_weight must be finite" in l.clb_last_error()
    args = [x, None, x, x, 2, 1, 4, x, None]                   # top, gid, mabs, eps, n_shards, B, k, tau_in, stream
    for i in (0, 2, 3, 7):
        a = list(args); a[i] = None
        assert l.clb_debug_prior_tau_device(*a) == 4, i
        assert b"null" in l.clb_last_error()
    for i in (4, 5, 6):
        a = list(args); a[i] = 0
        assert l.clb_debug_prior_tau_device(*a) == 4, i
    a = list(args); a[1] = x; a[4] = 257
    assert l.clb_debug_prior_tau_device(*a) == clb.Unsupported.code and b"256" in l.clb_last_error()
