"""Pass 1 on the device against the float64 model of tests/pass1_model.py: every candidate's approximate score inside the
model's interval, the constants of the error bound against values computed from the index, tau against the approximate
scores themselves, and the eps the test hook reports against the table the query really used.

Everything is read through Searcher.debug_scores, bound_consts and centroid_products.  The hook runs one query (B = 1), or
sixteen copies of it when 8-bit score rows are set.  With nprobe = 64 (all of K) every non-empty passage is a candidate, but
the centroid stage then takes its general path: the score table is the canonical fp32 chain stored as fp16, and neither 8-bit
rows nor the single-product table exist there.  The fused centroid kernels (three bf16 products; with sixteen copies the teams
kernel, its 8-bit rows and its single-product form) run for nprobe <= 2 only, so those cases use nprobe = 2 with a query whose
32 tokens probe all 64 centroids between them (covering_query): again every non-empty passage is a candidate.

The model cannot see an fp16 / bf16 operand mix-up; nothing here claims to."""
import functools

import numpy as np
import pytest

import colbert_jl_amd as clb
from tests import pass1_model as pm
from tests.test_gpu_append import head_index, tail
from tests.test_pass1_model_cpu import K, coherent_inputs, covering_query, friendly, friendly_operands, friendly_query
from tests.test_remove_cpu import reduced_index

pytestmark = pytest.mark.gpu

TOP = 10


def note(name, value):
    """a measured figure for profiles/pass1_model.md (shown with pytest -s)"""
    print(f"pass1_model: {name} = {value}")


def run_hook(idx, Q, nprobe, gather=-1, rows=0, products=-1, sync=False):
    s = clb.Searcher(index=idx)
    try:
        s.set_mode(1)
        s.set_pass1_gather(gather)
        s.set_score_rows(rows)
        s.set_centroid_products(products)
        if sync:
            s.raise_bound_consts(s.bound_consts)
        return s.debug_scores(Q, k=TOP, nprobe=nprobe)
    finally:
        s.close()


def excess(o, Q, d, products=3, rows8=False, delta3=pm.DELTA3, slack=True):
    """by how much every candidate's approximate score leaves [lo - gamma, hi + gamma] (<= 0: inside)"""
    p = d["pids"] - 1
    assert np.all(o.doclens[p] > 0), "an empty passage is a candidate"
    lo, hi = pm.passage_bounds(o, Q, products, rows8, delta3)
    g = pm.gamma(o, Q, rows8, products) if slack else 0.0
    a = d["approx"].astype(np.float64)
    return np.maximum(lo[p] - g - a, a - hi[p] - g)


def assert_inside(o, Q, d, what, **kw):
    ex = excess(o, Q, d, **kw)
    print(f"pass1_model: {what}: worst excess {ex.max():.3e} over {ex.size} candidates")
    assert np.all(ex <= 0), (what, np.count_nonzero(ex > 0), ex.size, ex.max())


def assert_every_passage_is_a_candidate(o, d):
    assert np.array_equal(d["pids"] - 1, np.nonzero(o.doclens > 0)[0])


# ---- the friendly index: T in {1, 5, 31, 32} x both gather forms through the general centroid path, T = 32 through the fused one
FIRST = [(T, g, K) for T in (1, 5, 31, 32) for g in (0, 1)] + [(32, 0, 2), (32, 1, 2)]


@functools.lru_cache(maxsize=None)
def first_run(T, gather, nprobe):
    idx = friendly()[0]
    Q = covering_query(idx) if nprobe == 2 else friendly_query(T)
    return Q, run_hook(idx, Q, nprobe, gather=gather)


@pytest.mark.parametrize("T,gather,nprobe", FIRST)
def test_interval_fp16_rows(T, gather, nprobe):
    o = friendly_operands()
    Q, d = first_run(T, gather, nprobe)
    assert_every_passage_is_a_candidate(o, d)
    assert np.isfinite(d["eps"])
    assert_inside(o, Q, d, f"fp16 rows T={T} gather={gather} nprobe={nprobe}")


@pytest.mark.parametrize("T,gather,nprobe", FIRST)
def test_tau_is_a_lower_bound_of_the_kth_approximate_score(T, gather, nprobe):
    """tau may be the lower edge of the 16-bit bin that holds the k-th approximate score, never above that score; and the
    re-scored list is exactly {approx >= tau - 2 eps} in the device's own fp32 arithmetic."""
    _, d = first_run(T, gather, nprobe)
    a = d["approx"]
    assert a.size > TOP
    kth = np.sort(a)[-TOP]
    tau, eps = np.float32(d["tau"]), np.float32(d["eps"])
    assert tau <= kth, (tau, kth)
    assert d["n_rescore"] == np.count_nonzero(a >= tau - np.float32(2.0) * eps)
    note(f"kth - tau (T={T} gather={gather} nprobe={nprobe})", f"{float(kth) - float(tau):.3e} (range {float(a.max() - a.min()):.3f})")


def test_friendly_error_against_eps_and_smallest_delta():
    """Figures only (no minimum is asserted for the ratio): max |approx - float64 canonical| / eps, and the smallest
    three-product delta at which every candidate would still be inside the interval."""
    o = friendly_operands()
    for nprobe in (K, 2):
        Q, d = first_run(32, 0, nprobe)
        s64 = pm.canonical_scores(o, Q)[d["pids"] - 1]
        err = np.abs(d["approx"].astype(np.float64) - s64).max()
        assert err <= d["eps"], (err, d["eps"])
        note(f"friendly max err / eps (nprobe={nprobe})", f"{err:.3e} / {d['eps']:.3e} = {err / d['eps']:.4f}")
        for slack in (True, False):        # without gamma the figure also absorbs the accumulation's roundings
            passes = lambda delta: bool(np.all(excess(o, Q, d, delta3=delta, slack=slack) <= 0))
            lo_d, hi_d = 0.0, 4 * pm.DELTA3
            if passes(0.0):
                hi_d = 0.0
            elif not passes(hi_d):
                hi_d = np.inf
            else:
                for _ in range(12):
                    mid = 0.5 * (lo_d + hi_d)
                    lo_d, hi_d = (lo_d, mid) if passes(mid) else (mid, hi_d)
            note(f"smallest passing delta / (qn cn) (nprobe={nprobe}, {'with' if slack else 'without'} gamma)",
                 f"{hi_d:.3e} (the bound: {pm.DELTA3:.1e})")


# ---- scaled inputs: the manipulations of test_gpu_sizes.test_two_pass_adversarial on this index
def scaled_case(case):
    idx, base = friendly()
    idx = dict(idx)
    Q = friendly_query()
    rng = np.random.default_rng(71)
    if case == "mixed_norms":
        scale = rng.choice(np.array([0.01, 0.3, 1.0, 7.0, 50.0], dtype=np.float32), size=(1, K))
        idx["centroids"] = np.asfortranarray((idx["centroids"] * scale).astype(np.float32))
    elif case == "big_weights":
        idx["bucket_weights"] = np.array([-0.5, -0.11, 0.13, 0.5], dtype=np.float32)
    elif case == "unnormalised_q":
        scale = rng.choice(np.array([0.05, 1.0, 20.0], dtype=np.float32), size=(1, K))
        idx["centroids"] = np.asfortranarray((idx["centroids"] * scale).astype(np.float32))
        f = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=(1, 32)))
        Q = np.ascontiguousarray((Q * f).astype(np.float32))
    elif case == "subnormal_q":        # components of about 1e-6: fp16 keeps them as subnormals, 6e-8 apart
        Q = np.ascontiguousarray((Q * np.float32(1.13e-5)).astype(np.float32))
        assert 5e-7 < np.median(np.abs(Q)) < 2e-6 and np.abs(Q).max() < 6.1e-5
    return idx, Q


@pytest.mark.parametrize("case", ["mixed_norms", "big_weights", "unnormalised_q", "subnormal_q"])
def test_interval_scaled_inputs(case):
    idx, Q = scaled_case(case)
    o = pm.Operands(idx)
    d = run_hook(idx, Q, K, gather=1 if case in ("mixed_norms", "subnormal_q") else 0)
    assert np.isfinite(d["eps"]), "a guarded query would skip the comparison"
    assert_every_passage_is_a_candidate(o, d)
    assert_inside(o, Q, d, case)


# ---- 8-bit rows (the teams kernel: sixteen copies, nprobe = 2)
@pytest.mark.parametrize("products,gather", [(3, 0), (1, 1)])
def test_interval_8_bit_rows(products, gather):
    idx = friendly()[0]
    o = friendly_operands()
    Q = covering_query(idx)
    d = run_hook(idx, Q, 2, gather=gather, rows=1, products=products)
    assert np.isfinite(d["eps"])
    assert_every_passage_is_a_candidate(o, d)
    # the 8-bit table was really in use: its scores are not the fp16 table's
    assert not np.array_equal(d["approx"], first_run(32, gather, 2)[1]["approx"])
    assert_inside(o, Q, d, f"8-bit rows, {products} product(s)", products=products, rows8=True)


# ---- conversion errors that add up instead of cancelling
def test_coherent_rounding():
    idx, Q, _ = coherent_inputs()
    o = pm.Operands(idx)
    d = run_hook(idx, Q, K)
    assert np.isfinite(d["eps"])
    assert_every_passage_is_a_candidate(o, d)
    s64 = pm.canonical_scores(o, Q)[d["pids"] - 1]
    err = np.abs(d["approx"].astype(np.float64) - s64).max()
    note("coherent max err / eps", f"{err:.3e} / {d['eps']:.3e} = {err / d['eps']:.4f}")
    assert err <= d["eps"], (err, d["eps"])
    assert_inside(o, Q, d, "coherent rounding")


# ---- the constants of the bound against the index
# What build_approx_tables (approx_kernels.hpp) multiplies each measured value by: cn 1.001 (max_row_norm_kernel), rn, inv_max,
# rb, dw and dc 1.0001, inv_qerr = 0.5 * step * 1.001 + 4 u * max inv.  FP32: the measured values are fp32 sums of 128 squares
# and their roots, off by less than 130 u = 2^-17 relative; 2^-14 for inv_qerr, a difference of two such values over 2^20 - 1.
FACTOR = np.array([1.001, 1.0001, 1.0001, 1.0001, 1.0001, 1.001, 1.0001])
FP32 = np.array([2.0 ** -17] * 5 + [2.0 ** -14, 2.0 ** -17])


def handle_constants(s):
    return np.concatenate([s.bound_consts.astype(np.float64), [s.centroid_products[1]]])


def assert_constants(s, idx, what, upper=True):
    got, truth = handle_constants(s), pm.bound_constants(idx)
    assert np.all(got >= truth), (what, got, truth)
    if upper:
        cap = truth * FACTOR * (1 + FP32)
        cap[5] += 4 * pm.U * truth[2] * 1.0001 * (1 + 2.0 ** -14)
        assert np.all(got <= cap), (what, got, cap)


def constants_index(case):
    idx = dict(friendly()[0])
    C = idx["centroids"].copy(order="F")
    if case == "scale_60":
        C *= np.float32(60.0)
    elif case == "outlier_centroid":
        C[:, 37] *= np.float32(40.0)
    idx["centroids"] = np.asfortranarray(C)
    return idx


@pytest.mark.parametrize("case", ["scale_1", "scale_60", "outlier_centroid"])
def test_constants_of_a_fresh_handle(case):
    idx = constants_index(case)
    s = clb.Searcher(index=idx)
    try:
        assert_constants(s, idx, case)
    finally:
        s.close()


def test_constants_after_an_append():
    """the head alone, then with the second half appended: both times the constants of the index the handle holds"""
    idx = friendly()[0]
    P = idx["doclens"].size // 2
    head = head_index(idx, P)
    s = clb.Searcher(index=head)
    try:
        assert_constants(s, head, "head")
        s.add_compressed(*tail(idx, P))
        assert_constants(s, idx, "head + tail")
    finally:
        s.close()


def test_constants_after_removals():
    """Remove the passages that hold the row of the largest inv_norm (the index repeats rows, so there are a few), then those
    with the largest ||r'||: a constant measured over the rows must come down to the reduced index's own, smaller value (the
    upper side) and never below it."""
    idx = friendly()[0]
    s = clb.Searcher(index=idx)
    try:
        gone = []
        for which, i in (("inv", 2), ("rb", 3)):
            cur, _ = reduced_index(idx, gone) if gone else (idx, None)
            o = pm.Operands(cur)
            v = o.inv if which == "inv" else np.linalg.norm(o.r16, axis=0)
            rows = np.nonzero(v >= v.max() * (1 - 1e-12))[0]
            pids = np.unique(np.searchsorted(o.starts, rows, side="right"))   # 1-based
            before = pm.bound_constants(cur)
            s.remove_passages(pids)
            gone += pids.tolist()
            after, _ = reduced_index(idx, gone)
            truth = pm.bound_constants(after)
            assert truth[i] < before[i], (which, truth[i], before[i])
            assert_constants(s, after, f"without the passages of the largest {which}")
    finally:
        s.close()


def test_constants_of_a_synced_handle_are_never_below_the_truth():
    """raised constants: only the lower side applies"""
    idx = friendly()[0]
    s = clb.Searcher(index=idx)
    try:
        s.raise_bound_consts(s.bound_consts * np.array([1, 2, 1, 1, 3, 1], np.float32))
        assert_constants(s, idx, "raised", upper=False)
    finally:
        s.close()


# ---- the eps the hook reports is the eps a search of the same table uses
def test_hook_eps_carries_the_single_product_term():
    """8-bit rows: the hook runs sixteen copies, so the centroid stage takes the teams kernel.  With one fp16 product per fp32
    product -- chosen, or the default of a handle whose bounds were synced -- the table is off by up to dq cn + qn dc, and eps
    has to say so: it exceeds the three-product eps by at least T * max inv * (b1 - b3), the two product bounds from numpy
    (the device adds safety factors on top)."""
    idx = friendly()[0]
    o = friendly_operands()
    Q = covering_query(idx)
    Q64 = Q.astype(np.float64)
    qn = np.linalg.norm(Q64, axis=0).max()
    dq = np.linalg.norm(Q64 - pm.f16(Q64), axis=0).max()
    b3 = pm.DELTA3 * qn * o.cn
    b1 = dq * o.cn + qn * o.dc + 384 * pm.U * qn * o.cn
    least = 32 * o.im * (b1 - b3)
    assert o.dc > 0 and least > 1e-3
    e3 = run_hook(idx, Q, 2, rows=1, products=3)["eps"]
    e1 = run_hook(idx, Q, 2, rows=1, products=1)["eps"]
    es = run_hook(idx, Q, 2, rows=1, products=-1, sync=True)["eps"]
    e3s = run_hook(idx, Q, 2, rows=1, products=3, sync=True)["eps"]
    note("hook eps, 8-bit rows: 3 products / 1 product / synced default / synced 3 products", (e3, e1, es, e3s))
    assert np.isfinite([e3, e1, es, e3s]).all()
    assert e1 > e3 and e1 - e3 >= least, (e1, e3, least)
    assert es > e3 and es - e3 >= least, (es, e3, least)
    assert e3s == e3                   # a synced handle told to use three products: no shard's table has the term
