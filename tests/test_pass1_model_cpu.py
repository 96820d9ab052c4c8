"""The float64 model of pass 1 (tests/pass1_model.py) checked against itself on the CPU: it contains its own centre, it is
narrow enough to mean something, and four injected errors of the kind a kernel can make leave it.  No kernel code runs
here; tests/test_gpu_pass1_model.py holds the device against the same model.  The input builders of both files live here."""
import functools

import numpy as np
import pytest

from colbert_jl_amd import synthetic
from tests import pass1_model as pm
from tests.test_gpu_pass1_packing import RAGGED, _with_doclens

K = 64


@functools.lru_cache(maxsize=None)
def friendly():
    """(index, base index): ~1 500 passages over 64 centroids, about 500 of them with the lengths of RAGGED -- packed steps,
    quad edges, step edges, the 256-row mask edge and empty passages all occur.  Queries are drawn from the base index (it has
    no empty passage)."""
    base = synthetic.make_index(seed=61, n_docs=1500, K=K, doclen_mean=12, doclen_std=14, doclen_max=400)
    dl = base["doclens"].copy()
    rng = np.random.default_rng(62)
    for j, pid in enumerate(rng.choice(1500, size=25 * len(RAGGED), replace=False)):
        dl[pid] = RAGGED[j % len(RAGGED)]
    return _with_doclens(base, dl), base


@functools.lru_cache(maxsize=None)
def friendly_operands():
    return pm.Operands(friendly()[0])


def friendly_query(T=32, seed=63):
    return np.ascontiguousarray(synthetic.make_queries(friendly()[1], seed, 1, T=T)[:, :, 0])


def covering_query(index, seed=64, noise=0.05):
    """32 unit tokens, token t between centroids 2t and 2t + 1: with nprobe = 2 the query probes all 64 centroids, so every
    non-empty passage is a candidate although the centroid stage runs its fused (nprobe <= 2) kernels."""
    C = np.asarray(index["centroids"], dtype=np.float64)
    assert C.shape[1] == 64
    Cn = C / np.linalg.norm(C, axis=0, keepdims=True)
    q = Cn[:, 0::2] + Cn[:, 1::2] + noise * np.random.default_rng(seed).standard_normal((128, 32)) / np.sqrt(128)
    q /= np.linalg.norm(q, axis=0, keepdims=True)
    return np.ascontiguousarray(q.astype(np.float32))


def _below_midpoint(x, toward_upper):
    """float32 values one ulp off the midpoint between the fp16 neighbours that enclose x: just below it (fp16 rounds down,
    x - fp16(x) > 0) or, toward_upper, just above it (fp16 rounds up, x - fp16(x) < 0)"""
    x = np.asarray(x, dtype=np.float32)
    h = x.astype(np.float16)
    h = np.where(h.astype(np.float32) > x, np.nextafter(h, np.float16(-np.inf)), h).astype(np.float16)     # fp16 floor
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float32)
    mid = (h.astype(np.float32) + up) * np.float32(0.5)                                                     # exact in fp32
    return np.where(toward_upper, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))).astype(np.float32)


def coherent_inputs(seed=65):
    """(index, Q): the friendly index with every bucket weight just below an fp16 midpoint (w - fp16(w) = +half an fp16 ulp
    for all four), and a query whose token t is a noisy copy of one row e_t of a passage with each component one float32 ulp off
    an fp16 midpoint, on the side that gives Q_d - fp16(Q_d) the sign of r'_{e_t}[d]: the terms of dQ.r' all add."""
    idx, base = friendly()
    w = _below_midpoint(idx["bucket_weights"], False)
    idx = dict(idx, bucket_weights=w)
    Q = synthetic.make_queries(dict(base, bucket_weights=w), seed, 1)[:, :, 0]
    # the rows the tokens were drawn from (make_queries' own draws)
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(base["doclens"])])
    p = rng.integers(0, base["doclens"].size, size=1)[0]
    eids = off[p] + rng.integers(0, base["doclens"][p], size=32)
    r16 = pm.f16(w)[pm.residual_indices(base)[:, eids]]                       # (128, 32): r' of row e_t
    Q = _below_midpoint(Q, r16 < 0)
    norms = np.linalg.norm(Q.astype(np.float64), axis=0)
    Q = Q * np.exp2(-np.rint(np.log2(norms))).astype(np.float32)[None, :]     # a power of two keeps every midpoint
    return idx, np.ascontiguousarray(Q.astype(np.float32)), r16


def outside(value, lo, hi, g):
    ok = ~np.isnan(lo)
    return np.count_nonzero((value[ok] < lo[ok] - g) | (value[ok] > hi[ok] + g)) / np.count_nonzero(ok)


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("T", [1, 5, 31, 32])
def test_centre_lies_inside_the_interval(T, products):
    o, Q = friendly_operands(), friendly_query(T)
    lo, hi = pm.passage_bounds(o, Q, products)
    c = pm.centre_scores(o, Q)
    ne = o.doclens > 0
    assert np.array_equal(np.isnan(lo), ~ne) and np.array_equal(np.isnan(c), ~ne)
    assert np.all(lo[ne] <= c[ne]) and np.all(c[ne] <= hi[ne])


@pytest.mark.parametrize("products", [3, 1])
def test_centre_lies_inside_the_interval_of_8_bit_rows(products):
    """The 8-bit table read back at fp16(s) is inside the 8-bit interval; a cell is uncertain only where a rounding edge can
    lie inside its position's interval, and by one cell at the most under the three-product delta."""
    o, Q = friendly_operands(), friendly_query()
    s_lo, s_hi = pm.table_interval(o, Q, products)
    V_lo, V_hi, c_lo, c_hi = pm.cell8_table(s_lo, s_hi)
    s = pm.as_query(Q).T @ o.C
    V, _, cell, cell2 = pm.cell8_table(s, s)
    assert np.array_equal(cell, cell2) and cell.min() == 0 and cell.max() == 254
    assert np.all(V_lo <= V) and np.all(V <= V_hi)
    assert np.abs(V - s).max() <= 0.5005 * pm.cell8_ranges(s, s)[3].max() + 2.0 ** -11 * np.abs(s).max()
    wide = c_hi - c_lo
    # a position's interval is at most 8 delta / step wide (X, lo and 254 steps of the step's own 2 delta / 254, each two-sided):
    # that is the largest share of cells that can have a rounding edge inside it
    share = 8.0 * ((s_hi - s_lo).max() / 2) / pm.cell8_ranges(s_lo, s_hi)[2].min()
    print("uncertain cells", wide.mean(), "of at most", share)
    assert wide.min() == 0 and wide.max() <= np.floor(share) + 1 and wide.mean() <= share, (wide.max(), wide.mean(), share)
    assert products == 1 or wide.max() == 1         # the three-product table: no cell is uncertain by more than one
    _, _, st_lo, st_hi, _ = pm.cell8_ranges(s, s)
    D = pm.cell8_residual_products(o, Q, st_lo, st_hi)
    centre = o.passage_sums((V[:, o.codes0] + D[0]) * o.inv)
    lo, hi = pm.passage_bounds(o, Q, products, rows8=True)
    ne = o.doclens > 0
    assert np.all(lo[ne] <= centre[ne]) and np.all(centre[ne] <= hi[ne])


def test_centre_is_within_the_observed_error_of_the_canonical_score():
    """the observed |approx - exact| is far below eps; 1e-2 is its figure for a passage score"""
    o, Q = friendly_operands(), friendly_query()
    c, s64 = pm.centre_scores(o, Q), pm.canonical_scores(o, Q)
    ne = o.doclens > 0
    assert np.abs(c[ne] - s64[ne]).max() < 1e-2


@pytest.mark.parametrize("T", [1, 5, 31])
def test_padded_tokens_contribute_zero(T):
    o, Q = friendly_operands(), friendly_query(T)
    Qp = np.zeros((128, 32), dtype=np.float32)
    Qp[:, :T] = Q
    for rows8 in (False, True):
        a, b = pm.passage_bounds(o, Q, rows8=rows8), pm.passage_bounds(o, Qp, rows8=rows8)
        # (to the rounding of the float64 products, which take another BLAS path for another T)
        assert np.allclose(a[0], b[0], rtol=1e-13, atol=1e-15, equal_nan=True) and np.allclose(a[1], b[1], rtol=1e-13, atol=1e-15, equal_nan=True)
        assert np.isclose(pm.gamma(o, Q, rows8=rows8), pm.gamma(o, Qp, rows8=rows8), rtol=1e-12, atol=0)
    assert np.allclose(pm.centre_scores(o, Q), pm.centre_scores(o, Qp), rtol=1e-13, atol=1e-15, equal_nan=True)


def test_interval_stays_narrow():
    """The cap that keeps the model from becoming vacuous: full width including 2 gamma at most 1.2e-2 on the friendly index
    at T = 32 (measured: 9e-3; the device's eps there is about 0.045), and gamma itself near its derived 6e-4."""
    o, Q = friendly_operands(), friendly_query()
    lo, hi = pm.passage_bounds(o, Q)
    g = pm.gamma(o, Q)
    ne = o.doclens > 0
    width = (hi - lo)[ne] + 2 * g
    print("width", width.min(), width.max(), "gamma", g)
    assert 4e-4 < g < 8e-4
    assert width.max() <= 1.2e-2


def test_mutations_leave_the_interval():
    """What the GPU test can catch: each of four errors a kernel can make, injected into the model's own centre, takes at
    least a quarter of the passages out of [lo - gamma, hi + gamma]."""
    o, Q = friendly_operands(), friendly_query()
    lo, hi = pm.passage_bounds(o, Q)
    g = pm.gamma(o, Q)
    X, qr = pm.table_centre(o, Q), pm.residual_products(o, Q)
    S = pm.token_scores(o, X, qr)
    assert outside(o.passage_sums(S), lo, hi, g) == 0.0
    ne = o.doclens > 0
    last = o.starts[1:][ne & (o.doclens > 1)] - 1
    dropped = S.copy()
    dropped[:, last] = -np.inf
    d0 = 17
    mutants = {
        "neighbouring row's inv_norm": pm.token_scores(o, X, qr, inv=np.roll(o.inv, -1)),
        "dropped last row": dropped,
        "token column shifted by one": pm.token_scores(o, np.roll(X, -1, axis=0), qr),
        "one dropped query dimension": pm.token_scores(o, X, qr - np.outer(pm.f16(Q)[d0], o.r16[d0])),
    }
    for name, Sm in mutants.items():
        frac = outside(o.passage_sums(Sm), lo, hi, g)
        print(name, frac)
        assert frac >= 0.25, (name, frac)


def test_constants_of_a_three_passage_index():
    """Two centroids, four rows in passages of 1, 2 and 1 rows; every value below is written out by hand."""
    f01, f03 = 0.100000001490116119384765625, 0.300000011920928955078125       # float32(0.1), float32(0.3)
    h01, h03 = 0.0999755859375, 0.300048828125                                 # fp16 of them
    C = np.zeros((128, 2), dtype=np.float32)
    C[0, 0] = 0.5
    C[:, 1] = 0.1
    res = np.empty((32, 4), dtype=np.uint8)
    res[:, 0], res[:, 1], res[:, 2], res[:, 3] = 0x00, 0xFF, 0xAA, 0x55        # bucket 0, 3, 2, 1 in every dim
    idx = {"dim": 128, "nbits": 2, "centroids": np.asfortranarray(C),
           "bucket_weights": np.array([-0.5, -0.25, 0.25, 0.3], dtype=np.float32),
           "codes": np.array([1, 2, 2, 1], dtype=np.uint32), "residuals": np.asfortranarray(res),
           "doclens": np.array([1, 2, 1], dtype=np.int64)}
    r128 = np.sqrt(128.0)
    eps = 2.0 ** -23
    inv = [1 / (np.sqrt(127.0) * 0.5 + eps),       # c0 - 0.5: component 0 vanishes
           1 / (r128 * (f01 + f03) + eps),
           1 / (r128 * (f01 + 0.25) + eps),
           1 / (r128 * 0.25 + eps)]                # c0 - 0.25: |component| 0.25 everywhere
    want = [r128 * f01,                            # max ||c||: 1.13 against 0.5
            r128 * 0.5,
            inv[3],
            r128 * 0.5,                            # max ||r'||: the row of bucket 0
            r128 * (h03 - f03),                    # only 0.3 is not an fp16 number
            0.5 * (inv[3] - inv[0]) / (2 ** 20 - 1),   # K = 2: one code bit, inv_norm keeps its 20-bit cap
            r128 * (f01 - h01)]
    got = pm.bound_constants(idx)
    assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)


def test_coherent_inputs_are_coherent():
    idx, Q, r16 = coherent_inputs()
    w = idx["bucket_weights"].astype(np.float64)
    dw = w - pm.f16(w)
    ulp = np.array([float(np.spacing(np.float16(v))) for v in pm.f16(w)])
    assert np.all(dw > 0) and np.all(dw > 0.499 * np.abs(ulp))
    dq = Q.astype(np.float64) - pm.f16(Q)
    assert np.all(dq * r16 > 0)
    n = np.linalg.norm(Q.astype(np.float64), axis=0)
    assert np.all((n > 0.70) & (n < 1.42))
    # every component loses (almost) half an fp16 ulp: ||dq|| is at least 1.7 times a random rounding's (ulp / sqrt(12) per component)
    rand = np.linalg.norm(synthetic.make_queries(friendly()[1], 65, 1)[:, :, 0].astype(np.float64)
                          - pm.f16(synthetic.make_queries(friendly()[1], 65, 1)[:, :, 0]), axis=0)
    assert np.all(np.linalg.norm(dq, axis=0) > 1.5 * rand)


def test_covering_query_probes_every_centroid():
    idx = friendly()[0]
    Q = covering_query(idx)
    s = Q.astype(np.float64).T @ idx["centroids"].astype(np.float64)
    order = np.argsort(-s, axis=1)
    assert np.array_equal(np.sort(order[:, :2], axis=1), np.arange(64).reshape(32, 2))
    gap = np.take_along_axis(s, order[:, 1:2], 1) - np.take_along_axis(s, order[:, 2:3], 1)
    assert gap.min() > 0.05            # far beyond any rounding of the centroid stage
