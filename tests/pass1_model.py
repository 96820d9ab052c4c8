"""A float64 model of what pass 1 of the two-pass search is DESIGNED to compute, in numpy alone.

For one query the model gives every passage an interval [lo, hi] that must hold the device's approximate score up to the
accumulation slack `gamma`.  What it takes from the kernels are their documented rules and nothing they compute:

  operands   Q' = fp16(Q), w' = fp16(bucket weights), r'[d] = w'[idx[d]] (bit order of synthetic.decompress_numpy),
             inv[e] = 1 / (||c + r|| + eps32) from the unrounded c and w, known to half a step of its packed grid;
  table      cell (t, c) holds fp16 of a value within `delta` of s = Q_t . c -- rounding is monotone, so the stored value
             lies in [fp16(s - delta), fp16(s + delta)];
  score      S[t][e] = (X[t][code_e] + Q'_t . r'_e) * inv[e];  passage = sum over t < T of max over its rows.

Two things are NOT modelled, only bounded:
  delta   the error of the centroid product.  Three bf16 products: the project's own bound 7.4e-5 ||Q_t|| max||c||, without the
          safety factor the device multiplies it by.  One fp16 product: centroid_product_bound,
          1.001 (dq_t max||c|| + ||Q_t|| dc) + 384 u ||Q_t|| max||c||, with dq_t = ||Q_t - fp16(Q_t)|| and
          dc = max ||c - fp16(c)|| computed here.  (A table made by the canonical fp32 chain, as for nprobe > 2, is 2 * 128 u
          from s and so inside the first bound as well.)
  gamma   the fp32 roundings behind the operands, by operation count with u = 2^-24:
            a cell's accumulator takes 2 selection products and 128 products of Q'.r' -- 130 additions, each rounding a partial
            sum of at most |X| + |Q'.r'| <= ||Q_t|| (cn + rb): 130 u of that; the dequantisation of inv and the product with it
            are 2 more roundings of a value below M_t = im ||Q_t|| (cn + rb)         => 132 u M_t per token,
            the passage score is a sum of 32 token maxima: 32 additions of partial sums below sum_t M_t
                                                                                     => 32 u sum_t M_t,
          gamma = (132 + 32) u sum_t M_t.  Unit vectors (cn ~ 1, rb ~ 0.33, im ~ 1.5, T = 32): 164 * 32 * 2^-24 * 2.0 = 6.3e-4.
          8-bit rows: the accumulator works in cell units, starts at k_t - 1024 and passes 1024 + cell: partial sums below
          A_t + 255 step_t + ||Q_t|| rb in score units, 1280 u step_t for the start value's own rounding, and one more product
          (with step_t): im (130 u (A_t + 255 step_t + ||Q_t|| rb) + 1280 u step_t) + 3 u M_t per token.
gamma is derived, not fitted: a change that loosens it or delta fails the width cap of tests/test_pass1_model_cpu.py.

The model cannot tell fp16 operands from bf16 ones where the bf16 value happens to lie inside the interval; see DESIGN.md.
"""
import numpy as np

U = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)
DELTA3 = 7.4e-5           # |three-product value - Q.c| / (||Q_t|| max||c||): approx_kernels.hpp, without kEpsSafety
CELL8_STEPS = 254.0       # kCell8Steps
DIM = 128


def f16(x):
    """fp16 by round to nearest even, subnormals kept (what v_cvt_f16_f32 does), as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def residual_indices(index):
    """(dim, n_emb) bucket indices, dims in the order of synthetic.decompress_numpy (2-bit fields, least significant first)."""
    res = index["residuals"]
    return np.stack([(res >> (2 * i)) & 3 for i in range(4)], axis=1).reshape(DIM, -1)


class Operands:
    """Everything of an index that does not depend on the query, in float64."""

    def __init__(self, index):
        assert index["dim"] == DIM and index["nbits"] == 2
        self.C = np.asarray(index["centroids"], dtype=np.float64)                  # (dim, K)
        self.w = np.asarray(index["bucket_weights"], dtype=np.float64)
        self.w16 = f16(self.w)
        self.codes0 = np.asarray(index["codes"]).astype(np.int64) - 1
        self.ridx = residual_indices(index)
        self.doclens = np.asarray(index["doclens"]).astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.doclens)])
        self.r16 = self.w16[self.ridx]                                             # r' (dim, n_emb)
        x = self.C[:, self.codes0] + self.w[self.ridx]
        self.inv = 1.0 / (np.linalg.norm(x, axis=0) + EPS32)
        K = self.C.shape[1]
        cbits = 1
        while (1 << cbits) < K:
            cbits += 1
        self.qmax = (1 << min(32 - cbits, 20)) - 1                                 # build_approx_tables
        n = self.inv.size
        self.inv_half_step = 0.5 * (self.inv.max() - self.inv.min()) / self.qmax if n else 0.0
        self.cn = float(np.linalg.norm(self.C, axis=0).max())
        self.dc = float(np.linalg.norm(self.C - f16(self.C), axis=0).max())
        self.rb = float(np.linalg.norm(self.r16, axis=0).max()) if n else 0.0
        self.im = float(self.inv.max()) if n else 0.0

    def xhat(self):
        """the canonical normalised embeddings (dim, n_emb), unrounded operands"""
        return (self.C[:, self.codes0] + self.w[self.ridx]) * self.inv

    def passage_sums(self, S):
        """sum over the tokens of the maximum over a passage's rows of S (T, n_emb); nan for an empty passage"""
        out = np.full(self.doclens.size, np.nan)
        ne = self.doclens > 0
        if ne.any():
            out[ne] = np.maximum.reduceat(S, self.starts[:-1][ne], axis=1).sum(axis=0)
        return out


def bound_constants(index):
    """The float64 truth of the seven constants of the error bound: max||c||, sqrt(dim) max|w|, max inv, max||r'|| over the
    index's rows, sqrt(dim) max|w - w'|, half an inv_norm step, max||c - fp16(c)||."""
    o = Operands(index)
    return np.array([o.cn, np.sqrt(DIM) * np.abs(o.w).max(), o.im, o.rb, np.sqrt(DIM) * np.abs(o.w - o.w16).max(),
                     o.inv_half_step, o.dc])


def as_query(Q):
    Q = np.asarray(Q)
    assert Q.ndim == 2 and Q.shape[0] == DIM and Q.dtype == np.float32, "Q: (128, T) float32, as the device receives it"
    return Q.astype(np.float64)


def table_interval(o, Q, products=3, delta3=DELTA3):
    """(s - delta, s + delta), each (T, K): where the centroid kernel's fp32 value of Q_t . c lies.  (delta3: for measuring
    how small the three-product delta could be; the tests leave it alone.)"""
    Q = as_query(Q)
    s = Q.T @ o.C
    qn = np.linalg.norm(Q, axis=0)[:, None]
    if products == 3:
        d = delta3 * qn * o.cn
    else:
        assert products == 1
        dq = np.linalg.norm(Q - f16(Q), axis=0)[:, None]
        d = 1.001 * (dq * o.cn + qn * o.dc) + 384.0 * U * qn * o.cn
    return s - d, s + d


def table_centre(o, Q):
    """the score table taken as fp16(s)"""
    return f16(as_query(Q).T @ o.C)


def residual_products(o, Q):
    """Q'_t . r'_e, (T, n_emb): fp16 x fp16 products are exact in fp32, the sum's rounding is in gamma"""
    return f16(as_query(Q)).T @ o.r16


def scaled(P_lo, P_hi, o):
    """[P_lo, P_hi] * [inv - half step, inv + half step] (inv > 0, P of either sign)"""
    i_lo, i_hi = o.inv - o.inv_half_step, o.inv + o.inv_half_step
    return np.minimum(P_lo * i_lo, P_lo * i_hi), np.maximum(P_hi * i_lo, P_hi * i_hi)


def token_scores(o, X, qr, inv=None):
    """S[t][e] = (X[t][code_e] + qr[t][e]) * inv[e] for ONE table X (T, K)"""
    return (X[:, o.codes0] + qr) * (o.inv if inv is None else inv)


def centre_scores(o, Q):
    """the passage scores of the model's centre: table fp16(s), operands Q', r', inv"""
    return o.passage_sums(token_scores(o, table_centre(o, Q), residual_products(o, Q)))


def canonical_scores(o, Q):
    """MaxSim of the unrounded operands in float64: what the exact pass computes in fp32"""
    return o.passage_sums(as_query(Q).T @ o.xhat())


def _absmin(a, b):
    """min |x| over x in [a, b]"""
    return np.where((a <= 0) & (b >= 0), 0.0, np.minimum(np.abs(a), np.abs(b)))


def cell8_ranges(s_lo, s_hi):
    """token_range_kernel on intervals.  The range is taken from the centroid kernel's fp32 values BEFORE the fp16 store:
    lo_t in [min_c s_lo, min_c s_hi], hi_t in [max_c s_lo, max_c s_hi]; step = max((hi - lo) / 254, 1e-6 A, 1e-30).
    -> (lo_lo, lo_hi, step_lo, step_hi, A_hi), each (T,)"""
    lo_lo, lo_hi = s_lo.min(axis=1), s_hi.min(axis=1)
    hi_lo, hi_hi = s_lo.max(axis=1), s_hi.max(axis=1)
    A_hi = np.maximum(np.maximum(np.abs(lo_lo), np.abs(lo_hi)), np.maximum(np.abs(hi_lo), np.abs(hi_hi)))
    A_lo = np.maximum(_absmin(lo_lo, lo_hi), _absmin(hi_lo, hi_hi))
    step_lo = np.maximum(np.maximum((hi_lo - lo_hi) / CELL8_STEPS, 1e-6 * A_lo), 1e-30)
    step_hi = np.maximum(np.maximum((hi_hi - lo_lo) / CELL8_STEPS, 1e-6 * A_hi), 1e-30)
    return lo_lo, lo_hi, step_lo, step_hi, A_hi


def cell8_table(s_lo, s_hi):
    """requantise_cells_kernel on intervals: cell = clamp(rint(X / step - lo / step), 0, 255) of the fp16 value X, and the
    value pass 1 reads back, lo + cell * step.  The position (X - lo) / step is monotone in X and, at a fixed step, in lo,
    and at a fixed lo in 1 / step: its extremes are at the corners.  A cell widens only when a rounding edge lies inside
    the position's interval.  -> (V_lo, V_hi, cell_lo, cell_hi), each (T, K)"""
    lo_lo, lo_hi, step_lo, step_hi, _ = cell8_ranges(s_lo, s_hi)
    X_lo, X_hi = f16(s_lo), f16(s_hi)
    col = lambda v: v[:, None]
    corners = [(lo, st) for lo in (col(lo_lo), col(lo_hi)) for st in (col(step_lo), col(step_hi))]
    p_lo = np.minimum.reduce([(X_lo - lo) / st for lo, st in corners])
    p_hi = np.maximum.reduce([(X_hi - lo) / st for lo, st in corners])
    # the fp32 roundings of 1 / step, lo / step and the fused multiply-add, in cells
    slack = 4.0 * U * (np.maximum(np.abs(X_lo), np.abs(X_hi)) + col(np.maximum(np.abs(lo_lo), np.abs(lo_hi)))) / col(step_lo)
    cell_lo = np.clip(np.rint(p_lo - slack), 0.0, 255.0)
    cell_hi = np.clip(np.rint(p_hi + slack), 0.0, 255.0)
    return col(lo_lo) + cell_lo * col(step_lo), col(lo_hi) + cell_hi * col(step_hi), cell_lo, cell_hi


def cell8_residual_products(o, Q, step_lo, step_hi):
    """step_t * (fp16(Q_t / step_t) . r') as an interval over step_t in [step_lo, step_hi], (T, n_emb) each"""
    Q = as_query(Q)
    q1, q2 = f16(Q / step_hi[None, :]), f16(Q / step_lo[None, :])
    q_min, q_max = np.minimum(q1, q2), np.maximum(q1, q2)
    r_pos, r_neg = np.maximum(o.r16, 0.0), np.minimum(o.r16, 0.0)
    D_lo = q_min.T @ r_pos + q_max.T @ r_neg
    D_hi = q_max.T @ r_pos + q_min.T @ r_neg
    a, b = step_lo[:, None], step_hi[:, None]
    return np.minimum(D_lo * a, D_lo * b), np.maximum(D_hi * a, D_hi * b)


def passage_bounds(o, Q, products=3, rows8=False, delta3=DELTA3):
    """(lo, hi), each (n_docs,): the interval of every passage's pass-1 score before the accumulation slack; nan for an
    empty passage."""
    s_lo, s_hi = table_interval(o, Q, products, delta3)
    if rows8:
        _, _, step_lo, step_hi, _ = cell8_ranges(s_lo, s_hi)
        V_lo, V_hi, _, _ = cell8_table(s_lo, s_hi)
        D_lo, D_hi = cell8_residual_products(o, Q, step_lo, step_hi)
        P_lo, P_hi = V_lo[:, o.codes0] + D_lo, V_hi[:, o.codes0] + D_hi
    else:
        qr = residual_products(o, Q)
        P_lo, P_hi = f16(s_lo)[:, o.codes0] + qr, f16(s_hi)[:, o.codes0] + qr
    S_lo, S_hi = scaled(P_lo, P_hi, o)
    return o.passage_sums(S_lo), o.passage_sums(S_hi)


def gamma(o, Q, rows8=False, products=3):
    """the accumulation slack of one passage score (the derivation is in the module's docstring)"""
    qn = np.linalg.norm(as_query(Q), axis=0)
    im = o.im + o.inv_half_step
    M = im * qn * (o.cn + o.rb)
    per_token = 132.0 * U * M
    if rows8:
        _, _, _, step_hi, A_hi = cell8_ranges(*table_interval(o, Q, products))
        per_token = im * (130.0 * U * (A_hi + 255.0 * step_hi + qn * o.rb) + 1280.0 * U * step_hi) + 3.0 * U * M
    return float(per_token.sum() + 32.0 * U * M.sum())
