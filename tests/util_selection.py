"""Inputs that put negative, zero and sign-mixed scores in front of the selection, ranking and merge kernels, shared by
tests/test_selection_model_cpu.py (which checks from the oracle alone that they do) and tests/test_gpu_selection_keys.py.

MaxSim takes a maximum over a passage's rows, and the candidates are the passages near the query's best centroids, so on the
synthetic indexes negating a query does NOT make its scores negative: some row of an 80-row passage always has a positive
product with -Q_t (measured: the scores of -Q on make_index(seed=3, n_docs=20_000, K=2048) lie in 5.2 .. 8.0).  Two
changes of the INDEX make the query variants do what their names say:

  shifted(idx)   every centroid moved by one fixed unit vector: all rows then share a large component, Q_t . row > 0 for
                 every token drawn from the index and every row, and every score of -Q is negative;
  short_index()  one row per passage: MaxSim is then linear in Q, and a query with half its tokens negated has candidates on
                 both sides of zero, spread over a dozen exponents.

No tests here."""
import functools

import numpy as np

from colbert_jl_amd import synthetic

N_MEDIUM, N_LARGE, N_SHORT = 20_000, 40_000, 60_000
LARGE_NPROBE = 16
VARIANTS = ("negated", "straddle", "zero", "one_hot_zero")
KS = (1, 10, 1000)
PRIOR_KS = (1, 10, 100, 1000)


def shifted(idx, amount=1.0, seed=90):
    m = np.random.default_rng(seed).standard_normal(idx["centroids"].shape[0])
    m /= np.linalg.norm(m)
    out = dict(idx)
    out["centroids"] = np.asfortranarray((idx["centroids"].astype(np.float64) + amount * m[:, None]).astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def medium_index():
    """the 20 000-passage index the prior and cursor tests share"""
    return synthetic.make_index(seed=3, n_docs=N_MEDIUM, K=2048)


@functools.lru_cache(maxsize=None)
def medium_shifted():
    return shifted(medium_index())


@functools.lru_cache(maxsize=None)
def short_index():
    """60 000 PASSAGES of one row each = 60 000 rows, a twenty-fifth of the medium index's 1.6 M: at K = 256 and nprobe = 2 a
    query then has 1 400 .. 3 000 candidates, enough for k = 1000 to cut inside the list (20 000 one-row passages give ~600)"""
    return shifted(synthetic.make_index(seed=3, n_docs=N_SHORT, K=256, constant_doclen=True, doclen_mean=1), 0.3)


@functools.lru_cache(maxsize=None)
def large_index():
    """every passage is a candidate with nprobe = 16: more than 32 768 candidates per query"""
    return shifted(synthetic.make_index(seed=5, n_docs=N_LARGE, K=16, doclen_mean=3))


@functools.lru_cache(maxsize=None)
def small_index():
    """300 passages: a cursor pages to its end"""
    return shifted(synthetic.make_index(seed=1, n_docs=300, K=64, constant_doclen=True, doclen_mean=1))


@functools.lru_cache(maxsize=None)
def general_index():
    """dim 64: the general-shape path (exact mode only, 64-bit sort keys)"""
    return shifted(synthetic.make_index(seed=77, n_docs=600, K=32, dim=64, nbits=2, doclen_mean=20, doclen_std=12))


INDEXES = {"medium": medium_index, "medium_shifted": medium_shifted, "short": short_index, "large": large_index,
           "small": small_index, "general": general_index}


def base_queries(idx, T=32, B=9, seed=4):
    return synthetic.make_queries(idx, seed, B, T=T)


def variant(Q, name):
    """Q (dim, T, B) -> the named variant, same shape"""
    Q = np.asfortranarray(Q, dtype=np.float32)
    T = Q.shape[1]
    if name == "plain":
        return Q.copy(order="F")
    if name == "negated":
        return np.asfortranarray(-Q)
    if name == "straddle":
        out = Q.copy(order="F")
        out[:, T // 2:, :] *= np.float32(-1)
        return out
    if name == "zero":
        return np.zeros_like(Q, order="F")
    if name == "one_hot_zero":                                 # ordinary, zero, negated, ordinary, zero, negated ...
        out = Q.copy(order="F")
        out[:, :, 1::3] = 0
        out[:, :, 2::3] *= np.float32(-1)
        return out
    if name == "zero_first":                                   # query 0 zero, its neighbours negated and ordinary
        out = Q.copy(order="F")
        out[:, :, 0] = 0
        out[:, :, 1::3] *= np.float32(-1)
        return out
    raise KeyError(name)


def tiled(Q, B):
    """the batch of B queries that repeats Q's: query j is Q[:, :, j % n]"""
    n = Q.shape[2]
    return np.asfortranarray(Q[:, :, np.arange(B) % n])


@functools.lru_cache(maxsize=None)
def queries(index_name, name, T=32):
    """shared between the tests: read-only"""
    Q = variant(base_queries(INDEXES[index_name](), T), name)
    Q.setflags(write=False)
    return Q


_RANKINGS = {}


def rankings(oracle, index_name, name, T=32, nprobe=2):
    """the oracle's full ranking of every query of queries(index_name, name, T): computed once, shared, never changed"""
    key = (index_name, name, T, nprobe)
    if key not in _RANKINGS:
        from tests.util_filter import filtered_ranking
        idx, Q = INDEXES[index_name](), queries(index_name, name, T)
        out = []
        for j in range(Q.shape[2]):
            rp, rs = filtered_ranking(oracle, idx, np.ascontiguousarray(Q[:, :, j]), nprobe)
            rp.setflags(write=False); rs.setflags(write=False)
            out.append((rp, rs))
        _RANKINGS[key] = out
    return _RANKINGS[key]


LOWEST = np.nextafter(np.float32(-np.finfo(np.float32).max), np.float32(0))      # -FLT_MAX + one ulp: |value| stays below FLT_MAX


# ---- priors (Route 2): values chosen from query 0's oracle scores so that E = fl32(e + fl32(w v)) is what the test wants ----
def prior_values(name, ranking0, n_docs, k=None):
    """one value per passage; `ranking0` = the oracle's full ranking (pids, scores) of query 0's candidates"""
    rp, rs = np.asarray(ranking0[0], np.int64), np.asarray(ranking0[1], np.float32)
    v = np.zeros(n_docs, np.float32)
    p = np.arange(1, n_docs + 1)
    if name == "mirror":                                       # E = fl32(e - fl32(2 e)) = -e exactly: the ranking reversed
        v[rp - 1] = np.float32(-2) * rs
    elif name == "zero_run":                                   # positives, a run of +0.0 across rank k, negatives
        lo, hi = k // 2, min(2 * k, rp.size - 1)
        v[rp[lo:hi + 1] - 1] = -rs[lo:hi + 1]
        v[rp[hi + 1:] - 1] = np.float32(-2) * rs[hi + 1:]
    elif name == "octaves":                                    # +-2^-20 .. 2^20
        sign = np.where((p // 41) % 2 == 0, 1.0, -1.0)
        v = (sign * np.exp2((p % 41) - 20.0)).astype(np.float32)
    elif name == "huge":                                       # one passage in fifty at 1e30 .. 1e38, either sign
        rng = np.random.default_rng(93)
        v = rng.normal(0.0, 0.5, n_docs).astype(np.float32)
        big = rng.random(n_docs) < 0.02
        v[big] = (rng.choice([-1.0, 1.0], n_docs) * 10.0 ** rng.uniform(30, 38, n_docs)).astype(np.float32)[big]
        v[rp[0] - 1], v[rp[-1] - 1] = np.float32(-1e38), np.float32(1e38)
    elif name == "huge_low":
        # all but one passage in 64 at one ulp above -FLT_MAX: for k = 1000 the k-th boosted score of every query is that value,
        # M = max |A| is it too, and tau - 2 delta (delta = 4 * 2^-24 * M = 8.1e31) overflows to -Inf: everything must be listed
        v = np.full(n_docs, LOWEST, np.float32)
        v[p % 64 == 0] = 0
    else:
        raise KeyError(name)
    assert v.dtype == np.float32 and np.all(np.isfinite(v))
    return v


def exponents(x):
    """the binary exponents of the non-zero finite values of x"""
    x = np.asarray(x, np.float32)
    return np.frexp(x[(x != 0) & np.isfinite(x)])[1]


# ---- records for the merge and threshold hooks (Route 3) ------------------------------------------------------------------
FLT_MAX = np.finfo(np.float32).max
TINY = np.float32(1e-45)                                       # the smallest subnormal


def special_scores(rng, n, kind):
    """n float32 scores of the named kind (no NaN, no -Inf: that is the padding)"""
    if kind == "negative":
        return -rng.uniform(0.5, 30.0, n).astype(np.float32)
    if kind == "mixed":
        return (rng.integers(-8, 9, n) / np.float32(4)).astype(np.float32)              # few values: ties, and +0.0 runs
    if kind == "octaves":
        return (rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-20, 21, n))).astype(np.float32)
    if kind == "edges":
        pool = np.array([FLT_MAX, -FLT_MAX, TINY, -TINY, 3 * TINY, np.float32(1e-39), np.float32(-1e-39), 0.0, 0.0, 0.0, 1.0, -1.0,
                         np.float32(2.0 ** -126), np.float32(-2.0 ** -126)], np.float32)
        return pool[rng.integers(0, pool.size, n)]
    raise KeyError(kind)


SCORE_KINDS = ("negative", "mixed", "octaves", "edges")


def sorted_lists(rng, n_lists, B, k, kind):
    """[n_lists][B][k] records as shards return them: every list sorted by (score descending, pid ascending), pids distinct
    over the lists of a query, padded with (0, -Inf) to a length of its own (0 .. k)"""
    P = np.zeros((n_lists, B, k), np.int64); S = np.full((n_lists, B, k), -np.inf, np.float32)
    for b in range(B):
        pool = rng.permutation(np.arange(1, n_lists * k + 1))
        for l in range(n_lists):
            m = k if (l == 0 and b == 0) else int(rng.integers(0, k + 1))
            p = np.sort(pool[l * k:l * k + m])
            s = special_scores(rng, m, kind)
            order = np.lexsort((p, -s.astype(np.float64)))
            P[l, b, :m], S[l, b, :m] = p[order], s[order]
    return P, S


def merged_reference(P, S, k):
    """the numpy stable sort of the union -> (pids (B, k), scores (B, k))"""
    L, B, _ = P.shape
    op = np.zeros((B, k), np.int64); os_ = np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        p, s = P[:, b].reshape(-1), S[:, b].reshape(-1)
        p, s = p[P[:, b].reshape(-1) > 0], s[P[:, b].reshape(-1) > 0]
        by_pid = np.argsort(p, kind="stable")
        p, s = p[by_pid], s[by_pid]
        order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
        op[b, :order.size], os_[b, :order.size] = p[order], s[order]
    return op, os_
