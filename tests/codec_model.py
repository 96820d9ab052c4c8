"""Plain numpy references of the residual codec (residual.jl, collection_indexer.jl:141-195, checkpoint.jl:27-71) and the
inputs that tests/test_codec_model_cpu.py and tests/test_gpu_codec_edges.py share.  Nothing here calls the CPU oracle or the
device: the oracle is one more implementation that the CPU file holds against these references.

  ref_pack         r = x - c[code] (one fp32 subtraction), idx = searchsortedfirst(cutoffs, r) - 1 under isless -- numpy's
                   searchsorted(side="left") orders NaN last as isless does --, bit b of idx[d] at flat position d*nbits + b,
                   least significant bit of a byte first (residual.jl:348-351, 197-208, 400-407)
  ref_quantile7    Statistics.quantile type 7 on sorted fp32 data with a float64 p, rounded to fp32 once
  ref_stats        cutoffs at q/2^nbits, weights at q/2^nbits + 0.5/2^nbits of ALL residual values pooled; float64 mean |r|
  ref_decompress   c[code] + w[idx] in fp32, divided by sqrt(canonical sum of squares) + eps
  ref_normalize, ref_doc_epilogue, ref_query_epilogue     mask by skiplist, D .* mask, normalise, compact per document

Exact inputs.  Centroid components are multiples of 2^-10 and cutoffs multiples of 2^-16, all below 1 in magnitude, so for a
residual r on the 2^-16 grid c + r and (c + r) - c are exact in fp32.  Residuals that are NOT on the grid (the neighbours
of a cutoff, -0.0) sit where the chosen centroid's component is +0.0, where x = r and x - 0 = r.  Every builder asserts
x - c[code] == r bit for bit before it returns, so "this residual equals that cutoff" is a fact about the input and not a hope.

Cached values are shared between tests and marked read-only.
"""
import functools

import numpy as np

EPS32 = np.float32(np.finfo(np.float32).eps)
GRID_C = 2.0 ** -10           # centroid components
GRID_R = 2.0 ** -16           # cutoffs and on-grid residuals
STEP = np.float32(37 * GRID_R)     # spacing of the distinct cutoff values (an odd multiple: all 16 grid bits in use)
ZERO_DIMS = (1, 2, 4, 7)      # d mod 8 where the K = 1 centroid is +0.0, the only slots that can hold an off-grid residual.
#   Each off-grid value (a cutoff's neighbour, -0.0, +-Inf) is placed ONCE, so it meets one bit offset only; these dims are
#   spread so that the off-grid values between them meet several offsets.  Only the cutoff hits cover every offset.


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


def bits_equal(a, b):
    """same fp32 bit patterns; a NaN matches a NaN whatever its payload"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- compress --------------------------------------------------------------------------------------------------------------
def pack_indices(idx, nbits):
    """(dim, n) bucket indices -> uint8 (dim/8*nbits, n): bit b of idx[d] at position d*nbits + b, LSB of each byte first"""
    idx = np.asarray(idx, dtype=np.int64)
    dim, n = idx.shape
    bits = (idx[:, None, :] >> np.arange(nbits, dtype=np.int64)[None, :, None]) & 1          # (dim, nbits, n)
    return np.packbits(bits.reshape(dim * nbits, n).astype(np.uint8), axis=0, bitorder="little")


def unpack_indices(res, dim, nbits):
    bits = np.unpackbits(np.asarray(res, np.uint8), axis=0, bitorder="little").reshape(dim, nbits, -1).astype(np.int64)
    return (bits << np.arange(nbits, dtype=np.int64)[None, :, None]).sum(axis=1)


def residuals_of(cent, embs, codes):
    with np.errstate(invalid="ignore"):
        return np.asarray(embs, np.float32) - np.asarray(cent, np.float32)[:, np.asarray(codes, np.int64) - 1]


def ref_indices(cent, cut, embs, codes):
    return np.searchsorted(np.asarray(cut, np.float32), residuals_of(cent, embs, codes), side="left")


def ref_pack(cent, cut, dim, nbits, embs, codes):
    assert cent.shape[0] == dim and len(cut) == (1 << nbits) - 1
    return pack_indices(ref_indices(cent, cut, embs, codes), nbits)


# ---- statistics ------------------------------------------------------------------------------------------------------------
def ref_quantile7(sorted32, p):
    v = np.asarray(sorted32, np.float32)
    n = v.size
    aleph = n * float(p) + (1.0 - float(p))
    j = min(max(int(np.trunc(aleph)), 1), n - 1)
    g = min(max(aleph - j, 0.0), 1.0)
    a, b = (v[0], v[0]) if n == 1 else (v[j - 1], v[j])
    diff = np.float32(b - a)                                    # the fp32 subtraction comes first
    return np.float32(np.float64(a) + g * np.float64(diff))


def ref_cutoffs_and_weights(nbits, values):
    v = np.sort(np.asarray(values, np.float32).ravel())
    nopt = 1 << nbits
    cut = np.array([ref_quantile7(v, q / nopt) for q in range(1, nopt)], np.float32)
    w = np.array([ref_quantile7(v, q / nopt + 0.5 / nopt) for q in range(nopt)], np.float32)
    return cut, w


def ref_stats(nbits, cent, held, codes):
    r = residuals_of(cent, held, codes)
    cut, w = ref_cutoffs_and_weights(nbits, r)
    return cut, w, float(np.mean(np.abs(r.astype(np.float64))))


# ---- decompress / normalise ------------------------------------------------------------------------------------------------
def canonical_sumsq(X):
    """fp32 sum of squares of every column: four partial sums over d mod 4, each ascending in d, then (p0 + p1) + (p2 + p3)"""
    X = np.asarray(X, np.float32)
    p = [np.zeros(X.shape[1], np.float32) for _ in range(4)]
    with np.errstate(over="ignore", invalid="ignore"):
        for d0 in range(0, X.shape[0], 4):
            for i in range(min(4, X.shape[0] - d0)):
                p[i] = p[i] + X[d0 + i] * X[d0 + i]
        return (p[0] + p[1]) + (p[2] + p[3])


def ref_normalize(X):
    X = np.asarray(X, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return X / (np.sqrt(canonical_sumsq(X)) + EPS32)[None, :]


def ref_decompress(dim, nbits, cent, w, codes, res):
    idx = unpack_indices(res, dim, nbits)
    x = np.asarray(cent, np.float32)[:, np.asarray(codes, np.int64) - 1] + np.asarray(w, np.float32)[idx]
    return ref_normalize(x)


def skip_mask(ids, skiplist):
    return ~np.isin(np.asarray(ids, np.int64), np.asarray(skiplist, np.int64))             # (L, N): True = kept


def ref_doc_epilogue(D, ids, skiplist):
    dim, L, N = D.shape
    keep = skip_mask(ids, skiplist)
    cols = np.asarray(D, np.float32).reshape(dim, L * N, order="F")
    flat = keep.reshape(L * N, order="F")                       # column l + n*L: documents in order, tokens in order
    return ref_normalize(cols[:, flat]), keep.sum(axis=0).astype(np.int64)


def ref_query_epilogue(Q, ids, skiplist):
    dim, L, N = Q.shape
    keep = skip_mask(ids, skiplist).astype(np.float32)
    masked = np.asarray(Q, np.float32) * keep[None, :, :]       # -0.0 where a negative entry is masked
    return ref_normalize(masked.reshape(dim, L * N, order="F")).reshape(dim, L, N, order="F")


# ---- inputs: centroids ---------------------------------------------------------------------------------------------------
def grid(rng, shape, lim, step):
    """random multiples of `step` in (-lim, lim) as fp32 (exact: |k| < 2^24)"""
    k = int(round(lim / step))
    return (rng.integers(-k + 1, k, size=shape) * step).astype(np.float32)


def edge_centroids(dim, K):
    """K = 1: a grid vector that is +0.0 at d mod 8 in ZERO_DIMS.  K > 1: 0.5 * one-hot vectors (all else +0.0)."""
    if K == 1:
        rng = np.random.default_rng(4100 + dim)
        c = grid(rng, (dim, 1), 1.0, GRID_C)
        c[c == 0] = np.float32(3 * GRID_C)
        c[[d for d in range(dim) if d % 8 in ZERO_DIMS], 0] = 0.0
        return c
    assert K <= dim
    c = np.zeros((dim, K), np.float32)
    c[np.arange(K), np.arange(K)] = 0.5
    return c


def assert_code_forced(cent, embs, codes, gap):
    """float64 inner products: the intended centroid beats every other by `gap` -- orders of magnitude above what 128 fp32
    roundings (or an fp16 candidate list with its proven margin) can move, so the code is a property of the input"""
    if cent.shape[1] == 1:
        return
    s = embs.astype(np.float64).T @ cent.astype(np.float64)                   # (n, K)
    won = s[np.arange(len(codes)), codes - 1].copy()
    s[np.arange(len(codes)), codes - 1] = -np.inf
    assert np.all(won - s.max(axis=1) >= gap), (won - s.max(axis=1)).min()


# ---- inputs: bucket edges ----------------------------------------------------------------------------------------------
NBITS_ALL = (1, 2, 3, 4, 5, 6, 7, 8, 16)
DIMS = (8, 24, 128)
EDGE = tuple((nbits, dim, 1) for nbits in NBITS_ALL for dim in DIMS) + tuple((3, dim, 8) for dim in DIMS)    # (nbits, dim, K)
NAN = tuple((nbits, dim) for nbits in NBITS_ALL for dim in DIMS)
MAX_DISTINCT = 255            # up to 8 bits the cutoffs are distinct values; 16 bits: see cutoff_variants
N_MIN = 261                   # columns: n * dim/8 * nbits output bytes fill more than one 256-thread block at every shape


def cutoff_variants(nbits):
    """The sorted cutoff vectors of one width.  From 3 bits on ONE vector has it all: a cutoff equal to 0.0, two equal
    adjacent cutoffs and three.  1 and 2 bits have too few cutoffs for that and take several vectors.
    16 bits: 65 535 distinct values would need 65 535 residuals per bit offset to hit each one, so the vector is 48 runs of
    equal values -- the shape quantiles of tied data have -- whose first two runs are 2 and 3 long and whose other boundaries are
    drawn at random, so that the indices of the runs' ends use all 16 bits.  A residual equal to a run's value hits every cutoff
    of the run."""
    s = STEP
    ncut = (1 << nbits) - 1
    if nbits == 1:
        return [np.array([0.0], np.float32), np.array([3 * s], np.float32)]
    if nbits == 2:
        return [np.array([-s, 0.0, 2 * s], np.float32), np.array([-s, -s, 0.0], np.float32), np.array([s, s, s], np.float32)]
    if ncut <= MAX_DISTINCT:
        cut = ((np.arange(ncut) - ncut // 2) * s).astype(np.float32)
        cut[1] = cut[2]
        cut[-3:] = cut[-1]
        return [cut]
    rng = np.random.default_rng(4200 + nbits)
    starts = np.concatenate([[0, 2, 5], 6 + np.sort(rng.choice(ncut - 7, size=45, replace=False))])
    lens = np.diff(np.concatenate([starts, [ncut]]))
    return [np.repeat(((np.arange(48) - 24) * s).astype(np.float32), lens)]


def edge_values(cut, with_inf):
    """(the distinct cutoff values, everything else the issue lists: both neighbours of each, one grid value below the
    first and one above the last, +0.0, -0.0, +-Inf)"""
    u = np.unique(cut)
    other = [np.nextafter(u, np.float32(-np.inf)), np.nextafter(u, np.float32(np.inf)),
             np.array([u[0] - STEP, u[-1] + STEP, 0.0, -0.0], np.float32)]
    if with_inf:
        other.append(np.array([np.inf, -np.inf], np.float32))
    return u.astype(np.float32), np.concatenate(other).astype(np.float32)


def offsets_of(dim, nbits):
    return (np.arange(dim) * nbits) % 8


def place_edges(cent, cut, nbits, codes, with_inf):
    """(dim, n) residuals or None when n columns are too few.  The other values go to slots whose centroid component is +0.0,
    last columns first, one dim after the other; every remaining slot takes a cutoff value, cycling through the distinct
    ones separately for each bit offset -- so each is hit at each offset, and hits are at least half of all entries."""
    dim, n = cent.shape[0], len(codes)
    u, other = edge_values(cut, with_inf)
    free0 = cent[:, codes - 1] == 0                                           # (dim, n): any residual is exact here
    slots = [(d, j) for j in range(n - 1, -1, -1) for d in range(dim) if free0[d, j]]
    if len(slots) < other.size or 2 * other.size > dim * n:
        return None
    R = np.zeros((dim, n), np.float32)
    taken = np.zeros((dim, n), bool)
    for v, (d, j) in zip(other, slots):
        R[d, j] = v
        taken[d, j] = True
    off = offsets_of(dim, nbits)
    for o in np.unique(off):
        dd, jj = np.nonzero(~taken & (off == o)[:, None])
        if dd.size < u.size:
            return None
        order = np.lexsort((dd, jj))                                          # column by column
        R[dd[order], jj[order]] = u[np.arange(dd.size) % u.size]
    return R


def embeddings_for(cent, codes, R):
    """x with x - c[code] == R bit for bit (asserted)"""
    c = cent[:, codes - 1]
    with np.errstate(invalid="ignore"):
        x = np.where(c == 0, R, c + R).astype(np.float32)
    got = residuals_of(cent, x, codes)
    assert bits_equal(got, R), "the input builder could not realise a residual exactly"
    return x


@functools.lru_cache(maxsize=None)
def edge_case(nbits, dim, K=1):
    """-> list of (cent, cut, embs, codes, R), one per cutoff vector of the width; n = the smallest from N_MIN on that fits (<= 400)"""
    out = []
    cent = edge_centroids(dim, K)
    for cut in cutoff_variants(nbits):
        for n in range(N_MIN, 401):
            codes = (np.arange(n) % K + 1).astype(np.uint32)
            R = place_edges(cent, cut, nbits, codes.astype(np.int64), with_inf=(K == 1))
            if R is not None:
                break
        else:
            raise AssertionError(f"no n <= 400 fits nbits={nbits} dim={dim} K={K}")
        embs = np.asfortranarray(embeddings_for(cent, codes.astype(np.int64), R))
        finite = np.where(np.isfinite(embs), embs, 0)
        assert_code_forced(cent, finite, codes.astype(np.int64), gap=0.02)
        out.append(frozen(np.asfortranarray(cent), cut, embs, codes, R))
    return out


@functools.lru_cache(maxsize=None)
def nan_case(nbits, dim):
    """K = 1, the first cutoff vector of the width; column j is NaN at dim j mod dim, so with n = 2 * dim + 3 every dim (and bit
    offset) carries a NaN; elsewhere the entries of the edge case.  -> (cent, cut, embs, codes, R)"""
    cent, cut, embs0, _, R0 = edge_case(nbits, dim)[0]
    n = 2 * dim + 3
    R = np.array(R0[:, (R0.shape[1] - 1 - np.arange(n)) % R0.shape[1]])          # the last columns hold the off-grid values
    R[np.arange(n) % dim, np.arange(n)] = np.nan
    codes = np.ones(n, np.uint32)
    embs = np.asfortranarray(embeddings_for(cent, codes.astype(np.int64), R))
    assert np.all(np.isnan(embs).sum(axis=0) == 1)
    return frozen(cent.copy(order="F"), cut.copy(), embs, codes, R)


# ---- inputs: statistics ------------------------------------------------------------------------------------------------
STATS_CASES = ((128, 7, 40, 2, 0.8), (8, 3, 1, 4, 0.0), (8, 3, 2, 8, 0.5), (16, 5, 33, 1, 1.0), (24, 4, 9, 4, 0.6),
               (128, 300, 700, 2, 0.0))        # (dim, K, n, nbits, share of held-out columns equal to a centroid)


@functools.lru_cache(maxsize=None)
def stats_case(dim, K, n, nbits, share):
    """-> (cent, held, codes): round(share * n) columns ARE their centroid (residual +0.0 in every dim), the others add a
    residual on the 2^-16 grid below 2^-5.  K <= dim: grid noise below 1/8 plus 0.5 on the diagonal; K > dim: grid noise
    below 1/4 (squared norms ~2.7 against cross products ~0.24 sigma).  The float64 gap is asserted."""
    rng = np.random.default_rng(4300 + dim + 7 * K + n)
    if K <= dim:
        cent = grid(rng, (dim, K), 0.125, GRID_C)
        cent[np.arange(K), np.arange(K)] = 0.5
    else:
        cent = grid(rng, (dim, K), 0.25, GRID_C)
    codes = rng.integers(1, K + 1, size=n).astype(np.uint32)
    R = grid(rng, (dim, n), 2.0 ** -5, GRID_R)
    R[:, rng.permutation(n)[: int(round(share * n))]] = 0.0
    held = np.asfortranarray(embeddings_for(cent, codes.astype(np.int64), R))
    assert_code_forced(cent, held, codes.astype(np.int64), gap=0.05)
    return frozen(np.asfortranarray(cent), held, codes)


# ---- inputs: decompress ----------------------------------------------------------------------------------------------------
DECOMPRESS_CASES = ((128, 1), (128, 2), (128, 4), (128, 8), (8, 2), (8, 8), (24, 2), (24, 8))     # (dim, nbits)
DECOMPRESS_NS = (1, 15, 16, 17, 63, 64, 65)
DECOMPRESS_K = 4
N_ENUM = 261                  # 256 byte values + the zero column and four more; 261 mod 16 = 5
N_LONG = 2048 * 64 + 17       # decompress_dim128_kernel: second grid-stride trip, last group clamped


def weight_variants(nbits):
    """Weight vectors on the 2^-16 grid: [0] has -0.0 and +0.0 side by side (and from 3 bits on a duplicate as well), [1] has a
    duplicate and no zero."""
    nw = 1 << nbits
    s = np.float32(53 * GRID_R)
    base = ((np.arange(nw) - nw // 2) * s + s / 2).astype(np.float32)          # no zero, no duplicate
    a = base.copy()
    if nw == 2:
        a[0] = -0.0
    else:
        a[nw // 2 - 1], a[nw // 2] = -0.0, 0.0
    if nw >= 8:
        a[1] = a[0]
    b = base.copy()
    b[-1] = b[-2]
    return [a, b]


def zero_index(nbits):
    return 0 if nbits == 1 else (1 << nbits) // 2              # where weight_variants(nbits)[0] holds a zero (+0.0 from 2 bits on)


@functools.lru_cache(maxsize=None)
def decompress_case(dim, nbits):
    """-> (cent (dim, 4), codes[N_ENUM], res (rows, N_ENUM)): byte i of column j is (j + 37 i) mod 256 for j < 256 -- every
    byte value at every byte position; codes cycle 1, K, 2, 3; centroid 2 is the zero vector (+0.0 and -0.0 components) and
    column 256 carries code 2 with every index = zero_index: with the first weight vector it decompresses to the zero vector."""
    rng = np.random.default_rng(4400 + dim + nbits)
    rows = dim // 8 * nbits
    cent = grid(rng, (dim, DECOMPRESS_K), 0.25, GRID_C)
    cent[:, 1] = np.where(np.arange(dim) % 3 == 0, np.float32(-0.0), np.float32(0.0))
    codes = np.array([1, DECOMPRESS_K, 2, 3], np.uint32)[np.arange(N_ENUM) % 4]
    res = ((np.arange(N_ENUM)[None, :] + 37 * np.arange(rows)[:, None]) % 256).astype(np.uint8)
    codes[256] = 2
    res[:, 256] = pack_indices(np.full((dim, 1), zero_index(nbits)), nbits)[:, 0]
    return frozen(np.asfortranarray(cent), codes, np.asfortranarray(res))


@functools.lru_cache(maxsize=None)
def decompress_ref(dim, nbits, variant):
    cent, codes, res = decompress_case(dim, nbits)
    return frozen(ref_decompress(dim, nbits, cent, weight_variants(nbits)[variant], codes, res))


@functools.lru_cache(maxsize=None)
def decompress_long():
    """dim 128, 2 bits, N_LONG columns: the enumeration tiled -> (cent, w, codes, res, reference)"""
    cent, codes, res = decompress_case(128, 2)
    w = weight_variants(2)[0]
    j = np.arange(N_LONG) % N_ENUM
    return cent, w, frozen(codes[j]), frozen(np.asfortranarray(res[:, j])), frozen(np.asfortranarray(decompress_ref(128, 2, 0)[:, j]))


# ---- inputs: encoder epilogue --------------------------------------------------------------------------------------------
EPILOGUE_CASES = ((8, 1, 1), (24, 1, 5), (128, 7, 1), (24, 5, 4), (128, 6, 3), (8, 3, 70))        # (dim, L, N)
SKIPLIST = (1, 3, 7, 11, 999)
EPI = tuple(c + (False,) for c in EPILOGUE_CASES) + ((8, 1, 1, True), (128, 7, 1, True))       # (dim, L, N, first_skipped)


@functools.lru_cache(maxsize=None)
def epilogue_case(dim, L, N, first_skipped=False):
    """-> (D (dim, L, N), ids (L, N)).  Document N // 2 has every token on the skiplist (with N = 1 only if first_skipped);
    token 0 of the last document is kept and all zero; about a third of the other tokens are skipped."""
    rng = np.random.default_rng(4500 + dim + 3 * L + N)
    D = rng.normal(size=(dim, L, N)).astype(np.float32)
    ids = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 999, 1000], np.int32), size=(L, N)).astype(np.int32)
    if N > 1 or first_skipped:
        ids[:, N // 2] = np.array(SKIPLIST, np.int32)[np.arange(L) % len(SKIPLIST)]
    if N > 1 or not first_skipped:
        ids[0, N - 1] = 2
        D[:, 0, N - 1] = 0.0
    return frozen(np.asfortranarray(D), np.asfortranarray(ids))
