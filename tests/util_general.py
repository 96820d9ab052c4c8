"""Helpers of the general-shape search tests (tests/test_general_shapes_cpu.py, tests/test_gpu_general_shapes.py): which
kernels a shape reaches, the case table both files walk, ragged indexes, and the float64 restatement of the exact score
with its derived error bound.  No tests here."""
import functools

import numpy as np

from colbert_jl_amd import synthetic

ROUTES = ("batched32", "batched64", "loop_mfma", "scalar")


def expected_route(dim, nbits, T):
    """The kernels a search of this shape runs, restated from the host code (csrc/search.hip):

        run_search:          if (s->generic || T > 128) return run_search_general(...)      generic = !(dim == 128 && nbits <= 4)
        general_batched_ok:  s->dim % 4 == 0 && s->dim <= 256 && T <= 128
        run_search_general:  batched ->  s->dim <= 128 ? generic_score_mfma_fast_kernel<32> : <64>   (generic_cells_mfma_kernel alike)
                             else, one query at a time (run_retrieve_general = generic_cells_kernel + select_by_sort):
                                 T <= 16 * kGenericMaxTokenGroups (= 512) && s->dim % 4 == 0 ? generic_score_mfma_kernel
                                                                                             : generic_score_kernel

    create enforces dim % 8 == 0, so the dim % 4 tests never fail.  In the batched route the query is staged in
    4 * ((1 << nbits) + T * (dim + 1)) bytes of LDS; above 64 KB run_search_general raises the kernel's limit first
    (`lds_bytes` below)."""
    if dim % 8 or nbits not in (1, 2, 4, 8) or T < 1:
        raise ValueError((dim, nbits, T))
    if dim == 128 and nbits <= 4 and T <= 128:
        raise ValueError("the tuned path, not a general shape")
    if dim <= 256 and T <= 128:
        return "batched32" if dim <= 128 else "batched64"
    return "loop_mfma" if T <= 512 else "scalar"


def lds_bytes(dim, nbits, T):
    """dynamic LDS of generic_score_mfma_fast_kernel (run_search_general: `lds`)"""
    return 4 * ((1 << nbits) + T * (dim + 1))


# The case table of the issue: (dim, nbits, T, K, route, n_docs).  nprobe = 2 (1 at K = 1), three queries, k = 30; the
# index is make_index(doclen_mean=20, doclen_std=12), the seed is 500 + the row's position -- except dim 200 / nbits 8 (705):
# with seed 505 four of the oracle's first 29 neighbouring float64 scores lie closer than twice the bound, more than the
# tenth tests/test_general_shapes_cpu.py lets the order check leave out; with 705 two do.
CASES = [
    (8, 1, 1, 1, "batched32", 600),        # smallest everything; K = 1 tile tail, nprobe = 1
    (8, 8, 600, 33, "scalar", 300),        # the scalar kernel, T > 256 threads (t += blockDim.x), K tail
    (128, 2, 513, 64, "scalar", 300),      # first T past the MFMA limit on the tuned index shape
    (128, 2, 512, 64, "loop_mfma", 300),   # last T inside it: all 32 token groups
    (136, 2, 17, 65, "batched64", 600),    # ks = 34 of KSMAX 64: predicated tail, T tail, K tail
    (200, 8, 33, 17, "batched64", 600),    # nbits 8 wide rows, one partial centroid tile
    (256, 8, 128, 96, "batched64", 400),   # more than 64 KB of LDS, all 8 token groups full
    (256, 4, 64, 96, "batched64", 600),    # first T whose staged query passes 64 KB
    (120, 4, 16, 80, "batched32", 600),    # ks = 30 of 32, exactly one token group
    (264, 4, 20, 96, "loop_mfma", 600),    # first dim past the batched route
    (768, 1, 40, 40, "loop_mfma", 300),    # encoder-width rows, nbits 1
    (384, 2, 130, 50, "loop_mfma", 300),   # dim > 256 and T > 128 together
]
CASE_IDS = [f"dim{c[0]}-nbits{c[1]}-T{c[2]}-K{c[3]}" for c in CASES]
CASE_K = 30
CASE_SEEDS = {5: 705}


@functools.lru_cache(maxsize=None)
def case_inputs(i):
    """(index, queries (dim, T, 3), nprobe) of row i of CASES -- read-only, shared by the tests that need them"""
    dim, nbits, T, K, _, n_docs = CASES[i]
    idx = synthetic.make_index(seed=CASE_SEEDS.get(i, 500 + i), n_docs=n_docs, K=K, dim=dim, nbits=nbits, doclen_mean=20, doclen_std=12)
    Qs = synthetic.make_queries(idx, 600 + i, 3, T=T)
    Qs.setflags(write=False)
    return idx, Qs, min(2, K)


def ragged_index(idx, forced, seed, reps=20):
    """`idx` with the lengths of `reps * len(forced)` randomly chosen passages forced to the values of `forced` (in turn):
    codes and residuals are extended by wrap-around where the forced lengths ask for more embeddings than were generated,
    cut where they ask for fewer, and the IVF is rebuilt from the codes (synthetic.build_ivf).  `idx` is left as it is."""
    dl = idx["doclens"].copy()
    n_docs = dl.size
    rng = np.random.default_rng(seed)
    for j, pid in enumerate(rng.choice(n_docs, size=reps * len(forced), replace=False)):
        dl[pid] = forced[j % len(forced)]
    n_emb = int(dl.sum())
    codes, res = idx["codes"], idx["residuals"]
    if n_emb > codes.shape[0]:
        extra = n_emb - codes.shape[0]
        codes = np.concatenate([codes, codes[:extra]])
        res = np.concatenate([res, res[:, :extra]], axis=1)
    out = dict(idx, doclens=dl, codes=codes[:n_emb], residuals=np.asfortranarray(res[:, :n_emb]))
    out["ivf"], out["ivf_lengths"] = synthetic.build_ivf(out["codes"], idx["ivf_lengths"].size)
    return out


def scores_float64(idx, Q, pids):
    """MaxSim of query Q (dim, T) with the passages `pids` (1-based) in float64: sum over the tokens of the largest dot
    product with the passage's decompressed, normalised embeddings (synthetic.decompress_numpy on float64 copies of the
    centroids and bucket weights: no step of it rounds to fp32).  An empty passage scores 0 here; it is never a candidate."""
    f64 = dict(idx, centroids=np.asarray(idx["centroids"], dtype=np.float64),
               bucket_weights=np.asarray(idx["bucket_weights"], dtype=np.float64))
    off = np.concatenate([[0], np.cumsum(np.asarray(idx["doclens"], dtype=np.int64))])
    q = np.asarray(Q, dtype=np.float64)
    out = np.zeros(len(pids), dtype=np.float64)
    for i, p in enumerate(np.asarray(pids, dtype=np.int64)):
        lo, hi = int(off[p - 1]), int(off[p])
        if hi > lo:
            D = synthetic.decompress_numpy(f64, np.arange(lo, hi))
            assert D.dtype == np.float64
            out[i] = (q.T @ D).max(axis=1).sum()
    return out


def score_bound(dim, T, Q):
    """An upper bound of |fp32 exact score - float64 score| of one passage: 2^-24 (2 dim + T + 16) sum_t ||q_t||.

    With u = 2^-24 (fp32 unit roundoff) and every decompressed row x normalised to unit length:
      * a dim-term fp32 fmaf chain <q_t, x> errs by at most about dim u ||q_t|| ||x|| = dim u ||q_t||;
      * x itself carries a relative error of at most about (dim / 4 + 6) u: the fp32 sum centroid + bucket weight (1),
        the four interleaved partial sums of squares of dim / 4 terms each and their two-level sum (dim / 4 + 2, halved by
        the square root), the square root, the added FLT_EPSILON and the division (3) -- each moves <q_t, x> by at most that
        times ||q_t||;
      * the sequential fp32 sum of the T maxima m_t adds at most (T - 1) u sum_t |m_t| <= (T - 1) u sum_t ||q_t||.
    Sum over the tokens: u (dim + dim / 4 + 6 + T - 1) sum_t ||q_t||, rounded up to the expression returned.  The maximum
    over a passage's rows moves by no more than the largest error of a row.  Derived, not measured; the measured ratios are
    in profiles/general_shapes.md."""
    norms = np.linalg.norm(np.asarray(Q, dtype=np.float64), axis=0)
    assert norms.shape == (T,)
    return 2.0 ** -24 * (2 * dim + T + 16) * float(norms.sum())


def msb_first_fields(residuals, nbits):
    """The packed residual bytes with the order of the 8 / nbits bit fields of every byte reversed: reading these
    LSB-first is reading the original bytes MSB-first (the layout error the float64 check has to see)."""
    r = np.asarray(residuals, dtype=np.uint8)
    per, mask = 8 // nbits, (1 << nbits) - 1
    out = np.zeros_like(r)
    for i in range(per):
        out |= ((r >> (nbits * i)) & mask) << (nbits * (per - 1 - i))
    return np.asfortranarray(out)


# ---- the random configurations of test_general_search_random_configurations ----------------------------------------------
FUZZ_DIMS = [8, 16, 24, 40, 64, 96, 120, 136, 200, 256, 264, 384]
FUZZ_T = [1, 3, 16, 17, 32, 33, 100, 128, 129, 200, 513]
FUZZ_BASE = 9000
# the route of each of the 10 default seeds (expected_route of its dim, nbits, T): all four occur.  Seed 6 (dim 64, T 513) is the
# scalar kernel; 3, 7, 9 (dim 384 / T 200, dim 264 / T 32, dim 264 / T 128) the loop-form MFMA kernel.
# tests/test_general_shapes_cpu.py keeps this list true.
FUZZ_ROUTES = ["batched64", "batched32", "batched32", "loop_mfma", "batched64", "batched64", "scalar", "loop_mfma", "batched32",
               "loop_mfma"]


def fuzz_configuration(seed):
    rng = np.random.default_rng(FUZZ_BASE + seed)
    cfg = dict(dim=int(rng.choice(FUZZ_DIMS)), nbits=int(rng.choice([1, 2, 4, 8])), K=int(rng.integers(1, 301)),
               n_docs=int(rng.integers(40, 3001)), T=int(rng.choice(FUZZ_T)), B=int(rng.integers(1, 10)))
    cfg["nprobe"] = int(rng.integers(1, min(cfg["K"], 8) + 1))
    cfg["k"] = int(min(cfg["n_docs"], rng.choice([1, 10, 100, cfg["n_docs"]])))
    cfg["scale"] = float(rng.choice([1.0, 0.25, 40.0])) if rng.integers(0, 3) == 0 else 1.0
    cfg["mean"], cfg["std"], cfg["topical"] = float(rng.integers(4, 60)), float(rng.integers(0, 30)), bool(rng.integers(0, 2))
    return cfg
