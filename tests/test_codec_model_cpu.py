"""The numpy references of tests/codec_model.py against the CPU oracle, on every input tests/test_gpu_codec_edges.py feeds the
device -- and the properties of those inputs that make the GPU file worth running, asserted from the references alone:

  bucket edges   at least half of all residual entries equal a cutoff bit for bit; every distinct cutoff value is hit at every
                 bit offset (d * nbits) mod 8 that the shape has; the neighbours of every cutoff, a value below the first and
                 above the last, +0.0, -0.0 and (K = 1) +-Inf all occur; the cutoffs hold a 0.0, a pair and a triple
  statistics     every case with tied held-out columns has fewer distinct cutoffs than cutoffs (1 bit: its one cutoff equals
                 both weights)
  decompress     every byte value at every byte position of a row; codes 1 and K; one column is the zero vector
  epilogue       a document with every token skipped, a kept all-zero token, masked query rows with negative entries

No GPU.  The oracle agreed with the references bit for bit on every finite case when they were written; for a NaN residual it
gave bucket 0 until its search was put under isless like residual.jl:350's searchsortedfirst (test_nan_*)."""
import numpy as np
import pytest

from tests import codec_model as cm

EDGE, NAN, EPI = cm.EDGE, cm.NAN, cm.EPI


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- bucket edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,dim,K", EDGE)
def test_edge_inputs_sit_on_the_cutoffs(nbits, dim, K):
    variants = cm.edge_case(nbits, dim, K)
    cuts = np.concatenate([v[1] for v in variants])
    assert np.any(u32(cuts) == 0), "no cutoff equal to +0.0"
    runs = [np.unique(v[1], return_counts=True)[1] for v in variants]
    if nbits >= 2:
        assert any(np.any(r == 2) for r in runs) and any(np.any(r == 3) for r in runs)
    for cent, cut, embs, codes, R in variants:
        assert np.all(np.diff(cut) >= 0) and len(cut) == (1 << nbits) - 1 and 256 < R.shape[1] <= 400
        assert cm.bits_equal(cm.residuals_of(cent, embs, codes), R)
        hit = np.isin(u32(R), u32(cut))
        assert hit.mean() >= 0.5, hit.mean()
        off = cm.offsets_of(dim, nbits)
        for o in np.unique(off):
            seen = np.unique(u32(R[off == o]))
            assert np.all(np.isin(np.unique(u32(cut)), seen)), f"a cutoff is never hit at bit offset {o}"
        u, other = cm.edge_values(cut, with_inf=(K == 1))
        assert np.all(np.isin(u32(other), u32(R))), "an off-cutoff value is missing"
        assert np.any(u32(R) == 0x80000000) and np.any(u32(R) == 0)
        assert np.any(R < cut[0]) and np.any(R > cut[-1])
        idx = cm.ref_indices(cent, cut, embs, codes)
        assert idx.min() == 0 and idx.max() == len(cut)
        if K > 1:
            assert np.array_equal(codes, np.arange(len(codes)) % K + 1) and np.all(np.isfinite(embs))


@pytest.mark.parametrize("nbits,dim,K", EDGE)
def test_ref_pack_equals_the_oracle_on_the_edges(oracle, nbits, dim, K):
    for cent, cut, embs, codes, R in cm.edge_case(nbits, dim, K):
        rc, rr = oracle.compress(cent, cut, dim, nbits, embs)
        assert np.array_equal(rc, codes)
        assert np.array_equal(rr, cm.ref_pack(cent, cut, dim, nbits, embs, codes))
        assert np.array_equal(oracle.bucket_indices(R, cut), cm.ref_indices(cent, cut, embs, codes))


def test_ref_pack_bit_positions():
    """a single bucket index of all ones at dim d sets exactly the bits d*nbits .. d*nbits + nbits - 1, LSB of a byte first"""
    for nbits in cm.NBITS_ALL:
        for d in (0, 1, 7):
            idx = np.zeros((8, 1), np.int64); idx[d, 0] = (1 << nbits) - 1
            bits = np.unpackbits(cm.pack_indices(idx, nbits)[:, 0], bitorder="little")
            assert np.array_equal(np.nonzero(bits)[0], np.arange(d * nbits, (d + 1) * nbits))
            assert np.array_equal(cm.unpack_indices(cm.pack_indices(idx, nbits), 8, nbits), idx)


@pytest.mark.parametrize("nbits,dim", NAN)
def test_nan_goes_to_the_last_bucket(oracle, nbits, dim):
    cent, cut, embs, codes, R = cm.nan_case(nbits, dim)
    idx = cm.ref_indices(cent, cut, embs, codes)
    nan = np.isnan(R)
    assert nan.sum() == R.shape[1] and np.all(nan.any(axis=1)) and np.all(idx[nan] == len(cut))
    clean = np.where(nan, np.float32(0), R)
    assert np.array_equal(idx[~nan], np.searchsorted(cut, clean, side="left")[~nan])     # every other dim: unaffected
    rc, rr = oracle.compress(cent, cut, dim, nbits, embs)
    assert np.array_equal(rc, codes)
    assert np.array_equal(rr, cm.ref_pack(cent, cut, dim, nbits, embs, codes))
    assert np.array_equal(oracle.bucket_indices(R, cut), idx)


def test_nan_bucket_index_of_the_oracle(oracle):
    got = oracle.bucket_indices(np.array([[np.nan, -np.inf, np.inf, 0.0]], np.float32), [-0.1, 0.0, 0.1])
    assert got.ravel().tolist() == [3, 0, 3, 1]


# ---- statistics ----------------------------------------------------------------------------------------------------------
def test_ref_quantile7_small_and_tied():
    one = np.array([0.375], np.float32)
    for p in (0.0, 0.25, 0.5, 1.0):
        assert cm.ref_quantile7(one, p) == one[0]                  # n = 1 is special-cased: both neighbours are v[0]
    v = np.array([-1.0, 0.0, 0.0, 0.0, 2.0], np.float32)
    assert cm.ref_quantile7(v, 0.5) == 0 and cm.ref_quantile7(v, 0.3) == 0 and cm.ref_quantile7(v, 0.75) == 0
    assert cm.ref_quantile7(v, 0.125) == np.float32(-0.5) and cm.ref_quantile7(v, 1.0) == 2 and cm.ref_quantile7(v, 0.0) == -1


@pytest.mark.parametrize("count", [1, 2, 3, 8, 16, 17])
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_ref_quantiles_equal_the_oracle_with_few_values(oracle, nbits, count):
    """fewer values than quantiles, one value, and runs of equal values across j, j + 1"""
    rng = np.random.default_rng(4600 + count)
    v = cm.grid(rng, count, 0.5, cm.GRID_R)
    v[: count // 2] = v[0]
    cut, w = cm.ref_cutoffs_and_weights(nbits, v)
    ocut, ow = oracle.bucket_cutoffs_and_weights(nbits, v)
    assert cm.bits_equal(cut, ocut) and cm.bits_equal(w, ow)


@pytest.mark.parametrize("dim,K,n,nbits,share", cm.STATS_CASES)
def test_ref_stats_equal_the_oracle(oracle, dim, K, n, nbits, share):
    cent, held, codes = cm.stats_case(dim, K, n, nbits, share)
    cut, w, avg = cm.ref_stats(nbits, cent, held, codes)
    ocut, ow, oavg, ocodes = oracle.compute_avg_residuals(nbits, cent, held)
    assert np.array_equal(ocodes, codes)
    assert cm.bits_equal(cut, ocut) and cm.bits_equal(w, ow)
    assert abs(float(oavg) - avg) <= 1e-6 * avg
    r = cm.residuals_of(cent, held, codes)
    assert np.count_nonzero(np.all(r == 0, axis=0)) == int(round(share * n))
    if share > 0 and nbits > 1:
        assert len(np.unique(cut)) < len(cut), "a tie-heavy case without tied cutoffs"
    if share > 0 and nbits == 1:                 # one cutoff cannot tie with another: it ties with both weights instead
        assert cut[0] == w[0] == w[1] == 0
    orc_codes, orc_res = oracle.compress(cent, cut, dim, nbits, held)
    assert np.array_equal(orc_codes, codes)
    assert np.array_equal(orc_res, cm.ref_pack(cent, cut, dim, nbits, held, codes))


# ---- decompress ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nbits", cm.DECOMPRESS_CASES)
def test_ref_decompress_equals_the_oracle(oracle, dim, nbits):
    cent, codes, res = cm.decompress_case(dim, nbits)
    assert res.shape == (dim // 8 * nbits, cm.N_ENUM)
    for i in range(res.shape[0]):
        assert np.array_equal(np.unique(res[i, :256]), np.arange(256)), f"byte position {i} misses a value"
    assert {1, cm.DECOMPRESS_K} <= set(codes.tolist())
    wa, wb = cm.weight_variants(nbits)
    assert np.any(u32(wa) == 0x80000000) and (nbits == 1 or np.any(u32(wa) == 0))
    assert len(np.unique(wb)) < len(wb) and (nbits < 3 or len(np.unique(wa[wa != 0])) < np.count_nonzero(wa != 0))
    for variant, w in enumerate((wa, wb)):
        ref = cm.decompress_ref(dim, nbits, variant)
        assert cm.bits_equal(ref, oracle.decompress(dim, nbits, cent, w, codes, res))
    assert np.all(cm.decompress_ref(dim, nbits, 0)[:, 256] == 0), "the zero column"
    idx = cm.unpack_indices(res, dim, nbits)
    assert idx.min() == 0 and idx.max() == (1 << nbits) - 1


def test_ref_decompress_long_equals_the_oracle(oracle):
    cent, w, codes, res, ref = cm.decompress_long()
    assert codes.size == cm.N_LONG > 2048 * 64 and cm.N_LONG % 16 == 1
    assert cm.bits_equal(ref, oracle.decompress(128, 2, cent, w, codes, res))


# ---- encoder epilogue ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,L,N,first_skipped", EPI)
def test_ref_epilogues_equal_the_oracle(oracle, dim, L, N, first_skipped):
    D, ids = cm.epilogue_case(dim, L, N, first_skipped)
    out, doclens = cm.ref_doc_epilogue(D, ids, cm.SKIPLIST)
    oout, odl = oracle.doc_epilogue(D, ids, cm.SKIPLIST)
    assert np.array_equal(doclens, odl) and out.shape[1] == doclens.sum()
    assert cm.bits_equal(out, oout)
    q = cm.ref_query_epilogue(D, ids, cm.SKIPLIST)
    assert cm.bits_equal(q, oracle.query_epilogue(D, ids, cm.SKIPLIST))
    keep = cm.skip_mask(ids, cm.SKIPLIST)
    if N > 1 or first_skipped:
        assert doclens[N // 2] == 0
    if N > 1 or not first_skipped:
        assert keep[0, N - 1] and not D[:, 0, N - 1].any()
    masked = np.broadcast_to(~keep[None], D.shape)
    assert np.array_equal(np.signbit(q[masked]), D[masked] < 0) and not q[masked].any()
    assert N == 1 or np.any(D[masked] < 0)
