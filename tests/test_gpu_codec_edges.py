"""The residual codec on the device against the plain numpy references of tests/codec_model.py, at the inputs where a codec
goes wrong without a Gaussian test noticing: residuals that EQUAL a cutoff, widths whose bucket index straddles bytes, quantiles
of tied or very few values, NaN, and every byte value at every byte position.  tests/test_codec_model_cpu.py holds the same
references against the CPU oracle on the same inputs and asserts the properties the inputs are built to have.

Which kernel and branch each case reaches (codec_kernels.hpp, codec.hip):

  test_bucket_edges[nbits-dim]       pack_residuals_kernel through clb_compress AND clb_codec_compress_device (host and device
      K = 1                          centroids, two chunks of n // 2 and n - n // 2 columns).  n = 261 here (edge_case takes the
                                     smallest n from 261 to 400 that fits): n * dim/8 * nbits bytes, one thread each, 2 .. 261
                                     blocks.  nbits 3, 5, 6, 7: an index straddles a byte at p = d * nbits + b; 16: an index
                                     fills two bytes and the binary search runs 16 levels.  At
                                     least half of the entries equal a cutoff: `cutoffs[m - 1] < r` false on equality, runs of
                                     2, 3 (and at 16 bits thousands of) equal cutoffs, +-0.0 against a 0.0 cutoff, denormal
                                     neighbours of 0.0, +-Inf.  Codes: nearest_centroid_mfma_kernel (dim 128, K < 32) and
                                     nearest_centroid_generic_kernel (dim 8, 24) with one centroid -- and non-finite scores.
  test_bucket_edges_eight_centroids  the same kernels with K = 8 one-hot centroids: the row `codes[e] - 1` the residual is taken
                                     from varies per column; codes asserted.
  test_nan_lands_in_the_last_bucket  pack_residuals_kernel: the `r != r` arm of the search.
  test_statistics[...]               clb_compute_avg_residuals: heldout_residual_kernel, sort_keys_f32, quantile7_device --
                                     (8, 3, 1, 4): 8 values for 31 quantiles; (8, 3, 2, 8): 16 values for 511, j clamped to
                                     n - 1 at the top; tied cases: v[j - 1] == v[j] so g must not matter; (16, 5, 33, 1, 1.0):
                                     every value 0.0, the atomicAdd of |r| never fires; (128, 300, 700, 2): the K >= 32 list path
                                     of nearest_centroids.  Then pack_residuals_kernel with the cutoffs the device itself produced.
  test_decompress[dim-nbits-n]       (128, 1 | 2 | 4): decompress_dim128_kernel<NBITS> -- n = 1, 15: one clamped group; 16: one
                                     full group; 17: a second, clamped; 63, 64, 65: 4 waves of a block, then a second block;
                                     261: the byte enumeration and the zero column (0 / eps, and -0.0 kept, through div_by_reciprocal_signed_zero).
                                     (128, 8) and dims 8, 24: decompress_generic_kernel, blocks of 64 columns.
  test_decompress_second_grid_stride_trip   decompress_dim128_kernel<2> at n = 2048 * 64 + 17: grid capped at 2048 blocks, block 0
                                     wave 0 takes group 8192 in a second trip, whose lanes 1 .. 15 are clamped to e = n - 1.
  test_epilogue[...]                 epilogue_mask_kernel + epilogue_normalize_kernel, both forms: compacting (doc_start, a
                                     document of length 0, n_out = 0 early return) and in place (masked rows: (x * 0) / eps keeps
                                     the sign); N = 70: a second block of the mask kernel.  epilogue_query_fused_kernel is reached
                                     through the encoder only and is not run here.
"""
import numpy as np
import pytest

from colbert_jl_amd import codec
from tests import codec_model as cm

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def compress_every_way(cent, cut, dim, nbits, embs):
    """(name, codes, residual bytes (rows, n)) from clb_compress and from the resident codec with host and with device
    centroids, the latter two fed in two chunks of n // 2 and n - n // 2 columns (n = 1: an empty call and one column)"""
    torch, dev = _torch()
    codes, res = codec.compress(cent, cut, dim, nbits, embs)
    yield "compress", codes, res
    dx = torch.from_numpy(np.array(embs.T, dtype=np.float32, order="C")).to(dev)         # (a copy: the shared inputs are read-only)
    n, rows = dx.shape[0], dim // 8 * nbits
    split = n // 2
    dcent = torch.from_numpy(np.array(cent.T, dtype=np.float32, order="C")).to(dev)
    for name, c in (("Codec(host centroids)", cent), ("Codec(device centroids)", dcent)):
        dcodes = torch.empty(n, dtype=torch.int32, device=dev)
        dres = torch.empty((n, rows), dtype=torch.uint8, device=dev)
        cdc = codec.Codec(c, cut, dim, nbits, device=0)
        try:
            cdc.compress_device(dx[:split], dcodes[:split], dres[:split])
            cdc.compress_device(dx[split:], dcodes[split:], dres[split:])
            torch.cuda.synchronize()
        finally:
            cdc.close()
        yield name, dcodes.cpu().numpy().view(np.uint32), dres.cpu().numpy().T


def assert_packed(case, dim, nbits, what):
    cent, cut, embs, codes, R = case
    want = cm.ref_pack(cent, cut, dim, nbits, embs, codes)
    for name, got_codes, got in compress_every_way(cent, cut, dim, nbits, embs):
        assert np.array_equal(got_codes, codes), (what, name)
        bad = np.argwhere(np.asarray(got) != want)
        if bad.size:
            i, j = bad[0]
            d = (8 * i) // nbits
            raise AssertionError(f"{what} via {name}: {len(bad)} of {want.size} bytes differ; first at byte {i} of column {j}: "
                                 f"got {got[i, j]:#04x}, want {want[i, j]:#04x} (dims from {d}: residuals {R[d:d + 3, j]}, cutoffs {cut[:4]}..)")


@pytest.mark.parametrize("nbits,dim", [(b, d) for b, d, K in cm.EDGE if K == 1])
def test_bucket_edges(nbits, dim):
    for v, case in enumerate(cm.edge_case(nbits, dim)):
        assert_packed(case, dim, nbits, f"nbits={nbits} dim={dim} cutoff vector {v}")


@pytest.mark.parametrize("nbits,dim", [(b, d) for b, d, K in cm.EDGE if K == 8])
def test_bucket_edges_eight_centroids(nbits, dim):
    for case in cm.edge_case(nbits, dim, 8):
        assert_packed(case, dim, nbits, f"K=8 nbits={nbits} dim={dim}")


@pytest.mark.parametrize("nbits,dim", cm.NAN)
def test_nan_lands_in_the_last_bucket(nbits, dim):
    """One NaN component per column (K = 1): searchsortedfirst under isless (residual.jl:350) puts it after every cutoff, so the
    index at that dim is 2^nbits - 1 and every other dim is what it would be without the NaN.  `cutoffs[m - 1] < r` alone sent
    it to bucket 0."""
    case = cm.nan_case(nbits, dim)
    cent, cut, embs, codes, R = case
    idx = cm.ref_indices(cent, cut, embs, codes)
    assert np.all(idx[np.isnan(R)] == (1 << nbits) - 1)
    assert_packed(case, dim, nbits, f"NaN nbits={nbits} dim={dim}")


@pytest.mark.parametrize("dim,K,n,nbits,share", cm.STATS_CASES)
def test_statistics(dim, K, n, nbits, share):
    cent, held, codes = cm.stats_case(dim, K, n, nbits, share)
    want_cut, want_w, want_avg = cm.ref_stats(nbits, cent, held, codes)
    cut, w, avg, got_codes = codec.compute_avg_residuals(nbits, cent, held)
    print(f"codec_edges: stats {(dim, K, n, nbits, share)}: avg_residual {float(avg)!r} vs {want_avg!r}, "
          f"{len(np.unique(want_cut))} distinct cutoffs of {len(want_cut)}")
    assert np.array_equal(got_codes, codes)
    assert cm.bits_equal(cut, want_cut), (cut, want_cut)
    assert cm.bits_equal(w, want_w), (w, want_w)
    assert abs(float(avg) - want_avg) <= 1e-6 * want_avg
    # the two stages chained, as a build chains them: the device's own (degenerate) cutoffs into compress
    assert_packed((cent, cut, held, codes, cm.residuals_of(cent, held, codes)), dim, nbits, f"stats -> compress {(dim, K, n, nbits, share)}")


@pytest.mark.parametrize("n", cm.DECOMPRESS_NS + (cm.N_ENUM,))
@pytest.mark.parametrize("dim,nbits", cm.DECOMPRESS_CASES)
def test_decompress(oracle, dim, nbits, n):
    cent, codes, res = cm.decompress_case(dim, nbits)
    for variant, w in enumerate(cm.weight_variants(nbits)):
        got = codec.decompress(dim, nbits, cent, w, codes[:n], res[:, :n])
        want = cm.decompress_ref(dim, nbits, variant)[:, :n]
        assert cm.bits_equal(got, want), (variant, np.argwhere(got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))[:4])
        if n == cm.N_ENUM:
            assert cm.bits_equal(got, oracle.decompress(dim, nbits, cent, w, codes, res))
            assert variant == 1 or not got[:, 256].any()


def test_decompress_second_grid_stride_trip(oracle):
    cent, w, codes, res, want = cm.decompress_long()
    got = codec.decompress(128, 2, cent, w, codes, res)
    assert cm.bits_equal(got, want)
    assert cm.bits_equal(got, oracle.decompress(128, 2, cent, w, codes, res))


@pytest.mark.parametrize("dim,L,N,first_skipped", cm.EPI)
def test_epilogue(oracle, dim, L, N, first_skipped):
    D, ids = cm.epilogue_case(dim, L, N, first_skipped)
    want, want_lens = cm.ref_doc_epilogue(D, ids, cm.SKIPLIST)
    out, doclens = codec.doc_epilogue(D, ids, cm.SKIPLIST)
    assert np.array_equal(doclens, want_lens) and np.array_equal(doclens, cm.skip_mask(ids, cm.SKIPLIST).sum(axis=0))
    assert out.shape == want.shape and cm.bits_equal(out, want)
    oout, _ = oracle.doc_epilogue(D, ids, cm.SKIPLIST)
    assert cm.bits_equal(out, oout)
    q = codec.query_epilogue(D, ids, cm.SKIPLIST)
    assert cm.bits_equal(q, cm.ref_query_epilogue(D, ids, cm.SKIPLIST))          # -0.0 where a negative entry is masked
    assert cm.bits_equal(q, oracle.query_epilogue(D, ids, cm.SKIPLIST))
