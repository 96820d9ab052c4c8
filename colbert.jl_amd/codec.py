"""Host-side mirrors of the reference's codec / index-build functions over the C ABI.
Same names and argument meaning as src/indexing/codecs/residual.jl, src/utils.jl and
src/indexing/collection_indexer.jl; arrays keep the Julia shapes (column-major)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import check, colmajor, fptr, i64, lib


def _normalize_array(X, dims: int = 1, device: int = 0):
    """_normalize_array!(X, dims=1)  (src/utils.jl:320-325); returns the normalised copy."""
    if dims != 1:
        raise NotImplementedError("only dims=1 runs on the device")
    X = colmajor(X, np.float32).copy(order="F")
    dim = X.shape[0]
    n = X.size // max(dim, 1)
    check(lib().clb_normalize_columns(device, fptr(X), i64(dim), i64(n)))
    return X


def compress_into_codes(centroids, embs, device: int = 0, n_codes=None):
    """compress_into_codes!  (residual.jl:67-81)"""
    c = colmajor(centroids, np.float32); x = colmajor(embs, np.float32)
    n = x.shape[1]
    codes = np.zeros(n if n_codes is None else n_codes, dtype=np.uint32)
    check(lib().clb_compress_into_codes(device, fptr(codes), i64(codes.size), fptr(c), i64(c.shape[0]),
                                        i64(c.shape[1]), fptr(x), i64(n)))
    return codes


def compress(centroids, bucket_cutoffs, dim: int, nbits: int, embs, device: int = 0):
    """compress  (residual.jl:586-604) -> (codes UInt32[n], residuals UInt8 (dim/8*nbits, n))"""
    c = colmajor(centroids, np.float32); cu = np.ascontiguousarray(bucket_cutoffs, dtype=np.float32)
    x = colmajor(embs, np.float32)
    n = x.shape[1]
    codes = np.zeros(n, dtype=np.uint32)
    res = np.zeros((max(dim // 8, 0) * nbits, n), dtype=np.uint8, order="F")
    check(lib().clb_compress(device, fptr(c), i64(c.shape[1]), fptr(cu), i64(cu.size), i64(dim), C.c_int(nbits),
                             fptr(x), i64(n), fptr(codes), fptr(res)))
    return codes, res


def decompress(dim: int, nbits: int, centroids, bucket_weights, codes, residuals, device: int = 0):
    """decompress  (residual.jl:759-784) -> Float32 (dim, n)"""
    c = colmajor(centroids, np.float32); w = np.ascontiguousarray(bucket_weights, dtype=np.float32)
    co = np.ascontiguousarray(codes, dtype=np.uint32); r = colmajor(residuals, np.uint8)
    out = np.zeros((dim, co.size), dtype=np.float32, order="F")
    check(lib().clb_decompress(device, i64(dim), C.c_int(nbits), fptr(c), i64(c.shape[1]), fptr(w), i64(w.size),
                               fptr(co), i64(co.size), fptr(r), i64(r.shape[0]), i64(r.shape[1]), fptr(out)))
    return out


def maxsim(Q, D, pids, doclens, device: int = 0):
    """maxsim  (src/search/ranking.jl:69-86)"""
    q = colmajor(Q, np.float32); d = colmajor(D, np.float32)
    p = np.ascontiguousarray(pids, dtype=np.int64); dl = np.ascontiguousarray(doclens, dtype=np.int64)
    scores = np.zeros(p.size, dtype=np.float32)
    check(lib().clb_maxsim(device, fptr(q), i64(q.shape[0]), i64(q.shape[1]), fptr(d),
                           i64(d.shape[1] if d.ndim == 2 else 0), fptr(p), i64(p.size), fptr(dl), i64(dl.size),
                           fptr(scores)))
    return scores


def kmeans(data, init_centroids, max_iters: int = 10, tol: float = 1e-4, point_bsize: int = 1000,
           device: int = 0):
    """kmeans_gpu_onehot!  (src/utils.jl:253-318) with the initial centroids injected.
    Returns (centroids, assignments Int32 1-based, iterations executed)."""
    x = colmajor(data, np.float32); c = colmajor(init_centroids, np.float32).copy(order="F")
    dim, n = x.shape
    assign = np.zeros(n, dtype=np.int32)
    iters = i64(0)
    check(lib().clb_kmeans(device, fptr(x), i64(dim), i64(n), fptr(c), i64(c.shape[1]), i64(max_iters),
                           C.c_float(tol), i64(point_bsize), fptr(assign), C.byref(iters)))
    return c, assign, iters.value


def _is_tensor(a) -> bool:
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def _dev_rows(t, dtype=None):
    """A torch CUDA tensor as the device array the ABI takes: (n, dim) row-major IS the reference's (dim, n) column-major
    matrix.  Returns the (contiguous) tensor; the caller keeps it alive across the call."""
    import torch
    if not (t.is_cuda and t.is_contiguous()):
        raise ValueError("device arrays must be contiguous CUDA tensors")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"expected {dtype}, got {t.dtype}")
    return t


def _stream_of(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


F32, F16, BF16 = 0, 1, 2                                      # CLB_F32 / CLB_F16 / CLB_BF16 (include/colbert_hip.h)


def to_bfloat16_bits(x) -> np.ndarray:
    """float32 -> bfloat16 bit patterns (uint16, same shape and layout), round to nearest, ties to even; a NaN stays a quiet NaN."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    rounded = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rounded).astype(np.uint16)


def _host_16bit(a, dtype: str) -> np.ndarray:
    """`a` rounded to nearest-even into `dtype`, column-major: the 16-bit host array clb_maxsim_batch_half takes"""
    return colmajor(a, np.float16) if dtype == "float16" else np.asfortranarray(to_bfloat16_bits(colmajor(a, np.float32)))


I8 = 3                                                         # CLB_I8


def quantize_rows(X):
    """Per-embedding int8 quantisation, the host statement of dense_quantize_kernel (include/colbert_hip.h), bit for bit: X
    (dim, ...) float32 -> (X8 int8 of X's shape, scale float32 of X.shape[1:]); s = fl32(amax / 127), q = clamp(rint(fl32(x / s)),
    -127, 127) with ties to even, s == 0 -> zeros.  A non-finite value is an ArgumentError naming the embedding."""
    from ._lib import ArgumentError
    x = colmajor(X, np.float32)
    bad = ~np.isfinite(x).all(axis=0)
    if bad.any():
        raise ArgumentError(f"quantize_rows: embedding {int(np.flatnonzero(bad.ravel(order='F'))[0])} holds a non-finite value")
    s = (np.abs(x).max(axis=0, initial=np.float32(0)) / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.rint(x / s)                                      # float32 / float32: one IEEE division, as on the device
    x8 = np.where(s == 0, np.float32(0), np.clip(y, -127, 127)).astype(np.int8)
    return np.asfortranarray(x8), s


def _int8_pair(a, what):
    """(values int8 column-major, scales float32) of an operand given as floats (quantised here) or as a (values, scales) pair"""
    if isinstance(a, tuple):
        v, s = colmajor(a[0], np.int8), np.ascontiguousarray(np.asarray(a[1], dtype=np.float32).ravel(order="F"))
        if s.size != v.size // max(v.shape[0], 1):
            raise ValueError(f"{what}: one scale per embedding")
        return v, s
    if getattr(a, "dtype", None) == np.int8:
        raise ValueError(f"{what}: int8 values need their scales, as a (values, scales) pair")
    v, s = quantize_rows(a)
    return v, np.ascontiguousarray(s.ravel(order="F"))


B1 = 16                                                        # CLB_B1


def binarize_rows(X):
    """One sign bit per dimension and one scale per embedding, the statement of the 1-bit format (include/colbert_hip.h): X (dim, ...)
    float32, dim % 128 == 0 -> (values uint8 (dim / 8, ...): bit k & 7 of byte k >> 3 is x_k >= 0, so -0.0 gives 1; scale float32 of
    X.shape[1:]: the float64 mean of |x|, rounded once).  A non-finite value is an ArgumentError naming the embedding; a dim that is
    no multiple of 128 is Unsupported."""
    from ._lib import ArgumentError, Unsupported
    x = colmajor(X, np.float32)
    dim = x.shape[0]
    if dim % 128 or not 128 <= dim <= 1024:
        raise Unsupported(f"binarize_rows serves dim % 128 == 0, 128 <= dim <= 1024 (dim = {dim})")
    bad = ~np.isfinite(x).all(axis=0)
    if bad.any():
        raise ArgumentError(f"binarize_rows: embedding {int(np.flatnonzero(bad.ravel(order='F'))[0])} holds a non-finite value")
    s = np.abs(x).astype(np.float64).mean(axis=0).astype(np.float32)
    return np.asfortranarray(np.packbits(x >= 0, axis=0, bitorder="little")), s


def unbinarize_rows(values, scales):
    """The float32 embeddings a 1-bit pair stands for: s (2 bit - 1)"""
    v, s = colmajor(values, np.uint8), np.asarray(scales, dtype=np.float32)
    if v.shape[1:] != s.shape:
        raise ValueError("one scale per embedding")
    signs = np.unpackbits(v, axis=0, bitorder="little").astype(np.float32) * np.float32(2) - np.float32(1)
    return np.asfortranarray(signs * s[None])


def _b1_pair(a, what):
    """(bits uint8 column-major, scales float32) of passages given as floats (binarised here) or as a (values uint8, scales) pair"""
    if isinstance(a, tuple):
        if getattr(a[0], "dtype", None) != np.uint8:
            raise ValueError(f"{what}: a 1-bit operand is a (values uint8, scales float32) pair")
        v, s = colmajor(a[0], np.uint8), np.ascontiguousarray(np.asarray(a[1], dtype=np.float32).ravel(order="F"))
        if s.size != v.size // max(v.shape[0], 1):
            raise ValueError(f"{what}: one scale per embedding")
        return v, s
    v, s = binarize_rows(a)
    return v, np.ascontiguousarray(s.ravel(order="F"))


MXFP8, MXFP4 = 4, 5                                            # CLB_MXFP8 / CLB_MXFP4
_MX = {"mxfp8": (MXFP8, 3, -6, 7, 448.0, 8), "mxfp4": (MXFP4, 1, 0, 1, 6.0, 2)}    # code, mantissa bits, emin, bias, max, emax


def _mx(fmt):
    if fmt not in _MX:
        raise ValueError("fmt must be 'mxfp8' or 'mxfp4'")
    return _MX[fmt]


def quantize_mx(X, fmt):
    """OCP MX v1.0 quantisation, the host statement of dense_quantize_mx_kernel (include/colbert_hip.h), bit for bit: X (dim, ...)
    float32, dim % 32 == 0 -> (values uint8 (dim, ...) for "mxfp8" / (dim / 2, ...) for "mxfp4", element 2 i in the low nibble of
    byte i; scales uint8 (dim / 32, ...)).  Per block of 32: e = max(-127, ilogb(amax) - emax), scale byte e + 127 (127 for an
    all-zero block), element = x 2^-e rounded to nearest-even in E4M3 / E2M1, saturated, sign kept.  A non-finite value is an
    ArgumentError naming the embedding; a dim that is no multiple of 32 is Unsupported."""
    from ._lib import ArgumentError, Unsupported
    _, M, emin, bias, vmax, emax = _mx(fmt)
    x = colmajor(X, np.float32)
    dim = x.shape[0]
    if dim % 32 or not 32 <= dim <= 1024:
        raise Unsupported(f"quantize_mx serves dim % 32 == 0, 32 <= dim <= 1024 (dim = {dim})")
    bad = ~np.isfinite(x).all(axis=0)
    if bad.any():
        raise ArgumentError(f"quantize_mx: embedding {int(np.flatnonzero(bad.ravel(order='F'))[0])} holds a non-finite value")
    blocks = x.reshape((32, dim // 32) + x.shape[1:], order="F").astype(np.float64)       # [element, block, ...]: exact in float64
    amax = np.abs(blocks).max(axis=0)
    E = (amax.astype(np.float32).view(np.uint32) >> np.uint32(23)).astype(np.int64)        # biased fp32 exponent: ilogb + 127, 0 below 2^-126
    byte = np.where(amax == 0, 127, np.maximum(E - emax, 0))
    y = np.ldexp(blocks, (127 - byte)[None])                                            # x 2^-e
    a = np.minimum(np.abs(y), vmax)
    eq = np.maximum(np.frexp(a)[1] - 1, emin) - M                                          # the grid's step at a is 2^eq (a == 0: any step, rint(0) = 0)
    r = np.ldexp(np.rint(np.ldexp(a, -eq)), eq)                                            # nearest-even, one rounding
    er = np.where(r == 0, emin - 1, np.frexp(r)[1] - 1)
    mant = np.where(er < emin, np.ldexp(r, M - emin), ((er + bias) << M) + (np.ldexp(r, M - er) - (1 << M))).astype(np.int64)
    code = (mant | (np.signbit(y).astype(np.int64) << (7 if M == 3 else 3))).astype(np.uint8).reshape(x.shape, order="F")
    if M == 1:
        code = code[0::2] | (code[1::2] << np.uint8(4))
    return np.asfortranarray(code), np.asfortranarray(byte.astype(np.uint8))


def dequantize_mx(values, scales, fmt):
    """The float32 embeddings an MX pair stands for: element code times 2^(scale byte - 127) per block of 32 (exact); NaN where
    a code (E4M3 0x7F / 0xFF) or a scale byte (0xFF) is one."""
    _, M, emin, bias, _, _ = _mx(fmt)
    v, s = colmajor(values, np.uint8), colmajor(scales, np.uint8)
    if M == 1:
        both = np.empty((2 * v.shape[0],) + v.shape[1:], np.uint8, order="F")
        both[0::2], both[1::2] = v & np.uint8(15), v >> np.uint8(4)
        v = both
    if v.shape[0] != 32 * s.shape[0] or v.shape[1:] != s.shape[1:]:
        raise ValueError("one scale byte per block of 32 elements")
    c = v.astype(np.int64)
    field, mant, neg = (c >> M) & (15 if M == 3 else 3), c & ((1 << M) - 1), c >> (7 if M == 3 else 3) & 1
    mag = np.where(field == 0, np.ldexp(mant.astype(np.float64), emin - M), np.ldexp(((1 << M) + mant).astype(np.float64), field - bias - M))
    if M == 3:
        mag = np.where((c & 0x7F) == 0x7F, np.nan, mag)
    x = np.where(neg == 1, -mag, mag) * np.repeat(np.where(s == 255, np.nan, np.ldexp(1.0, s.astype(np.int64) - 127)), 32, axis=0)
    return np.asfortranarray(x.astype(np.float32))


def _mx_pair(a, what, fmt):
    """(values, scale bytes) of an operand given as floats (quantised here) or as a (values uint8, scales uint8) pair"""
    if isinstance(a, tuple):
        v, s = colmajor(a[0], np.uint8), colmajor(a[1], np.uint8)
        if getattr(a[0], "dtype", None) != np.uint8 or getattr(a[1], "dtype", None) != np.uint8:
            raise ValueError(f"{what}: an MX operand is a (values uint8, scales uint8) pair")
        return v, s
    if getattr(a, "dtype", None) not in (np.float32, np.float64, np.float16):
        raise ValueError(f"{what}: float values (quantised here) or a (values uint8, scales uint8) pair")
    return quantize_mx(a, fmt)


def quantize_mx_device(d_X, fmt, out=None, stream=None):
    """`quantize_mx` on the device (clb_quantize_mx_device): d_X float32 (..., dim), contiguous, dim % 32 == 0 -> (values uint8
    (..., dim) or (..., dim / 2), scales uint8 (..., dim / 32)).  `out`: that pair, preallocated.  Stream-ordered, not waited for; it
    cannot report a non-finite value (defined, meaningless numbers)."""
    import torch
    code = _mx(fmt)[0]
    x = _dev_rows(d_X, torch.float32)
    if x.dim() < 2:
        raise ValueError("d_X must be (..., dim)")
    dim, lead = int(x.shape[-1]), tuple(x.shape[:-1])
    vb = dim // 2 if code == MXFP4 else dim
    v, s = out if out is not None else (torch.empty(lead + (vb,), dtype=torch.uint8, device=x.device),
                                        torch.empty(lead + (dim // 32,), dtype=torch.uint8, device=x.device))
    _dev_rows(v, torch.uint8); _dev_rows(s, torch.uint8)
    n = x.numel() // max(dim, 1)
    if v.numel() != n * vb or s.numel() != n * (dim // 32):
        raise ValueError("out: the values' bytes and one scale byte per block of 32")
    st = torch.cuda.current_stream(x.device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    check(lib().clb_quantize_mx_device(x.device.index, C.c_void_p(x.data_ptr()), i64(dim), i64(n), code, C.c_void_p(v.data_ptr()),
                                       C.c_void_p(s.data_ptr()), C.c_void_p(st)))
    return v, s


def quantize_rows_device(d_X, out=None, stream=None):
    """`quantize_rows` on the device (clb_quantize_rows_device): d_X float32 (..., dim), contiguous, dim % 16 == 0 -> (int8 of d_X's
    shape, float32 scales of its leading shape).  `out`: that pair, preallocated.  Stream-ordered, not waited for; it cannot
    report a non-finite value (defined, meaningless numbers)."""
    import torch
    x = _dev_rows(d_X, torch.float32)
    if x.dim() < 2:
        raise ValueError("d_X must be (..., dim)")
    x8, s = out if out is not None else (torch.empty(x.shape, dtype=torch.int8, device=x.device),
                                         torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device))
    _dev_rows(x8, torch.int8); _dev_rows(s, torch.float32)
    if x8.numel() != x.numel() or s.numel() * x.shape[-1] != x.numel():
        raise ValueError("out: int8 of d_X's shape and one float32 scale per embedding")
    st = torch.cuda.current_stream(x.device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    check(lib().clb_quantize_rows_device(x.device.index, C.c_void_p(x.data_ptr()), i64(x.shape[-1]), i64(s.numel()),
                                         C.c_void_p(x8.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(st)))
    return x8, s


def binarize_rows_device(d_X, out=None, stream=None):
    """`binarize_rows` on the device (clb_binarize_rows_device): d_X float32 (..., dim), contiguous, dim % 128 == 0 -> (uint8 bits
    (..., dim / 8), float32 scales of its leading shape; the scale is summed in fp32, so it lies within (dim + 1) 2^-24 of the host's).
    `out`: that pair, preallocated.  Stream-ordered, not waited for; it cannot report a non-finite value (defined, meaningless numbers)."""
    import torch
    x = _dev_rows(d_X, torch.float32)
    if x.dim() < 2:
        raise ValueError("d_X must be (..., dim)")
    dim, lead = int(x.shape[-1]), tuple(x.shape[:-1])
    v, s = out if out is not None else (torch.empty(lead + (dim // 8,), dtype=torch.uint8, device=x.device),
                                        torch.empty(lead, dtype=torch.float32, device=x.device))
    _dev_rows(v, torch.uint8); _dev_rows(s, torch.float32)
    if v.numel() * 8 != x.numel() or s.numel() * dim != x.numel():
        raise ValueError("out: one bit per element and one float32 scale per embedding")
    st = torch.cuda.current_stream(x.device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    check(lib().clb_binarize_rows_device(x.device.index, C.c_void_p(x.data_ptr()), i64(dim), i64(s.numel()),
                                         C.c_void_p(v.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(st)))
    return v, s


def maxsim_batch(Q, D, doclens, owner=None, device: int = 0, dtype=None):
    """maxsim (ranking.jl:69-86) of N un-indexed passages for a batch of queries in one call (clb_maxsim_batch): Q (dim, T, B),
    D (dim, n) -- the passages' embeddings back to back --, doclens [N].  `owner` [N], 0-based: passage j is scored against
    query owner[j] only -> (N,) float32; without it every query scores every passage -> (N, B).  Each score has the bits of
    `maxsim(Q[:, :, q], D_j)`.
    dtype="float16" / "bfloat16" (implied by an np.float16 D): Q and D are rounded to nearest-even into that type, uploaded in 16
    bits and multiplied by the 16-bit MFMA kernel (clb_maxsim_batch_half): exact products summed in fp32, within the bound of
    DESIGN 4.2a of the float64 value on the rounded operands -- not the oracle's bits.
    dtype="int8" (implied by a Q or D given as a `(values int8, scales)` pair, which is used as it is): float operands are
    quantised per embedding by `quantize_rows` and scored by the integer-MFMA kernel (clb_maxsim_batch_i8): exact integer dots,
    each score bit-identical to the restatement in include/colbert_hip.h; its distance from the fp32 score is the format's.
    dtype="mxfp8" / "mxfp4": MX block-scaled embeddings scored by the scaled-MFMA kernel (clb_maxsim_batch_mx).  Float operands
    are quantised by `quantize_mx` (Q always as "mxfp8", D as `dtype`); a `(values uint8, scales uint8)` pair is used as it is.
    dtype="binary": passages as one sign bit per dimension with one scale each, queries in int8 (clb_maxsim_batch_b1): a float Q is
    quantised by `quantize_rows`, a float D by `binarize_rows`; a `(values uint8, scales float32)` pair for D and an int8 pair for Q
    are used as they are.  Exact integer dots: each score bit-identical to the restatement in include/colbert_hip.h."""
    if dtype in _MX:
        (q, qs), (d, ds) = _mx_pair(Q, "Q", "mxfp8"), _mx_pair(D, "D", dtype)
        if q.ndim != 3 or qs.shape != (q.shape[0] // 32,) + q.shape[1:]:
            raise ValueError("Q must be (dim, T, B) with scales (dim / 32, T, B)")
        dim, T, B = q.shape
        n = d.shape[1] if d.ndim == 2 else 0
        if d.ndim != 2 or d.shape[0] * (2 if dtype == "mxfp4" else 1) != dim or ds.shape != (dim // 32, n):
            raise ValueError("D must hold (dim, n) elements with scales (dim / 32, n)")
        dl = np.ascontiguousarray(doclens, dtype=np.int64)
        ow = None if owner is None else np.ascontiguousarray(owner, dtype=np.int32)
        if ow is not None and ow.size != dl.size:
            raise ValueError("owner must hold one query number per passage")
        scores = np.zeros(dl.size if ow is not None else (dl.size, B), dtype=np.float32, order="F")
        check(lib().clb_maxsim_batch_mx(device, fptr(q), MXFP8, fptr(qs), i64(dim), i64(T), i64(B), fptr(d), fptr(ds), _MX[dtype][0], i64(n),
                                        fptr(dl), i64(dl.size), fptr(ow) if ow is not None else None, fptr(scores)))
        return scores
    binary = dtype == "binary"
    int8 = binary or dtype == "int8" or isinstance(Q, tuple) or isinstance(D, tuple) or (dtype is None and getattr(D, "dtype", None) == np.int8)
    if int8:
        if dtype not in (None, "int8", "binary"):
            raise ValueError("int8 operands take dtype None or 'int8'")
        (q, qs), (d, ds) = _int8_pair(Q, "Q"), (_b1_pair if binary else _int8_pair)(D, "D")
    else:
        if dtype is None and getattr(D, "dtype", None) == np.float16:
            dtype = "float16"
        if dtype not in (None, "float16", "bfloat16"):
            raise ValueError("dtype must be None, 'float16', 'bfloat16', 'int8', 'binary', 'mxfp8' or 'mxfp4'")
        q, d = (colmajor(Q, np.float32), colmajor(D, np.float32)) if dtype is None else (_host_16bit(Q, dtype), _host_16bit(D, dtype))
    if q.ndim != 3:
        raise ValueError("Q must be (dim, T, B)")
    dl = np.ascontiguousarray(doclens, dtype=np.int64)
    ow = None if owner is None else np.ascontiguousarray(owner, dtype=np.int32)
    if ow is not None and ow.size != dl.size:
        raise ValueError("owner must hold one query number per passage")
    dim, T, B = q.shape
    scores = np.zeros(dl.size if ow is not None else (dl.size, B), dtype=np.float32, order="F")
    shape = (i64(dim), i64(T), i64(B))
    tail = (i64(d.shape[1] if d.ndim == 2 else 0), fptr(dl), i64(dl.size), fptr(ow) if ow is not None else None, fptr(scores))
    if int8:
        check((lib().clb_maxsim_batch_b1 if binary else lib().clb_maxsim_batch_i8)(device, fptr(q), I8, fptr(qs), *shape, fptr(d), fptr(ds), *tail))
    elif dtype is None:
        check(lib().clb_maxsim_batch(device, fptr(q), *shape, fptr(d), *tail))
    else:
        ty = F16 if dtype == "float16" else BF16
        check(lib().clb_maxsim_batch_half(device, fptr(q), ty, *shape, fptr(d), ty, *tail))
    return scores


def maxsim_batch_device(d_Q, d_D, d_doclens, owner=None, out=None, work=None, stream=None, *, d_scale=None, q_scale=None, pids=None,
                        store_offsets=None):
    """`maxsim_batch` between the encoder's device outputs (clb_maxsim_batch_device): d_Q float32 (B, T, dim) -- what
    query_embeddings_device writes --, d_D float32 (n, dim) and d_doclens int64 (N,) -- what doc_embeddings_device /
    doc_embeddings_packed_device return --, owner int32 (N,) or None; all contiguous CUDA tensors.  Returns `out`: float32 (N,)
    with owners, else (B, N) (row q = query q's scores).  Enqueued on `stream` (default: torch's current stream) and not
    waited for; with `out` and `work` (uint8, clb_maxsim_batch_work_bytes long) given it allocates nothing, so it can be
    captured in a graph.  Device doclens are not validated: see include/colbert_hip.h for what bad ones score.
    A float16 / bfloat16 d_D takes the 16-bit kernel (clb_maxsim_batch_half_device): d_Q float32 (rounded on the device) or
    d_D's dtype, `work` clb_maxsim_batch_half_work_bytes long.
    An int8 d_D with `d_scale` (float32, one per embedding: what `quantize_rows_device` returns) takes the integer kernel
    (clb_maxsim_batch_i8_device): d_Q float32 (quantised on the device) or int8 with `q_scale` (B, T); `work`
    clb_maxsim_batch_i8_work_bytes long.  Any other mix of int8 operands and scales is a ValueError.
    A uint8 d_D (n, dim / 8) with a float32 `d_scale` is a 1-bit pair (what `binarize_rows_device` returns) and takes the same integer
    MFMA on bits widened in registers (clb_maxsim_batch_b1_device): d_Q float32 or int8 with `q_scale`, as for int8; `work`
    clb_maxsim_batch_b1_work_bytes long.  The dtype of `d_scale` chooses between 1-bit and MX.
    A uint8 d_D with a uint8 `d_scale` (n, dim / 32) is an MX pair (what `quantize_mx_device` returns) and takes the scaled-MFMA
    kernel (clb_maxsim_batch_mx_device): d_D (n, dim) is MXFP8, (n, dim / 2) MXFP4; d_Q float32 (quantised to MXFP8 on the device) or
    uint8 with a uint8 `q_scale` (B, T, dim / 32); `work` clb_maxsim_batch_mx_work_bytes long.  Any other mix is a ValueError.
    By passage id (clb_maxsim_store_device): with `pids` int64 (N,) and `store_offsets` int64 (P + 1,), d_D and d_scale are a
    resident store -- stored passage p is the rows store_offsets[p] .. store_offsets[p + 1] - 1 -- and d_doclens must be None:
    entry j scores stored passage pids[j], read where it lies, with the bits the contiguous call gives for the same rows; a pid
    outside 0..P-1 (pad with -1) or an empty range scores -inf.  The format is chosen by dtype and scales as above; `work` is
    clb_maxsim_store_work_bytes long."""
    import torch
    if pids is not None or store_offsets is not None:
        if pids is None or store_offsets is None or d_doclens is not None:
            raise ValueError("pids and store_offsets go together, and d_doclens must be None with them")
        return _maxsim_store_device(d_Q, d_D, pids, store_offsets, owner, out, work, stream, d_scale, q_scale)
    b1 = d_D.dtype == torch.uint8 and getattr(d_scale, "dtype", None) == torch.float32
    if not b1 and (torch.uint8 in (d_D.dtype, d_Q.dtype) or torch.uint8 in (getattr(d_scale, "dtype", None), getattr(q_scale, "dtype", None))):
        return _maxsim_batch_mx_device(d_Q, d_D, d_doclens, owner, out, work, stream, d_scale, q_scale)
    int8 = b1 or torch.int8 in (d_D.dtype, d_Q.dtype) or d_scale is not None or q_scale is not None
    half = None if int8 else {torch.float16: F16, torch.bfloat16: BF16}.get(d_D.dtype)
    if int8:
        if (d_D.dtype != torch.int8 and not b1) or d_scale is None:
            raise ValueError("int8 scoring takes an int8 d_D with d_scale, one float32 scale per embedding")
        if (d_Q.dtype == torch.int8) != (q_scale is not None) or d_Q.dtype not in (torch.int8, torch.float32):
            raise ValueError("d_Q must be float32 (quantised on the device) or int8 with q_scale")
    elif half is not None and d_Q.dtype not in (torch.float32, d_D.dtype):
        raise ValueError(f"d_Q must be float32 or {d_D.dtype}, got {d_Q.dtype}")
    plain = None if int8 or half is not None else torch.float32
    q, d, dl = _dev_rows(d_Q, plain), _dev_rows(d_D, plain), _dev_rows(d_doclens, torch.int64)
    ds = _dev_rows(d_scale, torch.float32) if int8 else None
    qs = None if q_scale is None else _dev_rows(q_scale, torch.float32)
    if q.dim() != 3 or d.dim() != 2 or d.shape[1] * (8 if b1 else 1) != q.shape[2]:
        raise ValueError("d_Q must be (B, T, dim) and d_D (n, dim), 1-bit rows (n, dim / 8)")
    B, T, dim = (int(x) for x in q.shape)
    N = int(dl.numel())
    if int8 and (ds.numel() != d.shape[0] or (qs is not None and qs.numel() != B * T)):
        raise ValueError("d_scale / q_scale: one scale per embedding")
    ow = None if owner is None else _dev_rows(owner, torch.int32)
    if ow is not None and ow.numel() != N:
        raise ValueError("owner must hold one query number per passage")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    shape, sizes = (i64(dim), i64(T), i64(B)), (i64(N), i64(B), i64(T))
    q_type = F32 if q.dtype == torch.float32 else (I8 if int8 else half)
    if b1:
        entry, work_bytes = lib().clb_maxsim_batch_b1_device, lambda: lib().clb_maxsim_batch_b1_work_bytes(*sizes, i64(dim))
        operands = (ptr(q), q_type, ptr(qs), *shape, ptr(d), ptr(ds))
    elif int8:
        entry, work_bytes = lib().clb_maxsim_batch_i8_device, lambda: lib().clb_maxsim_batch_i8_work_bytes(*sizes, i64(dim))
        operands = (ptr(q), q_type, ptr(qs), *shape, ptr(d), ptr(ds))
    elif half is not None:
        entry, work_bytes = lib().clb_maxsim_batch_half_device, lambda: lib().clb_maxsim_batch_half_work_bytes(*sizes, i64(dim))
        operands = (ptr(q), q_type, *shape, ptr(d), half)
    else:
        entry, work_bytes = lib().clb_maxsim_batch_device, lambda: lib().clb_maxsim_batch_work_bytes(*sizes)
        operands = (ptr(q), *shape, ptr(d))
    if out is None:
        out = torch.empty(N if ow is not None else (B, N), dtype=torch.float32, device=q.device)
    if work is None:
        work = torch.empty(int(work_bytes()), dtype=torch.uint8, device=q.device)
    o = _dev_rows(out, torch.float32); wk = _dev_rows(work)
    if o.numel() != (N if ow is not None else N * B):
        raise ValueError("out: one score per passage (owned) or per (query, passage)")
    st = torch.cuda.current_stream(q.device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    check(entry(q.device.index, *operands, i64(d.shape[0]), ptr(dl), i64(N), ptr(ow), ptr(o), ptr(wk), i64(wk.numel() * wk.element_size()),
                C.c_void_p(st)))
    return out


def _maxsim_batch_mx_device(d_Q, d_D, d_doclens, owner, out, work, stream, d_scale, q_scale):
    """maxsim_batch_device on an MX pair"""
    import torch
    if d_D.dtype != torch.uint8 or getattr(d_scale, "dtype", None) != torch.uint8:
        raise ValueError("MX scoring takes a uint8 d_D with a uint8 d_scale, one byte per block of 32")
    if d_Q.dtype not in (torch.uint8, torch.float32) or (d_Q.dtype == torch.uint8) != (q_scale is not None) or \
            (q_scale is not None and q_scale.dtype != torch.uint8):
        raise ValueError("d_Q must be float32 (quantised on the device) or uint8 with a uint8 q_scale")
    q, d, ds, dl = _dev_rows(d_Q), _dev_rows(d_D), _dev_rows(d_scale), _dev_rows(d_doclens, torch.int64)
    qs = None if q_scale is None else _dev_rows(q_scale)
    if q.dim() != 3 or d.dim() != 2 or d.shape[1] not in (q.shape[2], q.shape[2] // 2):
        raise ValueError("d_Q must be (B, T, dim) and d_D (n, dim) for MXFP8 or (n, dim / 2) for MXFP4")
    B, T, dim = (int(x) for x in q.shape)
    N, n = int(dl.numel()), int(d.shape[0])
    if ds.numel() != n * (dim // 32) or (qs is not None and qs.numel() != B * T * (dim // 32)):
        raise ValueError("d_scale / q_scale: one byte per block of 32 elements")
    ow = None if owner is None else _dev_rows(owner, torch.int32)
    if ow is not None and ow.numel() != N:
        raise ValueError("owner must hold one query number per passage")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    if out is None:
        out = torch.empty(N if ow is not None else (B, N), dtype=torch.float32, device=q.device)
    if work is None:
        work = torch.empty(int(lib().clb_maxsim_batch_mx_work_bytes(i64(N), i64(B), i64(T), i64(dim))), dtype=torch.uint8, device=q.device)
    o = _dev_rows(out, torch.float32); wk = _dev_rows(work)
    if o.numel() != (N if ow is not None else N * B):
        raise ValueError("out: one score per passage (owned) or per (query, passage)")
    st = torch.cuda.current_stream(q.device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    check(lib().clb_maxsim_batch_mx_device(q.device.index, ptr(q), F32 if q.dtype == torch.float32 else MXFP8, ptr(qs), i64(dim), i64(T), i64(B),
                                           ptr(d), ptr(ds), MXFP8 if d.shape[1] == dim else MXFP4, i64(n), ptr(dl), i64(N), ptr(ow), ptr(o),
                                           ptr(wk), i64(wk.numel() * wk.element_size()), C.c_void_p(st)))
    return out


def _maxsim_store_device(d_Q, d_D, pids, store_offsets, owner, out, work, stream, d_scale, q_scale):
    """maxsim_batch_device by passage id: the store's format from d_D's dtype and the scales' (one entry point for all seven)"""
    import torch
    q, d = _dev_rows(d_Q), _dev_rows(d_D)
    pid, off = _dev_rows(pids, torch.int64), _dev_rows(store_offsets, torch.int64)
    if q.dim() != 3 or d.dim() != 2 or off.numel() < 1:
        raise ValueError("d_Q must be (B, T, dim), d_D (n, dim) and store_offsets (P + 1,)")
    B, T, dim = (int(x) for x in q.shape)
    b1 = d.dtype == torch.uint8 and getattr(d_scale, "dtype", None) == torch.float32      # the scales' dtype tells 1-bit rows from MX
    mx = d.dtype == torch.uint8 and not b1
    if d.shape[1] not in ((dim // 8,) if b1 else (dim, dim // 2) if mx else (dim,)):
        raise ValueError("d_D must be (n, dim); an MXFP4 store (n, dim / 2), a 1-bit store (n, dim / 8)")
    types = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16, torch.int8: I8, torch.uint8: MXFP8}
    if d.dtype not in types or q.dtype not in types:
        raise ValueError(f"no dense format for d_D {d.dtype} and d_Q {q.dtype}")
    d_type = B1 if b1 else MXFP4 if mx and d.shape[1] != dim else types[d.dtype]
    # the scales each operand's dtype asks for: one float32 per embedding (int8, 1-bit), one uint8 per block of 32 (MX), else none
    want = {torch.int8: (torch.float32, 1), torch.uint8: (torch.float32, 1) if b1 else (torch.uint8, dim // 32)}
    scales = []
    for name, t, s, rows in (("d_scale", d, d_scale, int(d.shape[0])), ("q_scale", q, q_scale, B * T)):
        dt, per = want.get(t.dtype, (None, 0))
        if (s is None) != (dt is None) or (s is not None and (_dev_rows(s).dtype != dt or s.numel() != rows * per)):
            raise ValueError(f"{name}: {'none' if dt is None else f'{per} {dt} per embedding'} for a {t.dtype} operand")
        scales.append(s)
    ds, qs = scales
    N = int(pid.numel())
    ow = None if owner is None else _dev_rows(owner, torch.int32)
    if ow is not None and ow.numel() != N:
        raise ValueError("owner must hold one query number per entry of pids")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    if out is None:
        out = torch.empty(N if ow is not None else (B, N), dtype=torch.float32, device=q.device)
    if work is None:
        work = torch.empty(int(lib().clb_maxsim_store_work_bytes(i64(N), i64(B), i64(T), i64(dim), d_type)), dtype=torch.uint8, device=q.device)
    o = _dev_rows(out, torch.float32); wk = _dev_rows(work)
    if o.numel() != (N if ow is not None else N * B):
        raise ValueError("out: one score per entry (owned) or per (query, entry)")
    st = torch.cuda.current_stream(q.device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    check(lib().clb_maxsim_store_device(q.device.index, ptr(q), types[q.dtype], ptr(qs), i64(dim), i64(T), i64(B), ptr(d), ptr(ds), d_type,
                                        i64(d.shape[0]), ptr(off), i64(off.numel() - 1), ptr(pid), i64(N), ptr(ow), ptr(o), ptr(wk),
                                        i64(wk.numel() * wk.element_size()), C.c_void_p(st)))
    return out


class KMeansShard:
    """One rank's points of a sharded k-means (clb_kmeans_shard_*): uploaded once, one `pass_` per iteration.
    `data`: a (dim, n) numpy array (uploaded) or an (n, dim) float32 CUDA tensor (borrowed in place:
    clb_kmeans_shard_create_device -- the tensor is kept alive by this object)."""

    def __init__(self, data, K: int, point_bsize: int = 1000, device: int = 0):
        self._h = C.c_void_p()
        if _is_tensor(data):
            import torch
            x = _dev_rows(data, torch.float32)
            self._points = x                                    # borrowed by the handle
            self.n, self.dim = x.shape
            self.K, self.device = int(K), x.device.index
            check(lib().clb_kmeans_shard_create_device(self.device, C.c_void_p(x.data_ptr()), i64(self.dim), i64(self.n),
                                                       i64(K), i64(point_bsize), C.byref(self._h)))
            return
        x = colmajor(data, np.float32)
        self.dim, self.n = x.shape
        self.K, self.device = int(K), device
        check(lib().clb_kmeans_shard_create(device, fptr(x), i64(self.dim), i64(self.n), i64(K), i64(point_bsize),
                                            C.byref(self._h)))

    def pass_(self, centroids, want_assignments: bool = False):
        """-> (sums (dim,K) fp32, counts int64[K][, assignments int32 1-based])"""
        c = colmajor(centroids, np.float32)
        sums = np.zeros((self.dim, self.K), dtype=np.float32, order="F"); counts = np.zeros(self.K, dtype=np.int64)
        assign = np.zeros(self.n, dtype=np.int32) if want_assignments else None
        check(lib().clb_kmeans_shard_pass(self._h, fptr(c), fptr(sums), fptr(counts),
                                          fptr(assign) if want_assignments else None))
        return (sums, counts, assign) if want_assignments else (sums, counts)

    # -- the exchange on the device (torch CUDA tensors; enqueued on torch's current stream) ---------------------------
    @property
    def block_bytes(self) -> int:
        return int(lib().clb_kmeans_shard_block_bytes(self._h))

    def set_centroids(self, centroids):
        """(dim, K) numpy array or (K, dim) float32 CUDA tensor"""
        if _is_tensor(centroids):
            import torch
            c = _dev_rows(centroids, torch.float32)
            assert tuple(c.shape) == (self.K, self.dim)
            torch.cuda.current_stream(c.device).synchronize()
            check(lib().clb_kmeans_shard_set_centroids(self._h, C.c_void_p(c.data_ptr())))
            return
        c = colmajor(centroids, np.float32)
        assert c.shape == (self.dim, self.K)
        check(lib().clb_kmeans_shard_set_centroids(self._h, fptr(c)))

    def get_centroids(self, out=None):
        """-> (dim, K) numpy array, or into `out`, a (K, dim) float32 CUDA tensor"""
        if out is not None:
            import torch
            c = _dev_rows(out, torch.float32)
            assert tuple(c.shape) == (self.K, self.dim)
            torch.cuda.current_stream(c.device).synchronize()
            check(lib().clb_kmeans_shard_get_centroids(self._h, C.c_void_p(c.data_ptr())))
            return out
        c = np.zeros((self.dim, self.K), dtype=np.float32, order="F")
        check(lib().clb_kmeans_shard_get_centroids(self._h, fptr(c)))
        return c

    def get_assignments(self):
        """Int32[n], 1-based: the assignments of the last pass"""
        a = np.zeros(self.n, dtype=np.int32)
        check(lib().clb_kmeans_shard_get_assignments(self._h, fptr(a)))
        return a

    def pass_device(self, d_block):
        """this rank's [sums | counts] block into the uint8 CUDA tensor `d_block` (block_bytes long)"""
        import torch
        assert d_block.is_cuda and d_block.is_contiguous() and d_block.numel() * d_block.element_size() >= self.block_bytes
        st = torch.cuda.current_stream(d_block.device).cuda_stream
        check(lib().clb_kmeans_shard_pass_device(self._h, C.c_void_p(d_block.data_ptr()), C.c_void_p(st)))

    def update_device(self, d_gathered, world: int, tol: float = 1e-4):
        """rank-ordered reduction of the `world` gathered blocks + centroid update -> (delta, converged)"""
        import torch
        assert d_gathered.is_cuda and d_gathered.is_contiguous()
        assert d_gathered.numel() * d_gathered.element_size() >= world * self.block_bytes
        st = torch.cuda.current_stream(d_gathered.device).cuda_stream
        delta = C.c_float(0); conv = C.c_int(0)
        check(lib().clb_kmeans_shard_update_device(self._h, C.c_void_p(d_gathered.data_ptr()), i64(world), C.c_float(tol),
                                                   C.byref(delta), C.byref(conv), C.c_void_p(st)))
        return delta.value, bool(conv.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().clb_kmeans_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmeans_device(points, init_centroids, max_iters: int = 10, tol: float = 1e-4, point_bsize: int = 1000):
    """kmeans_gpu_onehot!  (src/utils.jl:253-318) on points that are already in HBM: `points` (n, dim) and
    `init_centroids` (K, dim) float32 CUDA tensors.  One shard, no exchange -- bit-identical to `kmeans` (the shard
    handle documents that).  Returns (centroids (K, dim) CUDA tensor, iterations executed, shard handle -- open, for
    `get_assignments`; close it)."""
    import torch
    sh = KMeansShard(points, init_centroids.shape[0], point_bsize)
    sh.set_centroids(init_centroids)
    blk = torch.empty(sh.block_bytes, dtype=torch.uint8, device=points.device)
    it = 0
    with torch.cuda.device(points.device):
        for it in range(1, max_iters + 1):
            sh.pass_device(blk)
            _delta, conv = sh.update_device(blk, 1, tol)
            if conv:
                break
    out = torch.empty_like(init_centroids)
    sh.get_centroids(out)
    return out, (it if max_iters > 0 else 0), sh


class Codec:
    """The chunk loop's resident codec (clb_codec_*): centroids and cutoffs uploaded once, `compress_device` per chunk
    of device-resident embeddings (compress, residual.jl:586-604)."""

    def __init__(self, centroids, bucket_cutoffs, dim: int, nbits: int, device: int = 0):
        self._h = C.c_void_p()
        self.dim, self.nbits = int(dim), int(nbits)
        cu = np.ascontiguousarray(bucket_cutoffs, dtype=np.float32)
        if _is_tensor(centroids):
            import torch
            c = _dev_rows(centroids, torch.float32)
            self.K, self.device = int(c.shape[0]), c.device.index
            torch.cuda.current_stream(c.device).synchronize()
            cptr = C.c_void_p(c.data_ptr())
        else:
            c = colmajor(centroids, np.float32)
            self.K, self.device = int(c.shape[1]), device
            cptr = fptr(c)
        check(lib().clb_codec_create(self.device, i64(dim), C.c_int(nbits), i64(self.K), cptr, fptr(cu), i64(cu.size),
                                     C.byref(self._h)))

    def compress_device(self, embs, out_codes=None, out_residuals=None):
        """embs (n, dim) float32 CUDA tensor -> (codes uint32-as-int32 [n] 1-based, residuals uint8 (n, dim/8*nbits)),
        enqueued on torch's current stream."""
        import torch
        x = _dev_rows(embs, torch.float32)
        n = x.shape[0]
        rows = self.dim // 8 * self.nbits
        codes = out_codes if out_codes is not None else torch.empty(n, dtype=torch.int32, device=x.device)
        res = out_residuals if out_residuals is not None else torch.empty((n, rows), dtype=torch.uint8, device=x.device)
        assert codes.is_contiguous() and res.is_contiguous() and codes.numel() == n and res.numel() == n * rows
        check(lib().clb_codec_compress_device(self._h, C.c_void_p(x.data_ptr()), i64(n), C.c_void_p(codes.data_ptr()),
                                              C.c_void_p(res.data_ptr()), _stream_of(x)))
        return codes, res

    def close(self):
        if getattr(self, "_h", None):
            lib().clb_codec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gather_rows_device(src, rows, out=None):
    """out[i, :] = src[rows[i], :] on the device (clb_gather_rows_device): the sampled / shuffled columns of the reference's
    (dim, n) matrices (`sample[:, randperm(...)]`, the sampled passages' embeddings -- collection_indexer.jl:56-91) cut out
    without torch indexing.  src: contiguous CUDA tensor (n_src, ...); rows: int64 CUDA tensor or numpy array, 0-based;
    out: optional contiguous destination (a slice of a larger buffer will do).  BoundsError for an index outside src."""
    import torch
    s_ = _dev_rows(src)
    if not _is_tensor(rows):
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(s_.device)
    r_ = _dev_rows(rows, torch.int64)
    n = int(r_.numel())
    row_bytes = int(s_[0].numel() * s_.element_size()) if s_.shape[0] else int(np.prod(s_.shape[1:]) * s_.element_size())
    if out is None:
        out = torch.empty((n,) + tuple(s_.shape[1:]), dtype=s_.dtype, device=s_.device)
    o_ = _dev_rows(out, s_.dtype)
    assert o_.numel() * o_.element_size() == n * row_bytes, "gather_rows_device: destination size"
    check(lib().clb_gather_rows_device(s_.device.index, C.c_void_p(s_.data_ptr()), i64(s_.shape[0]), i64(row_bytes),
                                       C.c_void_p(r_.data_ptr()), i64(n), C.c_void_p(o_.data_ptr()), _stream_of(s_)))
    return out


def device_memory(device: int = 0):
    """(free, total) bytes of HBM on `device` (clb_device_memory)."""
    f, t = i64(0), i64(0)
    check(lib().clb_device_memory(device, C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def build_ivf_device(codes, num_partitions: int):
    """_build_ivf  (collection_indexer.jl:349-353) over a device array: codes int32/uint32 CUDA tensor [n] (1-based) ->
    (ivf int64 CUDA tensor [n] 1-based, ivf_lengths int64 CUDA tensor [K])."""
    import torch
    co = _dev_rows(codes)
    assert co.element_size() == 4
    n = co.numel()
    ivf = torch.empty(n, dtype=torch.int64, device=co.device)
    lens = torch.empty(num_partitions, dtype=torch.int64, device=co.device)
    check(lib().clb_build_ivf_device(co.device.index, C.c_void_p(co.data_ptr()), i64(n), i64(num_partitions),
                                     C.c_void_p(ivf.data_ptr()), C.c_void_p(lens.data_ptr()), _stream_of(co)))
    return ivf, lens


def kmeans_reduce_update(centroids, gathered_sums, gathered_counts, tol: float = 1e-4, device: int = 0):
    """Rank-ordered reduction of the shards' partial sums + centroid update (clb_kmeans_reduce_update).
    gathered_sums: (world, dim*K) (each block a (dim,K) column-major matrix), gathered_counts: (world, K).
    Returns (centroids, delta, converged)."""
    c = colmajor(centroids, np.float32).copy(order="F")
    dim, K = c.shape
    gs = np.ascontiguousarray(np.asarray(gathered_sums, dtype=np.float32).reshape(-1, dim * K))
    gc = np.ascontiguousarray(np.asarray(gathered_counts, dtype=np.int64).reshape(gs.shape[0], K))
    delta = C.c_float(0); conv = C.c_int(0)
    check(lib().clb_kmeans_reduce_update(device, fptr(c), fptr(gs), fptr(gc), i64(gs.shape[0]), i64(dim), i64(K),
                                         C.c_float(tol), C.byref(delta), C.byref(conv)))
    return c, delta.value, bool(conv.value)


def compute_avg_residuals(nbits: int, centroids, heldout, device: int = 0, n_codes=None):
    """_compute_avg_residuals!  (collection_indexer.jl:177-195) -> (cutoffs, weights, avg_residual, codes)"""
    c = colmajor(centroids, np.float32); h = colmajor(heldout, np.float32)
    n = h.shape[1]
    codes = np.zeros(n if n_codes is None else n_codes, dtype=np.uint32)
    cut = np.zeros((1 << nbits) - 1, dtype=np.float32); w = np.zeros(1 << nbits, dtype=np.float32)
    avg = C.c_float(0)
    check(lib().clb_compute_avg_residuals(device, C.c_int(nbits), fptr(c), i64(c.shape[0]), i64(c.shape[1]),
                                          fptr(h), i64(n), fptr(codes), i64(codes.size), fptr(cut), fptr(w),
                                          C.byref(avg)))
    return cut, w, np.float32(avg.value), codes


NEAREST_CHUNK_MAX = 1 << 22          # points per launch of the build's nearest-centroid search (codec.hip)
TIER_LISTS, TIER_SECOND, TIER_EXHAUSTIVE = 0, 1, 2


class NearestScratch:
    """The device scratch of the nearest-centroid search, kept across debug_nearest calls the way k-means keeps it."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().clb_debug_nearest_scratch_create(device, C.byref(self._h)))

    def close(self):
        if self._h:
            check(lib().clb_debug_nearest_scratch_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def debug_nearest(centroids, embs, mode: int = 0, products: int = -1, chunk_max: int = NEAREST_CHUNK_MAX,
                  scratch: NearestScratch | None = None, device: int = 0) -> dict:
    """Test hook (clb_debug_nearest): the build's nearest-centroid search at dim 128 -- mode 0 argmax dot, 1 k-means distance --
    and what its tiers saw.  Returns codes (1-based), vals / gids (n, 2, L): the first tier's group lists per half (gid
    0x7fffffff = empty), margin (n,), tier (n,): TIER_LISTS / TIER_SECOND / TIER_EXHAUSTIVE, and the per-call words x1, cn, dc,
    chunks, undecided1, tier2_points, undecided2."""
    c = colmajor(centroids, np.float32); x = colmajor(embs, np.float32)
    if c.shape[0] != 128 or x.shape[0] != 128:
        raise ValueError("debug_nearest: dim must be 128")
    n, L = x.shape[1], 4
    codes = np.zeros(n, dtype=np.uint32)
    lists = np.zeros((n, 2, L), dtype=np.dtype([("v", "<f4"), ("i", "<i4")]))
    margin = np.zeros(n, dtype=np.float32); tier = np.zeros(n, dtype=np.uint8)
    stats = np.zeros(8, dtype=np.int64)
    check(lib().clb_debug_nearest(device, mode, products, chunk_max, fptr(c), c.shape[1], fptr(x), n,
                                  scratch._h if scratch is not None else None, fptr(codes), fptr(lists), fptr(margin), fptr(tier),
                                  fptr(stats)))
    if stats[7] != L:
        raise RuntimeError(f"debug_nearest: the library's lists hold {stats[7]} entries, this binding reads {L}")
    bits = lambda v: float(np.array([v], dtype=np.uint32).view(np.float32)[0])      # noqa: E731
    return {"codes": codes, "vals": lists["v"].copy(), "gids": lists["i"].copy(), "margin": margin, "tier": tier,
            "x1": bool(stats[0]), "cn": bits(stats[1]), "dc": bits(stats[2]), "chunks": int(stats[3]),
            "undecided1": int(stats[4]), "tier2_points": int(stats[5]), "undecided2": int(stats[6])}


def build_ivf(codes, num_partitions: int, device: int = 0):
    """_build_ivf  (collection_indexer.jl:349-353) -> (ivf Int64[n] 1-based, ivf_lengths Int64[K])"""
    co = np.ascontiguousarray(codes, dtype=np.uint32)
    ivf = np.zeros(co.size, dtype=np.int64); lens = np.zeros(num_partitions, dtype=np.int64)
    check(lib().clb_build_ivf(device, fptr(co), i64(co.size), i64(num_partitions), fptr(ivf), fptr(lens)))
    return ivf, lens


def doc_epilogue(D, integer_ids, skiplist, device: int = 0):
    """_doc_embeddings_and_doclens after the encoder forward  (checkpoint.jl:30-51)"""
    Dm = colmajor(D, np.float32)
    dim, L, N = Dm.shape
    ids = colmajor(integer_ids, np.int32); sk = np.ascontiguousarray(skiplist, dtype=np.int64)
    out = np.zeros((dim, max(L * N, 1)), dtype=np.float32, order="F")
    doclens = np.zeros(N, dtype=np.int64)
    n_out = i64(0)
    check(lib().clb_doc_epilogue(device, fptr(Dm), i64(dim), i64(L), i64(N), fptr(ids), fptr(sk), i64(sk.size),
                                 fptr(out), fptr(doclens), C.byref(n_out)))
    return np.asfortranarray(out[:, : n_out.value]), doclens


def query_epilogue(Q, integer_ids, skiplist, device: int = 0):
    """_query_embeddings after the encoder forward  (checkpoint.jl:61-69)"""
    Qm = colmajor(Q, np.float32).copy(order="F")
    dim, L, N = Qm.shape
    ids = colmajor(integer_ids, np.int32); sk = np.ascontiguousarray(skiplist, dtype=np.int64)
    check(lib().clb_query_epilogue(device, fptr(Qm), i64(dim), i64(L), i64(N), fptr(ids), fptr(sk), i64(sk.size)))
    return Qm


# ---- host-only planning helpers (collection_indexer.jl:17-24, 81-91, 115-139, 342-347) --------------
def num_sampled_pids(num_documents: int) -> int:
    v = 16 * math.sqrt(120 * num_documents)
    return int(min(1 + math.floor(v), num_documents))


def heldout_size(num_sample_embs: int, heldout_fraction: float = 0.05) -> int:
    prod = np.float32(heldout_fraction) * np.float32(num_sample_embs)
    return int(max(1, math.floor(min(np.float32(50000), prod))))


def setup(num_documents: int, avg_doclen_est: float, num_clustering_embs: int, chunksize, nranks: int) -> dict:
    if chunksize is None:
        chunksize = min(25000, 1 + num_documents // nranks)
    num_chunks = -(-num_documents // chunksize)
    est = np.float32(num_documents) * np.float32(avg_doclen_est)
    parts = math.floor(2 ** math.floor(math.log2(float(np.float32(16) * np.sqrt(est)))))
    return {"chunksize": int(chunksize), "num_chunks": int(num_chunks),
            "num_partitions": int(min(num_clustering_embs, parts)), "num_documents": int(num_documents),
            "num_embeddings_est": float(est), "avg_doclen_est": float(np.float32(avg_doclen_est))}


def collect_embedding_id_offset(chunk_emb_counts):
    cnt = list(chunk_emb_counts)
    if not cnt:
        return 0, np.zeros(1, dtype=np.int64)
    off = np.cumsum([1] + cnt[:-1]).astype(np.int64)
    return int(sum(cnt)), off
