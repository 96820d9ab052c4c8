"""The MX quantiser's host statement (codec.quantize_mx / dequantize_mx) is plain numpy and the MX dense MaxSim refuses bad
arguments before any device work, so these hold on a machine without a GPU."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

FMTS = ["mxfp8", "mxfp4"]
# per format: (values of one block, its scale byte, its elements as they decode before the scale)
KNOWN = {
    "mxfp8": [
        ([448, 17, 19, 2.0 ** -10, 1.5 * 2.0 ** -9, -1.0625, -1.1875, 0.40625], 127,      # ties go to the even mantissa (0.40625 is no tie: it is kept): among the
         [448, 16, 20, 0, 2.0 ** -8, -1, -1.25, 0.40625]),                               # subnormals, in a low and a high binade
        ([500, 464, -480, 3], 127, [448, 448, -448, 3]),                                  # ilogb(500) = 8: the scaled amax passes 448
        ([0, -0.0], 127, [0, -0.0]),                                                      # an all-zero block
        ([2.0 ** 20, 2.0 ** 11 + 2.0 ** 9], 139, [256, 0.625]),                           # amax an exact power of two: e = 20 - 8
        ([1e-40, 3e-41], 0, [9 / 512, 3 / 512]),           # fp32 subnormals 71362 and 21409 x 2^-149; e clamps at -127: 8.71 and 2.61 x 2^-9
    ],
    "mxfp4": [
        ([6, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5], 127, [6, 0, 1, 1, 2, 2, 4, 4]),
        ([7.9, 7, -6.5, 1], 127, [6, 6, -6, 1]),                                          # ilogb(7.9) = 2: the scaled amax passes 6
        ([0, -0.0], 127, [0, -0.0]),
        ([2.0 ** -3, 1.25 * 2.0 ** -5], 122, [4, 1]),                                     # e = -3 - 2; 1.25 is the tie of 1 and 1.5
        ([1e-40, 3e-41], 0, [0, 0]),                                                      # e clamps at -127; x 2^127 < 0.25 rounds to 0
    ],
}


@pytest.mark.parametrize("fmt,block,byte,want", [(f, *k) for f in FMTS for k in KNOWN[f]])
def test_quantize_mx_known_answers(fmt, block, byte, want):
    X = np.zeros((64, 2), np.float32)
    X[32:32 + len(block), 1] = block                                                      # the second block of the second embedding
    v, s = codec.quantize_mx(X, fmt)
    assert v.dtype == np.uint8 and s.dtype == np.uint8 and v.shape == (64 if fmt == "mxfp8" else 32, 2) and s.shape == (2, 2)
    assert s.tolist() == [[127, 127], [127, byte]]
    got = codec.dequantize_mx(v, s, fmt).astype(np.float64)
    np.testing.assert_array_equal(got[32:32 + len(block), 1], np.array(want) * 2.0 ** (byte - 127))
    np.testing.assert_array_equal(np.signbit(got[32:32 + len(block), 1]), np.signbit(np.array(block)))
    assert not got[:32].any() and not got[:, 0].any()


@pytest.mark.parametrize("fmt", FMTS)
def test_every_representable_value_survives_the_round_trip(fmt):
    codes = np.arange(256 if fmt == "mxfp8" else 16, dtype=np.uint8)
    codes = codes[(codes & 0x7F) != 0x7F] if fmt == "mxfp8" else codes
    v = np.zeros((32, codes.size), np.uint8)
    v[0], v[1] = codes, 0x7E if fmt == "mxfp8" else 7                                    # beside the largest magnitude: the scale is 2^0
    if fmt == "mxfp4":
        v = v[0::2] | (v[1::2] << np.uint8(4))
    for byte in (127, 1, 240):
        s = np.full((1, codes.size), byte, np.uint8)
        v2, s2 = codec.quantize_mx(codec.dequantize_mx(v, s, fmt), fmt)
        np.testing.assert_array_equal(v2, v)
        np.testing.assert_array_equal(s2, s)


def test_element_2i_is_the_low_nibble_of_byte_i():
    X = np.zeros((32, 1), np.float32)
    X[:4, 0] = [6, 0.5, -1, 3]
    v, s = codec.quantize_mx(X, "mxfp4")
    assert v[:2, 0].tolist() == [0x17, 0x5A] and not v[2:].any() and s.tolist() == [[127]]


def test_what_is_refused():
    Q, D = np.zeros((48, 4, 2), np.float32), np.zeros((48, 5), np.float32)
    with pytest.raises(clb.Unsupported, match="dim % 32"):
        codec.quantize_mx(D, "mxfp8")
    q, d = (np.zeros((48, 4, 2), np.uint8), np.zeros((1, 4, 2), np.uint8)), (np.zeros((48, 5), np.uint8), np.zeros((1, 5), np.uint8))
    with pytest.raises(clb.Unsupported, match="maxsim_batch_mx"):                        # CLB_EUNSUPPORTED from the library
        codec.maxsim_batch(q, d, [2, 3], dtype="mxfp8")
    X = np.ones((32, 3), np.float32)
    X[5, 2] = np.inf
    with pytest.raises(clb.ArgumentError, match="embedding 2"):
        codec.quantize_mx(X, "mxfp4")
    with pytest.raises(clb.ArgumentError, match="embedding 2"):                          # CLB_EARGUMENT from the library
        import ctypes as C
        out = np.zeros(64, np.uint8)
        Xf = np.asfortranarray(X)                                                        # (dim, n) column-major, as the library reads it
        clb._lib.check(clb.lib().clb_quantize_mx(0, Xf.ctypes.data_as(C.c_void_p), 32, 3, 5, out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    with pytest.raises(ValueError, match="pair"):                                        # mixed dtypes: int8 values, float scales
        codec.maxsim_batch((np.zeros((32, 4, 2), np.int8), np.zeros((1, 4, 2), np.uint8)), D[:32], [2, 3], dtype="mxfp8")
    with pytest.raises(ValueError, match="pair"):
        codec.maxsim_batch(Q[:32], (np.zeros((32, 5), np.uint8), np.ones((1, 5), np.float32)), [2, 3], dtype="mxfp4")
    with pytest.raises(ValueError, match="fmt"):
        codec.quantize_mx(D, "mxfp6")
    assert clb.lib().clb_maxsim_batch_mx_work_bytes(10, 2, 4, 64) >= clb.lib().clb_maxsim_batch_work_bytes(10, 2, 4) + 2 * 4 * 64 + 2 * 4 * 2
