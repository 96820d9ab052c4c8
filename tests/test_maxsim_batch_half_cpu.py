"""The 16-bit dense MaxSim refuses bad arguments before any device work, and the host's bf16 rounding is checked against a
table, so these hold on a machine without a GPU."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

Q = np.zeros((8, 4, 2), np.float32)
D = np.zeros((8, 5), np.float32)


@pytest.mark.parametrize("error,args", [
    (clb.Unsupported, (np.zeros((12, 4, 2), np.float32), np.zeros((12, 5), np.float32), [2, 3])),    # dim % 8 != 0
    (clb.Unsupported, (np.zeros((8, 129, 1), np.float32), D, [2, 3])),                               # T > 128
    (ValueError, (Q, D, [2, 3], [0])),                                                               # an owner of the wrong length
    (clb.DimensionMismatch, (Q, D, [2, 2])),                                                         # validated as maxsim_batch
])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_host_call_checks_its_arguments_first(dtype, error, args):
    with pytest.raises(error):
        codec.maxsim_batch(*args, dtype=dtype)


def test_float16_embeddings_imply_the_16_bit_call():
    with pytest.raises(clb.Unsupported, match="maxsim_batch_half"):
        codec.maxsim_batch(np.zeros((12, 4, 2), np.float32), np.zeros((12, 5), np.float16), [2, 3])   # dim 12 is served in fp32


@pytest.mark.parametrize("q_type,d_type", [(codec.F16, codec.BF16), (codec.BF16, codec.F16), (codec.F32, codec.F32), (codec.F16, 3)])
def test_type_pairs_that_are_not_served(q_type, d_type):
    h, dl, out = np.zeros(64, np.uint16), np.array([2, 3], np.int64), np.zeros(4, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                                        # noqa: E731
    assert clb.lib().clb_maxsim_batch_half(0, p(h), q_type, 8, 4, 2, p(h), d_type, 5, p(dl), 2, None, p(out)) == clb.Unsupported.code


def test_work_bytes_cover_the_offsets_and_the_rounded_queries():
    assert clb.lib().clb_maxsim_batch_half_work_bytes(10, 2, 4, 8) >= clb.lib().clb_maxsim_batch_work_bytes(10, 2, 4) + 2 * 2 * 4 * 8


def test_bfloat16_rounding_is_to_nearest_even():
    table = [(0x00000000, 0x0000), (0x80000000, 0x8000),                 # +-0
             (0x3F800000, 0x3F80), (0x3F807FFF, 0x3F80),                 # below the tie: down
             (0x3F808000, 0x3F80), (0x3F818000, 0x3F82),                 # ties: to the even neighbour, down and up
             (0x3F808001, 0x3F81), (0xBF818000, 0xBF82),                 # above the tie: up; a negative tie
             (0x3FFF8000, 0x4000), (0x3FFFFFFF, 0x4000),                 # a carry into the exponent
             (0x7F7FFFFF, 0x7F80), (0x7F800000, 0x7F80)]                 # the largest float rounds to Inf; Inf stays
    x = np.array([a for a, _ in table], np.uint32).view(np.float32)
    assert codec.to_bfloat16_bits(x).tolist() == [b for _, b in table]
