"""The int8 dense MaxSim refuses bad arguments before any device work, and the host quantiser is plain numpy, so these hold on
a machine without a GPU."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

Q8 = (np.ones((16, 4, 2), np.int8), np.ones((4, 2), np.float32))
D8 = np.ones((16, 5), np.int8)


def test_a_dim_that_is_not_served_names_the_call():
    with pytest.raises(clb.Unsupported, match="maxsim_batch_i8"):
        codec.maxsim_batch(np.zeros((24, 4, 2), np.float32), np.zeros((24, 5), np.float32), [2, 3], dtype="int8")


@pytest.mark.parametrize("scale", [-1.0, np.inf, np.nan])
@pytest.mark.parametrize("side", ["Q", "D"])
def test_a_negative_or_non_finite_scale_is_refused(side, scale):
    qs, ds = Q8[1].copy(), np.ones(5, np.float32)
    (qs if side == "Q" else ds).flat[3] = scale
    with pytest.raises(clb.ArgumentError, match="scale of"):
        codec.maxsim_batch((Q8[0], qs), (D8, ds), [2, 3])


def test_quantize_rows_refuses_a_non_finite_value():
    X = np.ones((16, 3), np.float32)
    X[5, 2] = np.inf
    with pytest.raises(clb.ArgumentError, match="embedding 2"):
        codec.quantize_rows(X)


def test_int8_embeddings_without_scales_are_refused():
    with pytest.raises(ValueError, match="scales"):
        codec.maxsim_batch(Q8, D8, [2, 3])


def test_work_bytes_cover_the_offsets_and_a_query_quantised_in_the_call():
    l = clb.lib()
    assert l.clb_maxsim_batch_i8_work_bytes(10, 2, 4, 16) >= l.clb_maxsim_batch_work_bytes(10, 2, 4) + 2 * 4 * 16 + 2 * 4 * 4


def test_quantize_rows_on_a_hand_made_example():
    X = np.zeros((16, 3), np.float32)
    X[:4, 0] = [127.0, -63.5, 62.5, 0.4]          # s = 1: the ties -63.5 and 62.5 go to the even neighbour
    X[:3, 2] = [-0.5, 0.25, 0.1]                  # s = fl32(0.5 / 127)
    X8, s = codec.quantize_rows(X)
    s2 = np.float32(0.5) / np.float32(127)
    assert s.dtype == np.float32 and s.tolist() == [1.0, 0.0, float(s2)]
    assert X8.dtype == np.int8 and X8[:4, 0].tolist() == [127, -64, 62, 0] and not X8[:, 1].any()
    assert X8[:3, 2].tolist() == [-127, int(np.rint(np.float32(0.25) / s2)), int(np.rint(np.float32(0.1) / s2))] and not X8[4:].any()
