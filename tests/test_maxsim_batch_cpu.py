"""codec.maxsim_batch refuses bad arguments before any device work, so these hold on a machine without a GPU."""
import numpy as np
import pytest

import colbert_jl_amd as clb

Q = np.zeros((8, 4, 2), np.float32)
D = np.zeros((8, 5), np.float32)


@pytest.mark.parametrize("error,args", [
    (clb.DimensionMismatch, (Q, D, [2, 2])),                               # sum(doclens) != n_D  (ranking.jl:71-74)
    (clb.ArgumentError, (Q, D, [5, 0])),                                   # reducing over an empty collection
    (clb.BoundsError, (Q, D, [2, 3], [0, 2])),                             # an owner outside 0..B-1
    (clb.BoundsError, (Q, D, [2, 3], [0, -1])),
    (clb.Unsupported, (np.zeros((10, 4, 2), np.float32), np.zeros((10, 5), np.float32), [2, 3])),     # dim % 4 != 0
    (clb.Unsupported, (np.zeros((8, 129, 1), np.float32), D, [2, 3])),     # T > 128
])
def test_host_call_checks_its_arguments_first(error, args):
    with pytest.raises(error) as e:
        clb.codec.maxsim_batch(*args)
    if error is clb.Unsupported:
        assert "clb_maxsim" in str(e.value)
    if error in (clb.ArgumentError, clb.BoundsError):
        assert "passage 1" in str(e.value)


def test_valid_arguments_reach_the_device():
    if clb.lib().clb_device_count() > 0:
        assert clb.codec.maxsim_batch(Q, D, [2, 3]).shape == (2, 2)
    else:
        with pytest.raises(clb.HipError):
            clb.codec.maxsim_batch(Q, D, [2, 3])
    assert clb.lib().clb_maxsim_batch_work_bytes(10, 2, 4) >= 88
