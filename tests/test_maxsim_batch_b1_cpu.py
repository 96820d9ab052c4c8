"""Dense MaxSim on 1-bit sign embeddings, the part that needs no GPU: the symbols are declared and exported, `binarize_rows` is
the numpy statement of the format, and argument errors are answered before any launch."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import codec

EARGUMENT, EUNSUPPORTED, EHIP = clb.ArgumentError.code, clb.Unsupported.code, clb.HipError.code
SOME = C.c_void_p(0x7000)                                       # 16-byte aligned, never read: no call here gets as far as a launch
i64 = C.c_int64


def call(store=False, dim=128, T=32, B=2, n=10, N=4, work_bytes=1 << 20, **ptrs):
    p = dict(Q=SOME, qscale=SOME, D=SOME, scale=SOME, lens=SOME, pids=SOME, scores=SOME, work=SOME)
    p.update(ptrs)
    head, tail = (0, p["Q"], codec.I8, p["qscale"], i64(dim), i64(T), i64(B), p["D"], p["scale"]), (None, p["scores"], p["work"], i64(work_bytes), None)
    if store:
        return clb.lib().clb_maxsim_store_device(*head, codec.B1, i64(n), p["lens"], i64(3), p["pids"], i64(N), *tail)
    return clb.lib().clb_maxsim_batch_b1_device(*head, i64(n), p["lens"], i64(N), *tail)


def test_symbols_are_declared_and_exported():
    for name in ("clb_maxsim_batch_b1_work_bytes", "clb_maxsim_batch_b1_device", "clb_maxsim_batch_b1", "clb_binarize_rows_device", "clb_binarize_rows"):
        assert name in clb.declared_symbols() and hasattr(clb.lib(), name), name
    assert codec.B1 == 16 and clb.binarize_rows is codec.binarize_rows and clb.binarize_rows_device and clb.unbinarize_rows


def test_binarize_rows_is_the_statement_of_the_format():
    X = np.random.default_rng(1).standard_normal((128, 4)).astype(np.float32)
    X[:8, 0] = [1, -1, -0.0, 2, -3, -4, 5, -6]                   # least significant bit first, -0.0 counts as >= 0: 0b01001101
    X[:, 1] = 0
    v, s = codec.binarize_rows(X)
    assert v.dtype == np.uint8 and v.shape == (16, 4) and v[0, 0] == 0b01001101 and np.all(v[:, 1] == 255)
    assert s.dtype == np.float32 and s[1] == 0 and s[0] == np.float32(np.abs(X[:, 0]).astype(np.float64).mean())
    back = codec.unbinarize_rows(v, s)
    assert back.dtype == np.float32 and np.array_equal(back, np.where(X >= 0, s, -s))
    X[5, 2] = np.inf
    with pytest.raises(clb.ArgumentError, match="embedding 2"):
        codec.binarize_rows(X)


@pytest.mark.parametrize("store", [False, True])
def test_argument_errors_come_before_any_launch(store):
    for dim in (64, 192):
        assert call(store, dim=dim) == EUNSUPPORTED, dim
    assert call(store, T=129) == EUNSUPPORTED
    for null in ("Q", "qscale", "D", "scale", "lens", "scores", "work") + (("pids",) if store else ()):
        assert call(store, **{null: None}) == EARGUMENT, null
    assert call(store, D=C.c_void_p(0x7008)) == EARGUMENT and call(store, work_bytes=8) == EARGUMENT
    if clb.lib().clb_device_count() == 0:
        assert call(store) == EHIP
    with pytest.raises(clb.Unsupported):
        codec.maxsim_batch(np.zeros((192, 4, 2), np.float32), (np.zeros((24, 5), np.uint8), np.ones(5, np.float32)), [2, 3], dtype="binary")


def test_work_bytes_are_the_offsets_and_a_query_quantised_in_the_call():
    pad = lambda n: (n + 255) // 256 * 256                                                                                  # noqa: E731
    l = clb.lib()
    assert l.clb_maxsim_batch_b1_work_bytes(i64(1000), i64(3), i64(33), i64(256)) == pad(8 * 1001) + pad(256 * 99) + pad(4 * 99)
    assert l.clb_maxsim_store_work_bytes(i64(1000), i64(3), i64(33), i64(256), codec.B1) == pad(256 * 99) + pad(4 * 99)
