"""Dense MaxSim by passage id (clb_maxsim_store_device), the part that needs no GPU: the two symbols are declared and exported,
argument errors are answered before any launch, and the work buffer holds the converted query alone."""
import ctypes as C

import pytest

import colbert_jl_amd as clb

F32, F16, BF16, I8, MXFP8, MXFP4 = range(6)
EARGUMENT, EUNSUPPORTED, EHIP = clb.ArgumentError.code, clb.Unsupported.code, clb.HipError.code
SOME = C.c_void_p(0x7000)                                       # 16-byte aligned, never read: no call here gets as far as a launch
i64 = C.c_int64


def call(q_type=F32, d_type=F32, dim=128, T=32, B=2, n_rows=10, P=3, N=4, work_bytes=1 << 20, **ptrs):
    p = dict(Q=SOME, qscale=SOME, store=SOME, scale=SOME, off=SOME, pids=SOME, owner=None, scores=SOME, work=SOME)
    p.update(ptrs)
    return clb.lib().clb_maxsim_store_device(0, p["Q"], q_type, p["qscale"], i64(dim), i64(T), i64(B), p["store"], p["scale"], d_type, i64(n_rows),
                                             p["off"], i64(P), p["pids"], i64(N), p["owner"], p["scores"], p["work"], i64(work_bytes), None)


def test_store_symbols_are_declared_and_exported():
    for name in ("clb_maxsim_store_work_bytes", "clb_maxsim_store_device"):
        assert name in clb.declared_symbols(), name
        assert hasattr(clb.lib(), name), name


@pytest.mark.parametrize("d_type", range(6))
def test_argument_errors_come_before_any_launch(d_type):
    q_own = (F32, F16, BF16, I8, MXFP8, MXFP8)[d_type]
    for null in ("Q", "store", "off", "pids", "scores", "work"):
        assert call(d_type=d_type, **{null: None}) == EARGUMENT == 4, null
    if d_type >= I8:                                            # a format with scales needs the store's, and its own query's
        assert call(d_type=d_type, scale=None) == EARGUMENT
        assert call(q_type=q_own, d_type=d_type, qscale=None) == EARGUMENT
    assert call(d_type=d_type, store=C.c_void_p(0x7008)) == EARGUMENT          # alignment
    assert call(d_type=d_type, work_bytes=8) == EARGUMENT
    assert call(d_type=d_type, P=-1) == EARGUMENT and call(d_type=d_type, B=0) == EARGUMENT
    for bad in [t for t in range(6) if t not in (F32, q_own)] + [-1, 6]:
        assert call(q_type=bad, d_type=d_type) == EUNSUPPORTED, bad
    for dim in (0, 4 if d_type else 2, 1040, 129):
        assert call(d_type=d_type, dim=dim) == EUNSUPPORTED, dim
    assert call(d_type=d_type, T=0) == EUNSUPPORTED and call(d_type=d_type, T=129) == EUNSUPPORTED and call(d_type=d_type + 6) == EUNSUPPORTED
    assert call(d_type=d_type, N=0, Q=None, store=None, pids=None, scores=None, work=None) == 0      # nothing to score, nothing launched
    if clb.lib().clb_device_count() == 0:
        assert call(d_type=d_type) == EHIP and call(q_type=q_own, d_type=d_type, owner=SOME) == EHIP


def test_work_bytes_cover_the_converted_query_and_no_offsets():
    wb = lambda N, d_type, B=3, T=33, dim=96: clb.lib().clb_maxsim_store_work_bytes(i64(N), i64(B), i64(T), i64(dim), d_type)   # noqa: E731
    pad = lambda n: (n + 255) // 256 * 256                                                                                   # noqa: E731
    bt = 3 * 33
    assert wb(1000, F32) == 16                                  # never empty, so the pointer is never null
    assert wb(1000, F16) == wb(1000, BF16) == pad(2 * 96 * bt)
    assert wb(1000, I8) == pad(96 * bt) + pad(4 * bt)
    assert wb(1000, MXFP8) == wb(1000, MXFP4) == pad(96 * bt) + pad(3 * bt)
    for d_type in range(6):
        assert wb(1, d_type) == wb(10 ** 9, d_type)             # the list's length costs nothing: no offsets are kept
        assert call(d_type=d_type, dim=96, T=33, B=3, work_bytes=wb(1, d_type) - 1) == EARGUMENT
