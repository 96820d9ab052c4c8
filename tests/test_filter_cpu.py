"""Filtered search, the part that needs no GPU: the composed reference of tests/util_filter.py is the oracle's search
when nothing is filtered, the C ABI declares and exports the filter entry points and refuses null handles before any
device work, and the Python keywords are validated on the host."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd.searcher import PassageFilter, Searcher
from tests.util_filter import filtered_reference

NEW_SYMBOLS = ("clb_filter_create_pids", "clb_filter_create_bitmap", "clb_filter_count", "clb_filter_destroy",
               "clb_search_batch_filtered", "clb_search_batch_filtered_device_slot")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("seed,n_docs,K,k", [(1, 300, 64, 10), (3, 20_000, 2048, 1000)])
def test_composed_reference_is_the_oracles_search_when_nothing_is_filtered(oracle, seed, n_docs, K, k):
    """retrieve -> gather -> decompress -> maxsim -> stable sort, composed from the oracle's pieces, against oracle.search:
    identical pids, bit-identical fp32 scores, the same candidate count -- and an all-ones filter changes nothing."""
    assert hasattr(clb, "PassageFilter")                       # the feature this helper is the reference of
    idx = synthetic.make_index(seed=seed, n_docs=n_docs, K=K)
    Qs = synthetic.make_queries(idx, seed + 1, 3)
    everything = np.arange(1, n_docs + 1)
    for j in range(3):
        rp, rs, rn = oracle.search(idx, Qs[:, :, j], nprobe=2, k=k)
        for allowed in (None, everything):
            p, s, n = filtered_reference(oracle, idx, Qs[:, :, j], 2, k, allowed)
            assert n == rn and np.array_equal(p, rp), (seed, j)
            assert np.array_equal(bits(s), bits(rs)), (seed, j)


def test_filter_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    header = open(clb._lib.HEADER).read()
    assert "CLB_FILTER_CANDIDATES = 0" in header and "CLB_FILTER_ALL = 1" in header
    assert "outlive" in header                                 # the lifetime rule is part of the contract


def test_filter_entry_points_check_their_arguments_first():
    """Null handles are ArgumentError (4) before any device work; counting a null filter is 0; destroying one is fine."""
    l = clb.lib()
    i64 = C.c_int64
    null, out = C.c_void_p(), C.c_void_p()
    pids = np.array([1, 2], np.int64)
    words = np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert l.clb_filter_create_pids(null, p(pids), i64(2), C.byref(out)) == 4
    assert b"null" in l.clb_last_error()
    assert l.clb_filter_create_bitmap(null, p(words), i64(1), C.byref(out)) == 4
    assert out.value is None
    # a null `out`: refused whatever the searcher (a non-null one cannot be made without a device, so the null one stands in)
    assert l.clb_filter_create_pids(null, p(pids), i64(2), None) == 4
    assert l.clb_filter_create_bitmap(null, p(words), i64(1), None) == 4
    q = np.zeros((128, 32, 1), np.float32, order="F")
    op, os_, nc = np.zeros(5, np.int64), np.zeros(5, np.float32), np.zeros(1, np.int64)
    handles = (C.c_void_p * 1)()
    assert l.clb_search_batch_filtered(null, p(q), i64(32), i64(1), i64(2), i64(5), handles, 0, p(op), p(os_), p(nc)) == 4
    assert l.clb_search_batch_filtered_device_slot(null, 0, None, i64(32), i64(1), i64(2), i64(5), handles, 0, None, None, None,
                                                   None) == 4
    assert l.clb_filter_count(null) == 0
    assert l.clb_filter_destroy(null) == 0                     # like clb_searcher_destroy


class _NoDevice(Searcher):
    """The host side of a Searcher without its handle: enough for the checks that run before the library is called."""

    def __init__(self, num_docs=100, dim=128):
        self.num_docs, self.dim, self._h = num_docs, dim, None
        self.config = clb.ColBERTConfig()


def test_python_keywords_are_validated_on_the_host():
    s = _NoDevice()
    with pytest.raises(clb.ColBERTError, match="exactly one"):
        s.make_filter()
    with pytest.raises(clb.ColBERTError, match="exactly one"):
        s.make_filter(pids=[1], mask=np.ones(100, bool))
    with pytest.raises(clb.ColBERTError, match="num_docs"):
        s.make_filter(mask=np.ones(99, bool))
    with pytest.raises(clb.ColBERTError, match="boolean"):
        s.make_filter(mask=np.ones(100, np.int32))
    Q = np.zeros((128, 4), np.float32)
    with pytest.raises(clb.ColBERTError, match="scope"):
        s.search_embeddings(Q, 5, scope="everything")
    with pytest.raises(clb.ColBERTError, match="scope"):
        s.search_batch(Q[:, :, None], 5, scope="none")
    with pytest.raises(clb.ColBERTError, match="scope"):
        clb.search(s, Q, 5, scope=1)
    with pytest.raises(clb.ColBERTError, match="scope"):
        s.search("a query", 5, scope="ALL")
    f = PassageFilter(s, None, 3)                              # closed: no handle
    assert f.count == 3 and len(f) == 3
    with pytest.raises(clb.ColBERTError, match="sequence of B=2"):
        s.search_batch(np.zeros((128, 4, 2), np.float32), 5, filters=[None])
    with pytest.raises(clb.ColBERTError, match="open PassageFilter"):
        s.search_batch(np.zeros((128, 4, 2), np.float32), 5, filters=[None, f])
    with f:                                                    # a context manager; closing a closed filter is fine
        pass
    f.close()
