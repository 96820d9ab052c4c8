"""The Searcher handle's lifecycle code (csrc/search.hip): what clb_searcher_create refuses, by either constructor, and what
it leaves behind when it does; the rules that more than one entry point applies (pass 1's default gather form)."""
import ctypes as C
import re

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd._lib import fptr, i64
from tests.test_gpu_append import Reference, check_search

pytestmark = pytest.mark.gpu


def device_arrays(idx):
    """the index with its large arrays as CUDA tensors in the layouts of clb_searcher_create_device"""
    import torch
    dev = torch.device("cuda", 0)
    d = dict(idx)
    d["centroids"] = torch.from_numpy(np.ascontiguousarray(idx["centroids"].T)).to(dev)
    d["codes"] = torch.from_numpy(np.ascontiguousarray(idx["codes"], np.uint32).view(np.int32)).to(dev)
    d["residuals"] = torch.from_numpy(np.ascontiguousarray(idx["residuals"].T)).to(dev)
    d["ivf"] = torch.from_numpy(np.ascontiguousarray(idx["ivf"], np.int64)).to(dev)
    return d


def changed(idx, name, at, value):
    bad = dict(idx)
    bad[name] = idx[name].copy()
    bad[name][at] = value
    return bad


def create_rc(idx):
    """clb_searcher_create on host arrays, called directly: (return code, the out handle, the message)"""
    l = clb.lib()
    c = np.asfortranarray(idx["centroids"], np.float32)
    w = np.ascontiguousarray(idx["bucket_weights"], np.float32)
    dl, il = np.ascontiguousarray(idx["doclens"], np.int64), np.ascontiguousarray(idx["ivf_lengths"], np.int64)
    co, iv = np.ascontiguousarray(idx["codes"], np.uint32), np.ascontiguousarray(idx["ivf"], np.int64)
    r = np.asfortranarray(idx["residuals"], np.uint8)
    out = C.c_void_p(0xdead0)          # not null before the call: a failed create must clear it
    rc = l.clb_searcher_create(0, i64(128), C.c_int(2), i64(c.shape[1]), fptr(c), fptr(w), i64(dl.size), fptr(dl), i64(co.size),
                               fptr(co), fptr(r), fptr(iv), fptr(il), i64(0), C.byref(out))
    return rc, out, l.clb_last_error().decode()


@pytest.mark.parametrize("constructor", ["host_arrays", "device_arrays"])
def test_create_rejections_leave_nothing_behind(oracle, constructor):
    """Every rejection of clb_searcher_create / clb_searcher_create_device, the two found on the host before any device work
    and the ones a kernel finds after the handle and most of its buffers exist: the documented exception, the out handle
    null, a bad ivf id before a bad code -- and afterwards a good create on the same device answers as the oracle does."""
    idx = synthetic.make_index(seed=21, n_docs=50, K=16)
    n_emb, K = idx["codes"].size, 16
    both = changed(changed(idx, "ivf", 0, n_emb + 1), "codes", 3, K + 1)
    cases = [("doclens sum", changed(idx, "doclens", -1, idx["doclens"][-1] + 1), clb.DimensionMismatch, "sum(doclens)="),
             ("negative doclen", changed(idx, "doclens", 2, -idx["doclens"][2]), clb.ArgumentError, "negative doclen at passage 3"),
             ("ivf_lengths sum", changed(idx, "ivf_lengths", 0, idx["ivf_lengths"][0] + 1), clb.DimensionMismatch, "sum(ivf_lengths)"),
             ("ivf id", changed(idx, "ivf", 0, n_emb + 1), clb.BoundsError, "outside 1..n_emb"),
             ("code", changed(idx, "codes", 3, K + 1), clb.DomainError, "valid range of centroid IDs"),
             ("ivf id and code", both, clb.BoundsError, "outside 1..n_emb")]
    for what, bad, exc, text in cases:
        with pytest.raises(exc, match=re.escape(text)):
            clb.Searcher(index=device_arrays(bad) if constructor == "device_arrays" else bad)
        if constructor == "host_arrays":
            rc, out, msg = create_rc(bad)
            assert rc == exc.code and text in msg and out.value is None, (what, rc, msg, out.value)
    Qs = synthetic.make_queries(idx, 22, 4)
    s = clb.Searcher(index=device_arrays(idx) if constructor == "device_arrays" else idx)
    try:
        check_search(s, Reference(oracle, idx, Qs), ks=(10,))
    finally:
        s.close()


def uniform_codes_index(K, n_docs=50, doclen=60, seed=5):
    """an index straight from arrays: uniformly random codes over K centroids (no two neighbours share a score-table line)"""
    rng = np.random.default_rng(seed)
    n = n_docs * doclen
    cent = rng.normal(size=(128, K)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=0, keepdims=True)
    codes = rng.integers(1, K + 1, size=n).astype(np.uint32)
    ivf, lens = synthetic.build_ivf(codes, K)
    return {"dim": 128, "nbits": 2, "centroids": np.asfortranarray(cent),
            "bucket_weights": np.array([-0.05, -0.01, 0.01, 0.05], np.float32), "doclens": np.full(n_docs, doclen, np.int64),
            "codes": codes, "residuals": np.asfortranarray(rng.integers(0, 256, size=(32, n), dtype=np.uint8)),
            "ivf": ivf, "ivf_lengths": lens}


@pytest.mark.parametrize("index", ["topical_K16", "uniform_K66048"])
def test_gather_form_reset_equals_a_fresh_handle(index):
    """set_pass1_gather(-1) after a forced form gives what a fresh handle has: VGPR on the small topical index; LDS-DMA on
    uniformly random codes over K = 66 048 centroids (K * 64 B beyond the 4-MB L2 of an XCD) -- the fresh handle must
    report that form there, or the reset would be compared with a rule that never says 1."""
    idx = synthetic.make_index(seed=21, n_docs=50, K=16) if index == "topical_K16" else uniform_codes_index(66048)
    fresh, s = clb.Searcher(index=idx), clb.Searcher(index=idx)
    try:
        form, adjacency = fresh.pass1_gather
        assert form == (1 if index == "uniform_K66048" else 0), (form, adjacency)
        for forced in (1, 0):
            s.set_pass1_gather(forced)
            assert s.pass1_gather[0] == forced
            s.set_pass1_gather(-1)
            assert s.pass1_gather == fresh.pass1_gather
    finally:
        fresh.close(); s.close()
