"""Appending to an index, the parts that need no GPU: the host IVF merge against `_build_ivf` of the concatenated codes, the
index directory after `append_chunk` (and after an interrupted one), the argument contracts of the new C entry points, and
the Julia binding."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import storage, synthetic
from tests.util_synth import tiny_index


def head_of(idx, P):
    """(codes, residuals, doclens) of the first P passages, and the number of their embeddings"""
    n = int(idx["doclens"][:P].sum())
    return idx["codes"][:n], idx["residuals"][:, :n], idx["doclens"][:P], n


def tail_of(idx, P, P2=None):
    a = int(idx["doclens"][:P].sum())
    b = int(idx["doclens"][:P2].sum()) if P2 is not None else idx["codes"].size
    return idx["codes"][a:b], idx["residuals"][:, a:b], idx["doclens"][P:P2]


@pytest.mark.parametrize("P", [1, 150, 299])
def test_merge_ivf_equals_build_ivf_of_the_concatenation(P):
    idx, _ = tiny_index()
    K = idx["ivf_lengths"].size
    hc, _, _, n = head_of(idx, P)
    ivf, lens = synthetic.build_ivf(hc, K)
    got_ivf, got_lens = storage.merge_ivf(ivf, lens, n, tail_of(idx, P)[0])
    assert got_ivf.dtype == np.int64 and np.array_equal(got_ivf, idx["ivf"])
    assert np.array_equal(got_lens, idx["ivf_lengths"])


def test_merge_ivf_three_successive_splits_and_a_first_ever_centroid():
    idx, _ = tiny_index()
    K = idx["ivf_lengths"].size
    cuts = [1, 101, 201, 300]
    hc, _, _, n = head_of(idx, cuts[0])
    # the one-passage head leaves most centroids empty: the tails hold their first-ever embeddings
    ivf, lens = synthetic.build_ivf(hc, K)
    first_ever = np.setdiff1d(tail_of(idx, 1, 101)[0], hc)
    assert first_ever.size > 0 and np.all(lens[first_ever.astype(np.int64) - 1] == 0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        tc = tail_of(idx, a, b)[0]
        ivf, lens = storage.merge_ivf(ivf, lens, n, tc)
        n += tc.size
        ref_ivf, ref_lens = synthetic.build_ivf(idx["codes"][:n], K)
        assert np.array_equal(ivf, ref_ivf) and np.array_equal(lens, ref_lens), (a, b)
    assert np.array_equal(ivf, idx["ivf"]) and np.array_equal(lens, idx["ivf_lengths"])


def test_merge_ivf_empty_tail_and_bad_codes():
    idx, _ = tiny_index()
    ivf, lens = storage.merge_ivf(idx["ivf"], idx["ivf_lengths"], idx["codes"].size, np.zeros(0, np.uint32))
    assert np.array_equal(ivf, idx["ivf"]) and np.array_equal(lens, idx["ivf_lengths"])
    with pytest.raises(ValueError):
        storage.merge_ivf(idx["ivf"], idx["ivf_lengths"], idx["codes"].size, np.array([65], np.uint32))


def write_index(path, idx, P):
    """the first P passages of idx as a one-chunk index directory"""
    hc, hr, hd, _ = head_of(idx, P)
    K = idx["ivf_lengths"].size
    storage.save_codec(path, idx["centroids"], idx["bucket_cutoffs"], idx["bucket_weights"], np.float32(0.01))
    storage.save_chunk(path, hc, hr, 1, 1, hd)
    storage.save_json(path, "config.json", {"dim": int(idx["dim"]), "nbits": int(idx["nbits"])})
    storage.save_json(path, "plan.json", {"num_chunks": 1, "num_partitions": K, "num_embeddings": int(hc.size)})
    ivf, lens = synthetic.build_ivf(hc, K)
    storage._save(os.path.join(path, "ivf"), ivf)
    storage._save(os.path.join(path, "ivf_lengths"), lens)


def assert_loads_as(path, idx, P):
    got = storage.load_index(path)
    hc, hr, hd, n = head_of(idx, P)
    ivf, lens = synthetic.build_ivf(hc, idx["ivf_lengths"].size)
    for name, want in (("codes", hc), ("residuals", hr), ("doclens", hd), ("ivf", ivf), ("ivf_lengths", lens)):
        assert np.array_equal(np.asarray(got[name]), want), name
    assert storage.check_all_files_are_saved(path)


def test_append_chunk_gives_the_full_index_on_disk(tmp_path):
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    write_index(path, idx, 150)
    assert_loads_as(path, idx, 150)
    storage.append_chunk(path, *tail_of(idx, 150, 250))
    storage.append_chunk(path, *tail_of(idx, 250))
    assert_loads_as(path, idx, 300)
    plan = storage.load_json(path, "plan.json")
    assert plan["num_chunks"] == 3 and plan["num_embeddings"] == idx["codes"].size
    meta = storage.load_json(path, "3.metadata.json")
    assert meta["passage_offset"] == 251 and meta["embedding_offset"] == int(idx["doclens"][:250].sum()) + 1
    assert meta["num_passages"] == 50
    assert not [f for f in os.listdir(path) if ".tmp" in f]


def test_interrupted_append_still_reads_as_the_old_index(tmp_path):
    """append_chunk rewrites plan.json last.  Stopped before that -- the new chunk's files and the merged ivf / ivf_lengths
    are in place, the plan still names one chunk -- the directory must load as the old index; so must the state one
    rename earlier (merged ivf, old ivf_lengths).  A later append_chunk then completes normally."""
    idx, _ = tiny_index()
    path, done = str(tmp_path / "index"), str(tmp_path / "done")
    write_index(path, idx, 150)
    old_plan = open(os.path.join(path, "plan.json")).read()
    old_lens = open(os.path.join(path, "ivf_lengths" + storage.EXT), "rb").read()
    shutil.copytree(path, done)
    storage.append_chunk(done, *tail_of(idx, 150))
    for stop_before_lengths in (False, True):
        shutil.rmtree(path)
        shutil.copytree(done, path)
        with open(os.path.join(path, "plan.json"), "w") as f:
            f.write(old_plan)
        if stop_before_lengths:
            with open(os.path.join(path, "ivf_lengths" + storage.EXT), "wb") as f:
                f.write(old_lens)
        assert json.loads(old_plan)["num_chunks"] == 1
        assert_loads_as(path, idx, 150)
        storage.append_chunk(path, *tail_of(idx, 150))
        assert_loads_as(path, idx, 300)


def test_new_entry_points_check_their_arguments_first():
    """Without a GPU: a null searcher is CLB_EARGUMENT (4) from all five new functions -- the three getters return counts,
    so they carry it negated (include/colbert_hip.h) -- and a bad argument is refused before any device work."""
    l = clb.lib()
    null = C.c_void_p()
    i64 = C.c_int64
    dl = np.array([2], np.int64); co = np.ones(2, np.uint32); r = np.zeros((32, 2), np.uint8, order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert l.clb_searcher_append(null, i64(1), p(dl), i64(2), p(co), p(r)) == 4
    assert b"null" in l.clb_last_error()
    assert l.clb_searcher_append_device(null, i64(1), p(dl), i64(2), p(co), p(r), None) == 4
    assert l.clb_searcher_append(null, i64(0), None, i64(0), None, None) == 4
    for getter in (l.clb_searcher_generation, l.clb_searcher_num_docs, l.clb_searcher_num_embeddings):
        assert getter.restype is C.c_int64
        assert getter(null) == -4
        assert b"null" in l.clb_last_error()


def test_python_surface_without_a_device():
    assert {"clb_searcher_append", "clb_searcher_append_device", "clb_searcher_generation", "clb_searcher_num_docs",
            "clb_searcher_num_embeddings"} <= set(clb.declared_symbols())
    for name in ("add_compressed", "add_embeddings", "add_passages", "generation"):
        assert hasattr(clb.Searcher, name), name


def test_the_julia_shim_binds_append():
    from tests.test_julia_shim_abi import julia_ccalls
    bound = {c[1] for c in julia_ccalls()}
    for name in ("clb_searcher_append", "clb_searcher_generation", "clb_searcher_num_docs", "clb_searcher_num_embeddings"):
        assert name in bound, name
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "ColBERT", "src",
                             "searching.jl")).read()
    assert "function add_compressed!(searcher::Searcher" in text
