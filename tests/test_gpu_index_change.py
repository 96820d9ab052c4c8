"""Append, remove and update share one transaction and one set of kernels (csrc/index_change_kernels.hpp, replace_passages and
commit_index_change in csrc/search.hip).  The cases here are the instantiations and branches that the sharing creates and that
tests/test_gpu_append.py, test_gpu_remove.py and test_gpu_update.py do not reach: byte pieces with staged rows, a tile edge of
the row kernel inside a replaced passage, one handle state reached through all three entry points on both list orders, and an
update without new entries (the lists are compacted, not spliced).  Every case compares with a fresh Searcher of the index
the handle should hold and with the CPU oracle searching it."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests.test_gpu_append import Reference, check_like_fresh, check_search
from tests.test_gpu_update import state
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index

pytestmark = pytest.mark.gpu

TILE = 2048         # kTile: the rows of one tile of splice_rows_kernel


@pytest.fixture(scope="module")
def small():
    idx = synthetic.make_index(0, 300, K=64)
    return idx, synthetic.make_queries(idx, 1000, 9)


def no_content(idx, n):
    return np.zeros(0, np.uint32), np.zeros((idx["residuals"].shape[0], 0), np.uint8, order="F"), np.zeros(n, np.int64)


def lists_in_another_order(idx, seed):
    """idx with every inverted list permuted internally: a handle of it keeps the caller's order"""
    rng = np.random.default_rng(seed)
    ivf = idx["ivf"].copy()
    off = np.concatenate([[0], np.cumsum(idx["ivf_lengths"])])
    for c in range(idx["ivf_lengths"].size):
        ivf[off[c]:off[c + 1]] = rng.permutation(ivf[off[c]:off[c + 1]])
    return dict(idx, ivf=ivf)


def appended_index(idx, codes, residuals, doclens):
    a = dict(idx, codes=np.concatenate([idx["codes"], codes]), doclens=np.concatenate([idx["doclens"], doclens]),
             residuals=np.asfortranarray(np.concatenate([idx["residuals"], residuals], axis=1)))
    a["ivf"], a["ivf_lengths"] = synthetic.build_ivf(a["codes"], idx["ivf_lengths"].size)
    return a


def test_update_with_one_byte_rows(oracle):
    """dim 8, nbits 1: a residual row is one byte, so the staged row kernel copies byte pieces"""
    idx = synthetic.make_index(0, 300, K=64, dim=8, nbits=1)
    assert idx["residuals"].shape[0] == 1
    Qs = synthetic.make_queries(idx, 1000, 9)
    pids = np.concatenate([np.arange(2, 300, 3), [1, 300]])
    co, re, dl = content_of(idx, (pids + 100) % 300 + 1)
    keep = np.ones(co.size, bool)
    o = np.concatenate([[0], np.cumsum(dl)])
    dl = dl.copy()
    for i in range(0, pids.size, 5):            # every fifth named passage is emptied
        keep[o[i]:o[i + 1]] = False
        dl[i] = 0
    args = (pids, co[keep], np.asfortranarray(re[:, keep]), dl)
    want = updated_index(idx, *args)
    s = clb.Searcher(index=idx)
    try:
        assert s.update_compressed(*args) == pids.size
        check_search(s, Reference(oracle, want, Qs), ks=(10,))
        check_like_fresh(s, want, Qs, 10)
    finally:
        s.close()


def test_a_tile_edge_inside_a_replaced_passage(oracle, small):
    """the passage that holds output rows 2047 and 2048 -- the last row of the row kernel's first tile and the first of its
    second -- before and after it is replaced by longer content"""
    idx, Qs = small
    off = np.concatenate([[0], np.cumsum(idx["doclens"])])
    pid = int(np.searchsorted(off, TILE, side="right"))          # the passage of row 2048, 1-based
    donor = pid + 7
    co, re, dl = content_of(idx, [pid, donor])                   # its own rows and another's, as ONE passage
    args = ([pid], co, re, np.array([dl.sum()], np.int64))
    want = updated_index(idx, *args)
    new_off = np.concatenate([[0], np.cumsum(want["doclens"])])
    assert want["doclens"][pid - 1] != idx["doclens"][pid - 1]
    for o in (off, new_off):
        assert o[pid - 1] <= TILE - 1 and o[pid] - 1 >= TILE
    assert idx["codes"].size > 2 * TILE and want["codes"].size > 2 * TILE          # at least three tiles of rows
    s = clb.Searcher(index=idx)
    try:
        assert s.update_compressed(*args) == 1
        assert s.num_embeddings == want["codes"].size > 4096
        check_search(s, Reference(oracle, want, Qs), ks=(10,))
        check_like_fresh(s, want, Qs, 10)
    finally:
        s.close()


@pytest.mark.parametrize("lists", ["sorted", "callers_order"])
def test_one_handle_state_through_all_three_entry_points(oracle, small, lists):
    """Removing R, updating R to empty content and a fresh handle of the reduced index agree bit for bit; removing R, appending
    and updating R back to its content gives the appended index.  On lists in the caller's order the update with new
    entries compacts and then merges; without new entries both orders only compact."""
    idx, Qs = small
    start = idx if lists == "sorted" else lists_in_another_order(idx, 62)
    R = np.array([290, 3, 151, 150, 77, 1, 300])
    reduced = reduced_index(idx, R)[0]
    extra = content_of(idx, [10, 200, 11])
    full = appended_index(idx, *extra)
    a, b, c = clb.Searcher(index=start), clb.Searcher(index=start), clb.Searcher(index=start)
    fresh_reduced, fresh_full = clb.Searcher(index=reduced), clb.Searcher(index=full)
    try:
        assert a.remove_passages(R) == R.size and a.generation == 1
        assert b.update_compressed(R, *no_content(idx, R.size)) == R.size and b.generation == 1
        assert a.device_bytes == b.device_bytes == fresh_reduced.device_bytes
        want = state(fresh_reduced, Qs)
        assert state(a, Qs) == want
        assert state(b, Qs) == want
        check_search(b, Reference(oracle, reduced, Qs), ks=(10,), singles=1)

        assert c.remove_passages(R) == R.size
        assert c.add_compressed(*extra) == range(301, 304)
        assert c.update_compressed(R, *content_of(idx, R)) == R.size and c.generation == 3
        assert state(c, Qs) == state(fresh_full, Qs)
        check_search(c, Reference(oracle, full, Qs), ks=(10,), singles=1)
        if lists == "sorted":
            check_like_fresh(c, full, Qs, 10)
    finally:
        for s in (a, b, c, fresh_reduced, fresh_full):
            s.close()


def test_an_update_without_new_entries_leaves_the_lists_of_a_fresh_handle(small):
    """retrieve returns the passages of the probed lists: after an update to empty content on a handle with sorted lists every
    candidate set is a fresh handle's"""
    idx, Qs = small
    R = np.arange(2, 300, 4)
    s, fresh = clb.Searcher(index=idx), clb.Searcher(index=reduced_index(idx, R)[0])
    try:
        assert s.update_compressed(R, *no_content(idx, R.size)) == R.size
        for nprobe in (1, 2, 8):
            for j in range(Qs.shape[2]):
                assert np.array_equal(s.retrieve(Qs[:, :, j], nprobe=nprobe), fresh.retrieve(Qs[:, :, j], nprobe=nprobe)), (nprobe, j)
    finally:
        s.close(); fresh.close()
