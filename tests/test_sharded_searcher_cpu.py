"""The sharded handle without a GPU: the library exports the two entry points it is built on and they check their arguments
before any device work, and the host logic of `ShardedSearcher` -- pid tiling, pid-to-shard routing, mask slicing, the
group-range BoundsError -- against numpy on stub shards that own no device."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import sharded


def test_library_exports_the_sharded_filter_entry_points():
    l = clb.lib()
    for name in ("clb_search_shard_phase1_filtered_slot", "clb_filter_create_pids_global"):
        assert name in clb.declared_symbols()
        assert hasattr(l, name)


def test_new_entry_points_check_their_arguments_first():
    l = clb.lib()
    null = C.c_void_p()
    out, n = C.c_void_p(), C.c_int64(7)
    top = (C.c_float * 4)()
    pids = np.array([1, 2], np.int64)
    assert l.clb_search_shard_phase1_filtered_slot(null, 0, None, 32, 1, 2, 4, None, 0, top, None) == 4
    assert b"null" in l.clb_last_error()
    assert l.clb_search_shard_phase1_filtered_slot(null, 0, None, 32, 1, 2, 4, None, 0, None, None) == 4
    assert l.clb_filter_create_pids_global(null, pids.ctypes.data_as(C.c_void_p), 2, C.byref(out), C.byref(n)) == 4
    assert out.value is None and n.value == 0               # the outputs are cleared even when the call is refused
    assert l.clb_filter_create_pids_global(null, None, 0, None, None) == 4
    assert b"null" in l.clb_last_error()


class StubShard:
    """What ShardedSearcher reads of a Searcher, with no device behind it."""

    def __init__(self, pid_offset, num_docs, dim=128, nbits=2, K=64):
        self.pid_offset, self.num_docs, self.dim, self.nbits, self.num_centroids = pid_offset, num_docs, dim, nbits, K
        self.bound_consts = np.full(6, 1.0 + pid_offset, np.float32)
        self.removed = []
        self.closed = False

    def raise_bound_consts(self, c):
        self.bound_consts = np.maximum(self.bound_consts, np.asarray(c, np.float32))

    def remove_passages(self, pids):
        assert np.all((pids > self.pid_offset) & (pids <= self.pid_offset + self.num_docs))
        self.removed.append(np.array(pids))
        return int(np.unique(pids).size)

    def close(self):
        self.closed = True


SIZES = [5, 1, 7, 3]


def stub_group():
    off = np.concatenate([[0], np.cumsum(SIZES)])
    return clb.ShardedSearcher([StubShard(int(off[i]), SIZES[i]) for i in range(len(SIZES))])


def test_tiling_is_validated():
    g = stub_group()
    assert g.num_docs == 16
    assert g.shard_ranges == [range(1, 6), range(6, 7), range(7, 14), range(14, 17)]
    # one error bound on every shard after construction: the element-wise maximum
    for s in g.shards:
        assert np.array_equal(s.bound_consts, np.full(6, 14.0, np.float32))
    with pytest.raises(clb.ColBERTError, match="tile"):
        clb.ShardedSearcher([StubShard(0, 5), StubShard(6, 4)])          # a gap
    with pytest.raises(clb.ColBERTError, match="tile"):
        clb.ShardedSearcher([StubShard(0, 5), StubShard(4, 4)])          # an overlap
    with pytest.raises(clb.ColBERTError, match="tile"):
        clb.ShardedSearcher([StubShard(5, 4), StubShard(0, 5)])          # not in pid order
    with pytest.raises(clb.ColBERTError, match="agree on K"):
        clb.ShardedSearcher([StubShard(0, 5), StubShard(5, 4, K=32)])
    with pytest.raises(clb.ColBERTError, match="agree on nbits"):
        clb.ShardedSearcher([StubShard(0, 5), StubShard(5, 4, nbits=4)])
    with pytest.raises(clb.ColBERTError, match="agree on dim"):
        clb.ShardedSearcher([StubShard(0, 5, dim=64), StubShard(5, 4)])
    with pytest.raises(clb.ColBERTError):
        clb.ShardedSearcher([])
    # a group need not start at passage 1
    g2 = clb.ShardedSearcher([StubShard(10, 5), StubShard(15, 2)])
    assert g2.shard_ranges == [range(11, 16), range(16, 18)] and g2.num_docs == 7
    with pytest.raises(clb.BoundsError):
        sharded.check_group_pids([10], g2._bounds)
    g.close()
    assert all(s.closed for s in g.shards)


def test_pid_routing_against_numpy():
    g = stub_group()
    bounds = g._bounds
    rng = np.random.default_rng(7)
    pids = rng.integers(1, 17, size=200)
    parts = sharded.route_pids(pids, bounds)
    assert len(parts) == len(SIZES)
    for i, r in enumerate(g.shard_ranges):
        want = pids[(pids >= r.start) & (pids < r.stop)]          # list order and duplicates kept
        assert np.array_equal(parts[i], want), i
    # both sides of every boundary
    edge = np.array([5, 6, 7, 13, 14, 16, 1])
    assert [p.tolist() for p in sharded.route_pids(edge, bounds)] == [[5, 1], [6], [7, 13], [14, 16]]
    assert [p.size for p in sharded.route_pids([], bounds)] == [0, 0, 0, 0]


def test_group_range_bounds_error_comes_before_any_shard_call():
    g = stub_group()
    for bad in ([0], [17], [3, -1], [1, 2, 10 ** 12]):
        with pytest.raises(clb.BoundsError, match="shard group"):
            g.remove_passages(bad)
        with pytest.raises(clb.BoundsError, match="shard group"):
            g.make_filter(pids=bad)                # raised before the library is called: the stubs have no handle
    assert all(s.removed == [] for s in g.shards)
    assert g.remove_passages([5, 6, 6, 16, 14]) == 4              # the sum of what the shards report
    assert [np.concatenate(s.removed).tolist() if s.removed else [] for s in g.shards] == [[5], [6, 6], [], [16, 14]]
    with pytest.raises(clb.ColBERTError):
        g.make_filter()
    with pytest.raises(clb.ColBERTError):
        g.make_filter(pids=[1], mask=np.ones(16, bool))


def test_mask_slicing_against_numpy():
    g = stub_group()
    rng = np.random.default_rng(3)
    m = rng.random(16) < 0.5
    parts = sharded.slice_mask(m, g._bounds)
    assert [p.size for p in parts] == SIZES
    assert np.array_equal(np.concatenate(parts), m)
    for bad in (np.ones(15, bool), np.ones(17, bool), np.ones(16, np.uint8), np.ones((4, 4), bool)):
        with pytest.raises(clb.ColBERTError, match="mask"):
            sharded.slice_mask(bad, g._bounds)


def test_filters_of_another_group_and_bad_protocols_are_refused():
    g, other = stub_group(), stub_group()
    f = sharded.ShardedFilter(other, [], 0)
    with pytest.raises(clb.ColBERTError, match="this shard group"):
        g._shard_filters([f, None], 2)
    with pytest.raises(clb.ColBERTError, match="B=3"):
        g._shard_filters([None, None], 3)
    assert g._shard_filters([None, None], 2) is None and g._shard_filters(None, 2) is None
    with pytest.raises(clb.ColBERTError, match="protocol"):
        g.search_batch(np.zeros((128, 32, 1), np.float32), 5, 2, protocol="three_phase")
    with pytest.raises(clb.ColBERTError, match="dim=128"):
        g.search_batch(np.zeros((64, 32, 1), np.float32), 5, 2)
