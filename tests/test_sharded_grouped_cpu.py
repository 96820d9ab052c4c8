"""Grouped search across a shard group, without a GPU: the library declares and exports the new entry points and they refuse
null and bad arguments before any device work, and the host logic of `ShardedSearcher.make_grouping` -- the cut of the ids
at the shard boundaries, the `group_base` of every shard, `groups_of`, the refusals -- against numpy on stub shards."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import sharded
from tests.test_sharded_searcher_cpu import SIZES, StubShard
from tests.util_group import ids_from_lens

NEW_SYMBOLS = ("clb_search_shard_phase1_grouped_slot", "clb_search_shard_phase2_grouped_slot", "clb_search_result_groups_slot",
               "clb_merge_topk_grouped_device", "clb_merge_topk_grouped_packed_device", "clb_packed_grouped_bytes",
               "clb_debug_group_tau_device")


def test_new_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    assert hasattr(clb, "ShardedGrouping") and hasattr(clb.ShardedSearcher, "make_grouping")
    for k, B in ((1, 1), (10, 6), (7, 3), (1000, 32)):
        topk = l.clb_packed_topk_bytes(C.c_int64(k), C.c_int64(B))
        assert l.clb_packed_grouped_bytes(k, B) == topk + 8 * B * k + 8 * B + 16 * B
        from colbert_jl_amd.distributed import packed_grouped_bytes
        assert packed_grouped_bytes(k, B) == l.clb_packed_grouped_bytes(k, B) and packed_grouped_bytes(k, B) % 8 == 0


def test_new_entry_points_check_their_arguments_first():
    """Null handles, null operands and bad sizes are ArgumentError (4) before any device work."""
    l = clb.lib()
    null = C.c_void_p()
    x = C.c_void_p(0x1000)              # a non-null address that is never read: every call below is refused before it
    assert l.clb_search_shard_phase1_grouped_slot(null, 0, None, 32, 1, 2, 4, None, 0, x, 0, x, x, None) == 4
    assert b"null" in l.clb_last_error()
    assert l.clb_search_shard_phase2_grouped_slot(null, 0, None, 32, 1, 2, 4, x, x, 2, x, 0, x, x, x, x, x, None) == 4
    assert l.clb_search_shard_phase2_grouped_slot(null, 0, None, 32, 1, 2, 4, x, x, 2, null, 0, x, x, x, x, x, None) == 4
    assert b"grouping is null" in l.clb_last_error()
    assert l.clb_search_result_groups_slot(null, 0, x, 0, x, 1, 4, x, x, None) == 4
    # the device-level calls: every null operand, and sizes below 1
    assert l.clb_debug_group_tau_device(None, x, 2, 1, 4, x, None) == 4
    assert l.clb_debug_group_tau_device(x, None, 2, 1, 4, x, None) == 4
    assert l.clb_debug_group_tau_device(x, x, 2, 1, 4, None, None) == 4
    for S, B, k in ((0, 1, 4), (2, 0, 4), (2, 1, 0)):
        assert l.clb_debug_group_tau_device(x, x, S, B, k, x, None) == 4
    assert l.clb_debug_group_tau_device(x, x, 257, 1, 4, x, None) == clb.Unsupported.code and b"256" in l.clb_last_error()
    args = [0, x, x, x, 4, 2, 1, x, x, x, x, x, None]       # device, pids, scores, gids, k, n_lists, B, n_cand, edges, 3 outputs, stream
    for i in (1, 2, 3, 7, 8, 9, 10, 11):
        a = list(args); a[i] = None
        assert l.clb_merge_topk_grouped_device(*a) == 4, i
        assert b"null" in l.clb_last_error()
    for i in (4, 5, 6):
        a = list(args); a[i] = 0
        assert l.clb_merge_topk_grouped_device(*a) == 4, i
    a = list(args); a[5] = 257
    assert l.clb_merge_topk_grouped_device(*a) == clb.Unsupported.code
    assert l.clb_merge_topk_grouped_packed_device(0, None, 4, 2, 1, x, x, x, None) == 4
    assert l.clb_merge_topk_grouped_packed_device(0, x, 4, 2, 1, x, None, x, None) == 4
    assert l.clb_merge_topk_grouped_packed_device(0, x, 0, 2, 1, x, x, x, None) == 4


class GroupingShard(StubShard):
    """A stub shard that records the ids its make_grouping is given."""

    class Part:
        def __init__(self, ids):
            self.ids, self.closed = np.array(ids), False

        def close(self):
            self.closed = True

    def make_grouping(self, group_ids=None, group_lens=None):
        assert group_lens is None and group_ids.size == self.num_docs
        self.part = self.Part(group_ids)
        return self.part


def stub_group(first=0):
    off = first + np.concatenate([[0], np.cumsum(SIZES)])
    return clb.ShardedSearcher([GroupingShard(int(off[i]), SIZES[i]) for i in range(len(SIZES))])


@pytest.mark.parametrize("seed", range(6))
def test_ids_are_cut_at_the_bounds_and_group_base_is_the_unique_index(seed):
    rng = np.random.default_rng(seed)
    g = stub_group(first=0 if seed % 2 == 0 else 40)
    n = g.num_docs
    ids = np.sort(rng.integers(-5, 6, size=n)) * 3            # sparse caller ids, negative ones too; runs straddle the cuts
    gr = g.make_grouping(group_ids=ids)
    uniq, inverse = np.unique(ids, return_inverse=True)
    assert len(gr) == gr.count == uniq.size
    cuts = np.concatenate([[0], np.cumsum(SIZES)])
    assert gr.bases == [int(inverse[c]) for c in cuts[:-1]]
    for i, s in enumerate(g.shards):
        assert np.array_equal(s.part.ids, ids[cuts[i]:cuts[i + 1]]) and s.part.ids.dtype == np.int64
        # the global index of every local passage: the shard's base plus its dense local index
        local = np.unique(s.part.ids, return_inverse=True)[1]
        assert np.array_equal(gr.bases[i] + local, inverse[cuts[i]:cuts[i + 1]])
    first = int(g._bounds[0])
    pids = rng.integers(1, n + 1, size=30) + first
    assert np.array_equal(gr.groups_of(pids), ids[pids - first - 1])
    for bad in ([first], [first + n + 1], [0]):
        with pytest.raises(clb.BoundsError):
            gr.groups_of(bad)
    gr.close()
    assert all(s.part.closed for s in g.shards)


def test_group_lens_and_straddling_bases():
    g = stub_group()                                           # shards of 5, 1, 7, 3 passages: cuts after 5, 6, 13
    gr = g.make_grouping(group_lens=[4, 4, 6, 2])              # groups 0..3: group 1 covers shard 1 and straddles two cuts
    assert gr.bases == [0, 1, 1, 2] and gr.count == 4
    assert np.array_equal(gr.groups_of(np.arange(1, 17)), ids_from_lens([4, 4, 6, 2]))
    one = g.make_grouping(group_lens=[16])
    assert one.bases == [0, 0, 0, 0] and len(one) == 1
    single = g.make_grouping(group_ids=np.arange(16))
    assert single.bases == [0, 5, 6, 13] and len(single) == 16
    assert sharded.slice_groups(np.arange(16), g._bounds)[1] == [0, 5, 6, 13]


def test_refusals_come_before_any_shard_is_called():
    g, other = stub_group(), stub_group()
    with pytest.raises(clb.ColBERTError, match="exactly one"):
        g.make_grouping()
    with pytest.raises(clb.ColBERTError, match="exactly one"):
        g.make_grouping(group_ids=np.zeros(16, np.int64), group_lens=[16])
    with pytest.raises(clb.ArgumentError, match="non-decreasing.*position 7"):
        g.make_grouping(group_ids=np.array([0] * 7 + [-1] + [2] * 8))
    for bad in (np.zeros(15, np.int64), np.zeros(17, np.int64), np.zeros(16, np.float32), np.zeros((4, 4), np.int64)):
        with pytest.raises(clb.ColBERTError, match="one per passage"):
            g.make_grouping(group_ids=bad)
    with pytest.raises(clb.ColBERTError, match="summing to num_docs"):
        g.make_grouping(group_lens=[8, 7])
    assert not any(hasattr(s, "part") for s in g.shards)
    # a grouping of another shard group, and anything that is no ShardedGrouping
    theirs = other.make_grouping(group_lens=[16])
    Q = np.zeros((128, 32, 1), np.float32)
    for bad in (theirs, "docs", theirs.parts[0]):
        with pytest.raises(clb.ColBERTError, match="ShardedGrouping of this shard group"):
            g.search_batch(Q, 5, 2, grouping=bad)
    # one made before an append
    mine = g.make_grouping(group_lens=[16])
    g._bounds[-1] += 2
    with pytest.raises(clb.ArgumentError, match="made before an append"):
        g.search_batch(Q, 5, 2, grouping=mine)
