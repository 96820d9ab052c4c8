"""ShardedSearcher.update_compressed / update_embeddings on the GPU: one update over 2 and 4 passage shards (all on device 0)
with GLOBAL pids, routed to the shards that own them, against the CPU oracle on the unsharded updated index
(tests/test_update_cpu.updated_index), under both exchange protocols."""
import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests.test_gpu_sharded_searcher import PROTOCOLS, assert_same_results, boundary_pids, check_group
from tests.test_update_cpu import content_of, updated_index
from tests.util_filter import filtered_ranking

pytestmark = pytest.mark.gpu

NPROBE = 2
WORLDS = (2, 4)


@pytest.fixture(scope="module")
def corpus(oracle):
    idx = synthetic.make_index(0, 300, K=64)
    Qs = synthetic.make_queries(idx, 1000, 9)
    Qs.setflags(write=False)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(Qs.shape[2])]


def the_update(idx, g, full):
    """pids in every shard and on both sides of every cut, the best passages of every query among them; in list order every
    third passage is emptied, every third gets two donors' rows (it grows), the rest one donor's"""
    top = np.unique(np.concatenate([r[0][:2] for r in full]))
    pids = np.unique(np.concatenate([top, boundary_pids(g), [r.start + 7 for r in g.shard_ranges], [1, 300]]))
    pids = np.random.default_rng(5).permutation(pids)              # any order
    for r in g.shard_ranges:
        assert np.any((pids >= r.start) & (pids < r.stop))
    co, re, dl = [], [], []
    for i, p in enumerate(pids):
        donors = [[], [(p + 50) % 300 + 1, (p + 90) % 300 + 1], [(p + 120) % 300 + 1]][i % 3]
        c, r, d = content_of(idx, donors)
        co.append(c); re.append(r); dl.append(d.sum())
    return pids, np.concatenate(co), np.asfortranarray(np.concatenate(re, axis=1)), np.array(dl, np.int64)


@pytest.mark.parametrize("world", WORLDS)
def test_update_across_the_shards(oracle, corpus, world):
    idx, Qs, full = corpus
    nq = Qs.shape[2]
    with clb.ShardedSearcher.from_index(idx, world) as g:
        args = the_update(idx, g, full)
        pids, dl = args[0], args[3]
        want = updated_index(idx, *args)
        assert np.any(want["doclens"][pids - 1] > idx["doclens"][pids - 1]) and np.any(dl == 0)
        allowed = np.union1d(np.arange(1, 301, 2), boundary_pids(g))
        keep = g.make_filter(pids=allowed)
        before = g.search_batch(Qs, 10, NPROBE, pad_short=True)
        gens = [s.generation for s in g.shards]
        # a pid beyond the group, a pid named twice: refused before any shard has changed
        beyond = (np.append(pids, 301), args[1], args[2], np.append(dl, 0))
        with pytest.raises(clb.BoundsError, match="shard group"):
            g.update_compressed(*beyond)
        with pytest.raises(clb.ArgumentError, match="twice"):
            g.update_compressed(np.append(pids, pids[0]), args[1], args[2], np.append(dl, 0))
        assert [s.generation for s in g.shards] == gens
        assert_same_results(before, g.search_batch(Qs, 10, NPROBE, pad_short=True), "after a refused update")
        assert g.update_compressed(*args) == pids.size
        assert [s.generation for s in g.shards] == [x + 1 for x in gens] and g.num_docs == 300
        assert sum(s.num_embeddings for s in g.shards) == want["codes"].size
        for s, r in zip(g.shards, g.shard_ranges):                 # every passage stayed on its shard
            assert s.num_embeddings == int(want["doclens"][r.start - 1:r.stop - 1].sum())
        consts = [s.bound_consts.tobytes() for s in g.shards]      # one bound over the group again
        assert len(set(consts)) == 1
        rankings = [filtered_ranking(oracle, want, Qs[:, :, j], NPROBE) for j in range(nq)]
        for k in (10, 100):
            check_group(g, Qs, rankings, k, f"after update world={world} k={k}")
        after = g.search_batch(Qs, 10, NPROBE, pad_short=True)
        assert not np.array_equal(before[1], after[1])             # the best passages were replaced: the answers changed
        for scope in ("candidates", "all"):                        # a filter made before stays valid
            fr = [filtered_ranking(oracle, want, Qs[:, :, j], NPROBE, allowed[want["doclens"][allowed - 1] > 0], scope)
                  for j in range(nq)]
            check_group(g, Qs, fr, 10, f"old filter after update world={world} scope={scope}", filters=keep, scope=scope)
        keep.close()
        # every named passage gets its old content back: the group answers as in the beginning
        assert g.update_compressed(pids, *content_of(idx, pids)) == pids.size
        check_group(g, Qs, full, 10, f"restored world={world}")


def test_update_embeddings_across_the_shards(oracle, corpus):
    idx, Qs, _ = corpus
    embs, dl = synthetic.make_embeddings(11, 8)
    co, re = oracle.compress(idx["centroids"], idx["bucket_cutoffs"], 128, 2, embs)
    pids = np.array([300, 1, 75, 76, 150, 151, 225, 226])
    want = updated_index(idx, pids, co, re, dl)
    rankings = [filtered_ranking(oracle, want, Qs[:, :, j], NPROBE) for j in range(Qs.shape[2])]
    with clb.ShardedSearcher.from_index(idx, 4) as g:
        assert g.update_embeddings(pids, embs, dl) == 8
        check_group(g, Qs, rankings, 10, "update_embeddings", protocols=PROTOCOLS)
        with pytest.raises(clb.ColBERTError, match="encoder"):
            g.update_passages([1], ["hello world"])
