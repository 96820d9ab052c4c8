"""ShardedSearcher over a real process group: two rank processes share the one GPU, each passes its own shard to
`ShardedSearcher(..., group=...)`, the exchanges go over gloo (staged through host memory: RCCL refuses two ranks on one
device) -- the pattern of tests/test_gpu_dist_search.py.  One unfiltered and one boundary-straddling filtered search under
both protocols; every rank's result against the oracle on the unsharded index, pids and score bits."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

K, NPROBE = 100, 2


def straddling(cut):
    """pids on both sides of the boundary after passage `cut`, and a stride of the rest so that candidates survive the filter"""
    return np.concatenate([[cut - 1, cut, cut + 1, cut + 2], np.arange(3, 6001, 3)]).astype(np.int64)


def _worker(rank, world, store, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    import colbert_jl_amd as clb
    from colbert_jl_amd.sharding import shard_index
    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    idx = clb.synthetic.make_index(seed=141, n_docs=6000, K=512)
    Qs = clb.synthetic.make_queries(idx, 142, 6)
    sub, off = shard_index(idx, rank, world)
    g = clb.ShardedSearcher([clb.Searcher(index=sub, device=0, pid_offset=off)], group=dist.group.WORLD)
    out = {"ranges": [(r.start, r.stop) for r in g.shard_ranges], "num_docs": g.num_docs}
    cut = g.shard_ranges[0].stop - 1
    with g.make_filter(pids=straddling(cut)) as f:
        out["count"] = f.count
        for proto in ("two_phase", "single"):
            out[proto] = g.search_batch(Qs, K, NPROBE, pad_short=True, protocol=proto)
            for scope in ("candidates", "all"):
                out[proto, scope] = g.search_batch(Qs, K, NPROBE, filters=f, scope=scope, protocol=proto)
    q.put((rank, out))
    dist.barrier()
    g.close()
    dist.destroy_process_group()


def test_two_rank_processes_one_sharded_handle_each(oracle):
    import torch.multiprocessing as mp

    import colbert_jl_amd as clb
    from tests.test_gpu_filtered_search import assert_result
    from tests.util_filter import filtered_ranking
    world = 2
    store = tempfile.NamedTemporaryFile(prefix="clb_pg_", delete=False); store.close(); os.unlink(store.name)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, store.name, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    idx = clb.synthetic.make_index(seed=141, n_docs=6000, K=512)
    Qs = clb.synthetic.make_queries(idx, 142, 6)
    from colbert_jl_amd.sharding import shard_bounds
    cut = int(shard_bounds(idx["doclens"], world)[1])
    allowed = straddling(cut)
    nq = Qs.shape[2]
    ref = {None: [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(nq)]}
    for scope in ("candidates", "all"):
        ref[scope] = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, allowed, scope) for j in range(nq)]
    rp, rs, rn = oracle.search(idx, Qs[:, :, 0], NPROBE, K)
    assert rn == ref[None][0][0].size and np.array_equal(rp, ref[None][0][0][:K])
    for r in range(world):                                          # identical on every rank
        out = res[r]
        assert out["ranges"] == [(1, cut + 1), (cut + 1, 6001)] and out["num_docs"] == 6000
        assert out["count"] == np.unique(allowed).size              # the population over the whole group
        for proto in ("two_phase", "single"):
            for key, rankings in ((proto, ref[None]), ((proto, "candidates"), ref["candidates"]), ((proto, "all"), ref["all"])):
                p, s, n = out[key]
                for j in range(nq):
                    assert_result(p[:, j], s[:, j], n[j], rankings[j], K, f"rank={r} {key} q={j}")
