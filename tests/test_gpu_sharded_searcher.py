"""ShardedSearcher on the GPU: one handle over 2 and 4 passage shards (all on device 0), both exchange protocols, against the
CPU oracle on the UNSHARDED index -- tests/util_filter.filtered_reference with filters, oracle.search without.  Bar: pids and
candidate counts identical, fp32 scores bit-identical, short results padded with pid 0 / -Inf.  Corpus of
tests/test_gpu_dist_search.py: make_index(seed=141, n_docs=6000, K=512), 6 queries, T = 32, nprobe = 2."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd._lib import check
from colbert_jl_amd.sharding import shard_index
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import assert_result, assert_same_f32
from tests.test_remove_cpu import reduced_index
from tests.util_filter import filtered_ranking

pytestmark = pytest.mark.gpu

NPROBE = 2
PROTOCOLS = ("two_phase", "single")
WORLDS = (2, 4)


@pytest.fixture(scope="module")
def corpus(oracle):
    idx = synthetic.make_index(seed=141, n_docs=6000, K=512)
    Qs = synthetic.make_queries(idx, 142, 6)
    Qs.setflags(write=False)
    full = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(Qs.shape[2])]      # unfiltered, every candidate
    return idx, Qs, full


@pytest.fixture(scope="module")
def groups(corpus):
    """one resident group per world, shared by the tests that do not change it"""
    g = {w: clb.ShardedSearcher.from_index(corpus[0], w) for w in WORLDS}
    yield g
    for x in g.values():
        x.close()


def check_group(g, Qs, rankings, k, what, filters=None, scope="candidates", protocols=PROTOCOLS, nprobe=NPROBE):
    """search_batch under every protocol against one ranking per query"""
    for proto in protocols:
        p, s, n = g.search_batch(Qs, k, nprobe, pad_short=True, filters=filters, scope=scope, protocol=proto)
        assert p.shape == s.shape == (k, Qs.shape[2]) and p.dtype == np.int64 and s.dtype == np.float32
        for j in range(Qs.shape[2]):
            assert_result(p[:, j], s[:, j], n[j], rankings[j], k, f"{what} protocol={proto} q={j}")


def assert_same_results(a, b, what):
    """two (pids, scores, n_cand) results, bit for bit"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), what
    assert_same_f32(a[1], b[1], what)


def boundary_pids(g):
    """for each cut c of shard_ranges (the last pid of a shard): c - 1, c, c + 1, c + 2"""
    cuts = [r.stop - 1 for r in g.shard_ranges[:-1]]
    return np.array([c + d for c in cuts for d in (-1, 0, 1, 2)], np.int64)


# ---- 1. unfiltered ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_unfiltered_both_protocols(oracle, corpus, groups, world):
    idx, Qs, full = corpus
    g = groups[world]
    assert g.num_docs == 6000 and len(g.shard_ranges) == world
    assert g.shard_ranges[0].start == 1 and g.shard_ranges[-1].stop == 6001
    for k in (100, 700):
        for j in range(2):                   # the composed ranking is the oracle's own search
            rp, rs, rn = oracle.search(idx, Qs[:, :, j], NPROBE, k)
            assert rn == full[j][0].size and np.array_equal(rp, full[j][0][:k])
            assert_same_f32(rs, full[j][1][:k], "composed ranking against oracle.search")
        check_group(g, Qs, full, k, f"unfiltered world={world} k={k}")
    # protocol "auto" on two-pass shards is the two-phase exchange, and the single-query entry point agrees
    p, s = g.search_embeddings(Qs[:, :, 3], 100, NPROBE)
    assert_result(p, s, g.last_num_candidates, full[3], 100, "search_embeddings")
    # the pad_short contract of Searcher.search_batch: fewer than k candidates in the whole group.  (With these queries
    # nearly every passage is a candidate, about 6000 / world per shard: every shard's block then travels padded.)
    few = min(r[0].size for r in full)
    with pytest.raises(clb.BoundsError, match="fewer than k"):
        g.search_batch(Qs, few + 1, NPROBE)
    check_group(g, Qs, full, few + 1, "short unfiltered")


# ---- 2. filters -------------------------------------------------------------------------------------------------------
def filter_sets(g):
    rng = np.random.default_rng(5)
    r1 = g.shard_ranges[1]
    return {
        "inside_one_shard": rng.choice(np.arange(r1.start, r1.stop), 300, replace=False),
        "straddling": boundary_pids(g),
        "below_k": rng.choice(np.arange(1, 6001), 40, replace=False),
        "half": rng.permutation(np.nonzero(rng.random(6000) < 0.5)[0] + 1),
        "empty": np.zeros(0, np.int64),
    }


@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("world", WORLDS)
def test_filtered_both_scopes_and_protocols(oracle, corpus, groups, world, scope):
    idx, Qs, full = corpus
    g = groups[world]
    k, nq = 100, Qs.shape[2]
    sets = filter_sets(g)
    live = idx["doclens"] > 0
    for name, allowed in sets.items():
        rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, allowed, scope) for j in range(nq)]
        with g.make_filter(pids=allowed) as f:
            assert f.count == np.unique(allowed).size == len(f)
            assert sum(x.n_inside for x in f.parts) == allowed.size
            check_group(g, Qs, rankings, k, f"{name} world={world} scope={scope}", filters=f, scope=scope)
            if scope == "all":
                _, _, n = g.search_batch(Qs, k, NPROBE, filters=f, scope="all")
                assert np.all(n == np.count_nonzero(live[np.unique(allowed) - 1])), name
                if name == "below_k":
                    assert n[0] < k
                if name == "inside_one_shard":      # the other shards have no candidate at all
                    assert [x.count for x in f.parts] == [300 if i == 1 else 0 for i in range(world)]
    # the same sets as masks over the group's passages
    m = np.zeros(6000, bool); m[sets["straddling"] - 1] = True
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, sets["straddling"], scope) for j in range(nq)]
    with g.make_filter(mask=m) as f:
        assert f.count == sets["straddling"].size
        check_group(g, Qs, rankings, k, f"mask world={world} scope={scope}", filters=f, scope=scope)
    # per-query filters with None entries mixed in
    order = ["half", None, "straddling", "inside_one_shard", None, "empty"]
    made = {name: g.make_filter(pids=sets[name]) for name in set(order) - {None}}
    try:
        rankings = [full[j] if o is None else filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, sets[o], scope)
                    for j, o in enumerate(order)]
        check_group(g, Qs, rankings, k, f"per-query world={world} scope={scope}",
                    filters=[None if o is None else made[o] for o in order], scope=scope)
    finally:
        for f in made.values():
            f.close()


def test_half_corpus_filter_grows_the_candidate_buffers_on_the_phase1_path(oracle, corpus):
    """Scope "all" with half the corpus.  With the 32-token queries nearly every passage is a candidate and a slot holds its
    whole shard from the start; with 2-token queries and nprobe = 1 the two longest lists of a shard hold far fewer passages
    than the filter, and the slot -- sized by an unfiltered search first -- has to grow inside the filtered phase 1
    (tests/test_gpu_filtered_search.py::test_scope_all_beyond_the_ivf_capacity on the sharded path)."""
    idx, Qs, _ = corpus
    Q2 = synthetic.make_queries(idx, 143, 6, T=2)
    allowed = np.arange(1, 6001, 2)
    for r in range(2):
        assert int(np.sort(shard_index(idx, r, 2)[0]["ivf_lengths"])[-2:].sum()) < 1400         # a shard holds ~1500 of the set
    with clb.ShardedSearcher.from_index(idx, 2) as g, g.make_filter(pids=allowed) as f:
        assert f.count == 3000
        plain = [filtered_ranking(oracle, idx, Q2[:, :, j], 1) for j in range(6)]
        for queries, nprobe, unfiltered in ((Q2, 1, plain), (Qs, NPROBE, None)):
            rankings = [filtered_ranking(oracle, idx, queries[:, :, j], nprobe, allowed, "all") for j in range(6)]
            assert all(r[0].size == 3000 for r in rankings)
            for proto in PROTOCOLS:
                if unfiltered is not None:
                    check_group(g, queries, unfiltered, 50, "T=2 unfiltered", protocols=(proto,), nprobe=nprobe)
                for k in (100, 3000):
                    p, s, n = g.search_batch(queries, k, nprobe, filters=f, scope="all", protocol=proto)
                    for j in range(6):
                        assert_result(p[:, j], s[:, j], n[j], rankings[j], k, f"half T={queries.shape[1]} k={k} {proto} q={j}")


def test_filters_of_another_group_are_refused(corpus, groups):
    _, Qs, _ = corpus
    with groups[4].make_filter(pids=[1, 2, 3]) as f:
        with pytest.raises(clb.ColBERTError, match="this shard group"):
            groups[2].search_batch(Qs, 10, NPROBE, filters=f)
    with pytest.raises(clb.BoundsError, match="shard group"):
        groups[2].make_filter(pids=[1, 6001])
    with pytest.raises(clb.BoundsError, match="shard group"):
        groups[2].make_filter(pids=[0])


# ---- 3. clb_filter_create_pids_global directly ------------------------------------------------------------------------
def make_global(shard, pids):
    p = np.ascontiguousarray(pids, dtype=np.int64)
    h, n_in = C.c_void_p(), C.c_int64(-1)
    check(clb.lib().clb_filter_create_pids_global(shard._h, p.ctypes.data_as(C.c_void_p), p.size, C.byref(h), C.byref(n_in)))
    return clb.PassageFilter(shard, h, clb.lib().clb_filter_count(h)), int(n_in.value)


def test_global_pid_list_per_shard_against_numpy(corpus, groups):
    _, Qs, _ = corpus
    g = groups[4]
    rng = np.random.default_rng(11)
    pids = np.concatenate([rng.integers(1, 6001, size=5000), boundary_pids(g), boundary_pids(g), [1, 6000, 6000]])
    # past the group: the shard does not know its group, only a pid < 1 is an error to it
    pids = np.concatenate([pids, [6001, 10 ** 12]])
    for shard, r in zip(g.shards, g.shard_ranges):
        inside = pids[(pids >= r.start) & (pids < r.stop)]
        f, n_in = make_global(shard, pids)
        try:
            assert n_in == inside.size and f.count == np.unique(inside).size, (r, n_in, f.count)
            with shard.make_filter(pids=inside) as f2:
                assert f2.count == f.count
                a = shard.search_batch(Qs, 50, NPROBE, filters=f, scope="all")          # the bitmap itself is the candidate set
                b = shard.search_batch(Qs, 50, NPROBE, filters=f2, scope="all")
                assert_same_results(a, b, f"global list against the local part, shard {r}")
                assert np.all(a[2] == f.count)
        finally:
            f.close()
    shard = g.shards[1]
    for n, lst in ((0, []), (3, [1, 2, 6000])):              # n = 0; wholly outside this shard: valid empty filters
        f, n_in = make_global(shard, lst)
        assert (f.count, n_in) == (0, 0)
        _, _, nc = shard.search_batch(Qs, 5, NPROBE, filters=f, scope="all")
        assert np.all(nc == 0)
        f.close()
    for bad in ([0], [g.shard_ranges[1].start, -5], [np.iinfo(np.int64).min]):
        with pytest.raises(clb.BoundsError, match="pid < 1"):
            make_global(shard, bad)


def test_new_exports_argument_contracts_on_a_live_handle(corpus, groups):
    import torch
    _, Qs, _ = corpus
    l = clb.lib()
    g = groups[2]
    s0, s1 = g.shards
    dev = torch.device("cuda", s0.device)
    B, T, k = Qs.shape[2], Qs.shape[1], 10
    Qd = torch.from_numpy(np.array(Qs.transpose(2, 1, 0), order="C")).to(dev)
    top = torch.empty((B, k), dtype=torch.float32, device=dev)
    pids = np.array([1, 2], np.int64)
    out, n = C.c_void_p(), C.c_int64(0)

    def phase1(s, filters, scope, d_top=top.data_ptr()):
        return l.clb_search_shard_phase1_filtered_slot(s._h, 0, Qd.data_ptr(), T, B, NPROBE, k, filters, scope, d_top, None)

    assert phase1(s0, None, 0, None) == clb.ArgumentError.code and b"d_local_top" in l.clb_last_error()
    assert l.clb_filter_create_pids_global(s0._h, pids.ctypes.data_as(C.c_void_p), 2, None, C.byref(n)) == clb.ArgumentError.code
    assert l.clb_filter_create_pids_global(s0._h, pids.ctypes.data_as(C.c_void_p), 2, C.byref(out), None) == clb.ArgumentError.code
    assert l.clb_filter_create_pids_global(s0._h, None, 2, C.byref(out), C.byref(n)) == clb.ArgumentError.code
    with s0.make_filter(pids=[1]) as f0:
        mine = s0._filter_handles([f0] * B, B)
        assert phase1(s0, mine, 2) == clb.ArgumentError.code and b"scope" in l.clb_last_error()
        assert phase1(s1, mine, 0) == clb.ArgumentError.code and b"another searcher" in l.clb_last_error()
        assert phase1(s0, mine, 0) == 0
    torch.cuda.synchronize()


# ---- 4. B one above the filter handles of a launch --------------------------------------------------------------------
def test_batch_one_above_the_filter_limit(oracle, corpus, groups):
    import torch
    idx, Qs, full = corpus
    g = groups[2]
    B, k, nq = 65, 20, Qs.shape[2]
    Qb = np.asfortranarray(np.concatenate([Qs] * 11, axis=2)[:, :, :B])
    sets = filter_sets(g)
    order = ["half", None, "straddling"]
    made = {name: g.make_filter(pids=sets[name]) for name in ("half", "straddling")}
    try:
        for scope in ("candidates", "all"):
            rank = {(j, o): (full[j] if o is None else filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, sets[o], scope))
                    for j in range(nq) for o in order}
            fb = [None if order[b % 3] is None else made[order[b % 3]] for b in range(B)]
            for proto in PROTOCOLS:
                p, s, n = g.search_batch(Qb, k, NPROBE, filters=fb, scope=scope, protocol=proto)
                for b in range(B):
                    assert_result(p[:, b], s[:, b], n[b], rank[(b % nq, order[b % 3])], k, f"B=65 {scope} {proto} q={b}")
        # the raw export: a filtered phase 1 takes at most 64 queries per call and says so; unfiltered it takes them all
        s0 = g.shards[0]
        dev = torch.device("cuda", s0.device)
        Qd = torch.from_numpy(np.ascontiguousarray(Qb.transpose(2, 1, 0))).to(dev)
        top = torch.empty((B, k), dtype=torch.float32, device=dev)
        l = clb.lib()
        handles = s0._filter_handles([made["half"].parts[0]] + [None] * (B - 1), B)
        args = (s0._h, 0, Qd.data_ptr(), Qs.shape[1], B, NPROBE, k)
        assert l.clb_search_shard_phase1_filtered_slot(*args, handles, 0, top.data_ptr(), None) == clb.Unsupported.code
        assert b"at most 64 queries" in l.clb_last_error()
        assert l.clb_search_shard_phase1_filtered_slot(*args, s0._filter_handles([None] * B, B), 0, top.data_ptr(), None) == 0
        assert l.clb_search_shard_phase1_filtered_slot(*args, None, 0, top.data_ptr(), None) == 0
        torch.cuda.synchronize()
    finally:
        for f in made.values():
            f.close()


# ---- 5. append --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_append_to_the_last_shard(oracle, corpus, world):
    idx, Qs, full = corpus
    P = 5950
    with clb.ShardedSearcher.from_index(head_index(idx, P), world) as g:
        old = g.make_filter(pids=[1, 2, P])
        g.search_batch(Qs, 100, NPROBE, pad_short=True, protocol="two_phase")       # the group has searched before it grows
        assert g.add_compressed(*tail(idx, P)) == range(P + 1, 6001)
        assert g.num_docs == 6000 and g.shard_ranges[-1].stop == 6001 and g.shards[-1].num_docs == 6000 - g.shards[-1].pid_offset
        consts = [s.bound_consts for s in g.shards]
        assert all(np.array_equal(c, consts[0]) for c in consts)                    # shared again
        for k in (100, 700):
            check_group(g, Qs, full, k, f"after append world={world} k={k}")
        for proto in PROTOCOLS:
            with pytest.raises(clb.ArgumentError, match="made before an append"):
                g.search_batch(Qs, 10, NPROBE, filters=old, protocol=proto)
        old.close()
        allowed = np.concatenate([np.arange(1, 6001, 3), np.arange(P - 5, 6001)])     # old and new passages
        with g.make_filter(pids=allowed) as f:
            assert f.count == np.unique(allowed).size
            for scope in ("candidates", "all"):
                rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, allowed, scope) for j in range(Qs.shape[2])]
                assert any(np.any(r[0][:100] > P) for r in rankings)
                check_group(g, Qs, rankings, 100, f"new filter world={world} scope={scope}", filters=f, scope=scope)
        with pytest.raises(clb.BoundsError):
            g.make_filter(pids=[6001])


# ---- 6. remove --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_remove_across_the_shards(oracle, corpus, world):
    idx, Qs, full = corpus
    nq = Qs.shape[2]
    with clb.ShardedSearcher.from_index(idx, world) as g:
        top = np.unique(np.concatenate([r[0][:3] for r in full]))                      # the answers must change
        removed = np.unique(np.concatenate([top, boundary_pids(g), [r.start + 7 for r in g.shard_ranges], [1, 6000]]))
        for r in g.shard_ranges:
            assert np.any((removed >= r.start) & (removed < r.stop))
        allowed = np.concatenate([np.arange(1, 6001, 2), boundary_pids(g)])
        keep = g.make_filter(pids=allowed)
        before = g.search_batch(Qs, 100, NPROBE, pad_short=True)
        with pytest.raises(clb.BoundsError, match="shard group"):
            g.remove_passages(np.concatenate([removed[:5], [6001]]))
        with pytest.raises(clb.BoundsError, match="shard group"):
            g.remove_passages([0])
        after = g.search_batch(Qs, 100, NPROBE, pad_short=True)                         # every shard unchanged
        assert_same_results(before, after, "after a refused removal")
        named = np.concatenate([removed[::-1], removed[:10]])                           # any order, duplicates
        assert g.remove_passages(named) == removed.size
        assert g.remove_passages(removed[:4]) == 0                                      # empty already
        assert g.num_docs == 6000
        red, _ = reduced_index(idx, removed)
        rankings = [filtered_ranking(oracle, red, Qs[:, :, j], NPROBE) for j in range(nq)]
        for k in (100, 700):
            check_group(g, Qs, rankings, k, f"after remove world={world} k={k}")
        p, _, _ = g.search_batch(Qs, 100, NPROBE, pad_short=True)
        assert not np.isin(p, removed).any()
        for scope in ("candidates", "all"):                                             # a filter made before stays valid
            fr = [filtered_ranking(oracle, red, Qs[:, :, j], NPROBE, allowed[red["doclens"][allowed - 1] > 0], scope)
                  for j in range(nq)]
            check_group(g, Qs, fr, 100, f"old filter after remove world={world} scope={scope}", filters=keep, scope=scope)
        keep.close()


# ---- 7. general-shape group -------------------------------------------------------------------------------------------
def test_general_shape_group_takes_the_single_exchange(oracle):
    idx = synthetic.make_index(seed=79, n_docs=900, K=96, dim=64, nbits=8, doclen_mean=20, doclen_std=12)
    Qs = synthetic.make_queries(idx, 80, 3, T=20)
    k = 50
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(3)]
    rp, rs, rn = oracle.search(idx, Qs[:, :, 0], NPROBE, k)
    assert rn == rankings[0][0].size and np.array_equal(rp, rankings[0][0][:k])
    with clb.ShardedSearcher.from_index(idx, 3) as g:
        assert all(s.mode == 0 for s in g.shards)
        check_group(g, Qs, rankings, k, "general auto", protocols=("auto", "single"))
        allowed = np.concatenate([boundary_pids(g), np.arange(1, 901, 4)])
        with g.make_filter(pids=allowed) as f:
            fr = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE, allowed, "candidates") for j in range(3)]
            check_group(g, Qs, fr, k, "general filtered", filters=f, protocols=("auto",))
            with pytest.raises(clb.Unsupported, match="two-pass mode"):
                g.search_batch(Qs, k, NPROBE, filters=f, protocol="two_phase")
        with pytest.raises(clb.Unsupported, match="two-pass mode"):
            g.search_batch(Qs, k, NPROBE, protocol="two_phase")


# ---- 8. constructor refusals ------------------------------------------------------------------------------------------
def test_constructor_refusals(corpus):
    idx, _, _ = corpus
    small = synthetic.make_index(seed=2, n_docs=400, K=64)
    other_k = synthetic.make_index(seed=2, n_docs=400, K=32)
    (a, off_a), (b, off_b) = shard_index(small, 0, 2), shard_index(small, 1, 2)
    assert off_a == 0 and off_b == a["doclens"].size
    made = []

    def searcher(index, off):
        made.append(clb.Searcher(index=index, pid_offset=off))
        return made[-1]

    try:
        with pytest.raises(clb.ColBERTError, match="tile"):
            clb.ShardedSearcher([searcher(a, 0), searcher(b, off_b + 1)])                # a gap of one passage
        with pytest.raises(clb.ColBERTError, match="tile"):
            clb.ShardedSearcher([searcher(b, off_b), searcher(a, 0)])                    # not in pid order
        with pytest.raises(clb.ColBERTError, match="agree on K"):
            clb.ShardedSearcher([searcher(a, 0), searcher(shard_index(other_k, 1, 2)[0], off_b)])
        g = clb.ShardedSearcher([searcher(a, 0), searcher(b, off_b)])
        assert g.num_docs == 400 and g.shard_ranges == [range(1, off_b + 1), range(off_b + 1, 401)]
    finally:
        for s in made:
            s.close()
