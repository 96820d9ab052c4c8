"""Grouped search across a shard group on the GPU: `ShardedSearcher.search_batch(grouping=)` over 2 and 4 shards (all on
device 0) under both exchange protocols against the grouped reference on the UNSHARDED index (tests/util_group: the oracle's
full ranking with the first occurrence of every group kept).  Bar: pids and candidate-group counts identical, fp32 scores
bit-identical, short results padded with pid 0 / -Inf.  Corpus of tests/test_gpu_sharded_searcher.py.  The two kernels
that make groups that straddle a cut count once -- the de-duplicated threshold and the grouped merge -- are also driven
alone, on crafted input, against numpy."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_filtered_search import assert_result, assert_same_f32
from tests.test_gpu_sharded_searcher import assert_same_results, boundary_pids
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import content_of, updated_index
from tests.util_filter import filtered_ranking
from tests.util_group import collapse, grouped_ranking, ids_from_lens, random_lens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NPROBE = 2
PROTOCOLS = ("two_phase", "single")
WORLDS = (2, 4)
KS = (10, 100, 700)
N = 6000


@pytest.fixture(scope="module")
def corpus(oracle):
    idx = synthetic.make_index(seed=141, n_docs=N, K=512)
    Qs = synthetic.make_queries(idx, 142, 6)
    Qs.setflags(write=False)
    full = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(Qs.shape[2])]      # unfiltered, every candidate
    return idx, Qs, full


@pytest.fixture(scope="module")
def groups(corpus):
    g = {w: clb.ShardedSearcher.from_index(corpus[0], w) for w in WORLDS}
    yield g
    for x in g.values():
        x.close()


def cuts_of(g):
    """the last pid of every shard but the last: passages c and c + 1 lie on different shards"""
    return [r.stop - 1 for r in g.shard_ranges[:-1]]


def straddling_ids(cuts, seed=17):
    """grouping (a): random_lens(N, 1, 6), and where a cut falls between two groups the passage after it joins the group
    before it, so that EVERY cut lies inside a group"""
    ids = ids_from_lens(random_lens(N, 1, 6, seed))
    for c in cuts:
        ids[c] = ids[c - 1]               # ids[c - 1]: passage c; ids[c]: passage c + 1 (its own group starts later, or vanishes)
    assert np.all(np.diff(ids) >= 0) and all(ids[c - 1] == ids[c] for c in cuts)
    return ids


def big_group_ids():
    """grouping (b): one group over pids 1400..3100, every other passage a singleton"""
    ids = np.arange(N, dtype=np.int64)
    ids[1399:3100] = 1399
    return ids


def aligned_ids(cuts, seed=23):
    """grouping (c): groups of 1..6 passages that END exactly at every cut"""
    edges = [0] + sorted(cuts) + [N]
    lens = np.concatenate([random_lens(edges[i + 1] - edges[i], 1, 6, seed + i) for i in range(len(edges) - 1)])
    ids = ids_from_lens(lens)
    assert ids.size == N and all(ids[c - 1] != ids[c] for c in cuts)
    return ids


def check_grouped(g, gr, Qs, rankings, k, what, filters=None, scope="candidates", protocols=PROTOCOLS):
    for proto in protocols:
        p, s, n = g.search_batch(Qs, k, NPROBE, pad_short=True, filters=filters, scope=scope, protocol=proto, grouping=gr)
        assert p.shape == s.shape == (k, Qs.shape[2]) and p.dtype == np.int64 and s.dtype == np.float32
        for j in range(Qs.shape[2]):
            assert_result(p[:, j], s[:, j], n[j], rankings[j], k, f"{what} protocol={proto} q={j}")
            kk = min(k, int(n[j]))
            assert np.unique(gr.groups_of(p[:kk, j])).size == kk, f"{what} protocol={proto} q={j}: a group twice"


# ---- 1. parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_parity_with_the_unsharded_grouped_reference(corpus, groups, world):
    idx, Qs, full = corpus
    g = groups[world]
    cuts = cuts_of(g)
    both = sorted(set(cuts_of(groups[2]) + cuts_of(groups[4])))
    big = big_group_ids()
    if world == 4:        # (b) covers all of the second shard and part of its neighbours
        r0, r1, r2 = g.shard_ranges[:3]
        assert r0.start < 1400 < r0.stop and 1400 <= r1.start and r1.stop - 1 <= 3100 and r2.start <= 3100 < r2.stop - 1
    for c in cuts:
        if 1400 <= c < 3100:
            assert big[c - 1] == big[c]
    assert any(1400 <= c < 3100 for c in cuts)
    cases = {"a_straddling": straddling_ids(both), "b_one_big_group": big, "c_aligned": aligned_ids(both),
             "d_singletons": np.arange(N, dtype=np.int64) * 7}
    for name, ids in cases.items():
        rankings = [collapse(r, ids) for r in full]
        with g.make_grouping(group_ids=ids) as gr:
            assert len(gr) == np.unique(ids).size and len(gr.parts) == world
            assert gr.bases == [int(np.unique(ids, return_inverse=True)[1][r.start - 1]) for r in g.shard_ranges]
            for k in KS:
                check_grouped(g, gr, Qs, rankings, k, f"{name} world={world} k={k}")
            if name == "d_singletons":          # equal to the ungrouped sharded search, bit for bit
                for proto in PROTOCOLS:
                    a = g.search_batch(Qs, 100, NPROBE, pad_short=True, protocol=proto, grouping=gr)
                    b = g.search_batch(Qs, 100, NPROBE, pad_short=True, protocol=proto)
                    assert_same_results(a, b, f"singletons against ungrouped, {proto}")
            if name == "a_straddling":          # the single-query entry point, protocol "auto"
                p, s = g.search_embeddings(Qs[:, :, 3], 100, NPROBE, grouping=gr)
                assert_result(p, s, g.last_num_candidates, rankings[3], 100, "search_embeddings")
                few = min(r[0].size for r in rankings)
                with pytest.raises(clb.BoundsError, match="candidate groups, fewer than k"):
                    g.search_batch(Qs, few + 1, NPROBE, grouping=gr)
                check_grouped(g, gr, Qs, rankings, few + 1, "short grouped")
    # (e) one group for the whole corpus
    with g.make_grouping(group_lens=[N]) as gr:
        assert gr.bases == [0] * world and len(gr) == 1
        rankings = [collapse(r, np.zeros(N, np.int64)) for r in full]
        assert all(r[0].size == 1 for r in rankings)
        for k in (1, 10):
            check_grouped(g, gr, Qs, rankings, k, f"one group world={world} k={k}")
        for proto in PROTOCOLS:
            p, s, n = g.search_batch(Qs, 10, NPROBE, pad_short=True, protocol=proto, grouping=gr)
            assert np.all(n == 1) and np.all(p[1:] == 0) and np.all(p[0] == [r[0][0] for r in full])
            with pytest.raises(clb.BoundsError, match="1 candidate groups"):
                g.search_batch(Qs, 10, NPROBE, protocol=proto, grouping=gr)


# ---- 2. the de-duplication is exercised -------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_a_straddling_group_is_returned_once(corpus, groups, world):
    idx, Qs, full = corpus
    g = groups[world]
    ids = big_group_ids()
    # the same grouping with the big group cut at the shard boundaries: what a merge WITHOUT removal would rank
    split = ids.copy()
    for i, r in enumerate(g.shard_ranges):
        inside = np.arange(max(r.start, 1400), min(r.stop - 1, 3100) + 1)
        split[inside - 1] = 1399 + i
    assert np.all(np.diff(split) >= 0)
    pieces = np.unique(split[1399:3100])
    assert pieces.size >= 2
    second = []          # per query: the 0-based place of the group's SECOND piece in the ranking without removal
    for r in full:
        rp, _ = collapse(r, split)
        at = np.nonzero(np.isin(split[rp - 1], pieces))[0]
        second.append(int(at[1]) if at.size >= 2 else 10 ** 9)
    k = min(second) + 1
    assert k <= 100, second         # the oracle alone: for some query both sides of a cut rank inside the first k
    j = int(np.argmin(second))
    rankings = [collapse(r, ids) for r in full]
    with g.make_grouping(group_ids=ids) as gr:
        check_grouped(g, gr, Qs, rankings, k, f"big group world={world} k={k}")
        for proto in PROTOCOLS:
            p, _, n = g.search_batch(Qs, k, NPROBE, pad_short=True, protocol=proto, grouping=gr)
            assert np.count_nonzero(gr.groups_of(p[:, j]) == 1399) == 1
            # candidate groups: counted once although every shard it touches has candidates of it
            assert n[j] == np.unique(ids[full[j][0] - 1]).size


# ---- 3. filters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("world", WORLDS)
def test_filters_compose_in_both_scopes(oracle, corpus, groups, world, scope):
    idx, Qs, _ = corpus
    g = groups[world]
    ids = straddling_ids(sorted(set(cuts_of(groups[2]) + cuts_of(groups[4]))))
    rng = np.random.default_rng(5)
    allowed = np.union1d(np.nonzero(rng.random(N) < 0.5)[0] + 1, boundary_pids(g))
    rankings = [grouped_ranking(oracle, idx, Qs[:, :, j], NPROBE, ids, allowed, scope) for j in range(Qs.shape[2])]
    with g.make_grouping(group_ids=ids) as gr, g.make_filter(pids=allowed) as f:
        check_grouped(g, gr, Qs, rankings, 100, f"filtered world={world} scope={scope}", filters=f, scope=scope)
        # per-query filters with None entries mixed in
        mixed = [f, None, f, None, None, f]
        plain = [grouped_ranking(oracle, idx, Qs[:, :, j], NPROBE, ids) for j in (1, 3, 4)]
        want = [rankings[0], plain[0], rankings[2], plain[1], plain[2], rankings[5]]
        check_grouped(g, gr, Qs, want, 100, f"per-query world={world} scope={scope}", filters=mixed, scope=scope)


# ---- 4. the de-duplicated threshold alone -----------------------------------------------------------------------------
def numpy_group_tau(top, gid, k):
    """(S, B, k) records -> tau[B]: the k-th largest over distinct indices, each with its largest score"""
    S, B, _ = top.shape
    out = np.full(B, -np.inf, np.float32)
    for b in range(B):
        best = {}
        for s, g_ in zip(top[:, b].reshape(-1), gid[:, b].reshape(-1)):
            if g_ >= 0:
                best[int(g_)] = max(best.get(int(g_), -np.inf), s)
        v = np.sort(np.array([x for x in best.values() if np.isfinite(x)], np.float32))[::-1]
        if v.size >= k:
            out[b] = v[k - 1]
    return out


def device_group_tau(top, gid):
    import torch
    S, B, k = top.shape
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(np.ascontiguousarray(top, np.float32)).to(dev)
    gd = torch.from_numpy(np.ascontiguousarray(gid, np.int64)).to(dev)
    tau = torch.full((B,), 123.0, dtype=torch.float32, device=dev)
    clb._lib.check(clb.lib().clb_debug_group_tau_device(t.data_ptr(), gd.data_ptr(), S, B, k, tau.data_ptr(), None))
    torch.cuda.synchronize()
    return tau.cpu().numpy()


def pick_groups(rng, width, m):
    """m distinct offsets into a shard's range of `width` groups, more often than not with the range's first and last among
    them (the groups that can straddle a cut)"""
    chosen = set(rng.choice(width, m, replace=False).tolist())
    if m >= 1 and 0 not in chosen and rng.random() < 0.8:
        chosen.remove(max(chosen)); chosen.add(0)
    if m >= 2 and width - 1 not in chosen and rng.random() < 0.8:
        chosen.remove(max(chosen - {0})); chosen.add(width - 1)
    assert len(chosen) == m
    return np.array(sorted(chosen), np.int64)


def shard_like_lists(rng, S, k, fill, straddle):
    """One query's records as phase 1 makes them: list s holds up to k DISTINCT indices of a contiguous range, in any order;
    the range of list s + 1 begins at the last index of list s (a straddling group) with probability `straddle`, else one
    past it; a list may hold a single index (a group over three shards)."""
    top = np.full((S, k), -np.inf, np.float32); gid = np.full((S, k), -1, np.int64)
    base = int(rng.integers(0, 50))
    for s in range(S):
        width = int(rng.integers(1, 2 * k + 2))
        m = min(width, int(rng.integers(0, k + 1)) if fill < 1 else k)
        gid[s, :m] = base + rng.permutation(pick_groups(rng, width, m))
        top[s, :m] = rng.integers(-8, 9, m).astype(np.float32) / 4          # few distinct values: ties
        base += width - 1 if rng.random() < straddle else width
    return top, gid


def test_group_tau_on_crafted_records():
    cases = []
    # a group in 2 lists and one in 3, the larger score in the later list; k-th value decided by them
    top = np.array([[[5, 4, 1]], [[2, 6, 3]], [[7, 0.5, 0.25]]], np.float32)
    gid = np.array([[[10, 11, 12]], [[12, 13, 14]], [[14, 15, 16]]], np.int64)
    cases.append((top, gid))
    top3 = np.array([[[5, 4, 1]], [[2, -np.inf, -np.inf]], [[7, 0.5, 0.25]]], np.float32)
    gid3 = np.array([[[10, 11, 12]], [[12, -1, -1]], [[12, 15, 16]]], np.int64)          # group 12 over three lists
    cases.append((top3, gid3))
    # repeated groups with EQUAL scores
    cases.append((np.array([[[3, 2, 2]], [[2, 2, 1]]], np.float32), np.array([[[0, 1, 2]], [[2, 3, 4]]], np.int64)))
    # padding; fewer than k distinct groups -> -inf (4 records, 3 distinct)
    cases.append((np.array([[[3, 2, -np.inf, -np.inf]], [[2.5, 1, -np.inf, -np.inf]]], np.float32),
                  np.array([[[0, 1, -1, -1]], [[1, 2, -1, -1]]], np.int64)))
    # everything padded
    cases.append((np.full((3, 2, 5), -np.inf, np.float32), np.full((3, 2, 5), -1, np.int64)))
    # S = 1
    cases.append((np.array([[[1, 9, 3, 7]]], np.float32), np.array([[[4, 2, 9, 0]]], np.int64)))
    # k = 1
    cases.append((np.array([[[1]], [[3]], [[2]]], np.float32), np.array([[[7]], [[7]], [[8]]], np.int64)))
    cases.append((np.array([[[-np.inf]], [[-np.inf]]], np.float32), np.array([[[-1]], [[-1]]], np.int64)))
    for top, gid in cases:
        k = top.shape[2]
        got, want = device_group_tau(top, gid), numpy_group_tau(top, gid, k)
        assert_same_f32(got, want, f"tau of {gid.tolist()}")
    # the k-th value: the first case by hand -- distinct scores {10: 5, 11: 4, 12: 2, 13: 6, 14: 7, 15: .5, 16: .25}, k = 3
    assert numpy_group_tau(cases[0][0], cases[0][1], 3)[0] == 5.0
    assert np.isneginf(numpy_group_tau(cases[3][0], cases[3][1], 4)[0])
    # random records of the shape phase 1 gives, several queries per call; S * k above and below one pass of 1024 threads
    rng = np.random.default_rng(3)
    for S, B, k, fill, straddle in ((2, 5, 7, 0.5, 1.0), (3, 4, 33, 1, 0.7), (5, 3, 64, 0.5, 0.5), (4, 3, 1000, 1, 1.0),
                                    (8, 2, 300, 0.5, 0.9), (1, 3, 50, 1, 0), (6, 4, 1, 0.5, 1.0), (256, 1, 5, 1, 0.8)):
        recs = [shard_like_lists(rng, S, k, fill, straddle) for _ in range(B)]
        top = np.stack([r[0] for r in recs], axis=1); gid = np.stack([r[1] for r in recs], axis=1)
        assert_same_f32(device_group_tau(top, gid), numpy_group_tau(top, gid, k), f"random S={S} B={B} k={k}")


# ---- 5. the grouped merge alone ---------------------------------------------------------------------------------------
def numpy_grouped_merge(P, S_, G, ncl, edges, k):
    """[L][B][k] records -> (pids (B, k), scores (B, k), n_cand [B])"""
    L, B, _ = P.shape
    op = np.zeros((B, k), np.int64); os_ = np.full((B, k), -np.inf, np.float32); on = np.zeros(B, np.int64)
    for b in range(B):
        recs = [(-float(S_[l, b, i]), int(P[l, b, i]), int(G[l, b, i])) for l in range(L) for i in range(k) if P[l, b, i] > 0]
        recs.sort()
        seen, out = set(), []
        for ns, p, g_ in recs:
            if g_ not in seen:
                seen.add(g_); out.append((p, -ns))
        for i, (p, s) in enumerate(out[:k]):
            op[b, i] = p; os_[b, i] = s
        total, prev_last = 0, -1
        for l in range(L):
            total += int(ncl[l, b])
            first, last = int(edges[l, b, 0]), int(edges[l, b, 1])
            if first < 0:
                continue
            total -= first == prev_last
            prev_last = last
        on[b] = total
    return op, os_, on


def device_grouped_merge(P, S_, G, ncl, edges, k, packed):
    import torch
    from colbert_jl_amd.distributed import merge_grouped_packed, packed_grouped_bytes, packed_topk_bytes
    L, B, _ = P.shape
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    if packed:
        nb, at_g = packed_grouped_bytes(k, B), packed_topk_bytes(k, B)
        blocks = np.zeros((L, nb), np.uint8)
        for l in range(L):
            blocks[l, :B * k * 8] = np.ascontiguousarray(P[l], np.int64).view(np.uint8).reshape(-1)
            blocks[l, B * k * 8:B * k * 12] = np.ascontiguousarray(S_[l], np.float32).view(np.uint8).reshape(-1)
            blocks[l, at_g:at_g + B * k * 8] = np.ascontiguousarray(G[l], np.int64).view(np.uint8).reshape(-1)
            blocks[l, at_g + B * k * 8:at_g + B * k * 8 + B * 8] = np.ascontiguousarray(ncl[l], np.int64).view(np.uint8)
            blocks[l, at_g + B * k * 8 + B * 8:] = np.ascontiguousarray(edges[l], np.int64).view(np.uint8).reshape(-1)
        op, os_, on = merge_grouped_packed(torch.from_numpy(blocks).to(dev), B, k)
    else:
        dP, dS, dG, dN, dE = up(P, np.int64), up(S_, np.float32), up(G, np.int64), up(ncl, np.int64), up(edges, np.int64)
        op = torch.full((B, k), -7, dtype=torch.int64, device=dev); os_ = torch.zeros((B, k), dtype=torch.float32, device=dev)
        on = torch.full((B,), -7, dtype=torch.int64, device=dev)
        clb._lib.check(clb.lib().clb_merge_topk_grouped_device(0, dP.data_ptr(), dS.data_ptr(), dG.data_ptr(), k, L, B, dN.data_ptr(),
                                                               dE.data_ptr(), op.data_ptr(), os_.data_ptr(), on.data_ptr(), None))
    torch.cuda.synchronize()
    return op.cpu().numpy(), os_.cpu().numpy(), on.cpu().numpy()


def as_lists(lists, k):
    """per list a sequence of (pid, score, gid) in any order -> sorted, padded [L][1][k] arrays"""
    L = len(lists)
    P = np.zeros((L, 1, k), np.int64); S_ = np.full((L, 1, k), -np.inf, np.float32); G = np.full((L, 1, k), -1, np.int64)
    for l, recs in enumerate(lists):
        recs = sorted(recs, key=lambda r: (-r[1], r[0]))
        assert len(recs) <= k and len({r[2] for r in recs}) == len(recs)
        for i, (p, s, g_) in enumerate(recs):
            P[l, 0, i], S_[l, 0, i], G[l, 0, i] = p, s, g_
    return P, S_, G


def merge_case(rng, L, k, straddle, empty=0.0):
    """One query's lists as grouped shards return them: list l holds up to k distinct groups of a contiguous range (pids of
    shard l in l * 10000 + 1 ..), ranges meet as in shard_like_lists; the edge groups are the ends of the range when the
    list has candidates; a list is empty with probability `empty`."""
    lists, ncl, edges = [], np.zeros(L, np.int64), np.full((L, 2), -1, np.int64)
    base = int(rng.integers(0, 50))
    for l in range(L):
        width = int(rng.integers(1, 2 * k + 2))
        if rng.random() < empty:
            lists.append([])
        else:
            m = int(rng.integers(1, min(k, width) + 1))
            chosen = pick_groups(rng, width, m)
            pids = l * 10000 + 1 + np.sort(rng.choice(9000, len(chosen), replace=False))
            lists.append([(int(p), float(rng.integers(-6, 7)) / 2, base + c) for p, c in zip(pids, chosen)])
            ncl[l] = width                                     # candidate groups: every group of the range
            edges[l] = (base, base + width - 1)
        base += width - 1 if rng.random() < straddle else width
    return lists, ncl, edges


@pytest.mark.parametrize("packed", [False, True])
def test_grouped_merge_on_crafted_lists(packed):
    def run(lists, ncl, edges, k, what):
        P, S_, G = as_lists(lists, k)
        ncl = np.asarray(ncl, np.int64).reshape(len(lists), 1); edges = np.asarray(edges, np.int64).reshape(len(lists), 1, 2)
        got = device_grouped_merge(P, S_, G, ncl, edges, k, packed)
        want = numpy_grouped_merge(P, S_, G, ncl, edges, k)
        assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
        assert_same_f32(got[1], want[1], what)
        assert np.array_equal(got[2], want[2]), (what, got[2], want[2])
        return got

    # a duplicate ranked first: group 5 leads both lists; the survivor is the higher score, everything moves up
    p, s, n = run([[(10, 9.0, 5), (11, 3.0, 4), (12, 1.0, 3)], [(20, 8.0, 5), (21, 2.0, 6), (22, 0.5, 7)]],
                  [3, 3], [(3, 5), (5, 7)], 4, "duplicate first")
    assert p[0].tolist() == [10, 11, 21, 12] and n[0] == 5
    # a duplicate ranked last: the loser is the last record of all; nothing above it moves
    p, s, n = run([[(10, 9.0, 3), (11, 3.0, 4), (12, 1.0, 5)], [(20, 0.25, 5), (21, 2.0, 6), (22, 0.5, 7)]],
                  [3, 3], [(3, 5), (5, 7)], 6, "duplicate last")
    assert p[0].tolist() == [10, 11, 21, 12, 22, 0] and np.isneginf(s[0, 5])
    # equal scores broken by pid, across the lists and inside the duplicate pair (the lower pid survives)
    p, s, n = run([[(10, 2.0, 3), (11, 2.0, 4), (12, 2.0, 5)], [(20, 2.0, 5), (21, 2.0, 6)]], [3, 2], [(3, 5), (5, 6)], 5, "ties")
    assert p[0].tolist() == [10, 11, 12, 21, 0]
    # all lists padded
    p, s, n = run([[], [], []], [0, 0, 0], [(-1, -1)] * 3, 3, "all padded")
    assert np.all(p == 0) and np.all(np.isneginf(s)) and n[0] == 0
    # a duplicate chain over three lists: group 5 is the last of list 0, the only group of list 1, the first of list 2
    p, s, n = run([[(10, 1.0, 4), (11, 2.0, 5)], [(20, 7.0, 5)], [(30, 3.0, 5), (31, 0.5, 6)]],
                  [2, 1, 2], [(4, 5), (5, 5), (5, 6)], 3, "chain")
    assert p[0].tolist() == [20, 10, 31] and n[0] == 3
    # the n_cand formula with an empty middle shard: the group straddles shards 0 and 2 across it
    p, s, n = run([[(10, 1.0, 4), (11, 2.0, 5)], [], [(30, 3.0, 5), (31, 0.5, 6)]], [2, 0, 2], [(4, 5), (-1, -1), (5, 6)], 3,
                  "empty middle")
    assert p[0].tolist() == [30, 10, 31] and n[0] == 3
    # ... and without a straddling group nothing is subtracted
    _, _, n = run([[(10, 1.0, 4)], [], [(30, 3.0, 6)]], [1, 0, 1], [(4, 4), (-1, -1), (6, 6)], 2, "no straddle")
    assert n[0] == 2
    # random lists, several queries per call: L * k above and below one work-group, up to the list limit
    rng = np.random.default_rng(9)
    for L, B, k, straddle, empty in ((2, 4, 5, 1.0, 0), (3, 5, 40, 0.8, 0.2), (4, 3, 300, 1.0, 0), (5, 4, 1, 1.0, 0.2),
                                     (1, 3, 20, 0, 0), (8, 2, 100, 0.6, 0.3), (256, 1, 3, 0.9, 0.1)):
        qs = [merge_case(rng, L, k, straddle, empty) for _ in range(B)]
        arrs = [as_lists(q[0], k) for q in qs]
        P, S_, G = (np.concatenate([a[i] for a in arrs], axis=1) for i in range(3))
        ncl = np.stack([q[1] for q in qs], axis=1); edges = np.stack([q[2] for q in qs], axis=1)
        got = device_grouped_merge(P, S_, G, ncl, edges, k, packed)
        want = numpy_grouped_merge(P, S_, G, ncl, edges, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (L, B, k)
        assert_same_f32(got[1], want[1], f"random merge L={L} B={B} k={k}")


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------
def test_a_grouping_survives_remove_and_update(oracle, corpus):
    idx, Qs, full = corpus
    nq = Qs.shape[2]
    with clb.ShardedSearcher.from_index(idx, 2) as g:
        ids = straddling_ids(cuts_of(g))
        gr = g.make_grouping(group_ids=ids)
        top = np.unique(np.concatenate([r[0][:3] for r in full]))                      # the answers must change
        removed = np.unique(np.concatenate([top, boundary_pids(g), [1, N]]))
        assert g.remove_passages(removed) == removed.size
        red, _ = reduced_index(idx, removed)
        rankings = [grouped_ranking(oracle, red, Qs[:, :, j], NPROBE, ids) for j in range(nq)]
        assert any(not np.array_equal(r[0][:10], collapse(f, ids)[0][:10]) for r, f in zip(rankings, full))
        for k in (10, 700):
            check_grouped(g, gr, Qs, rankings, k, f"after remove k={k}")
        # update: the removed passages get other passages' content, the next best ones are emptied
        c = cuts_of(g)[0]
        pids = np.array(list(dict.fromkeys(np.concatenate([removed[:6], [c, c + 1], rankings[0][0][:2]]).tolist())), np.int64)
        donors = [[(int(p) + 50) % N + 1] if i % 3 else [] for i, p in enumerate(pids)]
        parts = [content_of(idx, d) for d in donors]
        args = (pids, np.concatenate([x[0] for x in parts]), np.asfortranarray(np.concatenate([x[1] for x in parts], axis=1)),
                np.array([x[2].sum() for x in parts], np.int64))
        assert g.update_compressed(*args) > 0
        want = updated_index(red, *args)
        rankings = [grouped_ranking(oracle, want, Qs[:, :, j], NPROBE, ids) for j in range(nq)]
        for k in (10, 700):
            check_grouped(g, gr, Qs, rankings, k, f"after update k={k}")
        gr.close()


def test_a_grouping_is_refused_after_an_append_and_by_another_group(oracle, corpus, groups):
    idx, Qs, full = corpus
    P = 5950
    with clb.ShardedSearcher.from_index(head_index(idx, P), 2) as g:
        old = g.make_grouping(group_lens=random_lens(P, 1, 6, 3))
        g.search_batch(Qs, 10, NPROBE, pad_short=True, grouping=old)
        assert g.add_compressed(*tail(idx, P)) == range(P + 1, N + 1)
        for proto in PROTOCOLS:
            with pytest.raises(clb.ArgumentError, match="made before an append"):
                g.search_batch(Qs, 10, NPROBE, protocol=proto, grouping=old)
        # the library's own check, on the shard that grew
        last = g.shards[-1]
        import torch
        from colbert_jl_amd.distributed import DeviceSearch
        run = DeviceSearch(last, Qs.shape[1], Qs.shape[2], 10, NPROBE)
        Qd = torch.from_numpy(np.array(Qs.transpose(2, 1, 0), order="C")).to(run.dev)
        with pytest.raises(clb.ArgumentError, match="made before an append"):
            run.phase1(Qd, None, "candidates", old.parts[-1], old.bases[-1])
        old.close()
        ids = straddling_ids(cuts_of(g))
        with g.make_grouping(group_ids=ids) as gr:                  # a new one covers the new passages
            rankings = [collapse(r, ids) for r in full]
            check_grouped(g, gr, Qs, rankings, 100, "after append")
            for other in groups.values():
                with pytest.raises(clb.ColBERTError, match="ShardedGrouping of this shard group"):
                    other.search_batch(Qs, 10, NPROBE, grouping=gr)


def test_argument_contracts_on_a_live_handle(corpus, groups):
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    _, Qs, _ = corpus
    l = clb.lib()
    g = groups[2]
    s0, s1 = g.shards
    T, B, k = Qs.shape[1], Qs.shape[2], 10
    dev = torch.device("cuda", s0.device)
    Qd = torch.from_numpy(np.array(Qs.transpose(2, 1, 0), order="C")).to(dev)
    top = torch.empty((B, k), dtype=torch.float32, device=dev)
    gid = torch.full((B, k), -5, dtype=torch.int64, device=dev)
    out = torch.zeros((B, k), dtype=torch.int64, device=dev)
    with g.make_grouping(group_lens=[N]) as gr:
        h0, h1 = gr.parts[0]._h, gr.parts[1]._h
        p1 = lambda s, h, base, t=top.data_ptr(), gd=gid.data_ptr(): l.clb_search_shard_phase1_grouped_slot(
            s._h, 0, Qd.data_ptr(), T, B, NPROBE, k, None, 0, h, base, t, gd, None)
        assert p1(s0, h1, 0) == clb.ArgumentError.code and b"another searcher" in l.clb_last_error()
        assert p1(s0, h0, 0, None) == clb.ArgumentError.code and b"d_local_top" in l.clb_last_error()
        assert p1(s0, h0, 0, top.data_ptr(), None) == clb.ArgumentError.code and b"d_local_gid" in l.clb_last_error()
        assert p1(s0, h0, -1) == clb.ArgumentError.code and b"group_base" in l.clb_last_error()
        # grouping == NULL: the filtered phase 1, d_local_gid untouched
        assert p1(s0, None, 0) == 0
        torch.cuda.synchronize()
        assert torch.all(gid == -5)
        plain = top.clone()
        assert l.clb_search_shard_phase1_filtered_slot(s0._h, 0, Qd.data_ptr(), T, B, NPROBE, k, None, 0, top.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(plain.sort(dim=1).values, top.sort(dim=1).values)
        # phase 2: must follow the grouped phase 1 with the same grouping and base; null outputs
        n = torch.zeros(B, dtype=torch.int64, device=dev); e = torch.zeros((B, 2), dtype=torch.int64, device=dev)
        sc = torch.zeros((B, k), dtype=torch.float32, device=dev)
        og = torch.zeros((B, k), dtype=torch.int64, device=dev)
        p2 = lambda h, base, o=out.data_ptr(), ed=e.data_ptr(): l.clb_search_shard_phase2_grouped_slot(
            s0._h, 0, Qd.data_ptr(), T, B, NPROBE, k, top.data_ptr(), gid.data_ptr(), 1, h, base, o, sc.data_ptr(), og.data_ptr(),
            n.data_ptr(), ed, None)
        assert p2(h0, 0) == clb.ArgumentError.code and b"without a matching" in l.clb_last_error()      # phase 1 was ungrouped
        assert p1(s0, h0, 3) == 0
        assert p2(h0, 0) == clb.ArgumentError.code and b"without a matching" in l.clb_last_error()      # another base
        assert p2(h0, 3, None) == clb.ArgumentError.code and b"null" in l.clb_last_error()
        assert p2(h0, 3, out.data_ptr(), None) == clb.ArgumentError.code
        assert l.clb_search_shard_phase2_slot(s0._h, 0, Qd.data_ptr(), T, B, NPROBE, k, top.data_ptr(), 1, out.data_ptr(),
                                              sc.data_ptr(), n.data_ptr(), None) == clb.ArgumentError.code      # grouped phase 1 pending
        assert p2(h0, 3) == 0
        torch.cuda.synchronize()
        assert torch.all(n == 1) and torch.all(og[:, 0] == 3) and torch.all(og[:, 1:] == -1) and torch.all(e == 3)
        assert torch.all(out[:, 0] > 0) and torch.all(out[:, 1:] == 0)
        # the single exchange's second call needs the grouped search before it, on the same slot
        rg = lambda B_=B: l.clb_search_result_groups_slot(s0._h, 0, h0, 0, out.data_ptr(), B_, k, og.data_ptr(), e.data_ptr(), None)
        assert rg() == clb.ArgumentError.code and b"without a matching" in l.clb_last_error()
        run = DeviceSearch(s0, T, B, k, NPROBE)
        run.search_grouped_shard(Qd, None, "candidates", gr.parts[0], 0)
        assert rg(B - 1) == clb.ArgumentError.code
        assert rg() == 0
        torch.cuda.synchronize()
        # a handle outside the two-pass mode refuses the phase calls
        s0.set_mode(0)
        try:
            assert p1(s0, h0, 0) == clb.Unsupported.code and b"two-pass mode" in l.clb_last_error()
            with pytest.raises(clb.Unsupported, match="two-pass mode"):
                g.search_batch(Qs, k, NPROBE, protocol="two_phase", grouping=gr)
            # ... and the single exchange serves it
            rankings = [collapse(r, np.zeros(N, np.int64)) for r in corpus[2]]
            check_grouped(g, gr, Qs, rankings, 3, "mode 0", protocols=("single", "auto"))
        finally:
            s0.set_mode(1)
        # a filtered grouped phase 1 takes at most 64 queries
        B2 = 65
        Qb = torch.cat([Qd] * 11)[:B2].contiguous()
        top2 = torch.empty((B2, k), dtype=torch.float32, device=dev); gid2 = torch.empty((B2, k), dtype=torch.int64, device=dev)
        with s0.make_filter(pids=[1, 2, 3]) as f0:
            handles = s0._filter_handles([f0] + [None] * (B2 - 1), B2)
            args = (s0._h, 0, Qb.data_ptr(), T, B2, NPROBE, k)
            assert l.clb_search_shard_phase1_grouped_slot(*args, handles, 0, h0, 0, top2.data_ptr(), gid2.data_ptr(), None) \
                == clb.Unsupported.code and b"at most 64 queries" in l.clb_last_error()
            assert l.clb_search_shard_phase1_grouped_slot(*args, None, 0, h0, 0, top2.data_ptr(), gid2.data_ptr(), None) == 0
        torch.cuda.synchronize()


def test_batch_above_one_piece_and_general_shape_shards(oracle, corpus, groups):
    idx, Qs, full = corpus
    g = groups[4]
    ids = straddling_ids(sorted(set(cuts_of(groups[2]) + cuts_of(groups[4]))))
    B, k, nq = 65, 20, Qs.shape[2]
    Qb = np.asfortranarray(np.concatenate([Qs] * 11, axis=2)[:, :, :B])
    rankings = [collapse(r, ids) for r in full]
    with g.make_grouping(group_ids=ids) as gr:
        for proto in PROTOCOLS:
            p, s, n = g.search_batch(Qb, k, NPROBE, protocol=proto, grouping=gr)
            for b in range(B):
                assert_result(p[:, b], s[:, b], n[b], rankings[b % nq], k, f"B=65 {proto} q={b}")
    # general-shape shards (mode 0): protocol "auto" is the single exchange
    gen = synthetic.make_index(seed=79, n_docs=900, K=96, dim=64, nbits=8, doclen_mean=20, doclen_std=12)
    Qg = synthetic.make_queries(gen, 80, 3, T=20)
    with clb.ShardedSearcher.from_index(gen, 3) as gg:
        assert all(s.mode == 0 for s in gg.shards)
        gids = ids_from_lens(random_lens(900, 1, 5, 4))
        for c in cuts_of(gg):
            gids[c] = gids[c - 1]
        want = [grouped_ranking(oracle, gen, Qg[:, :, j], NPROBE, gids) for j in range(3)]
        with gg.make_grouping(group_ids=gids) as gr:
            for kk in (50, 10):
                for proto in ("auto", "single"):
                    p, s, n = gg.search_batch(Qg, kk, NPROBE, pad_short=True, protocol=proto, grouping=gr)
                    for j in range(3):
                        assert_result(p[:, j], s[:, j], n[j], want[j], kk, f"general {proto} k={kk} q={j}")
            with pytest.raises(clb.Unsupported, match="two-pass mode"):
                gg.search_batch(Qg, 10, NPROBE, protocol="two_phase", grouping=gr)


# ---- 7. two rank processes over gloo ----------------------------------------------------------------------------------
K_RANKS = 100


def _worker(rank, world, store, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    import colbert_jl_amd as clb
    from colbert_jl_amd.sharding import shard_index
    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    idx = clb.synthetic.make_index(seed=141, n_docs=N, K=512)
    Qs = clb.synthetic.make_queries(idx, 142, 6)
    sub, off = shard_index(idx, rank, world)
    g = clb.ShardedSearcher([clb.Searcher(index=sub, device=0, pid_offset=off)], group=dist.group.WORLD)
    ids = straddling_ids(cuts_of(g))                     # every rank passes the same array
    out = {"ranges": [(r.start, r.stop) for r in g.shard_ranges]}
    with g.make_grouping(group_ids=ids) as gr:
        out["bases"], out["count"] = gr.bases, gr.count
        out["two_phase"] = g.search_batch(Qs, K_RANKS, NPROBE, pad_short=True, protocol="two_phase", grouping=gr)
    q.put((rank, out))
    dist.barrier()
    g.close()
    dist.destroy_process_group()


def test_two_rank_processes_grouped(oracle):
    import torch.multiprocessing as mp

    from colbert_jl_amd.sharding import shard_bounds
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
    idx = synthetic.make_index(seed=141, n_docs=N, K=512)
    Qs = synthetic.make_queries(idx, 142, 6)
    cut = int(shard_bounds(idx["doclens"], world)[1])
    ids = straddling_ids([cut])
    dense = np.unique(ids, return_inverse=True)[1]
    rankings = [collapse(filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE), ids) for j in range(Qs.shape[2])]
    for r in range(world):                                          # identical on every rank
        out = res[r]
        assert out["ranges"] == [(1, cut + 1), (cut + 1, N + 1)]
        assert out["bases"] == [int(dense[0 if r == 0 else cut])] and out["count"] == np.unique(ids).size
        p, s, n = out["two_phase"]
        for j in range(Qs.shape[2]):
            assert_result(p[:, j], s[:, j], n[j], rankings[j], K_RANKS, f"rank={r} q={j}")
