"""Hits of a grouped search (`per_group=`) without a GPU: the reference helper pinned against an independent restatement,
a host model of the two-pass listing rule with its teeth, the two new C entry points and the Python
keywords."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from tests.test_group_cpu import _NoDevice
from tests.test_sharded_searcher_cpu import stub_group
from tests.util_group import collapse, ids_from_lens, random_lens
from tests.util_group_hits import hits_reference

NEW_SYMBOLS = ("clb_search_batch_grouped_hits", "clb_search_batch_grouped_hits_device_slot")


def stable_ranking(pids, scores):
    """(pids ascending, scores) -> the full ranking: score descending, the lower pid first among equal scores"""
    order = np.argsort(-np.asarray(scores, np.float32), kind="stable")
    return np.asarray(pids, np.int64)[order], np.asarray(scores, np.float32)[order]


def hits_by_dictionary(pids, scores, gids, k, m):
    """The specification restated without a ranking: per group its candidates by (-score, pid), the groups by their best."""
    groups = {}
    for p, s in zip(pids, scores):
        groups.setdefault(int(gids[p - 1]), []).append((-float(s), int(p)))
    for members in groups.values():
        members.sort()
    order = sorted(groups, key=lambda grp: groups[grp][0])
    out_p = np.zeros((m, k), np.int64); out_s = np.full((m, k), -np.inf, np.float32)
    for j, grp in enumerate(order[:k]):
        for i, (neg, p) in enumerate(groups[grp][:m]):
            out_p[i, j] = p; out_s[i, j] = -neg
    return out_p, out_s, len(groups)


@pytest.mark.parametrize("seed", range(6))
def test_helper_equals_the_dictionary_restatement(seed):
    """random candidate sets with planted exact score ties, groups of 1 .. 9 passages -- many with fewer than m members"""
    rng = np.random.default_rng(900 + seed)
    n_docs = int(rng.integers(30, 400))
    gids = ids_from_lens(random_lens(n_docs, 1, 9, 910 + seed)) * 3 + 5           # any non-decreasing ids
    pids = np.sort(rng.choice(np.arange(1, n_docs + 1), size=int(rng.integers(1, n_docs + 1)), replace=False))
    scores = rng.integers(0, 12, size=pids.size).astype(np.float32) / 4            # a dozen values: ties everywhere
    ranking = stable_ranking(pids, scores)
    for k in (1, 7, n_docs):
        for m in (1, 2, 5, 16):
            gp, gs, gn = hits_reference(ranking, gids, k, m)
            wp, ws, wn = hits_by_dictionary(pids, scores, gids, k, m)
            assert gn == wn and np.array_equal(gp, wp) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (seed, k, m)
            if m == 1:                                         # one hit per group is the grouped search itself
                cp, cs = collapse(ranking, gids)
                n = min(k, cp.size)
                assert np.array_equal(gp[0, :n], cp[:n]) and np.array_equal(gs[0, :n], cs[:n]) and np.all(gp[0, n:] == 0)
            members = np.bincount(np.searchsorted(np.unique(gids), gids[pids - 1]))
            short = np.nonzero(members[np.searchsorted(np.unique(gids), gids[gp[0, :min(k, gn)] - 1])] < m)[0]
            for j in short:                                    # fewer than m members: padded, never an error
                have = members[np.searchsorted(np.unique(gids), gids[gp[0, j] - 1])]
                assert np.all(gp[have:, j] == 0) and np.all(np.isneginf(gs[have:, j])) and np.all(gp[:have, j] > 0)
    assert hits_reference((np.zeros(0, np.int64), np.zeros(0, np.float32)), gids, 3, 2)[2] == 0
    off_p, _, _ = hits_reference(ranking, gids, 4, 2, pid_offset=1000)
    base_p, _, _ = hits_reference(ranking, gids, 4, 2)
    assert np.array_equal(off_p, np.where(base_p > 0, base_p + 1000, 0))


# ---- the listing rule of the two-pass mode, on the host --------------------------------------------------------------------
def group_best(values, gids):
    """per group (ascending group order) the largest of `values`"""
    uniq, inv = np.unique(gids, return_inverse=True)
    best = np.full(uniq.size, -np.inf)
    np.maximum.at(best, inv, values)
    return best, inv


def listing(a, gids, k, m, eps, lower_tau=0.0, extend=True):
    """The list of DESIGN section 5 from approximate scores a (one per candidate, candidates in pid order, gids their
    groups): L0 = {a >= tau_g - 2 eps}, tau_g = the k-th best group by approximate score (-inf with fewer than k groups)
    lowered by `lower_tau`; with `extend` the passages of every listed group at or above its m-th best approximate score
    minus 2 eps (a group of fewer than m candidates: all of them)."""
    best, inv = group_best(a, gids)
    tau = -np.inf if best.size < k else np.sort(best)[-k] - lower_tau
    listed = a >= tau - 2 * eps
    if not extend:
        return listed
    mth = np.full(best.size, -np.inf)
    for grp in range(best.size):
        mine = np.sort(a[inv == grp])[::-1]
        if mine.size >= m:
            mth[grp] = mine[m - 1]
    group_listed = np.zeros(best.size, bool)
    group_listed[inv[listed]] = True
    return listed | (group_listed[inv] & (a >= mth[inv] - 2 * eps))


def noisy(rng, s, eps):
    """a = s + noise, |noise| <= eps, a third of the draws pinned at -eps and at +eps"""
    kind = rng.integers(0, 3, size=s.size)
    return s + np.where(kind == 0, -eps, np.where(kind == 1, eps, rng.uniform(-eps, eps, size=s.size)))


@pytest.mark.parametrize("seed", range(5))
def test_hits_from_the_extended_list_equal_hits_from_everything(seed):
    """Exact scores on a grid of 1/64 (exact in fp32 and in the float64 of the model, with ties), eps = 1/4, random
    contiguous groups: the hits ranked from L alone are the hits ranked from every candidate, with tau_g exact and lowered."""
    rng = np.random.default_rng(1200 + seed)
    n = int(rng.integers(150, 1200))
    gids = ids_from_lens(random_lens(n, 1, int(rng.choice([3, 12, 60])), 1210 + seed))
    pids = np.arange(1, n + 1)
    s = rng.integers(0, 64 * 12, size=n) / 64.0
    eps = 0.25
    a = noisy(rng, s, eps)
    assert np.max(np.abs(a - s)) <= eps and np.any(a - s == eps) and np.any(s - a == eps)
    everything = stable_ranking(pids, s)
    for k in (1, 10, 100):
        for m in (1, 2, 5, 16):
            want = hits_reference(everything, gids, k, m)
            for lower_tau in (0.0, 0.37):
                L = listing(a, gids, k, m, eps, lower_tau)
                got = hits_reference(stable_ranking(pids[L], s[L]), gids, k, m)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (seed, k, m, lower_tau)
                L0 = listing(a, gids, k, m, eps, lower_tau, extend=False)
                assert np.all(L[L0])                           # the list only grows ...
                assert np.array_equal(np.unique(gids[L]), np.unique(gids[L0]))      # ... by passages of listed groups
                if m == 1:                                     # one hit per group needs nothing added: L0 alone is enough
                    alone = hits_reference(stable_ranking(pids[L0], s[L0]), gids, k, m)
                    assert np.array_equal(alone[0], want[0]) and np.array_equal(alone[1].view(np.uint32), want[1].view(np.uint32))


def test_teeth_the_list_of_the_grouped_search_alone_loses_a_hit():
    """Three groups of three, k = 2, m = 2, eps = 0.01.  Group 0 wins with 10.0; its second passage scores 1.0, far more than
    4 eps below the second group's 5.0: the list of the grouped search (L0) does not hold it, the extended list does, and
    only the hits ranked from the extended list are right."""
    gids = ids_from_lens([3, 3, 3])
    pids = np.arange(1, 10)
    s = np.array([10.0, 1.0, 0.5, 5.0, 4.99, 0.2, 3.0, 2.9, 2.8])
    eps, k, m = 0.01, 2, 2
    a = s.copy()
    assert s[1] < np.sort(group_best(s, gids)[0])[-k] - 4 * eps
    L0 = listing(a, gids, k, m, eps, extend=False)
    L = listing(a, gids, k, m, eps)
    assert not L0[1] and L[1]
    assert list(np.nonzero(L0)[0]) == [0, 3, 4] and list(np.nonzero(L)[0]) == [0, 1, 3, 4]
    want = hits_reference(stable_ranking(pids, s), gids, k, m)
    assert np.array_equal(want[0], [[1, 4], [2, 5]])
    from_L0 = hits_reference(stable_ranking(pids[L0], s[L0]), gids, k, m)
    from_L = hits_reference(stable_ranking(pids[L], s[L]), gids, k, m)
    assert not np.array_equal(from_L0[0], want[0]) and from_L0[0][1, 0] == 0       # the second hit of the winner is lost
    assert np.array_equal(from_L[0], want[0]) and np.array_equal(from_L[1], want[1])


# ---- the C ABI and the Python keywords ------------------------------------------------------------------------------------------
def test_hits_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    header = " ".join(open(clb._lib.HEADER).read().replace("*", " ").split())
    assert "enum { CLB_MAX_PER_GROUP = 16 };" in header and "per_group == 1 launches exactly what the grouped call launches" in header
    assert clb.searcher.MAX_PER_GROUP == 16


def test_hits_entry_points_check_their_arguments_first():
    """A null grouping and a per_group outside 1..16 are ArgumentError (4), named in the message, before anything else."""
    l = clb.lib()
    i64 = C.c_int64
    null, some = C.c_void_p(), C.c_void_p(0xdead0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    q = np.zeros((128, 32, 1), np.float32, order="F")
    op, os_, nc = np.zeros(10, np.int64), np.zeros(10, np.float32), np.zeros(1, np.int64)
    assert l.clb_search_batch_grouped_hits(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, null, i64(2), 1, p(op), p(os_), p(nc)) == 4
    assert b"grouping is null" in l.clb_last_error()
    for m in (0, 17, -1):
        assert l.clb_search_batch_grouped_hits(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, some, i64(m), 1, p(op), p(os_),
                                               p(nc)) == 4
        assert b"per_group must be 1..16" in l.clb_last_error()
        assert l.clb_search_batch_grouped_hits_device_slot(null, 0, None, i64(32), i64(1), i64(2), i64(5), None, 0, some, i64(m), None,
                                                           None, None, None) == 4
        assert b"per_group must be 1..16" in l.clb_last_error()
    assert l.clb_search_batch_grouped_hits_device_slot(null, 0, None, i64(32), i64(1), i64(2), i64(5), None, 0, null, i64(2), None, None,
                                                       None, None) == 4
    # in range, with a grouping: the searcher is looked at next
    assert l.clb_search_batch_grouped_hits(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, some, i64(16), 1, p(op), p(os_), p(nc)) == 4
    assert b"per_group" not in l.clb_last_error()


def test_per_group_is_validated_on_the_host():
    s = _NoDevice()
    Q = np.zeros((128, 32, 2), np.float32, order="F")
    g = clb.PassageGrouping(s, None, 2, ids_from_lens([60, 40]))
    for bad in (0, 17, -3):
        with pytest.raises(clb.ArgumentError, match="per_group must be 1..16"):
            s.search_batch(Q, 5, grouping=g, per_group=bad)
    for bad in (2.0, "2", True):
        with pytest.raises(clb.ArgumentError, match="integer"):
            s.search_batch(Q, 5, grouping=g, per_group=bad)
    with pytest.raises(clb.ArgumentError, match="needs grouping="):
        s.search_batch(Q, 5, per_group=2)
    with pytest.raises(clb.ArgumentError, match="needs grouping="):
        s.search_embeddings(Q[:, :, 0], 5, per_group=1)
    with pytest.raises(clb.ArgumentError, match="needs grouping="):
        clb.search(s, Q[:, :, 0], 5, per_group=3)
    with pytest.raises(clb.ColBERTError, match="open PassageGrouping"):          # in range: the (closed) grouping is looked at next
        s.search_batch(Q, 5, grouping=g, per_group=np.int64(16))


def test_a_shard_group_refuses_per_group_by_name():
    g = stub_group()
    Q = np.zeros((128, 32, 1), np.float32, order="F")
    for call in (lambda: g.search_batch(Q, 3, per_group=2), lambda: g.search_embeddings(Q[:, :, 0], 3, per_group=1),
                 lambda: g.search("a query", 3, per_group=2)):
        with pytest.raises(clb.Unsupported, match="per_group"):
            call()
