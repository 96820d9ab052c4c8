"""Grouped search, the part that needs no GPU: the reference helper of tests/util_group.py against a brute-force
dictionary maximum, a host model of the two-pass rule with the threshold at the k-th best GROUP, the
C ABI's new symbols and their argument checks, and the Python keywords."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd.searcher import Searcher
from tests.util_group import collapse, ids_from_lens, random_lens

NEW_SYMBOLS = ("clb_grouping_create", "clb_grouping_count", "clb_grouping_destroy", "clb_search_batch_grouped",
               "clb_search_batch_grouped_device_slot")


def stable_ranking(pids, scores):
    """the reference's ranking of candidates `pids` (ascending) with `scores`: score descending, stable"""
    order = np.argsort(-scores, kind="stable")
    return pids[order], scores[order]


def brute_force(pids, scores, group_ids):
    """best passage of every group by a dictionary (larger score, then lower pid), groups by (score desc, pid asc)"""
    best = {}
    for p, s in zip(pids.tolist(), scores.tolist()):
        g = int(group_ids[p - 1])
        if g not in best or s > best[g][0] or (s == best[g][0] and p < best[g][1]):
            best[g] = (s, p)
    rows = sorted(best.values(), key=lambda t: (-t[0], t[1]))
    return np.array([r[1] for r in rows], np.int64), np.array([r[0] for r in rows], np.float32)


@pytest.mark.parametrize("seed", range(20))
def test_collapse_is_the_dictionary_maximum(seed):
    rng = np.random.default_rng(seed)
    n_docs = int(rng.integers(1, 400))
    gids = ids_from_lens(random_lens(n_docs, 1, int(rng.integers(1, 30)), seed)) * 3 + 7      # any non-decreasing ids
    pids = np.sort(rng.choice(np.arange(1, n_docs + 1), size=int(rng.integers(1, n_docs + 1)), replace=False)).astype(np.int64)
    scores = rng.integers(0, 6, size=pids.size).astype(np.float32) / 4                       # many ties
    cp, cs = collapse(stable_ranking(pids, scores), gids)
    bp, bs = brute_force(pids, scores, gids)
    assert np.array_equal(cp, bp) and np.array_equal(cs, bs)
    assert np.unique(gids[cp - 1]).size == cp.size == np.unique(gids[pids - 1]).size


def test_collapse_edge_groupings():
    rng = np.random.default_rng(1)
    pids = np.arange(1, 51, dtype=np.int64)
    scores = rng.integers(0, 5, size=50).astype(np.float32)
    r = stable_ranking(pids, scores)
    sp, ss = collapse(r, np.arange(50))                        # all singletons: the identity
    assert np.array_equal(sp, r[0]) and np.array_equal(ss, r[1])
    op, os_ = collapse(r, np.zeros(50, np.int64))              # one group: its best passage, the lowest pid among equals
    assert op.size == 1 and op[0] == r[0][0] and os_[0] == scores.max() and op[0] == pids[np.argmax(scores)]
    ep, es = collapse((np.zeros(0, np.int64), np.zeros(0, np.float32)), np.arange(50))
    assert ep.size == 0 and es.size == 0


def two_pass_model(pids, exact, approx, gids, k, eps, tau_of="groups"):
    """The grouped two-pass rule on the host: tau_g = the k-th largest of the groups' best APPROXIMATE scores (-inf with
    fewer than k groups), listed = approx >= tau_g - 2 eps, then the collapse of the listed passages by EXACT score and its
    first k.  tau_of="passages": the ungrouped rule (k-th best passage), which is NOT enough for groups."""
    g = gids[pids - 1]
    best_approx = np.array([approx[g == x].max() for x in np.unique(g)])
    vals = best_approx if tau_of == "groups" else approx
    tau = np.sort(vals)[::-1][k - 1] if vals.size >= k else -np.inf
    listed = approx >= tau - 2 * eps
    cp, cs = collapse(stable_ranking(pids[listed], exact[listed]), gids)
    return cp[:k], cs[:k], int(listed.sum())


def model_case(seed):
    """one random case of the host model, checked; -> the number of its k with a group tied with the k-th right behind it"""
    rng = np.random.default_rng(1000 + seed)
    n_docs = int(rng.integers(30, 600))
    gids = ids_from_lens(random_lens(n_docs, 1, int(rng.choice([1, 3, 12, 60])), seed))
    pids = np.sort(rng.choice(np.arange(1, n_docs + 1), size=int(rng.integers(20, n_docs + 1)), replace=False)).astype(np.int64)
    exact = rng.integers(0, int(rng.choice([4, 16, 200])), size=pids.size).astype(np.float64) / 8
    eps = float(rng.choice([0.05, 0.3, 1.0]))
    approx = exact + rng.uniform(-eps, eps, size=pids.size)
    n_groups = np.unique(gids[pids - 1]).size
    tied_at_k = 0
    for k in sorted({1, 2, max(1, n_groups // 3), n_groups, n_groups + 5}):
        fp, fs = collapse(stable_ranking(pids, exact.astype(np.float32)), gids)
        mp, ms, n_listed = two_pass_model(pids, exact.astype(np.float32), approx, gids, k, eps)
        assert np.array_equal(mp, fp[:k]) and np.array_equal(ms, fs[:k]), (seed, k)
        if n_groups < k:
            assert n_listed == pids.size and mp.size == n_groups         # tau_g = -inf lists everything: the short result
        tied_at_k += k < fp.size and fs[k - 1] == fs[k]
    return tied_at_k


@pytest.mark.parametrize("seed", range(50))
def test_host_model_of_the_grouped_two_pass_rule(seed):
    """exact scores on a coarse grid (ties, also at rank k), approx = exact + noise of at most eps: the first k groups of the
    listed set equal the collapse of the full exact ranking."""
    model_case(seed)


def test_the_host_model_meets_ties_at_rank_k():
    """groups tied with the k-th are among the cases the rule is checked on"""
    assert sum(1 for seed in range(50) if model_case(seed)) >= 10


def test_the_passage_threshold_is_not_enough_for_groups():
    """Why tau moves to the k-th best group: with one group holding the k best passages, the ungrouped cut lists (almost)
    only that group and the model loses groups that belong to the answer."""
    pids = np.arange(1, 201, dtype=np.int64)
    gids = ids_from_lens([50] * 4)
    exact = np.concatenate([np.full(50, 10.0), np.linspace(5, 4, 50), np.linspace(3, 2, 50), np.linspace(1, 0, 50)]).astype(np.float32)
    full = collapse(stable_ranking(pids, exact), gids)
    good = two_pass_model(pids, exact, exact.astype(np.float64), gids, 3, 0.01)
    bad = two_pass_model(pids, exact, exact.astype(np.float64), gids, 3, 0.01, tau_of="passages")
    assert np.array_equal(good[0], full[0][:3])
    assert bad[0].size < 3 and good[2] > bad[2]


def test_grouping_symbols_are_declared_and_exported():
    """Fails before grouped search exists: the header declares and the library exports the five entry points."""
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    assert hasattr(clb, "PassageGrouping")
    header = " ".join(open(clb._lib.HEADER).read().replace("*", " ").split())       # comment text, line breaks folded
    assert "NON-DECREASING in pid" in header and "grouping made before an append; make another" in header


def test_grouping_entry_points_check_their_arguments_first():
    """Null handles and null outputs are ArgumentError (4) before any device work; counting a null grouping is 0,
    destroying one is fine.  Without a GPU no searcher handle can exist (its constructor is HipError, no CPU fallback), so
    that is as far as a grouped call can get on such a machine."""
    l = clb.lib()
    i64 = C.c_int64
    null, out = C.c_void_p(), C.c_void_p(0xdead0)
    ids = np.array([0, 0, 1], np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert l.clb_grouping_create(null, p(ids), i64(3), C.byref(out)) == 4
    assert b"null" in l.clb_last_error() and out.value is None           # a failed create leaves no handle
    assert l.clb_grouping_create(null, p(ids), i64(3), None) == 4
    assert l.clb_grouping_create(null, None, i64(-1), C.byref(out)) == 4
    assert l.clb_grouping_count(null) == 0
    assert l.clb_grouping_destroy(null) == 0
    q = np.zeros((128, 32, 1), np.float32, order="F")
    op, os_, nc = np.zeros(5, np.int64), np.zeros(5, np.float32), np.zeros(1, np.int64)
    assert l.clb_search_batch_grouped(null, p(q), i64(32), i64(1), i64(2), i64(5), None, 0, null, 1, p(op), p(os_), p(nc)) == 4
    assert l.clb_search_batch_grouped_device_slot(null, 0, None, i64(32), i64(1), i64(2), i64(5), None, 0, null, None, None, None,
                                                  None) == 4
    if l.clb_device_count() == 0:
        idx = synthetic.make_index(0, 20, K=8)
        with pytest.raises(clb.HipError):                      # CLB_EHIP: nothing is grouped, ranked or collapsed on the host
            clb.Searcher(index=idx).make_grouping(group_lens=[20])


class _NoDevice(Searcher):
    """The host side of a Searcher without its handle: enough for the checks that run before the library is called."""

    def __init__(self, num_docs=100, dim=128):
        self.num_docs, self.dim, self._h, self.pid_offset = num_docs, dim, None, 1000
        self.config = clb.ColBERTConfig()


def test_python_keywords_are_validated_on_the_host():
    s = _NoDevice()
    with pytest.raises(clb.ColBERTError, match="exactly one"):
        s.make_grouping()
    with pytest.raises(clb.ColBERTError, match="exactly one"):
        s.make_grouping(group_ids=np.zeros(100, np.int64), group_lens=[100])
    with pytest.raises(clb.ColBERTError, match="summing to num_docs"):
        s.make_grouping(group_lens=[50, 49])
    with pytest.raises(clb.ColBERTError, match="summing to num_docs"):
        s.make_grouping(group_lens=[101, -1])
    with pytest.raises(clb.ColBERTError, match="integers"):
        s.make_grouping(group_ids=np.zeros(100, np.float32))
    g = clb.PassageGrouping(s, None, 2, ids_from_lens([60, 40]) * 10)       # closed: no handle
    assert g.count == 2 and len(g) == 2
    assert np.array_equal(g.groups_of([1001, 1060, 1061, 1100]), [0, 0, 10, 10])
    with pytest.raises(clb.BoundsError):
        g.groups_of([0])                                       # the padding of a short result is no passage
    with pytest.raises(clb.BoundsError):
        g.groups_of([1101])
    Q = np.zeros((128, 4), np.float32)
    for call in (lambda: s.search_batch(Q[:, :, None], 5, grouping=g), lambda: s.search_embeddings(Q, 5, grouping=g),
                 lambda: clb.search(s, Q, 5, grouping=g), lambda: s.search_batch(Q[:, :, None], 5, grouping="docs")):
        with pytest.raises(clb.ColBERTError, match="open PassageGrouping"):
            call()
    with g:                                                    # a context manager; closing a closed grouping is fine
        pass
    g.close()
