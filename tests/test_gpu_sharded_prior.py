"""Score priors across a shard group on the GPU: `ShardedSearcher.search_batch(prior=, prior_weight=)` over 2 and 4 shards (all
on device 0) under both exchange protocols against the reference with a prior on the UNSHARDED index (tests/util_prior: the
oracle's full ranking, every score boosted with two separately rounded fp32 operations, ranked again by (E, pid)) and against
the unsharded `Searcher`.  Bar: pids and candidate counts identical, fp32 scores bit-identical, short results padded with
pid 0 / -Inf.  Corpus of tests/test_gpu_sharded_searcher.py.  The threshold kernel of phase 2 is also driven alone, on crafted
input, against numpy."""
import os
import sys
import tempfile

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests.test_gpu_append import head_index
from tests.test_gpu_filtered_search import assert_result, assert_same_f32
from tests.test_gpu_sharded_grouped import big_group_ids, cuts_of, numpy_group_tau, straddling_ids
from tests.test_gpu_sharded_searcher import assert_same_results, boundary_pids
from tests.test_remove_cpu import reduced_index
from tests.test_update_cpu import updated_index
from tests.util_filter import filtered_ranking
from tests.util_group import collapse
from tests.util_prior import boosted_ranking, prior_ranking
from tests.util_synth import tiny_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NPROBE = 2
PROTOCOLS = ("two_phase", "single")
WORLDS = (2, 4)
KS = (10, 100, 700)
N = 6000


def normal_values(n=N, seed=31):
    return np.random.default_rng(seed).normal(0, 0.5, n).astype(np.float32)


@pytest.fixture(scope="module")
def corpus(oracle):
    idx = synthetic.make_index(seed=141, n_docs=N, K=512)
    Qs = synthetic.make_queries(idx, 142, 6)
    Qs.setflags(write=False)
    full = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(Qs.shape[2])]      # unfiltered, every candidate
    # the reference the issue names, once: it is the boosted re-ranking of `full` that the cases below share
    v = normal_values()
    want = prior_ranking(oracle, idx, Qs[:, :, 0], NPROBE, v, -2.0)
    mine = boosted_ranking(full[0], v, -2.0)
    assert np.array_equal(want[0], mine[0]) and np.array_equal(want[1].view(np.int32), mine[1].view(np.int32))
    return idx, Qs, full


@pytest.fixture(scope="module")
def groups(corpus):
    g = {w: clb.ShardedSearcher.from_index(corpus[0], w) for w in WORLDS}
    yield g
    for x in g.values():
        x.close()


@pytest.fixture(scope="module")
def single(corpus):
    s = clb.Searcher(index=corpus[0])
    yield s
    s.close()


def check_prior(g, p, Qs, rankings, k, what, weight=1.0, filters=None, scope="candidates", grouping=None, protocols=PROTOCOLS):
    """search_batch with a prior under every protocol against one ranking per query; returns the last result"""
    out = None
    for proto in protocols:
        out = g.search_batch(Qs, k, NPROBE, pad_short=True, filters=filters, scope=scope, protocol=proto, grouping=grouping,
                             prior=p, prior_weight=weight)
        ps, s, n = out
        assert ps.shape == s.shape == (k, Qs.shape[2]) and ps.dtype == np.int64 and s.dtype == np.float32
        for j in range(Qs.shape[2]):
            assert_result(ps[:, j], s[:, j], n[j], rankings[j], k, f"{what} protocol={proto} q={j}")
            if grouping is not None:
                kk = min(k, int(n[j]))
                assert np.unique(grouping.groups_of(ps[:kk, j])).size == kk, f"{what} protocol={proto} q={j}: a group twice"
    return out


def shard_of(g, pids):
    bounds = np.array([r.start for r in g.shard_ranges] + [g.shard_ranges[-1].stop])
    return np.searchsorted(bounds, np.asarray(pids), side="right") - 1


# ---- 1. ordinary priors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_ordinary_priors_against_the_reference_and_the_single_handle(corpus, groups, single, world):
    idx, Qs, full = corpus
    g = groups[world]
    values = normal_values()
    with g.make_prior(values) as p, single.make_prior(values) as ps:
        assert len(p) == N and len(p.parts) == world and p.max_abs == float(np.abs(values).max())
        for weight in (1.0, -2.0):
            rankings = [boosted_ranking(r, values, weight) for r in full]
            for k in KS:
                got = check_prior(g, p, Qs, rankings, k, f"normal w={weight} world={world} k={k}", weight=weight)
                ref = single.search_batch(Qs, k, NPROBE, pad_short=True, prior=ps, prior_weight=weight)
                assert_same_results(got, ref, f"against the unsharded Searcher w={weight} k={k}")
        for proto in PROTOCOLS + ("auto",):      # weight 0: the call without a prior, bit for bit
            a = g.search_batch(Qs, 100, NPROBE, pad_short=True, protocol=proto, prior=p, prior_weight=0.0)
            b = g.search_batch(Qs, 100, NPROBE, pad_short=True, protocol=proto)
            assert_same_results(a, b, f"weight 0 against no prior, {proto}")
        pp, sp = g.search_embeddings(Qs[:, :, 3], 100, NPROBE, prior=p, prior_weight=-2.0)
        assert_result(pp, sp, g.last_num_candidates, boosted_ranking(full[3], values, -2.0), 100, "search_embeddings")
        pc, sc = clb.search(g, Qs[:, :, 3], 100, prior=p, prior_weight=-2.0)
        assert np.array_equal(pc, pp) and np.array_equal(sc.view(np.int32), sp.view(np.int32))


# ---- 2. one-sided priors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", (1.0, -1.0))
@pytest.mark.parametrize("world", WORLDS)
def test_one_sided_priors_move_the_threshold(corpus, groups, world, sign):
    """+c on the last shard's passages: the top 100 lies wholly there although the ranking without a prior draws from several
    shards; -c: none of it lies there.  A threshold formed from unboosted scores cuts these results away."""
    idx, Qs, full = corpus
    g = groups[world]
    last = g.shard_ranges[-1]
    c = np.float32(max(float(r[1].max() - r[1].min()) for r in full) + 1.0)
    values = np.zeros(N, np.float32)
    values[last.start - 1:last.stop - 1] = sign * c
    rankings = [boosted_ranking(r, values) for r in full]
    for r, plain in zip(rankings, full):          # from the reference alone
        on_last = shard_of(g, r[0][:100]) == world - 1
        assert on_last.all() if sign > 0 else not on_last.any()
        assert np.unique(shard_of(g, plain[0][:100])).size >= 2
        if sign < 0:
            assert (shard_of(g, plain[0][:100]) == world - 1).any()
    with g.make_prior(values) as p:
        for k in KS:
            check_prior(g, p, Qs, rankings, k, f"one-sided {sign:+} world={world} k={k}")


# ---- 3. large values with exact ties ----------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_large_values_with_exact_ties_are_ordered_by_global_pid(corpus, groups, single, world):
    idx, Qs, full = corpus
    g = groups[world]
    values = np.where(np.random.default_rng(7).random(N) < 0.5, np.float32(2.0 ** 20), np.float32(0.0)).astype(np.float32)
    rankings = [boosted_ranking(r, values) for r in full]
    crossing = 0
    for rp, rs in rankings:
        top = rs[:700]
        assert np.all(top >= 2.0 ** 20) and np.all(top * 8 == np.round(top * 8))            # a grid of 1/8
        sh = shard_of(g, rp[:700])
        for v in np.unique(top):
            run = np.nonzero(top == v)[0]
            if run.size > 1:
                assert np.all(np.diff(rp[run]) > 0)            # the reference orders a run by pid
                crossing += np.unique(sh[run]).size > 1
    assert crossing >= 10                                      # runs of equal E whose pids lie on different shards
    with g.make_prior(values) as p, single.make_prior(values) as ps:
        for k in KS:
            got = check_prior(g, p, Qs, rankings, k, f"ties world={world} k={k}")
            assert_same_results(got, single.search_batch(Qs, k, NPROBE, pad_short=True, prior=ps), f"ties against Searcher k={k}")


# ---- 4. filters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("world", WORLDS)
def test_filters_compose_in_both_scopes(oracle, corpus, groups, world, scope):
    idx, Qs, full = corpus
    g = groups[world]
    values = normal_values()
    allowed = np.union1d(np.nonzero(np.random.default_rng(5).random(N) < 0.5)[0] + 1, boundary_pids(g))
    filtered = [prior_ranking(oracle, idx, Qs[:, :, j], NPROBE, values, 1.5, allowed, scope) for j in range(Qs.shape[2])]
    plain = [boosted_ranking(r, values, 1.5) for r in full]
    with g.make_prior(values) as p, g.make_filter(pids=allowed) as f:
        check_prior(g, p, Qs, filtered, 100, f"filtered world={world} {scope}", weight=1.5, filters=f, scope=scope)
        mixed = [f, None, f, None, None, f]
        want = [filtered[j] if mixed[j] is not None else plain[j] for j in range(6)]
        check_prior(g, p, Qs, want, 100, f"per-query world={world} {scope}", weight=1.5, filters=mixed, scope=scope)


# ---- 5. groupings -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_groupings_compose_and_straddle_the_cuts(oracle, corpus, groups, single, world):
    idx, Qs, full = corpus
    g = groups[world]
    values = normal_values()
    both = sorted(set(cuts_of(groups[2]) + cuts_of(groups[4])))
    allowed = np.union1d(np.nonzero(np.random.default_rng(6).random(N) < 0.5)[0] + 1, boundary_pids(g))
    with g.make_prior(values) as p, single.make_prior(values) as ps:
        for name, ids in (("straddling", straddling_ids(both)), ("one_big_group", big_group_ids())):
            rankings = [collapse(boosted_ranking(r, values, -2.0), ids) for r in full]
            with g.make_grouping(group_ids=ids) as gr, single.make_grouping(group_ids=ids) as gs:
                for k in KS:
                    got = check_prior(g, p, Qs, rankings, k, f"{name} world={world} k={k}", weight=-2.0, grouping=gr)
                    ref = single.search_batch(Qs, k, NPROBE, pad_short=True, grouping=gs, prior=ps, prior_weight=-2.0)
                    assert_same_results(got, ref, f"{name} against the unsharded Searcher k={k}")
                if name == "straddling":            # ... and with a filter
                    with g.make_filter(pids=allowed) as f:
                        fr = [prior_ranking(oracle, idx, Qs[:, :, j], NPROBE, values, 1.0, allowed, "candidates", ids)
                              for j in range(Qs.shape[2])]
                        check_prior(g, p, Qs, fr, 100, f"{name} filtered world={world}", filters=f, grouping=gr)
                    with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
                        g.search_batch(Qs, 10, NPROBE, grouping=gr, per_group=2, prior=p)


# ---- 6. short results -------------------------------------------------------------------------------------------------
def test_short_results_are_padded_or_raise(corpus, groups):
    idx, Qs, full = corpus
    g = groups[4]
    values = normal_values()
    rankings = [boosted_ranking(r, values) for r in full]
    few = min(r[0].size for r in full)
    with g.make_prior(values) as p:
        check_prior(g, p, Qs, rankings, few + 1, "short")
        for proto in PROTOCOLS:
            with pytest.raises(clb.BoundsError) as with_prior:
                g.search_batch(Qs, few + 1, NPROBE, protocol=proto, prior=p)
            with pytest.raises(clb.BoundsError) as without:
                g.search_batch(Qs, few + 1, NPROBE, protocol=proto)
            assert str(with_prior.value) == str(without.value) and "fewer than k" in str(without.value)


def sparse_corpus(oracle):
    """300 passages in 256 short lists, queries of two tokens and nprobe 1: 7 to 25 candidates per query"""
    idx, _ = tiny_index(seed=3, K=256, doclen_mean=2, doclen_std=1)
    Qs = synthetic.make_queries(idx, 1003, 6, T=2)
    return idx, Qs, [filtered_ranking(oracle, idx, Qs[:, :, j], 1) for j in range(6)]


def test_a_shard_without_candidates(oracle):
    idx, Qs, full = sparse_corpus(oracle)
    values = normal_values(300, 9)
    rankings = [boosted_ranking(r, values, 3.0) for r in full]
    with clb.ShardedSearcher.from_index(idx, 4) as g:
        empty = [(j, i) for j, r in enumerate(full) for i in range(4) if not (shard_of(g, r[0]) == i).any()]
        assert empty and all(r[0].size > 0 for r in full)      # from the reference: some shard has no candidate for some query
        ids = np.arange(300, dtype=np.int64) // 3
        with g.make_prior(values) as p, g.make_grouping(group_ids=ids) as gr:
            for k in (1, 5, 40):
                for proto in PROTOCOLS:
                    out = g.search_batch(Qs, k, 1, pad_short=True, protocol=proto, prior=p, prior_weight=3.0)
                    for j in range(6):
                        assert_result(out[0][:, j], out[1][:, j], out[2][j], rankings[j], k, f"sparse {proto} k={k} q={j}")
                    out = g.search_batch(Qs, k, 1, pad_short=True, protocol=proto, prior=p, prior_weight=3.0, grouping=gr)
                    for j in range(6):
                        assert_result(out[0][:, j], out[1][:, j], out[2][j], collapse(rankings[j], ids), k,
                                      f"sparse grouped {proto} k={k} q={j}")


# ---- 7. a batch above one piece ---------------------------------------------------------------------------------------
def test_batch_of_seventy_runs_in_pieces(corpus, groups):
    idx, Qs, full = corpus
    g = groups[4]
    values = normal_values()
    B, k, nq = 70, 20, Qs.shape[2]
    Qb = np.asfortranarray(np.concatenate([Qs] * 12, axis=2)[:, :, :B])
    rankings = [boosted_ranking(r, values) for r in full]
    ids = straddling_ids(sorted(set(cuts_of(groups[2]) + cuts_of(groups[4]))))
    with g.make_prior(values) as p, g.make_grouping(group_ids=ids) as gr:
        for proto in PROTOCOLS:
            ps, s, n = g.search_batch(Qb, k, NPROBE, protocol=proto, prior=p)
            for b in range(B):
                assert_result(ps[:, b], s[:, b], n[b], rankings[b % nq], k, f"B=70 {proto} q={b}")
        ps, s, n = g.search_batch(Qb, k, NPROBE, protocol="two_phase", prior=p, grouping=gr)
        for b in range(B):
            assert_result(ps[:, b], s[:, b], n[b], collapse(rankings[b % nq], ids), k, f"B=70 grouped q={b}")


# ---- 8. index changes -------------------------------------------------------------------------------------------------
def test_a_prior_survives_remove_and_update_but_not_an_append(oracle):
    full_idx, _ = tiny_index(seed=4, n_docs=330)
    idx = head_index(full_idx, 300)
    Qs = synthetic.make_queries(idx, 1004, 6)
    values = normal_values(300, 10)
    before = [filtered_ranking(oracle, idx, Qs[:, :, j], NPROBE) for j in range(6)]
    with clb.ShardedSearcher.from_index(idx, 4) as g:
        p = g.make_prior(values)
        check_prior(g, p, Qs, [boosted_ranking(r, values) for r in before], 10, "before")
        removed = np.unique(np.concatenate([boosted_ranking(before[0], values)[0][:3], boundary_pids(g)]))
        assert g.remove_passages(removed) == removed.size
        red, _ = reduced_index(idx, removed)
        rankings = [prior_ranking(oracle, red, Qs[:, :, j], NPROBE, values) for j in range(6)]
        for k in (10, 100):
            check_prior(g, p, Qs, rankings, k, f"after remove k={k}")
        embs, dl = synthetic.make_embeddings(11, 8)
        co, re = oracle.compress(idx["centroids"], idx["bucket_cutoffs"], 128, 2, embs)
        pids = np.array([300, 1, 75, 76, 150, 151, 225, 226])
        assert g.update_embeddings(pids, embs, dl) == 8
        want = updated_index(red, pids, co, re, dl)
        rankings = [prior_ranking(oracle, want, Qs[:, :, j], NPROBE, values) for j in range(6)]
        for k in (10, 100):
            check_prior(g, p, Qs, rankings, k, f"after update k={k}")
        embs2, dl2 = synthetic.make_embeddings(12, 30)
        assert g.add_embeddings(embs2, dl2) == range(301, 331)
        for proto in PROTOCOLS:
            with pytest.raises(clb.ArgumentError, match="prior made before an append; make another"):
                g.search_batch(Qs, 10, NPROBE, protocol=proto, prior=p)
        # the library's own check, on the shard that grew
        import torch
        from colbert_jl_amd.distributed import DeviceSearch
        run = DeviceSearch(g.shards[-1], Qs.shape[1], Qs.shape[2], 10, NPROBE)
        Qd = torch.from_numpy(np.array(Qs.transpose(2, 1, 0), order="C")).to(run.dev)
        with pytest.raises(clb.ArgumentError, match="prior made before an append; make another"):
            run.phase1(Qd, prior=p.parts[-1], prior_weight=1.0)
        p.close()
        with pytest.raises(clb.ColBERTError, match="open ShardedPrior"):
            g.search_batch(Qs, 10, NPROBE, prior=p)
        with g.make_prior(np.concatenate([values, np.ones(30, np.float32)])) as p2:
            g.search_batch(Qs, 10, NPROBE, pad_short=True, prior=p2)


# ---- 9. errors --------------------------------------------------------------------------------------------------------
def test_host_refusals(corpus, groups):
    idx, Qs, full = corpus
    g, other = groups[2], groups[4]
    with pytest.raises(clb.ArgumentError, match="one value per passage"):
        g.make_prior(np.zeros(N - 1))
    second = g.shard_ranges[1].start + 10
    v = np.zeros(N)
    v[second - 1] = np.nan
    with pytest.raises(clb.ArgumentError, match=f"passage {second} is not a finite number"):
        g.make_prior(v)
    v = np.zeros(N, np.float32)
    v[0], v[N - 1] = 1.0, 4.0                                  # the first shard alone would take the weight below
    with g.make_prior(v) as p, other.make_prior(v) as theirs:
        assert p.parts[0].max_abs == 1.0 and p.max_abs == 4.0
        with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
            g.search_batch(Qs, 10, NPROBE, prior=p, prior_weight=1e38)
        with pytest.raises(clb.ColBERTError, match="ShardedPrior of this shard group"):
            g.search_batch(Qs, 10, NPROBE, prior=theirs)
        with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
            g.search_batch(Qs, 10, NPROBE, prior=p, per_group=2)
        with pytest.raises(clb.Unsupported, match="after="):
            g.search_batch(Qs, 10, NPROBE, prior=p, after=(np.zeros(6, np.float32), np.zeros(6, np.int64)))
        for s in g.shards:
            s.set_mode(0)
        try:
            with pytest.raises(clb.Unsupported, match="two-pass mode"):
                g.search_batch(Qs, 10, NPROBE, protocol="two_phase", prior=p)
            rankings = [boosted_ranking(r, v) for r in full]      # ... and the single exchange serves mode 0
            check_prior(g, p, Qs, rankings, 10, "mode 0", protocols=("single", "auto"))
        finally:
            for s in g.shards:
                s.set_mode(1)


def test_argument_contracts_of_the_phase_calls(corpus, groups):
    import torch
    _, Qs, _ = corpus
    l = clb.lib()
    g = groups[2]
    s0, s1 = g.shards
    T, B, k = Qs.shape[1], Qs.shape[2], 10
    dev = torch.device("cuda", s0.device)
    Qd = torch.from_numpy(np.array(Qs.transpose(2, 1, 0), order="C")).to(dev)
    top = torch.empty((B, k), dtype=torch.float32, device=dev)
    gid = torch.full((B, k), -5, dtype=torch.int64, device=dev)
    mabs = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    out = torch.zeros((B, k), dtype=torch.int64, device=dev)
    sc = torch.zeros((B, k), dtype=torch.float32, device=dev)
    n = torch.zeros(B, dtype=torch.int64, device=dev)
    with g.make_prior(normal_values()) as pr:
        h0, h1 = pr.parts[0]._h, pr.parts[1]._h

        def p1(s, h, w=1.0, t=top.data_ptr(), m=mabs.data_ptr()):
            return l.clb_search_shard_phase1_prior_slot(s._h, 0, Qd.data_ptr(), T, B, NPROBE, k, None, 0, None, 0, h, w, t, None, m, None)

        def p2(h, w=1.0, o=out.data_ptr(), m=mabs.data_ptr()):
            return l.clb_search_shard_phase2_prior_slot(s0._h, 0, Qd.data_ptr(), T, B, NPROBE, k, top.data_ptr(), None, m, 1, None, 0,
                                                        h, w, o, sc.data_ptr(), None, n.data_ptr(), None, None)

        assert p1(s0, h1) == clb.ArgumentError.code and b"another searcher" in l.clb_last_error()
        assert p1(s0, h0, 1.0, None) == clb.ArgumentError.code and b"d_local_top" in l.clb_last_error()
        assert p1(s0, h0, 1.0, top.data_ptr(), None) == clb.ArgumentError.code and b"d_local_mabs" in l.clb_last_error()
        assert p1(s0, h0, float("nan")) == clb.ArgumentError.code and b"prior_weight must be finite" in l.clb_last_error()
        assert p1(s0, h0, 3e38) == clb.ArgumentError.code and b"not below FLT_MAX" in l.clb_last_error()
        # prior == NULL: the grouped phase 1 (here without a grouping: the filtered one), d_local_mabs untouched
        assert p1(s0, None) == 0
        torch.cuda.synchronize()
        assert torch.all(mabs == -7.0)
        plain = top.clone()
        assert l.clb_search_shard_phase1_grouped_slot(s0._h, 0, Qd.data_ptr(), T, B, NPROBE, k, None, 0, None, 0, top.data_ptr(),
                                                      gid.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(plain.sort(dim=1).values.view(torch.int32), top.sort(dim=1).values.view(torch.int32))
        assert torch.all(gid == -5)
        # phase 2 must follow the prior phase 1 with the same prior and weight
        assert p2(h0) == clb.ArgumentError.code and b"without a matching" in l.clb_last_error()         # phase 1 had no prior
        assert p2(None) == clb.ArgumentError.code and b"prior is null" in l.clb_last_error()
        assert p1(s0, h0, 0.5) == 0
        assert p2(h0, 0.25) == clb.ArgumentError.code and b"without a matching" in l.clb_last_error()   # another weight
        with s0.make_prior(np.zeros(s0.num_docs, np.float32)) as another:
            assert p2(another._h, 0.5) == clb.ArgumentError.code and b"without a matching" in l.clb_last_error()
        assert p2(h0, 0.5, None) == clb.ArgumentError.code and b"null" in l.clb_last_error()
        assert p2(h0, 0.5, out.data_ptr(), None) == clb.ArgumentError.code and b"d_all_mabs" in l.clb_last_error()
        assert l.clb_search_shard_phase2_slot(s0._h, 0, Qd.data_ptr(), T, B, NPROBE, k, top.data_ptr(), 1, out.data_ptr(),
                                              sc.data_ptr(), n.data_ptr(), None) == clb.ArgumentError.code      # prior phase 1 pending
        torch.cuda.synchronize()
        assert torch.all(mabs >= 0) and torch.all(mabs >= top.abs().max(dim=1).values)      # M_i covers what was published
        assert p2(h0, 0.5) == 0
        torch.cuda.synchronize()
        assert torch.all(out > 0) and torch.all(n > k)
        assert p2(h0, 0.5) == clb.ArgumentError.code                                        # phase 1 is used up


# ---- 10. the threshold kernel alone -----------------------------------------------------------------------------------
def numpy_prior_tau(top, gid, mabs, eps, k):
    """tau_in[B] of prior_global_tau_kernel in fp32 steps: fl(tau - fl(2 * fl(4 u * fl(M + eps)))), -inf when that is not
    above -inf (fewer than k, a non-finite M or eps)"""
    S, B, _ = top.shape
    if gid is None:
        tau = np.full(B, -np.inf, np.float32)
        for b in range(B):
            v = np.sort(top[:, b].reshape(-1))[::-1]
            tau[b] = v[k - 1]
    else:
        tau = numpy_group_tau(top, gid, k)
    out = np.full(B, -np.inf, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        M = np.max(np.abs(mabs), axis=0).astype(np.float32)
        M = np.where(np.isnan(mabs).any(axis=0), np.float32(np.nan), M)
        delta = np.float32(4.0) * np.float32(2.0 ** -24) * (M + eps.astype(np.float32))
        t = tau - np.float32(2.0) * delta
    ok = t > -np.inf
    out[ok] = t[ok]
    return out


def device_prior_tau(top, gid, mabs, eps):
    import torch
    S, B, k = top.shape
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    t, m, e = up(top, np.float32), up(mabs, np.float32), up(eps, np.float32)
    gd = None if gid is None else up(gid, np.int64)
    tau = torch.full((B,), 123.0, dtype=torch.float32, device=dev)
    clb._lib.check(clb.lib().clb_debug_prior_tau_device(t.data_ptr(), None if gd is None else gd.data_ptr(), m.data_ptr(),
                                                        e.data_ptr(), S, B, k, tau.data_ptr(), None))
    torch.cuda.synchronize()
    return tau.cpu().numpy()


def test_prior_tau_on_crafted_records():
    inf = np.inf
    f = lambda a: np.array(a, np.float32)
    cases = []
    # -inf padding, k = 3 of 4 finite entries
    cases.append((f([[[5, 4, -inf]], [[4.5, -inf, -inf]]]), None, f([[5], [4.5]]), f([0.25])))
    # fewer than k finite entries -> -inf
    cases.append((f([[[5, -inf, -inf]], [[4.5, -inf, -inf]]]), None, f([[5], [4.5]]), f([0.25])))
    # a repeated group index on two lists counts once, with its larger value
    cases.append((f([[[5, 4, 1]], [[2, 6, 3]]]), np.array([[[10, 11, 12]], [[12, 13, 14]]], np.int64), f([[5], [6]]), f([0.125])))
    # ... which leaves fewer than k distinct groups
    cases.append((f([[[5, 4, -inf]], [[4.5, -inf, -inf]]]), np.array([[[7, 8, -1]], [[8, -1, -1]]], np.int64), f([[5], [4.5]]), f([0.0])))
    # one shard with M = 2^20 beside one with M = 1: delta comes from the maximum, whichever list holds it
    big = f([[[2 ** 20 + 3, 2 ** 20 + 1]], [[1.0, 0.5]]])
    cases.append((big, None, f([[2 ** 20 + 3], [1.0]]), f([0.01])))
    cases.append((big[::-1].copy(), None, f([[1.0], [2 ** 20 + 3]]), f([0.01])))
    # M = Inf, M = NaN, eps = Inf: everything is listed
    cases.append((f([[[5, 4]], [[3, 2]]]), None, f([[5], [inf]]), f([0.25])))
    cases.append((f([[[5, 4]], [[3, 2]]]), None, f([[np.nan], [3]]), f([0.25])))
    cases.append((f([[[5, 4]], [[3, 2]]]), None, f([[5], [3]]), f([inf])))
    # negative scores, two queries with different M and eps
    cases.append((f([[[-1, -2], [7, 6]], [[-1.5, -3], [6.5, 1]]]), None, f([[3, 7], [2 ** 10, 6.5]]), f([0.5, 0.001])))
    for top, gid, mabs, eps in cases:
        k = top.shape[2]
        got, want = device_prior_tau(top, gid, mabs, eps), numpy_prior_tau(top, gid, mabs, eps, k)
        assert_same_f32(got, want, f"tau_in of {top.tolist()} M={mabs.tolist()} eps={eps.tolist()}")
    want = [numpy_prior_tau(t, g_, m, e, t.shape[2]) for t, g_, m, e in cases]
    assert want[0][0] == np.float32(4.0) - np.float32(2.0) * (np.float32(2.0 ** -22) * np.float32(5.25)) and np.isneginf(want[1][0])
    assert want[2][0] < 4.0 and want[2][0] > 3.99 and np.isneginf(want[3][0])               # distinct: {10: 5, 11: 4, 12: 2, 13: 6, 14: 3}
    assert want[4][0] == want[5][0] and float(2 ** 20 + 1) - float(want[4][0]) >= 0.5       # 8 * 2^-24 * 2^20 = 0.5: not M = 1's slack
    assert all(np.isneginf(w[0]) for w in want[6:9])
    # random records, several queries per call; n_shards * k above and below one pass of 1024 threads
    rng = np.random.default_rng(4)
    for S, B, k in ((2, 5, 7), (3, 4, 33), (4, 3, 1000), (8, 2, 300), (1, 3, 50), (6, 4, 1), (300, 2, 5)):
        top = (rng.integers(-64, 65, (S, B, k)).astype(np.float32) / 8) * rng.choice([1.0, 1024.0], (S, B, 1)).astype(np.float32)
        top[rng.random((S, B, k)) < 0.2] = -np.inf
        mabs = np.abs(np.where(np.isinf(top), 0, top)).max(axis=2) + rng.random((S, B)).astype(np.float32)
        eps = rng.random(B).astype(np.float32)
        assert_same_f32(device_prior_tau(top, None, mabs, eps), numpy_prior_tau(top, None, mabs, eps, k), f"random S={S} B={B} k={k}")


# ---- 11. the cut is a cut ---------------------------------------------------------------------------------------------
def rescored_and_candidates(g, Qs, k, **kw):
    """(re-scored passages, candidate passages) summed over the shards and the queries, from the shards' work counters"""
    _, _, n = g.search_batch(Qs, k, NPROBE, pad_short=True, protocol="two_phase", **kw)
    st = [s.last_batch_stats() for s in g.shards]
    assert sum(x["cand_docs"] for x in st) == int(n.sum())
    return sum(x["rescored_docs"] for x in st), int(n.sum())


@pytest.mark.parametrize("world", WORLDS)
def test_the_boosted_threshold_still_cuts(corpus, world):
    idx, Qs, full = corpus
    with clb.ShardedSearcher.from_index(idx, world) as g:
        for s in g.shards:
            s.profile_enable(True, counters=True)
        resc, cand = rescored_and_candidates(g, Qs, 10)
        print(f"world={world} without a prior: rescored {resc} of {cand} candidate passages")
        assert cand == sum(r[0].size for r in full) and 10 * Qs.shape[2] <= resc < cand      # the precondition
        with g.make_prior(normal_values()) as p:
            resc_p, cand_p = rescored_and_candidates(g, Qs, 10, prior=p)
            print(f"world={world} with the N(0, 0.5) prior: rescored {resc_p} of {cand_p} candidate passages")
            assert cand_p == cand and 10 * Qs.shape[2] <= resc_p < cand


# ---- 12. two rank processes over gloo ---------------------------------------------------------------------------------
K_RANKS = 100
CHILD_TIMEOUT = 240          # seconds a rank process may take (a few in practice: it builds its shard and searches four times)


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
    values = normal_values()                           # every rank passes the same array
    out = {}
    with g.make_prior(values) as p:
        out["max_abs"], out["own_max_abs"] = p.max_abs, p.parts[0].max_abs
        for proto in PROTOCOLS:
            for weight in (1.0, -2.0):
                out[proto, weight] = g.search_batch(Qs, K_RANKS, NPROBE, pad_short=True, protocol=proto, prior=p, prior_weight=weight)
    q.put((rank, out))
    dist.barrier()
    g.close()
    dist.destroy_process_group()


def test_two_rank_processes_with_a_prior(corpus):
    import queue

    import torch.multiprocessing as mp
    idx, Qs, full = corpus
    world = 2
    store = tempfile.NamedTemporaryFile(prefix="clb_pg_", delete=False); store.close(); os.unlink(store.name)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, store.name, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            rank, out = q.get(timeout=CHILD_TIMEOUT)
            res[rank] = out
    except queue.Empty:
        pass
    for p in procs:                                     # every child under its own limit; nothing is started after a failure
        p.join(timeout=CHILD_TIMEOUT if len(res) == world else 1)
        if p.is_alive():
            p.kill()
            p.join()
    assert [p.exitcode for p in procs] == [0] * world and sorted(res) == list(range(world))
    values = normal_values()
    for r in range(world):                              # identical on every rank
        out = res[r]
        assert out["max_abs"] == float(np.abs(values).max()) and out["own_max_abs"] <= out["max_abs"]
        for proto in PROTOCOLS:
            for weight in (1.0, -2.0):
                ps, s, n = out[proto, weight]
                for j in range(Qs.shape[2]):
                    assert_result(ps[:, j], s[:, j], n[j], boosted_ranking(full[j], values, weight), K_RANKS,
                                  f"rank={r} {proto} w={weight} q={j}")
    assert res[0]["own_max_abs"] != res[1]["own_max_abs"]      # the group's maximum had to be gathered
