"""Filtered search on the GPU against the composed oracle (tests/util_filter.py: the oracle's own retrieve -> gather ->
decompress -> maxsim -> stable sort with the filter applied to the candidate list).  Bar: the project's own -- pids and
candidate counts exact, fp32 scores bit-identical, short results padded with pid 0 / -Inf."""
import ctypes as C
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from tests.util_filter import filtered_ranking, first_k

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_f32(a, b, what=""):
    a = np.asarray(a, dtype=np.float32); b = np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(bits(a), bits(b)):
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        raise AssertionError(f"{what}: {np.count_nonzero(bits(a) != bits(b))} of {a.size} differ, max |d| = {diff.max()}")


def assert_result(got_p, got_s, got_n, ranking, k, what, pid_offset=0):
    """One query's (pids[k], scores[k], n_cand) against the first k of `ranking`, padding included."""
    rp, rs, rn = first_k(ranking, k, pid_offset)
    assert int(got_n) == rn, (what, int(got_n), rn)
    assert np.array_equal(np.asarray(got_p), rp), (what, np.nonzero(np.asarray(got_p) != rp)[0][:5])
    assert_same_f32(got_s, rs, what)
    kk = min(k, rn)
    assert np.all(np.asarray(got_p)[kk:] == 0) and np.all(np.isneginf(np.asarray(got_s)[kk:])), what


def random_allowed(n_docs, selectivity, seed):
    """1-based pids of a random subset of about selectivity * n_docs passages (1.0: every passage)."""
    if selectivity >= 1.0:
        return np.arange(1, n_docs + 1, dtype=np.int64)
    rng = np.random.default_rng(seed)
    return (np.nonzero(rng.random(n_docs) < selectivity)[0] + 1).astype(np.int64)


def check_filtered(oracle, s, idx, Qs, alloweds, scope, ks, nprobe=2, modes=(0, 1), pid_offset=0, batch=9):
    """The shape of check_search for one filter per query: `alloweds[j]` (local 1-based pids, or None) is query j's.
    Every mode -- exact, two-pass, two-pass with the other gather form (2), 8-bit score rows with either gather form
    (3 / 4: batches of 18) -- runs single queries (atomic marking) and a batch of `batch` (sliced marking from 8)."""
    nq = Qs.shape[2]
    rankings = [filtered_ranking(oracle, idx, Qs[:, :, j], nprobe, alloweds[j], scope) for j in range(nq)]
    filters = [None if a is None else s.make_filter(pids=np.asarray(a) + pid_offset) for a in alloweds]
    for f, a in zip(filters, alloweds):
        assert f is None or f.count == np.unique(a).size
    auto_form = s.pass1_gather[0]
    try:
        for mode in tuple(modes) + ((2, 3, 4) if 1 in modes else ()):
            if mode >= 1 and s.mode != 1:
                try:
                    s.set_mode(1)
                except clb.Unsupported:
                    continue
            s.set_mode(min(mode, 1))
            s.set_pass1_gather(-1 if mode not in (2, 4) else 1 - auto_form)
            rows8 = mode >= 3
            if rows8:
                try:
                    s.set_score_rows(1)
                except clb.Unsupported:
                    continue
            else:
                s.set_score_rows(0)
            nb = 18 if rows8 else batch
            Qb = np.asfortranarray(np.concatenate([Qs] * (-(-nb // nq)), axis=2)[:, :, :nb])
            fb = [filters[j % nq] for j in range(nb)]
            for k in ks:
                if not rows8:
                    for j in range(nq):
                        if filters[j] is None:      # an unfiltered query of the set (the plain single call raises on a short result)
                            p, sc, n = s.search_batch(Qs[:, :, j:j + 1], k, nprobe=nprobe, pad_short=True)
                            p, sc, n = p[:, 0], sc[:, 0], n[0]
                        else:
                            p, sc = s.search_embeddings(Qs[:, :, j], k, nprobe=nprobe, filter=filters[j], scope=scope)
                            n = s.last_num_candidates
                        assert_result(p, sc, n, rankings[j], k, f"single scope={scope} mode={mode} k={k} q={j}", pid_offset)
                bp, bs, bn = s.search_batch(Qb, k, nprobe=nprobe, filters=fb, scope=scope)
                for j in range(nb):
                    assert_result(bp[:, j], bs[:, j], bn[j], rankings[j % nq], k, f"batch scope={scope} mode={mode} k={k} q={j}",
                                  pid_offset)
            s.set_score_rows(0)
    finally:
        s.set_score_rows(0)
        s.set_pass1_gather(-1)
        for f in filters:
            if f is not None:
                f.close()


@pytest.fixture(scope="module")
def medium():
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    return idx, synthetic.make_queries(idx, 4, 3)


@pytest.mark.parametrize("scope", ["candidates", "all"])
@pytest.mark.parametrize("selectivity", [1.0, 0.5, 0.05, 0.002])
def test_filtered_search_both_scopes_modes_and_score_forms(oracle, medium, scope, selectivity):
    """20 000 passages, k = 1000 and 10, selectivity 1.0 ... 0.002, both scopes, exact / two-pass / other gather form /
    8-bit score rows.  An all-ones filter in scope "candidates" must give the unfiltered oracle.search result."""
    idx, Qs = medium
    n_docs = idx["doclens"].size
    alloweds = [random_allowed(n_docs, selectivity, 900 + j) for j in range(3)]
    s = clb.Searcher(index=idx)
    try:
        check_filtered(oracle, s, idx, Qs, alloweds, scope, ks=(1000, 10))
        if selectivity == 1.0 and scope == "candidates":
            with s.make_filter(mask=np.ones(n_docs, bool)) as f:
                for j in range(3):
                    rp, rs, rn = oracle.search(idx, Qs[:, :, j], nprobe=2, k=1000)
                    p, sc = s.search_embeddings(Qs[:, :, j], 1000, filter=f)
                    assert s.last_num_candidates == rn and np.array_equal(p, rp)
                    assert_same_f32(sc, rs, "all-ones filter")
    finally:
        s.close()


def test_empty_and_disjoint_filters(oracle, medium):
    """An empty filter and one that shares no passage with the candidates: n_cand = 0, all padding, no error -- single
    query and batch, both scopes and modes."""
    idx, Qs = medium
    n_docs = idx["doclens"].size
    cands = [oracle.retrieve(idx["ivf"], idx["ivf_lengths"], idx["centroids"], oracle.build_emb2pid(idx["doclens"]), 2, Qs[:, :, j])
             for j in range(3)]
    outside = np.setdiff1d(np.arange(1, n_docs + 1), np.concatenate(cands))
    assert outside.size > 100
    s = clb.Searcher(index=idx)
    try:
        check_filtered(oracle, s, idx, Qs, [np.zeros(0, np.int64)] * 3, "candidates", ks=(10,), modes=(0, 1))
        check_filtered(oracle, s, idx, Qs, [np.zeros(0, np.int64)] * 3, "all", ks=(10,), modes=(0, 1))
        check_filtered(oracle, s, idx, Qs, [outside] * 3, "candidates", ks=(1000, 10), modes=(0, 1))
        with s.make_filter(pids=[]) as f:
            assert f.count == 0
            p, sc, n = s.search_batch(Qs, 7, filters=f)
            assert np.all(n == 0) and np.all(p == 0) and np.all(np.isneginf(sc))
    finally:
        s.close()


def test_per_query_filters_in_one_batch(oracle):
    """B = 9 with [f0, None, f1, f0, None, empty, f2, f1, None]: column j is the single-query result of (query j, filter j),
    the None columns are the unfiltered search -- both scopes, both modes."""
    idx = synthetic.make_index(seed=23, n_docs=6000, K=1024)
    Qs = synthetic.make_queries(idx, 31, 9)
    a = [random_allowed(6000, 0.5, 1), random_allowed(6000, 0.1, 2), random_allowed(6000, 0.01, 3), np.zeros(0, np.int64)]
    order = [0, None, 1, 0, None, 3, 2, 1, None]
    s = clb.Searcher(index=idx)
    f = [s.make_filter(pids=x) for x in a]
    k = 100
    try:
        for scope in ("candidates", "all"):
            for mode in (0, 1):
                s.set_mode(mode)
                fb = [None if o is None else f[o] for o in order]
                bp, bs, bn = s.search_batch(Qs, k, filters=fb, scope=scope)
                for j, o in enumerate(order):
                    what = f"scope={scope} mode={mode} q={j}"
                    if o is None:
                        rp, rs, rn = oracle.search(idx, Qs[:, :, j], nprobe=2, k=k)
                        assert bn[j] == rn and np.array_equal(bp[:, j], rp), what
                        assert_same_f32(bs[:, j], rs, what)
                        continue
                    p1, s1 = s.search_embeddings(Qs[:, :, j], k, filter=f[o], scope=scope)
                    assert bn[j] == s.last_num_candidates and np.array_equal(bp[:, j], p1), what
                    assert_same_f32(bs[:, j], s1, what)
                    assert_result(bp[:, j], bs[:, j], bn[j], filtered_ranking(oracle, idx, Qs[:, :, j], 2, a[o], scope), k, what)
    finally:
        for x in f:
            x.close()
        s.close()


@pytest.mark.parametrize("n_docs", [131071, 131073, 262145])
def test_filter_at_bitmap_slice_boundaries(oracle, n_docs):
    """Corpora that end one passage before / after a marking slice of 131 072 passages: filters holding only the first and
    last passage of every slice and the last passage of the index (scope "all": exactly those are ranked), and the same
    passages on top of a random half (scope "candidates") -- a batch of 9 (sliced marking) and single queries (atomic)."""
    idx = synthetic.make_index(seed=n_docs, n_docs=n_docs, K=2048, doclen_mean=12.0, doclen_std=3.0)
    Qs = synthetic.make_topic_queries(idx["centroids"], seed=81, n_queries=9)
    edges = np.array(sorted({p for p in (1, 131072, 131073, 262144, 262145, n_docs - 1, n_docs) if 1 <= p <= n_docs}), np.int64)
    half = np.union1d(random_allowed(n_docs, 0.5, 5), edges)
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(pids=edges) as fe, s.make_filter(pids=half) as fh:
            assert fe.count == edges.size and fh.count == half.size
            for scope, f, allowed in (("all", fe, edges), ("candidates", fe, edges), ("candidates", fh, half)):
                bp, bs, bn = s.search_batch(Qs, 50, filters=f, scope=scope)
                for j in range(9):
                    r = filtered_ranking(oracle, idx, Qs[:, :, j], 2, allowed, scope)
                    assert_result(bp[:, j], bs[:, j], bn[j], r, 50, f"sliced {scope} q={j}")
                    if j < 2:
                        p1, s1 = s.search_embeddings(Qs[:, :, j], 50, filter=f, scope=scope)
                        assert_result(p1, s1, s.last_num_candidates, r, 50, f"atomic {scope} q={j}")
        # the last word of the bitmap: bits past n_docs in a caller's bitmap are cleared, not trusted
        W = (n_docs + 31) // 32
        words = np.zeros(W, np.uint32)
        words[-1] = 0xFFFFFFFF
        h = C.c_void_p()
        clb._lib.check(clb.lib().clb_filter_create_bitmap(s._h, words.ctypes.data_as(C.c_void_p), C.c_int64(W), C.byref(h)))
        assert clb.lib().clb_filter_count(h) == n_docs - 32 * (W - 1)
        assert clb.lib().clb_filter_destroy(h) == 0
    finally:
        s.close()


def test_filtered_marking_large_shard(oracle):
    """2.2 M passages, more than 16 slices: the batch marks behind slice_bounds_kernel.  A random half in scope "candidates",
    a caller's list of 2 000 passages in scope "all"."""
    n_docs = 2_200_000
    idx = synthetic.make_index(seed=61, n_docs=n_docs, K=4096, doclen_mean=3, doclen_std=1)
    Qs = synthetic.make_queries(idx, 63, 8)
    half = random_allowed(n_docs, 0.5, 64)
    some = np.union1d(np.random.default_rng(65).integers(1, n_docs + 1, size=2000), [1, 524288, 524289, n_docs])
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(mask=np.isin(np.arange(1, n_docs + 1), half)) as fh, s.make_filter(pids=some) as fs:
            assert fh.count == half.size and fs.count == some.size
            for scope, f, allowed in (("candidates", fh, half), ("all", fs, some)):
                bp, bs, bn = s.search_batch(Qs, 100, filters=f, scope=scope)
                for j in (0, 3, 7):
                    assert_result(bp[:, j], bs[:, j], bn[j], filtered_ranking(oracle, idx, Qs[:, :, j], 2, allowed, scope), 100,
                                  f"large shard {scope} q={j}")
        bp, bs, bn = s.search_batch(Qs, 100)                  # ... and the handle still searches unfiltered
        rp, rs, rn = oracle.search(idx, Qs[:, :, 5], nprobe=2, k=100)
        assert bn[5] == rn and np.array_equal(bp[:, 5], rp)
        assert_same_f32(bs[:, 5], rs, "unfiltered after filtered")
    finally:
        s.close()


def test_filtered_search_with_wide_selection_and_sub_batches(oracle, medium):
    """Wide selection forced on (sixteen work-groups per query), and a call of 70 queries (sub-batches of 64 and 6) with a
    filter on two of every three queries."""
    idx, Qs3 = medium
    n_docs = idx["doclens"].size
    a = [random_allowed(n_docs, 0.5, 11), random_allowed(n_docs, 0.03, 12)]
    s = clb.Searcher(index=idx)
    try:
        s.set_wide_select(1)
        for scope in ("candidates", "all"):
            check_filtered(oracle, s, idx, Qs3, [a[0], a[1], a[0]], scope, ks=(1000, 10), modes=(1,))
        s.set_wide_select(-1)
        Qs = synthetic.make_queries(idx, 70, 70)
        f = [s.make_filter(pids=x) for x in a]
        fb = [None if j % 3 == 2 else f[j % 3] for j in range(70)]
        for scope in ("candidates", "all"):
            bp, bs, bn = s.search_batch(Qs, 200, filters=fb, scope=scope)
            for j in (0, 1, 2, 62, 63, 64, 65, 68, 69):
                allowed = None if j % 3 == 2 else a[j % 3]
                assert_result(bp[:, j], bs[:, j], bn[j], filtered_ranking(oracle, idx, Qs[:, :, j], 2, allowed, scope), 200,
                              f"B=70 {scope} q={j}")
        for x in f:
            x.close()
    finally:
        s.close()


@pytest.mark.parametrize("dim,nbits,T", [(64, 2, 20), (128, 8, 20), (128, 2, 150)])
def test_filtered_search_general_shapes(oracle, dim, nbits, T):
    """dim != 128 and nbits = 8 take the batched general path, T = 150 the per-query general path: both scopes."""
    if T > 128:
        idx = synthetic.make_index(seed=43, n_docs=6000, K=256, doclen_mean=24, doclen_std=6)
    else:
        idx = synthetic.make_index(seed=41 + dim + nbits, n_docs=900, K=96, dim=dim, nbits=nbits, doclen_mean=30, doclen_std=12)
    n_docs = idx["doclens"].size
    Qs = synthetic.make_queries(idx, 42, 3, T=T)
    alloweds = [random_allowed(n_docs, 0.4, 7), None, random_allowed(n_docs, 0.02, 8)]
    s = clb.Searcher(index=idx)
    try:
        for scope in ("candidates", "all"):
            check_filtered(oracle, s, idx, Qs, alloweds, scope, ks=(40,), modes=(0,), batch=3)
            check_filtered(oracle, s, idx, Qs, alloweds, scope, ks=(7,), nprobe=5, modes=(0,), batch=3)
    finally:
        s.close()


def test_scope_all_beyond_the_ivf_capacity(oracle):
    """Uniform codes, nprobe 1, a 2-token query: the T * nprobe longest lists hold far fewer passages than the filter, so
    the workspace has to grow for the filter's own count.  Afterwards the same handle searches unfiltered as ever."""
    idx = synthetic.make_index(seed=5, n_docs=5000, K=512, topical=False)
    Qs = synthetic.make_queries(idx, 6, 2, T=2)
    ivf_cap = int(np.sort(idx["ivf_lengths"])[-2:].sum())
    allowed = random_allowed(5000, 0.9, 9)
    assert allowed.size > 2 * ivf_cap
    s = clb.Searcher(index=idx)
    try:
        rp0, rs0, rn0 = oracle.search(idx, Qs[:, :, 0], nprobe=1, k=20)
        p, sc = s.search_embeddings(Qs[:, :, 0], 20, nprobe=1)          # sizes the workspace for the IVF bound first
        assert np.array_equal(p, rp0)
        with s.make_filter(pids=allowed) as f:
            for mode in (0, 1):
                s.set_mode(mode)
                for k in (4800, 50):
                    bp, bs, bn = s.search_batch(Qs, k, nprobe=1, filters=f, scope="all")
                    for j in range(2):
                        assert_result(bp[:, j], bs[:, j], bn[j], filtered_ranking(oracle, idx, Qs[:, :, j], 1, allowed, "all"), k,
                                      f"beyond capacity mode={mode} k={k} q={j}")
                p, sc = s.search_embeddings(Qs[:, :, 0], 20, nprobe=1)
                assert s.last_num_candidates == rn0 and np.array_equal(p, rp0), mode
                assert_same_f32(sc, rs0, "unfiltered after the workspace grew")
    finally:
        s.close()


def test_reuse_and_cleanliness(oracle, medium):
    """filtered / unfiltered / other filter / unfiltered ... on one handle and slot: every unfiltered result is the
    oracle's (a candidate bitmap not cleared, or a filter that scope "all" wrote to, would show), and the filters still
    hold their passages afterwards."""
    idx, Qs = medium
    n_docs = idx["doclens"].size
    a = [random_allowed(n_docs, 0.3, 21), random_allowed(n_docs, 0.01, 22)]
    Q9 = np.asfortranarray(np.concatenate([Qs] * 3, axis=2))
    refs = [oracle.search(idx, Qs[:, :, j], nprobe=2, k=100) for j in range(3)]
    s = clb.Searcher(index=idx)
    f = [s.make_filter(pids=x) for x in a]
    try:
        def unfiltered(what):
            for Q in (Qs, Q9):
                bp, bs, bn = s.search_batch(Q, 100)
                for j in range(Q.shape[2]):
                    rp, rs, rn = refs[j % 3]
                    assert bn[j] == rn and np.array_equal(bp[:, j], rp), what
                    assert_same_f32(bs[:, j], rs, what)
        for mode in (1, 0):
            s.set_mode(mode)
            for step, (fi, scope, Q) in enumerate([(0, "candidates", Q9), (1, "all", Q9), (0, "all", Qs), (1, "candidates", Qs),
                                                   (0, "all", Q9), (1, "all", Qs)]):
                bp, bs, bn = s.search_batch(Q, 100, filters=f[fi], scope=scope)
                r = filtered_ranking(oracle, idx, Q[:, :, 1], 2, a[fi], scope)
                assert_result(bp[:, 1], bs[:, 1], bn[1], r, 100, f"mode={mode} step={step}")
                unfiltered(f"unfiltered after step {step} mode={mode}")
        for x, fx in zip(a, f):
            assert fx.count == x.size == clb.lib().clb_filter_count(fx._h)
            with s.make_filter(pids=x) as again:              # ... and on the device: the same results as a fresh filter
                p1, s1, n1 = s.search_batch(Qs, 50, filters=fx, scope="all")
                p2, s2, n2 = s.search_batch(Qs, 50, filters=again, scope="all")
                assert np.array_equal(p1, p2) and np.array_equal(n1, n2) and np.array_equal(bits(s1), bits(s2))
    finally:
        for x in f:
            x.close()
        s.close()


def test_both_constructors_agree_and_pid_offset(oracle):
    """make_filter(pids=) and make_filter(mask=) of the same set give identical results; duplicate, unordered pids are
    accepted; with pid_offset = 1000 the pids go in and come out with the offset."""
    idx = synthetic.make_index(seed=1, n_docs=300, K=64)
    Qs = synthetic.make_queries(idx, 2, 3)
    off = 1000
    allowed = random_allowed(300, 0.4, 3)
    rng = np.random.default_rng(4)
    messy = rng.permutation(np.concatenate([allowed, allowed[:40], allowed[-7:]])) + off
    mask = np.zeros(300, bool)
    mask[allowed - 1] = True
    s = clb.Searcher(index=idx, pid_offset=off)
    try:
        with s.make_filter(pids=messy) as fp, s.make_filter(mask=mask) as fm:
            assert fp.count == fm.count == allowed.size
            for scope in ("candidates", "all"):
                a1 = s.search_batch(Qs, 30, filters=fp, scope=scope)
                a2 = s.search_batch(Qs, 30, filters=fm, scope=scope)
                assert np.array_equal(a1[0], a2[0]) and np.array_equal(a1[2], a2[2]) and np.array_equal(bits(a1[1]), bits(a2[1]))
                for j in range(3):
                    assert_result(a1[0][:, j], a1[1][:, j], a1[2][j], filtered_ranking(oracle, idx, Qs[:, :, j], 2, allowed, scope),
                                  30, f"pid_offset {scope} q={j}", pid_offset=off)
                    got = a1[0][:, j][a1[0][:, j] != 0]
                    assert np.all(np.isin(got, allowed + off))
        check_filtered(oracle, s, idx, Qs, [allowed] * 3, "candidates", ks=(10,), pid_offset=off)
        for bad in ([off], [off + 301], [1], [off + 5, -3]):      # local pids, or outside the shard: BoundsError
            with pytest.raises(clb.BoundsError):
                s.make_filter(pids=bad)
    finally:
        s.close()


def test_filter_contracts_on_a_live_searcher():
    """A wrong n_words, a bad scope and a filter of another searcher are ArgumentError; an out-of-range pid is BoundsError;
    a filter may be destroyed after its searcher."""
    l = clb.lib()
    i64 = C.c_int64
    idx = synthetic.make_index(seed=1, n_docs=300, K=64)
    Qs = synthetic.make_queries(idx, 2, 2)
    s, other = clb.Searcher(index=idx), clb.Searcher(index=idx)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    words = np.zeros(11, np.uint32)
    assert l.clb_filter_create_bitmap(s._h, p(words), i64(11), C.byref(h)) == 4           # ceil(300 / 32) = 10
    assert l.clb_filter_create_bitmap(s._h, p(words), i64(9), C.byref(h)) == 4
    assert l.clb_filter_create_bitmap(s._h, p(words), i64(10), None) == 4
    pid = np.array([5, 301], np.int64)
    assert l.clb_filter_create_pids(s._h, p(pid), i64(2), C.byref(h)) == 3 and h.value is None
    assert l.clb_filter_create_pids(s._h, p(pid), i64(2), None) == 4
    f, g = s.make_filter(pids=[3, 4, 5]), other.make_filter(pids=[3, 4, 5])
    q = np.asfortranarray(Qs)
    op, os_, nc = np.zeros((5, 2), np.int64, order="F"), np.zeros((5, 2), np.float32, order="F"), np.zeros(2, np.int64)
    hs = (C.c_void_p * 2)(f._h.value, None)
    args = lambda handles, scope: (s._h, p(q), i64(32), i64(2), i64(2), i64(5), handles, scope, p(op), p(os_), p(nc))
    assert l.clb_search_batch_filtered(*args(hs, 0)) == 0
    assert l.clb_search_batch_filtered(*args(hs, 2)) == 4 and b"scope" in l.clb_last_error()
    assert l.clb_search_batch_filtered(*args(hs, -1)) == 4
    assert l.clb_search_batch_filtered(*args((C.c_void_p * 2)(None, g._h.value), 0)) == 4
    assert b"another searcher" in l.clb_last_error()
    with pytest.raises(clb.ArgumentError):
        s.search_batch(Qs, 5, filters=g)
    with pytest.raises(clb.ColBERTError):
        s.search_batch(Qs, 5, filters=f, scope="some")
    assert l.clb_search_batch_filtered(*args(None, 1)) == 0                               # no array: nothing is filtered
    other.close()
    g.close()                                                                             # after its searcher: just frees
    f.close()
    s.close()


def test_captured_graph_replays_the_filtered_search(oracle):
    """The device-slot entry point captured as a HIP graph over a static query buffer, per-query filters included: every
    replay equals the direct call and the composed oracle."""
    import torch
    from colbert_jl_amd.distributed import DeviceSearch
    idx = synthetic.make_index(seed=23, n_docs=6000, K=1024)
    k = 60
    a = [random_allowed(6000, 0.5, 1), random_allowed(6000, 0.02, 2)]
    s = clb.Searcher(index=idx)
    f = [s.make_filter(pids=x) for x in a]
    try:
        for B, scope in ((1, "candidates"), (17, "candidates"), (17, "all")):
            Qs = synthetic.make_queries(idx, 31, 2 * B)
            Qdev = torch.from_numpy(np.ascontiguousarray(Qs.transpose(2, 1, 0))).cuda()
            run = DeviceSearch(s, 32, B, k, 2)
            order = [(j % 3) if j % 3 < 2 else None for j in range(B)]
            fb = [None if o is None else f[o] for o in order]
            q_static = Qdev[:B].clone()
            graph = run.capture(q_static, fb, scope)
            for it in range(2):
                q_static.copy_(Qdev[it * B:(it + 1) * B])
                graph.replay()
                torch.cuda.synchronize()
                gp, gs, gn = run.out_p.cpu().numpy().copy(), run.out_s.cpu().numpy().copy(), run.ncand.cpu().numpy().copy()
                run(Qdev[it * B:(it + 1) * B], fb, scope)
                torch.cuda.synchronize()
                assert np.array_equal(gp, run.out_p.cpu().numpy()) and np.array_equal(gn, run.ncand.cpu().numpy())
                assert np.array_equal(bits(gs), bits(run.out_s.cpu().numpy()))
                for j in range(0, B, 4):
                    allowed = None if order[j] is None else a[order[j]]
                    r = filtered_ranking(oracle, idx, Qs[:, :, it * B + j], 2, allowed, scope)
                    assert_result(gp[j], gs[j], gn[j], r, k, f"graph B={B} {scope} it={it} q={j}")
            del graph
    finally:
        for x in f:
            x.close()
        s.close()


def test_filtered_counts_reach_the_batch_stats(medium):
    """clb_last_batch_stats reports the candidates AFTER the filter; the time lands in the existing profile rows."""
    idx, Qs = medium
    s = clb.Searcher(index=idx)
    try:
        with s.make_filter(pids=random_allowed(20_000, 0.1, 5)) as f:
            s.profile_enable(True, counters=True)
            _, _, n = s.search_batch(Qs, 10, filters=f)
            assert s.last_batch_stats()["cand_docs"] == int(n.sum())
            _, _, n_all = s.search_batch(Qs, 10, filters=f, scope="all")
            assert np.all(n_all == f.count) and s.last_batch_stats()["cand_docs"] == 3 * f.count
            prof = s.profile_read()
            assert prof["mark_candidates"]["launches"] == 2 and prof["compact_candidates"]["launches"] == 2
            s.profile_enable(False)
    finally:
        s.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("COLBERT_TEST_FUZZ_SEEDS", "8"))))
def test_filtered_search_random_configurations(oracle, seed):
    """Randomly drawn shapes (corpus, centroids, nbits, passage lengths, query length, batch, k, nprobe, topical or uniform
    codes), selectivity and scope, a filter on most queries: pids, counts and padding exact, scores bit-identical."""
    rng = np.random.default_rng(9000 + seed)
    n_docs = int(rng.integers(40, 6000))
    K = int(2 ** rng.integers(3, 11))
    nbits = int(rng.choice([1, 2, 2, 2, 4]))
    idx = synthetic.make_index(seed=9100 + seed, n_docs=n_docs, K=K, nbits=nbits, doclen_mean=float(rng.integers(4, 120)),
                               doclen_std=float(rng.integers(0, 40)), topical=bool(rng.integers(0, 2)))
    T = int(rng.choice([1, 3, 17, 32, 32, 32, 33, 48]))
    nq = int(rng.integers(1, 10))
    Qs = synthetic.make_queries(idx, 9200 + seed, nq, T=T)
    k = int(min(n_docs, rng.choice([1, 10, 100, 1000, n_docs])))
    nprobe = int(min(K, rng.choice([1, 2, 2, 3, 8])))
    scope = str(rng.choice(["candidates", "all"]))
    alloweds = [None if rng.integers(0, 5) == 0 else random_allowed(n_docs, float(rng.choice([1.0, 0.5, 0.1, 0.01])), 9300 + 10 * seed + j)
                for j in range(nq)]
    s = clb.Searcher(index=idx)
    try:
        check_filtered(oracle, s, idx, Qs, alloweds, scope, ks=(k,), nprobe=nprobe, batch=max(nq, int(rng.choice([nq, 9]))))
    finally:
        s.close()
