"""Composing filters on the device, on the GPU: set algebra (`&`, `|`, `-`, `~`, `combine_filters`), attribute ranges over a
resident prior (`make_range_filter`), carrying a filter over an append (`extended`) and the read-back (`to_mask`,
clb_filter_bitmap).  Every expected bitmap is numpy's on the host -- np.packbits(mask, bitorder="little") as little-endian u32
words, zero-padded to ceil(n_docs / 32) -- and every expected search result is the search of the same handle with
`make_filter(mask=` the host-composed mask `)`: pids, score bits and candidate counts identical."""
import ctypes as C
from contextlib import closing

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import sharded, synthetic
from tests.test_gpu_append import head_index, tail
from tests.test_gpu_sharded_searcher import assert_same_results
from tests.util_synth import tiny_index

pytestmark = pytest.mark.gpu

NPROBE = 2
# a lone partial word, an odd number of words for the two-word store of the range kernel, the 256-lane block edge (255..257),
# the 256-word block edge (8191..8193), many blocks with a ragged end
EDGE_SIZES = (1, 31, 32, 33, 63, 64, 65, 95, 255, 256, 257, 8191, 8192, 8193, 65_573)
DENSITIES = (0.0, 0.03, 0.5, 1.0)
FLT_MAX = np.finfo(np.float32).max
SUBNORMAL = np.float32(np.finfo(np.float32).smallest_subnormal)


# ---- the reference: numpy on the host ---------------------------------------------------------------------------------
def words_of(mask):
    w = np.packbits(np.asarray(mask, bool), bitorder="little")
    return np.concatenate([w, np.zeros(-w.size % 4, np.uint8)]).view("<u4")


def raw_words(f):
    """the words of a filter straight from clb_filter_bitmap"""
    words = np.full((f.num_docs + 31) // 32, 0xdeadbeef, dtype="<u4")
    clb._lib.check(clb.lib().clb_filter_bitmap(f._h, words.ctypes.data_as(C.c_void_p), C.c_int64(words.size)))
    return words


def check_filter(f, mask, what):
    mask = np.asarray(mask, bool)
    assert f.count == int(mask.sum()) and len(f) == f.count, (what, f.count, int(mask.sum()))
    got = f.to_mask()
    assert got.dtype == np.bool_ and got.shape == mask.shape, what
    assert np.array_equal(got, mask), (what, np.nonzero(got != mask)[0][:8])
    assert np.array_equal(raw_words(f), words_of(mask)), what          # the tail bits of the last word included


def random_mask(n, density, seed):
    return np.random.default_rng([seed, n]).random(n) < density


def small_index(n_docs, seed=7):
    """n_docs passages of 8 embeddings each: what a filter is sized by is the passage count alone"""
    return synthetic.make_index(seed, n_docs, K=64, doclen_mean=8, constant_doclen=True, topical=False)


def in_range(v, lo, hi, lo_open, hi_open):
    lo, hi = np.float32(-np.inf if lo is None else lo), np.float32(np.inf if hi is None else hi)
    return (v > lo if lo_open else v >= lo) & (v < hi if hi_open else v <= hi)


def same_search(s, Qs, k, got, ref, scope, what):
    a = s.search_batch(Qs, k, NPROBE, filters=got, scope=scope)
    b = s.search_batch(Qs, k, NPROBE, filters=ref, scope=scope)
    assert_same_results(a, b, what)
    return a


# ---- word and block edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", EDGE_SIZES)
def test_set_algebra_and_ranges_at_word_and_block_edges(n_docs):
    with closing(clb.Searcher(index=small_index(n_docs))) as s:
        assert s.num_docs == n_docs
        W = (n_docs + 31) // 32
        cases = [(d, d, d) for d in DENSITIES] + [(0.5, 0.03, 1.0)]
        for ci, (da, db, dc) in enumerate(cases):
            ma, mb, mc = random_mask(n_docs, da, 10 + ci), random_mask(n_docs, db, 20 + ci), random_mask(n_docs, dc, 30 + ci)
            what = f"n_docs={n_docs} densities={da, db, dc}"
            with s.make_filter(mask=ma) as a, s.make_filter(mask=mb) as b, s.make_filter(mask=mc) as c:
                before = raw_words(a)
                made = [(a & b, ma & mb, "a & b"), (a | b, ma | mb, "a | b"), (a - b, ma & ~mb, "a - b"), (b - a, mb & ~ma, "b - a"),
                        (~a, ~ma, "~a"),
                        (s.combine_filters("and", [a, b, c]), ma & mb & mc, "and [a b c]"),
                        (s.combine_filters("or", [a, b, c]), ma | mb | mc, "or [a b c]"),
                        (s.combine_filters("andnot", [a, b, c]), ma & ~(mb | mc), "andnot [a b c]"),
                        (s.combine_filters("and", [a]), ma, "and [a]"), (s.combine_filters("or", [a]), ma, "or [a]"),
                        (s.combine_filters("andnot", [a]), ma, "andnot [a]"), (s.combine_filters("not", [a]), ~ma, "not [a]"),
                        # the same handle more than once in one call
                        (s.combine_filters("and", [a, a]), ma, "and [a a]"), (s.combine_filters("andnot", [a, a]), ma & False, "andnot [a a]"),
                        (s.combine_filters("andnot", [a, b, b, c, b]), ma & ~(mb | mc), "andnot [a b b c b]")]
                for f, want, name in made:
                    assert isinstance(f, clb.PassageFilter) and f is not a and f.num_docs == n_docs
                    check_filter(f, want, f"{what}: {name}")
                # ~a sets the bits past n_docs in its kernel; the finished filter has none: the last word itself
                inv = raw_words(made[4][0])
                assert inv.size == W
                if n_docs % 32:
                    assert int(inv[-1]) >> (n_docs % 32) == 0, (what, hex(int(inv[-1])))
                    assert int(inv[-1]) == int(words_of(~ma)[-1])
                for f, _, _ in made:
                    f.close()
                assert np.array_equal(raw_words(a), before), what          # operands are only read
        # the range kernel at the same sizes: values on a few levels, so that every bound meets ties
        v = np.random.default_rng([40, n_docs]).integers(-2, 3, n_docs).astype(np.float32) * np.float32(0.5)
        with s.make_prior(v) as p:
            for lo, hi, lo_open, hi_open in ((None, None, False, False), (-0.5, 0.5, False, False), (-0.5, 0.5, True, True),
                                             (0.0, None, True, False), (None, 0.0, False, True), (1.0, 1.0, False, False),
                                             (0.5, -0.5, False, False)):
                with s.make_range_filter(p, lo, hi, lo_open, hi_open) as r:
                    check_filter(r, in_range(v, lo, hi, lo_open, hi_open), f"n_docs={n_docs} range {lo, hi, lo_open, hi_open}")


def test_sixteen_operands_work_and_seventeen_are_refused():
    n = 8193
    with closing(clb.Searcher(index=small_index(n))) as s:
        masks = [random_mask(n, 0.05, 50 + i) for i in range(17)]
        filters = [s.make_filter(mask=m) for m in masks]
        try:
            with s.combine_filters("or", filters[:16]) as f:
                check_filter(f, np.any(masks[:16], axis=0), "or of 16")
            with s.combine_filters("and", filters[:16]) as f:
                check_filter(f, np.all(masks[:16], axis=0), "and of 16")
            with s.combine_filters("andnot", filters[1:17]) as f:
                check_filter(f, masks[1] & ~np.any(masks[2:17], axis=0), "andnot of 16")
            with pytest.raises(clb.ArgumentError, match="1..16"):
                s.combine_filters("or", filters)
            arr, out = (C.c_void_p * 17)(*[f._h.value for f in filters]), C.c_void_p(0xdead0)
            assert clb.lib().clb_filter_combine(s._h, 1, arr, C.c_int64(17), C.byref(out)) == 4 and out.value is None
            assert b"n must be 1..16" in clb.lib().clb_last_error()
        finally:
            for f in filters:
                f.close()


# ---- ranges -----------------------------------------------------------------------------------------------------------
def range_values(n=300):
    v = np.random.default_rng(11).normal(0, 1, n).astype(np.float32)
    v[0:8] = [0.0, -0.0, FLT_MAX, -FLT_MAX, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny, SUBNORMAL, -SUBNORMAL]
    v[10:14], v[14:16], v[16] = 0.5, -1.0, np.nextafter(np.float32(0.5), np.float32(1))      # exact ties at the bounds, one ulp off
    v[60:71] = 0.25                                    # a run of equal values across the wave edge at 64
    v[255:258] = [0.5, -0.0, 0.25]                     # ... and ties on both sides of the block edge
    return v


BOUNDS = (-np.inf, -FLT_MAX, -1.0, -0.0, 0.0, float(SUBNORMAL), 0.25, 0.5, float(FLT_MAX), np.inf)


@pytest.mark.parametrize("device_prior", (False, True))
def test_ranges_equal_numpy_on_the_float32_values(device_prior):
    idx, _ = tiny_index(seed=2)
    v = range_values()
    with closing(clb.Searcher(index=idx)) as s:
        if device_prior:                               # a prior made through clb_prior_create_device
            import torch
            t = torch.from_numpy(v).to(torch.device("cuda", s.device))
            p = s.make_prior(t)
        else:
            p = s.make_prior(v)
        with p:
            empty = 0
            for lo in BOUNDS:
                for hi in BOUNDS:
                    for lo_open in (False, True):
                        for hi_open in (False, True):
                            want = in_range(v, lo, hi, lo_open, hi_open)
                            empty += not want.any()
                            with s.make_range_filter(p, lo, hi, lo_open, hi_open) as r:
                                check_filter(r, want, f"range {lo, hi, lo_open, hi_open}")
            assert empty > 100                         # lo > hi, and lo == hi with an open end, among them
            # what the cases above contain, spelled out on the reference
            assert in_range(v, 0.0, 0.0, False, False).sum() == 3 and in_range(v, -0.0, -0.0, False, False)[[0, 1, 256]].all()
            assert not in_range(v, 0.5, 0.5, True, False).any() and in_range(v, 0.5, 0.5, False, False).sum() == 5
            assert in_range(v, 0.25, 0.25, False, False)[60:71].all()
            assert in_range(v, -np.inf, np.inf, True, True).all()              # infinite bounds are open ends: open or closed
            for lo, hi, kw in ((None, None, {}), (None, 0.5, {}), (0.25, None, dict(lo_open=True)), (np.float64(0.25), 1, {})):
                with s.make_range_filter(p, lo, hi, **kw) as r:
                    check_filter(r, in_range(v, lo, hi, kw.get("lo_open", False), False), f"range {lo, hi, kw}")
            # several values: the OR of equalities
            eq = [s.make_range_filter(p, x, x) for x in (0.25, 0.5, -1.0)]
            with s.combine_filters("or", eq) as r:
                check_filter(r, np.isin(v, np.float32([0.25, 0.5, -1.0])), "isin")
            for f in eq:
                f.close()
            with pytest.raises(clb.ArgumentError, match="lo must be a real number"):
                s.make_range_filter(p, float("nan"), 1.0)
            out = C.c_void_p(0xdead0)
            assert clb.lib().clb_filter_create_range(s._h, p._h, 0.0, float("nan"), 0, C.byref(out)) == 4 and out.value is None
            assert b"hi is NaN" in clb.lib().clb_last_error()


# ---- use in search ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medium():
    """the 20 000-passage, K = 2048 fixture of tests/test_gpu_filtered_search.py; predicates a, an attribute and c"""
    idx = synthetic.make_index(seed=3, n_docs=20_000, K=2048)
    Qs = synthetic.make_queries(idx, 4, 3)
    rng = np.random.default_rng(77)
    ma, mc = rng.random(20_000) < 0.5, rng.random(20_000) < 0.1
    values = rng.uniform(0, 1, 20_000).astype(np.float32)
    host = ma & in_range(values, 0.3, 0.9, False, True) & ~mc
    for x in (Qs, ma, mc, values, host):
        x.setflags(write=False)
    return idx, Qs, ma, mc, values, host


@pytest.fixture(scope="module")
def medium_handle(medium):
    idx, Qs, ma, mc, values, host = medium
    s = clb.Searcher(index=idx)
    default_mode = s.mode
    with s.make_filter(mask=ma) as a, s.make_filter(mask=mc) as c, s.make_prior(values) as p:
        with s.make_range_filter(p, 0.3, 0.9, hi_open=True) as r, (a & r) as ar:
            composed = ar - c
    ref = s.make_filter(mask=host)                     # the operands, the prior and the temporaries are closed by now
    yield s, composed, ref
    s.set_mode(default_mode)
    composed.close(), ref.close(), s.close()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("scope", ("candidates", "all"))
def test_a_composed_filter_searches_as_the_uploaded_mask(medium, medium_handle, scope, mode):
    idx, Qs, ma, mc, values, host = medium
    s, composed, ref = medium_handle
    check_filter(composed, host, "(a & range) - c")
    s.set_mode(mode)
    assert s.mode == mode
    for k in (10, 1000):
        got = same_search(s, Qs, k, composed, ref, scope, f"scope={scope} mode={mode} k={k}")
        assert got[2].min() > 0 and (got[0][0] > 0).all()
        assert host[got[0][got[0] > 0] - 1].all()      # every returned passage satisfies the host predicate
    # inside a mixed batch: unfiltered queries beside filtered ones
    Qb = np.asfortranarray(Qs[:, :, [0, 1, 2, 0, 1]])
    same_search(s, Qb, 100, [composed, None, composed, None, composed], [ref, None, ref, None, ref], scope,
                f"mixed batch scope={scope} mode={mode}")
    p, sc = s.search_embeddings(Qs[:, :, 1], 100, NPROBE, filter=composed, scope=scope)
    n = s.last_num_candidates
    rp, rs = s.search_embeddings(Qs[:, :, 1], 100, NPROBE, filter=ref, scope=scope)
    assert np.array_equal(p, rp) and np.array_equal(sc.view(np.int32), rs.view(np.int32)) and n == s.last_num_candidates


def test_a_composed_filter_across_two_shards_under_both_protocols(medium, medium_handle):
    idx, Qs, ma, mc, values, host = medium
    s, _, ref = medium_handle
    s.set_mode(1)
    with clb.ShardedSearcher.from_index(idx, 2) as g:
        with g.make_filter(mask=ma) as a, g.make_filter(mask=mc) as c, g.make_prior(values) as p:
            with g.make_range_filter(p, 0.3, 0.9, hi_open=True) as r, (a & r) as ar:
                composed = ar - c
                check_filter_parts(g, r, in_range(values, 0.3, 0.9, False, True))
        with composed, g.make_filter(mask=host) as gref:
            assert isinstance(composed, sharded.ShardedFilter) and composed.count == int(host.sum()) == gref.count
            assert np.array_equal(composed.to_mask(), host) and len(composed.parts) == 2
            for proto in ("two_phase", "single"):
                for scope in ("candidates", "all"):
                    what = f"2 shards protocol={proto} scope={scope}"
                    got = g.search_batch(Qs, 100, NPROBE, pad_short=True, filters=composed, scope=scope, protocol=proto)
                    same = g.search_batch(Qs, 100, NPROBE, pad_short=True, filters=gref, scope=scope, protocol=proto)
                    assert_same_results(got, same, what + " against the group's uploaded mask")
                    single = s.search_batch(Qs, 100, NPROBE, filters=ref, scope=scope)
                    assert_same_results(got, single, what + " against the unsharded handle")
            with g.combine_filters("not", [composed]) as inv, (inv | gref) as everything:
                assert inv.count == 20_000 - int(host.sum()) and np.array_equal(inv.to_mask(), ~host)
                assert everything.count == 20_000
            with clb.ShardedSearcher.from_index(tiny_index()[0], 2) as other, other.make_filter(mask=np.ones(300, bool)) as foreign:
                with pytest.raises(clb.ColBERTError, match=r"filters\[1\] is not a ShardedFilter of this shard group"):
                    composed & foreign


def check_filter_parts(g, f, mask):
    """a ShardedFilter of a one-process group: count, mask and every part against its slice of the host mask"""
    assert f.count == int(mask.sum()) and np.array_equal(f.to_mask(), mask)
    for part, r in zip(f.parts, g.shard_ranges):
        check_filter(part, mask[r.start - 1:r.stop - 1], f"part {r}")


# ---- lifetime ---------------------------------------------------------------------------------------------------------
def test_results_outlive_their_operands_and_survive_removals_and_updates():
    idx, _ = tiny_index(seed=5)
    Qs = synthetic.make_queries(idx, 6, 3)
    n = 300
    ma, mb = random_mask(n, 0.5, 1), random_mask(n, 0.6, 2)
    v = np.random.default_rng(3).uniform(0, 1, n).astype(np.float32)
    with closing(clb.Searcher(index=idx)) as s:
        a, b, p = s.make_filter(mask=ma), s.make_filter(mask=mb), s.make_prior(v)
        wa, wb = raw_words(a), raw_words(b)
        both, rng_f = a & b, s.make_range_filter(p, 0.2, None, lo_open=True)
        # operands stay usable and unchanged after the call
        assert np.array_equal(raw_words(a), wa) and np.array_equal(raw_words(b), wb) and a.count == int(ma.sum())
        with s.make_filter(mask=ma) as a2:
            same_search(s, Qs, 50, a, a2, "all", "an operand after the call")
        a.close(), b.close(), p.close()
        want_both, want_rng = ma & mb, v > np.float32(0.2)
        check_filter(both, want_both, "a & b after closing a and b")
        check_filter(rng_f, want_rng, "a range after closing its prior")
        with (both | rng_f) as u, s.make_filter(mask=want_both | want_rng) as ref:
            for scope in ("candidates", "all"):
                same_search(s, Qs, 50, u, ref, scope, f"after closing every operand, scope={scope}")
        # a composed filter stays valid over a removal and an update: n_docs does not change
        s.remove_passages(np.array([2, 3, 64, 65, 299]))
        s.update_compressed(np.array([10, 130]), *tail(idx, 290, 292))
        check_filter(both, want_both, "a & b after remove and update")
        with s.make_filter(mask=want_both) as ref, (~both) as inv:
            check_filter(inv, ~want_both, "~(a & b) after remove and update")
            for scope in ("candidates", "all"):
                got = same_search(s, Qs, 50, both, ref, scope, f"after remove and update, scope={scope}")
                assert not np.isin(got[0], [2, 3, 64, 65, 299]).any()
        both.close(), rng_f.close()


# ---- append -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("old,new", [(33, 64), (33, 70), (33, 300), (64, 65), (64, 96), (64, 300)])
def test_extended_carries_a_filter_over_an_append(old, new):
    """old n_docs 33 (inside a word) and 64 (at a word's end); the append stays in the word, crosses one, crosses several"""
    idx, _ = tiny_index(seed=6)
    Qs = synthetic.make_queries(idx, 7, 3)
    m = random_mask(old, 0.5, old + new)
    v = np.linspace(0, 1, old).astype(np.float32)
    stale_filter, stale_prior = "filter made before an append; make another", "prior made before an append; make another"
    with closing(clb.Searcher(index=head_index(idx, old))) as s:
        f, p = s.make_filter(mask=m), s.make_prior(v)
        with f.extended() as copy, f.extended(True) as copy1:          # of a current filter: a copy
            check_filter(copy, m, "extended of a current filter")
            check_filter(copy1, m, "extended(True) of a current filter")
            assert copy is not f and copy._h.value != f._h.value
        s.add_compressed(*tail(idx, old, new))
        assert s.num_docs == new and f.num_docs == old
        for call in (lambda: f & f, lambda: ~f, lambda: s.combine_filters("or", [f]),
                     lambda: s.search_batch(Qs, 10, NPROBE, filters=f), lambda: s.search_embeddings(Qs[:, :, 0], 10, NPROBE, filter=f)):
            with pytest.raises(clb.ArgumentError, match=stale_filter):
                call()
        with pytest.raises(clb.ArgumentError, match=stale_prior):
            s.make_range_filter(p, 0.0, 1.0)
        with s.make_filter(mask=np.ones(new, bool)) as fresh:
            with pytest.raises(clb.ArgumentError, match="operand 1: " + stale_filter):
                fresh & f
        check_filter(f, m, "the stale filter still reads back")
        pad0, pad1 = np.concatenate([m, np.zeros(new - old, bool)]), np.concatenate([m, np.ones(new - old, bool)])
        with f.extended(False) as e0, f.extended(True) as e1, s.make_filter(mask=pad0) as r0, s.make_filter(mask=pad1) as r1:
            assert e0.num_docs == e1.num_docs == new
            check_filter(e0, pad0, f"{old} -> {new} extended(False)")
            check_filter(e1, pad1, f"{old} -> {new} extended(True)")
            for scope in ("candidates", "all"):
                same_search(s, Qs, 20, e0, r0, scope, f"{old} -> {new} fill 0 scope={scope}")
                same_search(s, Qs, 20, e1, r1, scope, f"{old} -> {new} fill 1 scope={scope}")
            with (e1 - e0) as added:                                    # the results compose like any filter
                check_filter(added, np.arange(new) >= old, "the appended passages")
        with pytest.raises(clb.ArgumentError, match=stale_filter):     # f itself stays refused
            s.search_batch(Qs, 10, NPROBE, filters=f)
        f.close(), p.close()


# ---- refusals on a live searcher --------------------------------------------------------------------------------------
def test_refusals_on_a_live_searcher():
    idx, _ = tiny_index(seed=8)
    with closing(clb.Searcher(index=idx)) as s, closing(clb.Searcher(index=idx)) as other:
        m = random_mask(300, 0.5, 9)
        a, b, fo = s.make_filter(mask=m), s.make_filter(mask=~m), other.make_filter(mask=m)
        p, po = s.make_prior(np.zeros(300, np.float32)), other.make_prior(np.zeros(300, np.float32))
        l, out = clb.lib(), C.c_void_p(0xdead0)
        try:
            with pytest.raises(clb.ArgumentError, match="the filter of operand 1 was made for another searcher"):
                s.combine_filters("and", [a, fo])
            with pytest.raises(clb.ArgumentError, match="the filter of operand 0 was made for another searcher"):
                s.combine_filters("not", [fo])
            with pytest.raises(clb.ArgumentError, match="the prior was made for another searcher"):
                s.make_range_filter(po, 0.0, 1.0)
            assert l.clb_filter_extend(s._h, fo._h, 0, C.byref(out)) == 4 and out.value is None
            assert b"made for another searcher" in l.clb_last_error()
            # NOT with two operands: on the host, and by the library itself
            with pytest.raises(clb.ArgumentError, match="'not' takes exactly one"):
                s.combine_filters("not", [a, b])
            arr, out = (C.c_void_p * 2)(a._h.value, b._h.value), C.c_void_p(0xdead0)
            assert l.clb_filter_combine(s._h, 3, arr, C.c_int64(2), C.byref(out)) == 4 and out.value is None
            assert b"CLB_FILTER_OP_NOT takes n = 1" in l.clb_last_error()
            words = np.zeros(20, "<u4")
            for n_words in (9, 11, 0):                 # 300 passages: 10 words
                assert l.clb_filter_bitmap(a._h, words.ctypes.data_as(C.c_void_p), C.c_int64(n_words)) == 4
                assert b"n_words" in l.clb_last_error()
            assert l.clb_filter_bitmap(a._h, None, C.c_int64(10)) == 4 and b"words is null" in l.clb_last_error()
            # closed handles
            b.close(), p.close()
            for call in (lambda: a & b, lambda: b | a, lambda: ~b, lambda: s.combine_filters("or", [a, a, b])):
                with pytest.raises(clb.ColBERTError, match="is not an open PassageFilter"):
                    call()
            with pytest.raises(clb.ColBERTError, match="not an open PassageFilter"):
                b.to_mask()
            with pytest.raises(clb.ColBERTError, match="not an open PassageFilter"):
                b.extended()
            with pytest.raises(clb.ColBERTError, match="open PassagePrior"):
                s.make_range_filter(p, 0.0, 1.0)
            check_filter(a, m, "a after the refusals")
        finally:
            for x in (a, b, fo, p, po):
                x.close()
    # a filter outlives its searcher: it still reads back
    s2 = clb.Searcher(index=idx)
    f = ~s2.make_filter(mask=m)
    s2.close()
    check_filter(f, ~m, "after the searcher is gone")
    f.close()
