"""The search request, the part that needs no GPU: the four entry points that take a clb_search_request are declared and
exported, every refusal that needs no searcher is answered on a NULL searcher -- on every route --, and the Python builder
(searcher.search_request) sets exactly the fields its keywords name and raises what the search methods have always raised."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd._lib import SearchRequest
from colbert_jl_amd.searcher import search_request
from tests.test_group_cpu import _NoDevice
from tests.test_prior_cpu import fake_prior
from tests.util_group import ids_from_lens

NEW_SYMBOLS = ("clb_search_batch_request", "clb_search_batch_request_device_slot", "clb_search_shard_phase1_request_slot",
               "clb_search_shard_phase2_request_slot")
SOME = 0xdead0                                     # a handle that is never dereferenced: the refusal comes first
EARGUMENT, EUNSUPPORTED = clb.ArgumentError.code, clb.Unsupported.code


def request(**fields):
    return SearchRequest(struct_bytes=C.sizeof(SearchRequest), **fields)


def routes():
    """name -> call(req) on a NULL searcher, B = 2 queries; req: a SearchRequest or None"""
    l = clb.lib()
    q = np.zeros((128, 32, 2), np.float32, order="F")
    op, os_, nc = np.zeros(64, np.int64), np.zeros(64, np.float32), np.zeros(2, np.int64)
    p = lambda a: a.ctypes.data
    return {
        "host": lambda r: l.clb_search_batch_request(None, p(q), 32, 2, 2, 2, r, p(op), p(os_), p(nc)),
        "device": lambda r: l.clb_search_batch_request_device_slot(None, 0, SOME, 32, 2, 2, 2, r, SOME, SOME, SOME, None),
        "phase1": lambda r: l.clb_search_shard_phase1_request_slot(None, 0, SOME, 32, 2, 2, 2, r, SOME, SOME, SOME, None),
        "phase2": lambda r: l.clb_search_shard_phase2_request_slot(None, 0, SOME, 32, 2, 2, 2, r, SOME, SOME, SOME, 1, SOME, SOME, SOME,
                                                                   SOME, SOME, None),
    }


def test_request_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    header = open(clb._lib.HEADER).read()
    assert "typedef struct clb_search_request {" in header and "} clb_search_request;" in header


def test_the_struct_itself_is_checked_first():
    l = clb.lib()
    for name, call in routes().items():
        assert call(None) == EARGUMENT and b"request is null" in l.clb_last_error(), name
        for wrong in (0, C.sizeof(SearchRequest) - 8, C.sizeof(SearchRequest) + 8):
            assert call(SearchRequest(struct_bytes=wrong)) == EARGUMENT, (name, wrong)
            assert b"struct_bytes" in l.clb_last_error(), (name, wrong)
        # the mirror's own size is the library's: a valid request gets as far as the searcher
        assert call(request()) == EARGUMENT and b"null searcher" in l.clb_last_error(), name


def test_field_rules_are_answered_before_the_searcher_is_looked_at():
    l = clb.lib()
    cs, cp = np.array([np.inf, 3.0], np.float32), np.zeros(2, np.int64)
    for name, call in routes().items():
        for m in (-1, 17):
            assert call(request(grouping=SOME, per_group=m)) == EARGUMENT and b"per_group must be 1..16" in l.clb_last_error(), (name, m)
        assert call(request(per_group=2)) == EARGUMENT and b"grouping is null" in l.clb_last_error(), name
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(request(prior=SOME, prior_weight=bad)) == EARGUMENT, (name, bad)
            assert b"prior_weight must be finite" in l.clb_last_error(), (name, bad)
        assert call(request(prior_weight=float("nan"))) == EARGUMENT and b"null searcher" in l.clb_last_error(), name  # no prior: not looked at
        assert call(request(after_scores=cs.ctypes.data)) == EARGUMENT and b"both be given or both be null" in l.clb_last_error(), name
        assert call(request(after_pids=cp.ctypes.data)) == EARGUMENT and b"both be given or both be null" in l.clb_last_error(), name
    bad = np.array([1.0, np.nan], np.float32)
    host = routes()["host"]
    assert host(request(after_scores=bad.ctypes.data, after_pids=cp.ctypes.data)) == EARGUMENT
    assert b"the cursor score of query 1 is NaN" in l.clb_last_error()


def test_combinations_that_are_not_offered_are_unsupported():
    """What used to hold only because no entry point was written for it: now a code, on every route."""
    l = clb.lib()
    cs, cp = np.array([np.inf, 3.0], np.float32), np.zeros(2, np.int64)
    cur = dict(after_scores=cs.ctypes.data, after_pids=cp.ctypes.data)
    for name, call in routes().items():
        assert call(request(grouping=SOME, per_group=2, prior=SOME, prior_weight=1.0)) == EUNSUPPORTED, name
        assert b"per_group together with a prior" in l.clb_last_error(), name
        assert call(request(grouping=SOME, **cur)) == EUNSUPPORTED and b"cursors together with a grouping" in l.clb_last_error(), name
        assert call(request(prior=SOME, prior_weight=1.0, **cur)) == EUNSUPPORTED and b"cursors together with a prior" in l.clb_last_error(), name
        # per_group = 1 is the grouped search: it combines with a prior
        assert call(request(grouping=SOME, per_group=1, prior=SOME, prior_weight=1.0)) == EARGUMENT and b"null searcher" in l.clb_last_error()
    for name in ("phase1", "phase2"):           # the phases of a shard group take no hits and no cursors
        call = routes()[name]
        assert call(request(grouping=SOME, per_group=2)) == EUNSUPPORTED and b"no per_group" in l.clb_last_error(), name
        assert call(request(**cur)) == EUNSUPPORTED and b"no cursors" in l.clb_last_error(), name
    handles = (C.c_void_p * 2)()
    assert routes()["phase2"](request(filters=handles)) == EARGUMENT and b"phase 2 takes no filters" in l.clb_last_error()


def test_a_valid_request_on_a_null_searcher_is_a_null_searcher():
    l = clb.lib()
    cs, cp = np.array([np.inf, 3.0], np.float32), np.zeros(2, np.int64)
    handles = (C.c_void_p * 2)()
    plain, grouped_prior = request(), request(grouping=SOME, per_group=1, group_base=5, prior=SOME, prior_weight=0.5)
    filtered, hits = request(filters=handles, scope=1, pad_short=1), request(grouping=SOME, per_group=16)
    cursors = request(filters=handles, after_scores=cs.ctypes.data, after_pids=cp.ctypes.data)
    valid = {"host": (plain, grouped_prior, filtered, hits, cursors), "device": (plain, grouped_prior, filtered, hits, cursors),
             "phase1": (plain, grouped_prior, filtered), "phase2": (plain, grouped_prior)}
    for name, call in routes().items():
        for i, r in enumerate(valid[name]):
            assert call(r) == EARGUMENT and b"null searcher" in l.clb_last_error(), (name, i)


# ---- the Python builder ---------------------------------------------------------------------------------------------------
def fields_of(r):
    """the fields of a request that differ from "none" (struct_bytes aside)"""
    none = dict(filters=False, scope=0, pad_short=0, grouping=None, per_group=0, group_base=0, prior=None, prior_weight=0.0,
                after_scores=None, after_pids=None)
    got = {name: (bool(getattr(r, name)) if name == "filters" else getattr(r, name)) for name in none}
    assert r.struct_bytes == C.sizeof(SearchRequest)
    return {k: v for k, v in got.items() if v != none[k]}


def open_handles(s):
    g = clb.PassageGrouping(s, C.c_void_p(0xbee0), 2, ids_from_lens([60, 40]))
    f = clb.PassageFilter(s, C.c_void_p(0xfee0), 3)
    return g, f, fake_prior(s, 2.0)


def test_the_builder_sets_exactly_the_fields_its_keywords_name():
    s = _NoDevice()
    g, f, pr = open_handles(s)
    cur = (np.array([3.0, np.inf], np.float32), np.array([5, 0]))
    try:
        assert fields_of(search_request(s, 2)) == {}
        assert fields_of(search_request(s, 2, pad_short=True)) == dict(pad_short=1)
        assert fields_of(search_request(s, 2, scope="all")) == dict(scope=1)
        r = search_request(s, 2, filters=[f, None], scope="all")
        assert fields_of(r) == dict(filters=True, scope=1, pad_short=1)         # with filters the host route always pads
        assert r.filters[0] == 0xfee0 and r.filters[1] is None
        assert search_request(s, 2, filters=f).filters[1] == 0xfee0             # one filter for every query
        assert fields_of(search_request(s, 2, grouping=g)) == dict(grouping=0xbee0)
        assert fields_of(search_request(s, 2, grouping=g, pad_short=True)) == dict(grouping=0xbee0, pad_short=1)
        assert fields_of(search_request(s, 2, grouping=g, per_group=np.int64(3))) == dict(grouping=0xbee0, per_group=3)
        assert fields_of(search_request(s, 2, grouping=g, per_group=1, filters=f)) == dict(grouping=0xbee0, per_group=1, filters=True,
                                                                                          pad_short=1)
        assert fields_of(search_request(s, 2, prior=pr)) == dict(prior=0xdead0, prior_weight=1.0)
        assert fields_of(search_request(s, 2, prior=pr, prior_weight=-0.5, grouping=g, group_base=7)) == dict(
            prior=0xdead0, prior_weight=-0.5, grouping=0xbee0, group_base=7)
        assert fields_of(search_request(s, 2, prior_weight=3.0)) == {}           # without a prior the weight is not looked at
        r = search_request(s, 2, after=cur, filters=[None, f])
        assert fields_of(r) == dict(after_scores=r._keep[1][0].ctypes.data, after_pids=r._keep[1][1].ctypes.data, filters=True,
                                    pad_short=1)
        assert r._keep[1][1].dtype == np.int64 and r._keep[1][0][0] == 3.0       # the converted arrays live with the request
        assert fields_of(search_request(s, 2, after=cur))["pad_short"] == 1      # a page is always padded
        # cursors on the device route: whatever `cursor_arrays` hands back, by its data_ptr
        tensor = type("T", (), {"data_ptr": lambda self: 0x1230})()
        r = search_request(s, 2, after=("a", "b"), cursor_arrays=lambda after, B: (tensor, tensor))
        assert r.after_scores == 0x1230 and r.after_pids == 0x1230
    finally:
        g._h = f._h = pr._h = None                         # never destroyed: they were never created


def test_the_builder_raises_what_the_methods_raise():
    s = _NoDevice()
    g, f, pr = open_handles(s)
    closed = clb.PassageGrouping(s, None, 2, ids_from_lens([60, 40]))
    cur = (np.array([3.0, np.inf], np.float32), np.array([5, 0]))
    try:
        with pytest.raises(clb.ColBERTError, match="scope must be"):
            search_request(s, 2, scope="some")
        for kw, name in ((dict(grouping=g), "grouping"), (dict(grouping=g, per_group=2), "grouping"), (dict(per_group=2), "per_group"),
                         (dict(prior=pr), "prior")):
            with pytest.raises(clb.Unsupported, match=f"after together with {name}"):
                search_request(s, 2, after=cur, **kw)
        with pytest.raises(clb.ArgumentError, match="the cursor score of query 1 is NaN"):
            search_request(s, 2, after=(np.array([1.0, np.nan]), cur[1]))
        with pytest.raises(clb.ArgumentError, match="one cursor per query"):
            search_request(s, 3, after=cur)
        with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
            search_request(s, 2, grouping=g, per_group=2, prior=pr)
        for bad in (float("nan"), 1e39, "1", None, True):
            with pytest.raises(clb.ArgumentError, match="prior_weight"):
                search_request(s, 2, prior=pr, prior_weight=bad)
        with pytest.raises(clb.ArgumentError, match="not below FLT_MAX"):
            search_request(s, 2, prior=pr, prior_weight=2e38)
        with pytest.raises(clb.ColBERTError, match="open PassagePrior"):
            search_request(s, 2, prior=np.zeros(100, np.float32))
        for bad in (0, 17, -3):
            with pytest.raises(clb.ArgumentError, match="per_group must be 1..16"):
                search_request(s, 2, grouping=g, per_group=bad)
        with pytest.raises(clb.ArgumentError, match="integer"):
            search_request(s, 2, grouping=g, per_group=2.0)
        with pytest.raises(clb.ArgumentError, match="needs grouping="):
            search_request(s, 2, per_group=2)
        with pytest.raises(clb.ColBERTError, match="B=2 entries"):
            search_request(s, 2, filters=[f])
        with pytest.raises(clb.ColBERTError, match=r"filters\[1\] is not an open PassageFilter"):
            search_request(s, 2, filters=[f, "x"])
        with pytest.raises(clb.ColBERTError, match="open PassageGrouping"):        # the grouping is looked at last
            search_request(s, 2, grouping=closed, prior=pr, filters=f)
    finally:
        g._h = f._h = pr._h = None


def test_a_library_without_the_request_entries_is_named(monkeypatch):
    """COLBERT_HIP_LIB pointing at a build of an earlier commit: the search fails with the missing symbol's name."""
    class Old:
        clb_search_batch = staticmethod(lambda *a: 0)
    monkeypatch.setattr(clb._lib, "_lib", Old())
    monkeypatch.setattr(clb._lib, "_entries", {})
    with pytest.raises(clb.ColBERTError, match="lacks clb_search_batch_request: .*its own checkout"):
        _NoDevice().search_batch(np.zeros((128, 32, 2), np.float32, order="F"), 5)
