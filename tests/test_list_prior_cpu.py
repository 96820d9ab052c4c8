"""Re-rank with first-stage scores (list priors), the part that needs no GPU: the field and the two entries are declared and
exported, the mirror keeps the struct's order, every rule that needs no searcher is answered with its message on a NULL
searcher -- on the host and the device route --, and the Python builder sets exactly `list_prior` and `prior_weight`, pads
ragged values beside ragged pids and raises what the search methods raise."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd._lib import SearchRequest
from colbert_jl_amd.searcher import search_request
from tests.test_group_cpu import _NoDevice
from tests.test_rerank_cpu import lists
from tests.test_search_request_cpu import SOME, fields_of, open_handles, request, routes

NEW_SYMBOLS = ("clb_search_batch_listed_prior", "clb_search_batch_listed_prior_device_slot")
EARGUMENT, EUNSUPPORTED = clb.ArgumentError.code, clb.Unsupported.code
FLT_MAX = float(np.finfo(np.float32).max)


def values(L=3, fill=0.5):
    """a value block for the B = 2 queries of routes(), beside lists(L)"""
    v = np.full(2 * L, fill, np.float32)
    return v.ctypes.data, v


def test_the_field_and_both_entries_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    header = open(clb._lib.HEADER).read()
    body = header.split("typedef struct clb_search_request {")[1].split("} clb_search_request;")[0]
    assert "const float* list_prior;" in body
    assert body.index("prior_weight;") < body.index("list_prior;") < body.index("after_scores;")      # with the prior fields
    names = [f[0] for f in SearchRequest._fields_]
    assert names == ["struct_bytes", "filters", "scope", "pad_short", "grouping", "per_group", "group_base", "prior", "prior_weight",
                     "list_prior", "after_scores", "after_pids", "list_pids", "list_lens", "list_stride", "list_scores"]
    assert names[-4:] == ["list_pids", "list_lens", "list_stride", "list_scores"]      # the last four are still the list fields


def test_list_prior_rules_are_answered_before_the_searcher_is_looked_at():
    l = clb.lib()
    ok, keep = lists()
    vp, v = values()
    cs, cp = np.array([np.inf, 3.0], np.float32), np.zeros(2, np.int64)
    for name in ("host", "device"):
        call = routes()[name]
        assert call(request(list_prior=vp, prior_weight=1.0, prior=SOME, **ok)) == EUNSUPPORTED, name
        assert b"list priors together with a prior are not supported" in l.clb_last_error(), name
        assert call(request(list_prior=vp, prior_weight=1.0, grouping=SOME, per_group=2, **ok)) == EUNSUPPORTED, name
        assert b"per_group together with list priors" in l.clb_last_error(), name
        assert call(request(list_prior=vp, prior_weight=1.0, after_scores=cs.ctypes.data, after_pids=cp.ctypes.data, **ok)) == EUNSUPPORTED
        assert b"cursors together with list priors" in l.clb_last_error(), name
        assert call(request(list_prior=vp, prior_weight=1.0)) == EARGUMENT, name
        assert b"list_prior without candidate lists" in l.clb_last_error(), name
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(request(list_prior=vp, prior_weight=bad, **ok)) == EARGUMENT, (name, bad)
            assert b"prior_weight must be finite" in l.clb_last_error(), (name, bad)
        # a weight with neither prior nor list_prior stays unlooked-at
        assert call(request(prior_weight=float("nan"), **ok)) == EARGUMENT and b"null searcher" in l.clb_last_error(), name
        # what composes gets as far as the searcher: alone, and with a grouping (per_group 0 or 1)
        for more in ({}, dict(grouping=SOME), dict(grouping=SOME, per_group=1)):
            assert call(request(list_prior=vp, prior_weight=-1.5, **more, **ok)) == EARGUMENT, (name, more)
            assert b"null searcher" in l.clb_last_error(), (name, more)
    for name in ("phase1", "phase2"):               # the phase routes already refuse the lists
        assert routes()[name](request(list_prior=vp, prior_weight=1.0, **ok)) == EUNSUPPORTED
        assert b"take no candidate lists" in l.clb_last_error(), name
    del keep, v


def test_host_route_values_are_checked_before_the_searcher():
    l = clb.lib()
    host, device = routes()["host"], routes()["device"]
    ok, keep = lists(3, (2, 1))
    for bad in (np.nan, np.inf, -np.inf):
        v = np.array([0.5, 0.5, 9.0, bad, 0.5, 0.5], np.float32)                # query 1, position 0
        assert host(request(list_prior=v.ctypes.data, prior_weight=1.0, **ok)) == EARGUMENT
        assert b"the list prior of query 1, position 0 is not a finite number" in l.clb_last_error(), bad
        v = np.array([0.5, 0.5, bad, 0.5, bad, bad], np.float32)                # past the lengths: never read as values
        assert host(request(list_prior=v.ctypes.data, prior_weight=1.0, **ok)) == EARGUMENT
        assert b"null searcher" in l.clb_last_error(), bad
    v = np.array([1.0, -3e38, 0.0, 2.0, 0.0, 0.0], np.float32)
    assert host(request(list_prior=v.ctypes.data, prior_weight=2.0, **ok)) == EARGUMENT
    assert b"is not below FLT_MAX" in l.clb_last_error()
    assert host(request(list_prior=v.ctypes.data, prior_weight=-1.0, **ok)) == EARGUMENT and b"null searcher" in l.clb_last_error()
    # lengths are answered first: a bad length is never used to read values
    bad_len, keep2 = lists(3, (2, 4))
    assert host(request(list_prior=v.ctypes.data, prior_weight=1.0, **bad_len)) == EARGUMENT
    assert b"has length 4" in l.clb_last_error()
    # the device route cannot see the values
    assert device(request(list_prior=SOME, prior_weight=1.0, list_pids=SOME, list_lens=SOME, list_stride=3)) == EARGUMENT
    assert b"null searcher" in l.clb_last_error()
    del keep, keep2


def test_the_named_entries_fill_a_request():
    l = clb.lib()
    ok, keep = lists(3, (3, 0))
    vp, v = values()
    q = np.zeros((128, 32, 2), np.float32, order="F")
    op, os_, nc = np.zeros(4, np.int64), np.zeros(4, np.float32), np.zeros(2, np.int64)
    p = lambda a: a.ctypes.data
    w = C.c_float
    host = lambda pids, lens, vals, weight: l.clb_search_batch_listed_prior(None, p(q), 32, 2, 2, 2, pids, lens, 3, vals, w(weight), None,
                                                                            p(op), p(os_), p(nc))
    assert host(None, None, vp, 1.0) == EARGUMENT and b"list_pids and list_lens are null" in l.clb_last_error()
    assert host(ok["list_pids"], None, vp, 1.0) == EARGUMENT and b"both be given or both be null" in l.clb_last_error()
    assert host(ok["list_pids"], ok["list_lens"], vp, float("nan")) == EARGUMENT and b"prior_weight must be finite" in l.clb_last_error()
    assert host(ok["list_pids"], ok["list_lens"], vp, 0.5) == EARGUMENT and b"null searcher" in l.clb_last_error()
    assert host(ok["list_pids"], ok["list_lens"], None, float("nan")) == EARGUMENT and b"null searcher" in l.clb_last_error()
    v[1] = np.nan
    assert host(ok["list_pids"], ok["list_lens"], vp, 0.5) == EARGUMENT and b"query 0, position 1" in l.clb_last_error()
    dev = lambda vals, weight, stride=5: l.clb_search_batch_listed_prior_device_slot(None, 0, SOME, 32, 2, 2, 2, SOME, SOME, stride, vals,
                                                                                     w(weight), None, SOME, SOME, SOME, None)
    assert dev(SOME, 1.0, 0) == EARGUMENT and b"list_stride must be" in l.clb_last_error()
    assert dev(SOME, float("inf")) == EARGUMENT and b"prior_weight must be finite" in l.clb_last_error()
    assert dev(SOME, 1.0) == EARGUMENT and b"null searcher" in l.clb_last_error()
    assert dev(None, float("inf")) == EARGUMENT and b"null searcher" in l.clb_last_error()
    del keep


# ---- the Python builder ---------------------------------------------------------------------------------------------------
def test_the_builder_sets_exactly_list_prior_and_prior_weight():
    s = _NoDevice()
    r = search_request(s, 3, candidates=[[5, 2, 5], [], [9]], candidate_priors=[[0.5, -2, 7], [], np.array([3], np.int8)],
                       prior_weight=0.25)
    pids, lens, L, scores, ragged, vals = r.lists
    assert fields_of(r) == dict(pad_short=1, prior_weight=0.25) and r.list_prior == vals.ctypes.data
    assert vals.dtype == np.float32 and vals.shape == (3, 3) and vals.flags.f_contiguous      # padded beside the pids
    assert vals.T.tolist() == [[0.5, -2.0, 7.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]] and pids.T.tolist() == [[5, 2, 5], [0, 0, 0], [9, 0, 0]]
    # the default weight is 1; without the keyword nothing is set
    r = search_request(s, 1, candidates=[[1, 2]], candidate_priors=[[1, 2]])
    assert fields_of(r) == dict(pad_short=1, prior_weight=1.0)
    r = search_request(s, 1, candidates=[[1, 2]], prior_weight=3.0)
    assert fields_of(r) == dict(pad_short=1) and r.list_prior is None and len(r.lists) == 5
    # the pair form takes an (L, B) block; values past a length are not looked at
    block = np.array([[4, 7], [6, 0], [4, 0]], np.int32)
    vb = np.array([[1.5, 2.5], [0.5, np.nan], [-1.0, np.inf]])
    r = search_request(s, 2, candidates=(block, [3, 1]), candidate_priors=vb, prior_weight=-1.5, candidate_scores=True)
    assert r.lists[5].dtype == np.float32 and r.lists[5].flags.f_contiguous and r.list_prior == r.lists[5].ctypes.data
    assert r.lists[5][:, 0].tolist() == [1.5, 0.5, -1.0] and r.prior_weight == -1.5 and r.list_scores
    # with a grouping
    g, f, pr = open_handles(s)
    try:
        r = search_request(s, 2, candidates=(block, [3, 1]), candidate_priors=vb, grouping=g)
        assert fields_of(r) == dict(grouping=0xbee0, pad_short=1, prior_weight=1.0) and r.list_prior
    finally:
        g._h = f._h = pr._h = None
    # on the device route: whatever `candidate_prior_arrays` hands back, by its data_ptr
    tensor = type("T", (), {"data_ptr": lambda self: 0x1230})()
    r = search_request(s, 2, candidates="x", candidate_arrays=lambda c, sc, B: (tensor, tensor, 11, sc, False),
                       candidate_priors="y", candidate_prior_arrays=lambda v, ls, B: (tensor, 0.0), prior_weight=2.0)
    assert (r.list_prior, r.prior_weight, r.list_stride) == (0x1230, 2.0, 11)


def test_the_builder_refuses_what_are_no_list_priors():
    s = _NoDevice()
    g, f, pr = open_handles(s)
    two = dict(candidates=[[1, 2], [3]])
    try:
        with pytest.raises(clb.ArgumentError, match="the candidate priors of query 1 hold 2 values for a list of 1 pids"):
            search_request(s, 2, candidate_priors=[[1, 2], [3, 4]], **two)
        with pytest.raises(clb.ArgumentError, match="one array of values per candidate list"):
            search_request(s, 2, candidate_priors=[[1, 2]], **two)
        with pytest.raises(clb.ArgumentError, match="the candidate priors of query 0 must be numbers"):
            search_request(s, 2, candidate_priors=[["a", "b"], [3]], **two)
        with pytest.raises(clb.ArgumentError, match="must be numbers"):
            search_request(s, 2, candidate_priors=[[1, 2], [None]], **two)
        for bad in (np.nan, np.inf, -np.inf, 1e39):
            with pytest.raises(clb.ArgumentError, match="the candidate prior of query 0, position 1 is not a finite number"):
                search_request(s, 2, candidate_priors=[[1, bad], [3]], **two)
        block = np.ones((3, 2), np.int64)
        with pytest.raises(clb.ArgumentError, match=r"candidate_priors must be an \(L=3, B=2\) block"):
            search_request(s, 2, candidates=(block, [1, 1]), candidate_priors=np.ones((2, 3)))
        with pytest.raises(clb.ArgumentError, match="the candidate prior of query 1, position 2 is not a finite number"):
            search_request(s, 2, candidates=(block, [1, 3]), candidate_priors=np.array([[1, 1], [np.nan, 1], [1, np.nan]]))
        # the weight, through the prior's own check against the largest listed |value|
        with pytest.raises(clb.ArgumentError, match="is not below FLT_MAX"):
            search_request(s, 2, candidate_priors=[[1, -3e38], [3]], prior_weight=2.0, **two)
        for bad in (np.nan, np.inf, "1", None, True):
            with pytest.raises(clb.ArgumentError, match="prior_weight must be a finite"):
                search_request(s, 2, candidate_priors=[[1, 2], [3]], prior_weight=bad, **two)
        # the three refusals, naming both keywords, and the keyword without lists -- on the builder and on every method
        cur = (np.zeros(2, np.float32), np.zeros(2, np.int64))
        q = np.zeros((128, 32), np.float32, order="F")
        for kw, message in ((dict(prior=pr), "candidate_priors together with prior is not supported"),
                            (dict(grouping=g, per_group=2), "per_group together with candidate_priors is not supported"),
                            (dict(after=cur), "after together with candidate_priors is not supported")):
            with pytest.raises(clb.Unsupported, match=message):
                search_request(s, 2, candidate_priors=[[1, 2], [3]], **two, **kw)
            one = {**kw, **({"after": (0.0, 0)} if "after" in kw else {})}
            with pytest.raises(clb.Unsupported, match=message):
                s.search_embeddings(q, 5, candidates=[1, 2], candidate_priors=[1, 2], **one)
            with pytest.raises(clb.Unsupported, match=message):
                s.search("a query", 5, candidates=[1, 2], candidate_priors=[1, 2], **one)
            with pytest.raises(clb.Unsupported, match=message):
                clb.search(s, q, 5, candidates=[1, 2], candidate_priors=[1, 2], **one)
            with pytest.raises(clb.Unsupported, match=message):
                s.search_batch(q.reshape(128, 32, 1), 5, candidates=[[1, 2]], candidate_priors=[[1, 2]],
                               **{**kw, **({"after": (cur[0][:1], cur[1][:1])} if "after" in kw else {})})
        for call in (lambda: search_request(s, 2, candidate_priors=[[1], [2]]), lambda: s.search_embeddings(q, 5, candidate_priors=[1]),
                     lambda: s.search("a query", 5, candidate_priors=[1]), lambda: clb.search(s, q, 5, candidate_priors=[1]),
                     lambda: s.search_batch(q.reshape(128, 32, 1), 5, candidate_priors=[[1]])):
            with pytest.raises(clb.ArgumentError, match="candidate_priors needs candidates="):
                call()
    finally:
        g._h = f._h = pr._h = None


def test_sharded_searcher_takes_the_keyword_and_still_refuses_by_candidates():
    from colbert_jl_amd.sharded import ShardedSearcher
    ss = ShardedSearcher.__new__(ShardedSearcher)          # no shards: the refusal comes before anything is looked at
    q = np.zeros((128, 32, 2), np.float32, order="F")
    with pytest.raises(clb.Unsupported, match="candidates= .* is not supported across a shard group"):
        ss.search_batch(q, 5, candidates=[[1], [2]], candidate_priors=[[0.5], [0.5]])
    with pytest.raises(clb.Unsupported, match="candidates= "):
        ss.search_embeddings(q[:, :, 0], 5, candidates=[1], candidate_priors=[0.5])
    with pytest.raises(clb.Unsupported, match="candidates= "):
        ss.search("a query", 5, candidates=[1], candidate_priors=[0.5], prior_weight=2.0)
    with pytest.raises(clb.Unsupported, match="candidates= "):
        ss.search_batch(q, 5, candidate_priors=[[0.5], [0.5]])
