"""Re-rank given passages, the part that needs no GPU: the listed entry points are declared and exported, the rules of the
list fields of a clb_search_request are answered on a NULL searcher on every route, and the Python builder pads ragged
lists, keeps the converted arrays with the request and raises what the search methods raise."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd._lib import SearchRequest
from colbert_jl_amd.searcher import search_request
from tests.test_group_cpu import _NoDevice
from tests.test_search_request_cpu import SOME, fields_of, open_handles, request, routes

NEW_SYMBOLS = ("clb_search_batch_listed", "clb_search_batch_listed_device_slot")
EARGUMENT, EUNSUPPORTED = clb.ArgumentError.code, clb.Unsupported.code


def lists(L=3, lens=(2, 0)):
    """list fields of a request for the B = 2 queries of routes(): host arrays, which a NULL searcher never reads past the lengths"""
    pids, n = np.arange(1, 2 * L + 1, dtype=np.int64), np.array(lens, np.int64)
    fields = dict(list_pids=pids.ctypes.data, list_lens=n.ctypes.data, list_stride=L)
    return fields, (pids, n)


def test_listed_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    header = open(clb._lib.HEADER).read()
    for field in ("list_pids;", "list_lens;", "list_stride;", "list_scores;"):
        assert field in header.split("typedef struct clb_search_request {")[1].split("} clb_search_request;")[0], field
    names = [f[0] for f in SearchRequest._fields_]
    assert names[-4:] == ["list_pids", "list_lens", "list_stride", "list_scores"]      # the struct grew at its end


def test_list_field_rules_are_answered_before_the_searcher_is_looked_at():
    l = clb.lib()
    ok, keep = lists()
    handles = (C.c_void_p * 2)()
    one = (C.c_void_p * 2)(None, SOME)
    sc = np.zeros(6, np.float32)
    for name, call in routes().items():
        # the pair
        assert call(request(list_pids=ok["list_pids"], list_stride=3)) == EARGUMENT, name
        assert b"list_pids and list_lens must both be given or both be null" in l.clb_last_error(), name
        assert call(request(list_lens=ok["list_lens"], list_stride=3)) == EARGUMENT, name
        assert b"list_pids and list_lens must both be given or both be null" in l.clb_last_error(), name
        # the stride
        for bad in (0, -1):
            assert call(request(**{**ok, "list_stride": bad})) == EARGUMENT and b"list_stride must be" in l.clb_last_error(), (name, bad)
        # the output needs lists
        assert call(request(list_scores=sc.ctypes.data)) == EARGUMENT and b"list_scores without candidate lists" in l.clb_last_error(), name
        # none: stride alone is not looked at
        assert call(request(list_stride=7)) == EARGUMENT and b"null searcher" in l.clb_last_error(), name
    for name in ("host", "device", "phase1"):
        call = routes()[name]
        assert call(request(filters=one, **ok)) == EUNSUPPORTED, name
        assert b"candidate lists together with filters" in l.clb_last_error(), name
    for name in ("host", "device"):
        call = routes()[name]
        # an array of NULL handles filters nothing: the lists stand
        assert call(request(filters=handles, **ok)) == EARGUMENT and b"null searcher" in l.clb_last_error(), name
    for name in ("phase1", "phase2"):
        assert routes()[name](request(**ok)) == EUNSUPPORTED and b"take no candidate lists" in l.clb_last_error(), name
    del keep


def test_host_route_lengths_are_checked_before_the_searcher():
    l = clb.lib()
    host = routes()["host"]
    for lens, b in (((2, 4), 1), ((-1, 0), 0)):
        bad, keep = lists(3, lens)
        assert host(request(**bad)) == EARGUMENT
        assert f"the candidate list of query {b} has length {lens[b]}, outside 0..list_stride=3".encode() in l.clb_last_error()
    # the device route cannot see them: it clamps on the device
    bad, keep = lists(3, (2, 4))
    assert routes()["device"](request(list_pids=SOME, list_lens=SOME, list_stride=3)) == EARGUMENT and b"null searcher" in l.clb_last_error()


def test_a_valid_listed_request_on_a_null_searcher_is_a_null_searcher():
    l = clb.lib()
    ok, keep = lists(3, (3, 0))
    sc = np.zeros(6, np.float32)
    cs, cp = np.array([np.inf, 3.0], np.float32), np.zeros(2, np.int64)
    valid = (request(**ok), request(list_scores=sc.ctypes.data, **ok), request(grouping=SOME, per_group=3, **ok),
             request(prior=SOME, prior_weight=0.5, **ok), request(after_scores=cs.ctypes.data, after_pids=cp.ctypes.data, **ok))
    for name in ("host", "device"):
        for i, r in enumerate(valid):
            assert routes()[name](r) == EARGUMENT and b"null searcher" in l.clb_last_error(), (name, i)
    # the named entries: their own refusal, then the request's
    q = np.zeros((128, 32, 2), np.float32, order="F")
    op, os_, nc = np.zeros(4, np.int64), np.zeros(4, np.float32), np.zeros(2, np.int64)
    p = lambda a: a.ctypes.data
    assert l.clb_search_batch_listed(None, p(q), 32, 2, 2, 2, None, None, 3, None, p(op), p(os_), p(nc)) == EARGUMENT
    assert b"list_pids and list_lens are null" in l.clb_last_error()
    assert l.clb_search_batch_listed(None, p(q), 32, 2, 2, 2, ok["list_pids"], ok["list_lens"], 3, None, p(op), p(os_), p(nc)) == EARGUMENT
    assert b"null searcher" in l.clb_last_error()
    assert l.clb_search_batch_listed(None, p(q), 32, 2, 2, 2, ok["list_pids"], None, 3, None, p(op), p(os_), p(nc)) == EARGUMENT
    assert b"both be given or both be null" in l.clb_last_error()
    assert l.clb_search_batch_listed_device_slot(None, 0, SOME, 32, 2, 2, 2, SOME, SOME, 0, None, SOME, SOME, SOME, None) == EARGUMENT
    assert b"list_stride must be" in l.clb_last_error()
    assert l.clb_search_batch_listed_device_slot(None, 0, SOME, 32, 2, 2, 2, SOME, SOME, 5, SOME, SOME, SOME, SOME, None) == EARGUMENT
    assert b"null searcher" in l.clb_last_error()
    del keep


# ---- the Python builder ---------------------------------------------------------------------------------------------------
def test_the_builder_pads_ragged_lists_to_their_longest():
    s = _NoDevice()
    r = search_request(s, 3, candidates=[[5, 2, 5], np.array([], np.int32), np.array([9], np.uint8)])
    pids, lens, L, scores, ragged = r.lists
    assert fields_of(r) == dict(pad_short=1)                                  # with lists the host route always pads
    assert (r.list_pids, r.list_lens, r.list_stride, r.list_scores) == (pids.ctypes.data, lens.ctypes.data, 3, None)
    assert L == 3 and ragged and scores is None
    assert pids.dtype == np.int64 and lens.dtype == np.int64                  # the converted arrays live with the request
    assert pids.shape == (3, 3) and pids.flags.f_contiguous                    # column b = row b of the C block
    assert pids.T.tolist() == [[5, 2, 5], [0, 0, 0], [9, 0, 0]] and lens.tolist() == [3, 0, 1]
    # the output, when asked for: one block of the lists' shape
    r = search_request(s, 2, candidates=[[1], [2, 3]], candidate_scores=True)
    assert r.lists[3].shape == (2, 2) and r.lists[3].dtype == np.float32 and r.list_scores == r.lists[3].ctypes.data
    # every list empty: one padded row
    r = search_request(s, 2, candidates=[[], []])
    assert r.list_stride == 1 and r.lists[1].tolist() == [0, 0]
    # without lists nothing is set
    r = search_request(s, 2)
    assert (r.list_pids, r.list_lens, r.list_stride, r.list_scores, r.lists) == (None, None, 0, None, None)


def test_the_builder_takes_a_block_and_lengths():
    s = _NoDevice()
    block = np.array([[4, 7], [6, 0], [4, 0]], np.int32)                      # (L, B): column b is query b's list
    r = search_request(s, 2, candidates=(block, [3, 1]), candidate_scores=True)
    pids, lens, L, scores, ragged = r.lists
    assert L == 3 and not ragged and pids.dtype == np.int64 and pids.flags.f_contiguous
    assert pids.T.tolist() == [[4, 6, 4], [7, 0, 0]] and lens.tolist() == [3, 1] and scores.shape == (3, 2)
    # cursors, a grouping and a prior ride along
    g, f, pr = open_handles(s)
    try:
        r = search_request(s, 2, candidates=(block, [3, 1]), grouping=g, per_group=2)
        assert fields_of(r) == dict(grouping=0xbee0, per_group=2, pad_short=1) and r.list_stride == 3
        r = search_request(s, 2, candidates=(block, [3, 1]), prior=pr, prior_weight=0.25)
        assert fields_of(r) == dict(prior=0xdead0, prior_weight=0.25, pad_short=1)
        r = search_request(s, 2, candidates=(block, [0, 0]), after=(np.array([3.0, np.inf], np.float32), np.array([5, 0])))
        assert r.after_scores and r.list_pids
        # lists on the device route: whatever `candidate_arrays` hands back, by its data_ptr
        tensor = type("T", (), {"data_ptr": lambda self: 0x1230})()
        r = search_request(s, 2, candidates="x", candidate_scores=tensor,
                           candidate_arrays=lambda c, sc, B: (tensor, tensor, 11, sc, False))
        assert (r.list_pids, r.list_lens, r.list_stride, r.list_scores) == (0x1230, 0x1230, 11, 0x1230)
    finally:
        g._h = f._h = pr._h = None


def test_the_builder_refuses_what_is_no_list():
    s = _NoDevice()
    g, f, pr = open_handles(s)
    try:
        for n in (1, 3):
            with pytest.raises(clb.ArgumentError, match=f"one list per query: {n} lists for 2 queries"):
                search_request(s, 2, candidates=[[1]] * n)
        with pytest.raises(clb.ArgumentError, match="the candidate list of query 1 must be integers"):
            search_request(s, 2, candidates=[[1], [2.5]])
        with pytest.raises(clb.ArgumentError, match="the candidate list of query 0 must be integers"):
            search_request(s, 2, candidates=[np.array([2 ** 63], np.uint64), [1]])
        with pytest.raises(clb.ArgumentError, match="sequence of integer arrays"):
            search_request(s, 2, candidates=7)
        block = np.ones((3, 2), np.int64)
        for bad in ([1.0, 2.0], [True, False]):
            with pytest.raises(clb.ArgumentError, match="the candidate list lengths must be integers"):
                search_request(s, 2, candidates=(block, np.array(bad)))
        for bad in ([-1, 0], [0, 4]):
            with pytest.raises(clb.ArgumentError, match=r"the candidate list lengths must lie in 0\.\.3"):
                search_request(s, 2, candidates=(block, bad))
        with pytest.raises(clb.ArgumentError, match="the candidate pids must be integers"):
            search_request(s, 2, candidates=(block.astype(np.float32), [1, 1]))
        for bad in ((block, [1]), (block[:, :1], [1, 1]), (np.ones((0, 2), np.int64), [0, 0])):
            with pytest.raises(clb.ArgumentError, match="holds one list per query"):
                search_request(s, 2, candidates=bad)
        with pytest.raises(clb.ArgumentError, match="candidate scores need candidates="):
            search_request(s, 2, candidate_scores=True)
        # a list is the candidate set: no filters beside it, on the builder and on every method
        for filters in (f, [f, None], [None, f]):
            with pytest.raises(clb.Unsupported, match=r"candidates= together with filter\(s\)= is not supported"):
                search_request(s, 2, candidates=[[1], [2]], filters=filters)
        q = np.zeros((128, 32), np.float32, order="F")
        with pytest.raises(clb.Unsupported, match=r"candidates= together with filter\(s\)="):
            s.search_embeddings(q, 5, candidates=[1, 2], filter=f)
        with pytest.raises(clb.Unsupported, match=r"candidates= together with filter\(s\)="):
            s.search("a query", 5, candidates=[1, 2], filter=f)
        with pytest.raises(clb.Unsupported, match=r"candidates= together with filter\(s\)="):
            s.search_batch(q.reshape(128, 32, 1), 5, candidates=[[1, 2]], filters=f)
        with pytest.raises(clb.Unsupported, match=r"candidates= together with filter\(s\)="):
            clb.search(s, q, 5, candidates=[1, 2], filter=f)
        with pytest.raises(clb.ArgumentError, match="candidate scores need candidates="):
            s.search_embeddings(q, 5, return_candidate_scores=True)
        # what the other keywords refuse among themselves stays refused with lists
        with pytest.raises(clb.Unsupported, match="after together with grouping"):
            search_request(s, 2, candidates=[[1], [2]], grouping=g, after=(np.zeros(2, np.float32), np.zeros(2, np.int64)))
        with pytest.raises(clb.Unsupported, match="per_group together with a prior"):
            search_request(s, 2, candidates=[[1], [2]], grouping=g, per_group=2, prior=pr)
    finally:
        g._h = f._h = pr._h = None


def test_sharded_searcher_accepts_the_keyword_and_refuses_it():
    from colbert_jl_amd.sharded import ShardedSearcher
    ss = ShardedSearcher.__new__(ShardedSearcher)          # no shards: the refusal comes before anything is looked at
    q = np.zeros((128, 32, 2), np.float32, order="F")
    with pytest.raises(clb.Unsupported, match="candidates= .* is not supported across a shard group"):
        ss.search_batch(q, 5, candidates=[[1], [2]])
    with pytest.raises(clb.Unsupported, match="candidates= "):
        ss.search_embeddings(q[:, :, 0], 5, candidates=[1])
    with pytest.raises(clb.Unsupported, match="candidates= "):
        ss.search("a query", 5, candidates=[1])
    with pytest.raises(clb.Unsupported, match="candidates= "):
        ss.search_batch(q, 5, return_candidate_scores=True)
