"""Searcher / search -- the reference's src/searching.jl over the C ABI.

`Searcher(index_path)` loads an index directory, uploads it once into HBM (the reference keeps the
index in host memory, searching.jl:50-59) and `search` runs the whole post-encoder pipeline
(searching.jl:102-127) on the device in one library call."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from . import storage
from ._lib import BoundsError, ColBERTError, SearchRequest, check, colmajor, fptr, i64, lib, request_entry
from .config import ColBERTConfig


_SCOPES = {"candidates": 0, "all": 1}      # CLB_FILTER_CANDIDATES / CLB_FILTER_ALL


def _scope_code(scope) -> int:
    if scope not in _SCOPES:
        raise ColBERTError(f"scope must be 'candidates' or 'all', got {scope!r}")
    return _SCOPES[scope]


MAX_PER_GROUP = 16                         # CLB_MAX_PER_GROUP

_FILTER_OPS = {"and": 0, "or": 1, "andnot": 2, "not": 3}      # CLB_FILTER_OP_AND / _OR / _ANDNOT / _NOT
MAX_FILTER_OPERANDS = 16                   # CLB_MAX_FILTER_OPERANDS


def _range_bound(x, name: str, open_end: float) -> float:
    """A bound of `make_range_filter` as the float32 the C ABI takes: None is the open end (-Inf / +Inf), anything but a
    real number (a string, a bool, NaN) an ArgumentError."""
    import numbers
    from ._lib import ArgumentError
    if x is None:
        return float(open_end)
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (numbers.Real, np.floating, np.integer)):
        raise ArgumentError(f"{name} must be a real number or None, got {x!r}")
    with np.errstate(over="ignore"):
        v = np.float32(x)
    if np.isnan(v):
        raise ArgumentError(f"{name} must be a real number or None, got NaN")
    return float(v)


def _per_group(per_group, grouping) -> int:
    """The `per_group=` of a search call as the integer the C ABI takes: it needs a grouping and lies in 1..16."""
    from ._lib import ArgumentError
    if isinstance(per_group, bool) or not isinstance(per_group, (int, np.integer)):
        raise ArgumentError(f"per_group must be an integer 1..{MAX_PER_GROUP} or None, got {per_group!r}")
    if grouping is None:
        raise ArgumentError("per_group needs grouping=: the hits are the best passages of every GROUP")
    if not 1 <= int(per_group) <= MAX_PER_GROUP:
        raise ArgumentError(f"per_group must be 1..{MAX_PER_GROUP}, got {int(per_group)}")
    return int(per_group)


class Owned:
    """Owns one resource and closes it once: `close()` (any number of times), the end of a `with` block, or collection --
    also of an object whose constructor raised half way.  A subclass names `_release()`; `len()` is its `count`."""
    closed = False

    def close(self):
        self.closed = True
        self._release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.count


class ResidentHandle(Owned):
    """An Owned library handle `_h` of one searcher; `_destroy` names the entry point that frees it."""

    def _release(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None


class PassageFilter(ResidentHandle):
    """A set of passages resident in HBM as one bitmap (clb_filter, include/colbert_hip.h): made once by
    `Searcher.make_filter`, reused over any number of searches of that searcher.  Keep it alive while a search that uses
    it may still be running (or a graph that captured it may be replayed).
    Filters of one searcher compose on the device into new filters (`Searcher.combine_filters`): `a & b`, `a | b`, `a - b`
    (a's passages that are not in b), `~a`; the operands are only read and may be closed as soon as the call returns.
    `to_mask()` reads a filter back, `extended()` carries one over an append."""
    _destroy = "clb_filter_destroy"

    def __init__(self, searcher: "Searcher", handle, count: int):
        self.searcher, self._h, self.count = searcher, handle, int(count)
        self.num_docs = int(getattr(searcher, "num_docs", 0))      # the searcher's passages when the filter was made

    def __and__(self, other):
        return self.searcher.combine_filters("and", [self, other])

    def __or__(self, other):
        return self.searcher.combine_filters("or", [self, other])

    def __sub__(self, other):
        return self.searcher.combine_filters("andnot", [self, other])

    def __invert__(self):
        return self.searcher.combine_filters("not", [self])

    def to_mask(self) -> np.ndarray:
        """The set as a boolean array of the `num_docs` entries the filter was made for (entry i = local passage i + 1), read
        back from the device (clb_filter_bitmap)."""
        if not self._h:
            raise ColBERTError("to_mask: not an open PassageFilter")
        words = np.zeros((self.num_docs + 31) // 32, dtype="<u4")
        check(lib().clb_filter_bitmap(self._h, fptr(words), i64(words.size)))
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:self.num_docs].astype(np.bool_)

    def extended(self, fill: bool = False) -> "PassageFilter":
        """A new filter over the searcher's passages as they are NOW: the passages this filter was made for keep their bit,
        the passages appended since are all out (`fill=False`) or all in (`fill=True`).  This filter is unchanged -- if an
        append made it stale it stays refused by every search.  Of a current filter: a copy (clb_filter_extend)."""
        from ._lib import ArgumentError
        if not self._h:
            raise ColBERTError("extended: not an open PassageFilter")
        if not isinstance(fill, (bool, np.bool_)):
            raise ArgumentError(f"fill must be True or False, got {fill!r}")
        h = C.c_void_p()
        check(lib().clb_filter_extend(self.searcher._h, self._h, C.c_int(int(fill)), C.byref(h)))
        return PassageFilter(self.searcher, h, lib().clb_filter_count(h))


class PassageGrouping(ResidentHandle):
    """A map passage -> group (document) resident in HBM (clb_grouping, include/colbert_hip.h): made once by
    `Searcher.make_grouping`, reused over any number of grouped searches of that searcher.  Immutable; valid across
    `remove_passages` and `update_*`, not across an append (make another).  Keep it alive while a search that uses it may
    still be running (or a graph that captured it may be replayed).  `count`: the number of groups."""
    _destroy = "clb_grouping_destroy"

    def __init__(self, searcher: "Searcher", handle, count: int, group_ids: np.ndarray):
        self.searcher, self._h, self.count = searcher, handle, int(count)
        self._ids = group_ids                  # host copy of the caller's ids, entry i = local passage i + 1
        self._pid_offset = int(getattr(searcher, "pid_offset", 0))

    def groups_of(self, pids) -> np.ndarray:
        """The caller's group ids of passages as a search returns them (1-based, the searcher's pid_offset included)."""
        p = np.asarray(pids, dtype=np.int64) - self._pid_offset
        if p.size and (p.min() < 1 or p.max() > self._ids.size):
            raise BoundsError(f"pid outside {self._pid_offset + 1}..{self._pid_offset + self._ids.size} "
                              "(pid 0 pads a short result: cut the result at n_candidates first)")
        return self._ids[p - 1]


FLT_MAX = float(np.finfo(np.float32).max)


class PassagePrior(ResidentHandle):
    """One finite fp32 value per passage resident in HBM (clb_prior, include/colbert_hip.h): made once by
    `Searcher.make_prior`, reused over any number of searches of that searcher (`prior=`, `prior_weight=`: rank by
    MaxSim + prior_weight * value).  Immutable; valid across `remove_passages` and `update_*`, not across an append (make
    another).  Keep it alive while a search that uses it may still be running (or a graph that captured it may be
    replayed).  `max_abs`: the largest |value|; `count`, `len()`: the number of values."""
    _destroy = "clb_prior_destroy"

    def __init__(self, searcher: "Searcher", handle, n: int, max_abs: float):
        self.searcher, self._h, self.count, self.max_abs = searcher, handle, int(n), float(max_abs)


def _prior_weight(prior, prior_weight, per_group) -> float:
    """The `prior=` / `prior_weight=` of a search call, checked on the host -> the weight as the float the C ABI takes."""
    _no_prior_hits(per_group)
    if not isinstance(prior, PassagePrior) or not prior._h:
        raise ColBERTError("prior is not an open PassagePrior")
    return _weight_value(prior_weight, prior.max_abs)


def _no_prior_hits(per_group):
    from ._lib import Unsupported
    if per_group is not None:
        raise Unsupported("per_group together with a prior is not supported: the hits of a grouped search take no prior")


def _weight_value(prior_weight, max_abs: float) -> float:
    """`prior_weight=` against the largest |value| of the prior it multiplies (of a shard group: the largest over all shards)."""
    from ._lib import ArgumentError
    if isinstance(prior_weight, bool) or not isinstance(prior_weight, (int, float, np.integer, np.floating)):
        raise ArgumentError(f"prior_weight must be a finite number, got {prior_weight!r}")
    w = float(prior_weight)
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(w)):
            raise ArgumentError(f"prior_weight must be a finite fp32 number, got {prior_weight!r}")
    if not abs(float(np.float32(w))) * max_abs < FLT_MAX:
        raise ArgumentError(f"prior_weight {w!r} times the prior's largest |value| {max_abs!r} is not below FLT_MAX")
    return w


def _after_keywords(after, grouping, per_group, prior):
    """The `after=` of a search call against the keywords it is not offered with."""
    from ._lib import Unsupported
    if after is None:
        return
    for name, value in (("grouping", grouping), ("per_group", per_group), ("prior", prior)):
        if value is not None:
            raise Unsupported(f"after together with {name} is not supported: a cursor continues the ranking of passages by MaxSim")


def _after_arrays(after, B: int):
    """`after=(scores[B], pids[B])` of Searcher.search_batch as the two host arrays the C ABI takes."""
    from ._lib import ArgumentError
    if not isinstance(after, (tuple, list)) or len(after) != 2:
        raise ArgumentError("after must be a pair (scores, pids)")
    try:
        s = np.ascontiguousarray(after[0], dtype=np.float32).reshape(-1)
        raw = np.asarray(after[1]).reshape(-1)
        p = np.ascontiguousarray(raw, dtype=np.int64)
    except (TypeError, ValueError, OverflowError) as e:
        raise ArgumentError(f"after must be a pair (scores float32[{B}], pids int64[{B}]): {e}") from None
    if raw.dtype.kind not in "iu" or (raw.size and raw.dtype.kind == "u" and int(raw.max()) > np.iinfo(np.int64).max):
        raise ArgumentError(f"the cursor pids must be integers that fit int64, got dtype {raw.dtype}")
    if s.size != B or p.size != B:
        raise ArgumentError(f"after holds one cursor per query: {s.size} scores and {p.size} pids for {B} queries")
    if np.isnan(s).any():
        raise ArgumentError(f"the cursor score of query {int(np.nonzero(np.isnan(s))[0][0])} is NaN")
    return s, p


def _candidate_keywords(candidates, filters, want_scores=False):
    """The `candidates=` of a search call against the keywords it is not offered with, and the score output against it."""
    from ._lib import ArgumentError, Unsupported
    if candidates is None:
        if want_scores:
            raise ArgumentError("candidate scores need candidates=: they are the scores of the listed passages")
        return
    if filters is not None and (not isinstance(filters, (list, tuple)) or any(f is not None for f in filters)):
        raise Unsupported("candidates= together with filter(s)= is not supported: a list is the candidate set")


def _candidate_prior_keywords(candidate_priors, candidates, prior=None, per_group=None, after=None):
    """The `candidate_priors=` of a search call against the keywords it is not offered with: it needs `candidates=`, and a call
    has one additive term (the rules of `prior=`)."""
    from ._lib import ArgumentError, Unsupported
    if candidate_priors is None:
        return
    if candidates is None:
        raise ArgumentError("candidate_priors needs candidates=: it holds one value per listed passage")
    if prior is not None:
        raise Unsupported("candidate_priors together with prior is not supported: a call has one additive term")
    if isinstance(per_group, (int, np.integer)) and not isinstance(per_group, bool) and int(per_group) > 1:
        raise Unsupported("per_group together with candidate_priors is not supported: the hits of a grouped search take no "
                          "additive term (per_group=1 is the grouped search itself)")
    if after is not None:
        raise Unsupported("after together with candidate_priors is not supported: a cursor continues the ranking of passages "
                          "by MaxSim")


def _one_cursor(after):
    """The `after=(score, pid)` of a one-query call as the pair of one-element arrays search_batch takes."""
    from ._lib import ArgumentError
    if not isinstance(after, (tuple, list)) or len(after) != 2:
        raise ArgumentError("after must be a pair (score, pid)")
    return ([after[0]], [after[1]])


@dataclass(frozen=True)
class SearchKeywords:
    """The keywords of one search call (Searcher.search_batch describes each), in DeviceSearch's positional order.  Every
    public search method makes one from its own parameters; below that only the record travels, down to search_request.
    `candidate_scores`: where a call returns the list scores, whether it is to (`return_candidate_scores`); on the device
    route, the tensor they go to."""
    filters: object = None
    scope: object = "candidates"
    grouping: object = None
    per_group: object = None
    prior: object = None
    prior_weight: object = 1.0
    after: object = None
    candidates: object = None
    candidate_scores: object = None
    candidate_priors: object = None

    def check(self):
        """The keywords against each other, before anything is looked at more closely: the scope, then what `after`,
        `candidates` and `candidate_priors` are not offered with."""
        _scope_code(self.scope)
        _after_keywords(self.after, self.grouping, self.per_group, self.prior)
        _candidate_keywords(self.candidates, self.filters, self.candidate_scores is not None and self.candidate_scores is not False)
        _candidate_prior_keywords(self.candidate_priors, self.candidates, self.prior, self.per_group, self.after)

    @property
    def plain(self) -> bool:
        """No keyword is given: every field is at its default.  Spelled out, not looped, because DeviceSearch asks on every
        call; tests/test_search_keywords_cpu.py walks the fields, so one that is missing here fails there."""
        return (self.filters is None and self.scope == "candidates" and self.grouping is None and self.per_group is None
                and self.prior is None and self.prior_weight == 1.0 and self.after is None and self.candidates is None
                and self.candidate_scores is None and self.candidate_priors is None)

    def for_one_query(self) -> "SearchKeywords":
        """The keywords of a one-query call (`filter=`, `after=(score, pid)`, one list of candidates and of their priors) as
        those of a batch of one."""
        one = lambda v: None if v is None else [v]
        return replace(self, filters=one(self.filters), after=None if self.after is None else _one_cursor(self.after),
                       candidates=one(self.candidates), candidate_priors=one(self.candidate_priors))


def _float32_list(a, what: str) -> np.ndarray:
    """An array of numbers as float32, or ArgumentError."""
    from ._lib import ArgumentError
    try:
        raw = np.asarray(a)
    except (TypeError, ValueError) as e:
        raise ArgumentError(f"{what} must be numbers: {e}") from None
    if raw.dtype.kind not in "iuf" and raw.size:
        raise ArgumentError(f"{what} must be numbers, got dtype {raw.dtype}")
    with np.errstate(over="ignore"):
        return raw.astype(np.float32)


def _candidate_prior_arrays(candidate_priors, lists, B: int):
    """`candidate_priors=` of Searcher.search_batch beside the arrays of `candidates=` (`lists`, from _candidate_arrays) as the
    host block the C ABI takes and the largest listed |value|: (values (L, B) column-major float32, max_abs).  Ragged lists
    take a sequence of B arrays of the lists' lengths, padded with 0; the pair form takes an (L, B) block.  Only the values
    at positions below a list's length count: one of them that is not finite is ArgumentError."""
    from ._lib import ArgumentError
    _, lens, L, _, ragged = lists
    if ragged:
        if isinstance(candidate_priors, (str, bytes)) or not hasattr(candidate_priors, "__len__") or len(candidate_priors) != B:
            raise ArgumentError(f"candidate_priors holds one array of values per candidate list: {B} arrays for {B} queries")
        vals = np.zeros((L, B), dtype=np.float32, order="F")
        for b, v in enumerate(candidate_priors):
            v = _float32_list(v, f"the candidate priors of query {b}").reshape(-1)
            if v.size != int(lens[b]):
                raise ArgumentError(f"the candidate priors of query {b} hold {v.size} values for a list of {int(lens[b])} pids")
            vals[:v.size, b] = v
    else:
        vals = _float32_list(candidate_priors, "the candidate priors")
        if vals.shape != (L, B):
            raise ArgumentError(f"candidate_priors must be an (L={L}, B={B}) block beside candidates=(pids, lens), got {vals.shape}")
        vals = np.asfortranarray(vals)
    listed = np.arange(L)[:, None] < np.asarray(lens)[None, :]
    bad = np.argwhere(listed & ~np.isfinite(vals))
    if bad.size:
        b = int(bad[:, 1].min()); i = int(bad[bad[:, 1] == b, 0].min())
        raise ArgumentError(f"the candidate prior of query {b}, position {i} is not a finite number")
    return vals, float(np.abs(vals[listed]).max()) if listed.any() else 0.0


def _int64_list(a, what: str) -> np.ndarray:
    """An array of integers as int64, or ArgumentError: a float or a value past int64 is no pid and no length."""
    from ._lib import ArgumentError
    try:
        raw = np.asarray(a)
    except (TypeError, ValueError) as e:
        raise ArgumentError(f"{what} must be integers: {e}") from None
    if raw.size == 0 and raw.dtype.kind == "f":       # np.asarray([]) is float64
        raw = raw.astype(np.int64)
    if raw.dtype.kind not in "iu" or (raw.size and raw.dtype.kind == "u" and int(raw.max()) > np.iinfo(np.int64).max):
        raise ArgumentError(f"{what} must be integers that fit int64, got dtype {raw.dtype}")
    return raw.astype(np.int64, copy=False)


def _candidate_arrays(candidates, want_scores, B: int):
    """`candidates=` of Searcher.search_batch as the host arrays the C ABI takes: (pids, lens, L, scores or None, ragged).
    A sequence of B integer arrays (ragged) is padded with 0 into one block whose stride is the longest list; a pair
    `(pids (L, B), lens [B])` is taken as it is.  pids / scores are (L, B) column-major: row b of the C arrays is [:, b]."""
    from ._lib import ArgumentError
    pair = isinstance(candidates, tuple) and len(candidates) == 2 and np.ndim(candidates[0]) == 2
    if pair:
        block = _int64_list(candidates[0], "the candidate pids")
        lens = _int64_list(candidates[1], "the candidate list lengths").reshape(-1)
        L = block.shape[0]
        if L < 1 or block.shape[1] != B or lens.size != B:
            raise ArgumentError(f"candidates=(pids, lens) holds one list per query: pids {block.shape} (L >= 1, B) and {lens.size} "
                                f"lengths for {B} queries")
        if lens.size and (int(lens.min()) < 0 or int(lens.max()) > L):
            raise ArgumentError(f"the candidate list lengths must lie in 0..{L}, got {int(lens.min())}..{int(lens.max())}")
        pids = np.asfortranarray(block)
    else:
        if isinstance(candidates, (str, bytes)) or not hasattr(candidates, "__len__"):
            raise ArgumentError("candidates must be a sequence of integer arrays, one per query, or a pair (pids (L, B), lens [B])")
        if len(candidates) != B:
            raise ArgumentError(f"candidates holds one list per query: {len(candidates)} lists for {B} queries")
        lists = [_int64_list(c, f"the candidate list of query {b}").reshape(-1) for b, c in enumerate(candidates)]
        lens = np.array([c.size for c in lists], dtype=np.int64)
        L = max(1, int(lens.max()) if B else 1)
        pids = np.zeros((L, B), dtype=np.int64, order="F")
        for b, c in enumerate(lists):
            pids[:c.size, b] = c
    scores = np.full((L, B), -np.inf, dtype=np.float32, order="F") if want_scores else None
    return pids, np.ascontiguousarray(lens), L, scores, not pair


def search_request(searcher, B: int, *, filters=None, scope="candidates", grouping=None, per_group=None, prior=None,
                   prior_weight=1.0, after=None, pad_short=False, group_base: int = 0, cursor_arrays=_after_arrays,
                   candidates=None, candidate_scores=None, candidate_arrays=_candidate_arrays, candidate_priors=None,
                   candidate_prior_arrays=_candidate_prior_arrays, keywords: Optional[SearchKeywords] = None) -> SearchRequest:
    """The keywords of a search call of `searcher` over B queries -- by name, or as the ready-made record `keywords`, which then
    counts alone -- checked on the host, as the clb_search_request every
    search entry point takes (include/colbert_hip.h).  Raises what the helpers above raise, in their order: scope, `after`
    against the keywords it is not offered with, the cursors, the prior and its weight (never with `per_group`), `per_group`,
    the filters, the grouping.  With filters or cursors the host route always pads.  `cursor_arrays(after, B)` gives the two cursor
    arrays: host arrays here, DeviceSearch passes its own check of device tensors.  The request holds a reference to every
    array it points at (`_keep`): it is valid as long as it lives.
    `candidates` (Searcher.search_batch) with `candidate_scores` (true: the call is to leave the list scores): never with
    filters (Unsupported); `candidate_arrays(candidates, candidate_scores, B)` gives (pids, lens, L, scores or None, ragged) --
    host arrays here, with the int64 conversion and the padding of ragged lists, device tensors from DeviceSearch -- which
    the request keeps as `lists`; with lists the host route always pads.
    `candidate_priors` (Searcher.search_batch) with `prior_weight`: needs `candidates` (ArgumentError), never with `prior`,
    `per_group` > 1 or `after` (Unsupported); `candidate_prior_arrays(candidate_priors, lists, B)` gives (values, max_abs) -- the
    host block here, checked value by value, the device tensor from DeviceSearch with max_abs 0 (nothing is read back) -- and
    the weight is checked against that max_abs as a prior's is."""
    kw = keywords if keywords is not None else SearchKeywords(
        filters=filters, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
        candidates=candidates, candidate_scores=candidate_scores, candidate_priors=candidate_priors)
    kw.check()
    r = SearchRequest(struct_bytes=C.sizeof(SearchRequest), scope=_scope_code(kw.scope), group_base=int(group_base),
                      pad_short=1 if (pad_short or kw.filters is not None or kw.after is not None or kw.candidates is not None) else 0)
    r.lists = None
    ptr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    if kw.candidates is not None:
        r.lists = tuple(candidate_arrays(kw.candidates, kw.candidate_scores, B))
        r.list_pids, r.list_lens, r.list_stride, r.list_scores = ptr(r.lists[0]), ptr(r.lists[1]), int(r.lists[2]), ptr(r.lists[3])
        if kw.candidate_priors is not None:
            values, max_abs = candidate_prior_arrays(kw.candidate_priors, r.lists, B)
            r.prior_weight = _weight_value(kw.prior_weight, max_abs)
            r.list_prior = ptr(values)
            r.lists += (values,)
    cursors = ()
    if kw.after is not None:
        cursors = tuple(cursor_arrays(kw.after, B))
        r.after_scores, r.after_pids = (ptr(a) for a in cursors)
    if kw.prior is not None:
        r.prior_weight = _prior_weight(kw.prior, kw.prior_weight, kw.per_group)
        r.prior = kw.prior._h
    if kw.per_group is not None:
        r.per_group = _per_group(kw.per_group, kw.grouping)
    handles = None if kw.filters is None else searcher._filter_handles(kw.filters, B)
    if handles is not None:
        r.filters = handles
    if kw.grouping is not None:
        r.grouping = searcher._grouping_handle(kw.grouping)
    r._keep = (handles, cursors)
    return r


def next_cursor(pids, scores):
    """The cursor that continues after a result: its last row, `(scores[k-1], pids[k-1])` -- per query for the (k, B) arrays of
    `search_batch` (pass it as `after=`), a `(score, pid)` pair for the k-vectors of `search_embeddings` / `search`.  A padded
    last row yields (-Inf, 0): the ranking is finished, and the page after it is empty."""
    p, s = np.asarray(pids), np.asarray(scores, dtype=np.float32)
    if p.shape != s.shape or p.ndim not in (1, 2) or p.shape[0] < 1:
        raise ColBERTError(f"next_cursor takes the pids and scores of one result, got shapes {p.shape} and {s.shape}")
    last_s, last_p = s[-1].copy(), p[-1].astype(np.int64)
    if p.ndim == 1:
        return (float("-inf"), 0) if last_p == 0 else (np.float32(last_s), int(last_p))
    last_s[last_p == 0] = -np.inf
    return last_s, last_p


class Searcher:
    """struct Searcher (searching.jl:1-16).  Fields that the reference holds as arrays live in HBM
    behind `self._h`; the shapes/meta are kept for introspection."""

    def __init__(self, index_path: Optional[str] = None, *, config: Optional[ColBERTConfig] = None,
                 index: Optional[dict] = None, device: int = 0, pid_offset: int = 0, encoder=None):
        if index is None:
            if index_path is None:
                raise ValueError("Searcher needs an index_path or an in-memory index")
            config = ColBERTConfig.load(index_path)
            index = storage.load_index(index_path)
        self.config = config or ColBERTConfig(nbits=int(index["nbits"]), dim=int(index["dim"]))
        self.device = device
        self.encoder = encoder
        self.index_path = index_path          # where add_*(..., persist=True) writes
        self.pid_offset = int(pid_offset)
        # what add_embeddings compresses with: the index's own centroids and cutoffs (references, not copies)
        self._codec_src = (index["centroids"], index.get("bucket_cutoffs"))
        self._codec = None
        self.dim = int(index["dim"]); self.nbits = int(index["nbits"])
        if hasattr(index["codes"], "data_ptr"):
            self._create_from_device_arrays(index, pid_offset)
            return
        c = colmajor(index["centroids"], np.float32)
        w = np.ascontiguousarray(index["bucket_weights"], dtype=np.float32)
        dl = np.ascontiguousarray(index["doclens"], dtype=np.int64)
        co = np.ascontiguousarray(index["codes"], dtype=np.uint32)
        r = colmajor(index["residuals"], np.uint8)
        iv = np.ascontiguousarray(index["ivf"], dtype=np.int64)
        il = np.ascontiguousarray(index["ivf_lengths"], dtype=np.int64)
        if c.shape[0] != self.dim:
            raise ColBERTError("centroids must be (dim, K)")
        if r.shape != (self.dim // 8 * self.nbits, co.size):
            raise ColBERTError("residuals must be (dim/8*nbits, n_emb)")
        if il.size != c.shape[1]:
            raise ColBERTError("ivf_lengths must have one entry per centroid")
        self.num_centroids = c.shape[1]; self.num_docs = dl.size; self.num_embeddings = co.size
        self._h = C.c_void_p()
        check(lib().clb_searcher_create(device, i64(self.dim), C.c_int(self.nbits), i64(c.shape[1]), fptr(c), fptr(w),
                                        i64(dl.size), fptr(dl), i64(co.size), fptr(co), fptr(r), fptr(iv), fptr(il),
                                        i64(pid_offset), C.byref(self._h)))

    def _create_from_device_arrays(self, index: dict, pid_offset: int):
        """An index that was built in HBM (indexer.index_device): centroids (K, dim) float32, codes int32/uint32 [n],
        residuals uint8 (n, dim/8*nbits), ivf int64 [n] as CUDA tensors; doclens / ivf_lengths / bucket_weights on the
        host (numpy or tensors) -- clb_searcher_create_device."""
        import torch
        c, co, r, iv = index["centroids"], index["codes"], index["residuals"], index["ivf"]
        for t in (c, co, r, iv):
            if not (t.is_cuda and t.is_contiguous()):
                raise ColBERTError("device index arrays must be contiguous CUDA tensors")
        host = lambda a, dt: np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "data_ptr") else a, dtype=dt)
        w, dl, il = host(index["bucket_weights"], np.float32), host(index["doclens"], np.int64), host(index["ivf_lengths"], np.int64)
        if c.dtype != torch.float32 or c.shape[1] != self.dim:
            raise ColBERTError("centroids must be a (K, dim) float32 tensor")
        if co.element_size() != 4 or r.dtype != torch.uint8 or iv.dtype != torch.int64:
            raise ColBERTError("codes must be 32-bit, residuals uint8, ivf int64")
        if tuple(r.shape) != (co.numel(), self.dim // 8 * self.nbits):
            raise ColBERTError("residuals must be (n_emb, dim/8*nbits)")
        if il.size != c.shape[0]:
            raise ColBERTError("ivf_lengths must have one entry per centroid")
        self.device = c.device.index
        self.num_centroids = int(c.shape[0]); self.num_docs = dl.size; self.num_embeddings = co.numel()
        torch.cuda.synchronize(c.device)
        self._h = C.c_void_p()
        check(lib().clb_searcher_create_device(self.device, i64(self.dim), C.c_int(self.nbits), i64(c.shape[0]),
                                               C.c_void_p(c.data_ptr()), fptr(w), i64(dl.size), fptr(dl), i64(co.numel()),
                                               C.c_void_p(co.data_ptr()), C.c_void_p(r.data_ptr()), C.c_void_p(iv.data_ptr()),
                                               fptr(il), i64(pid_offset), C.byref(self._h)))

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_codec", None) is not None:
            self._codec.close()
            self._codec = None
        if getattr(self, "_h", None):
            lib().clb_searcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ingest: append passages to the resident index (clb_searcher_append) ---------------------------
    @property
    def generation(self) -> int:
        """Number of appends, removals and updates that changed this searcher (0 after the constructor).  A HIP graph captured
        over the searcher belongs to the generation it was made in; a PassageFilter outlives removals and updates, not appends."""
        return int(lib().clb_searcher_generation(self._h))

    def _check_device_rows(self, codes, residuals):
        """compressed rows as CUDA tensors -- `codes` 32-bit [n], `residuals` uint8 (n, dim/8*nbits) on this searcher's
        device -> the HIP stream that produced them"""
        import torch
        if not (codes.is_cuda and residuals.is_cuda and codes.is_contiguous() and residuals.is_contiguous()
                and codes.device.index == self.device and residuals.device.index == self.device):
            raise ColBERTError("device arrays must be contiguous CUDA tensors on the searcher's device")
        if codes.element_size() != 4 or codes.dim() != 1 or residuals.dtype != torch.uint8:
            raise ColBERTError("codes must be a 32-bit vector, residuals uint8")
        if tuple(residuals.shape) != (codes.numel(), self.dim // 8 * self.nbits):
            raise ColBERTError("residuals must be (n_emb, dim/8*nbits)")
        return torch.cuda.current_stream(codes.device).cuda_stream

    @staticmethod
    def _rows_to_host(codes, residuals):
        """device rows in the layout of the index directory: codes UInt32[n], residuals (dim/8*nbits, n) column-major"""
        return codes.cpu().numpy().view(np.uint32), np.asfortranarray(residuals.cpu().numpy().T)

    def _check_host_rows(self, codes, residuals):
        """compressed rows as numpy arrays -> codes UInt32[n], residuals (dim/8*nbits, n) column-major"""
        co = np.ascontiguousarray(codes, dtype=np.uint32)
        r = colmajor(residuals, np.uint8)
        if co.ndim != 1 or r.shape != (self.dim // 8 * self.nbits, co.size):
            raise ColBERTError("residuals must be (dim/8*nbits, n_emb)")
        return co, r

    def add_compressed(self, codes, residuals, doclens, persist: bool = False) -> range:
        """Append passages compressed with the index's own codec behind the last passage, without rebuilding the resident
        index; returns the range of their pids.  Layouts as in the constructor: numpy `codes` UInt32[n] (1-based) and
        `residuals` (dim/8*nbits, n), or CUDA tensors `codes` 32-bit [n] and `residuals` uint8 (n, dim/8*nbits) on this
        searcher's device (clb_searcher_append_device); `doclens` on the host.  Afterwards every search answers as a
        Searcher made from the concatenated index would; filters made before must be made again.  If the call raises,
        the searcher is unchanged.  `persist`: also write the passages to the index directory the searcher was opened
        from (storage.append_chunk), after the device append has succeeded."""
        if persist and self.index_path is None:
            raise ColBERTError("persist=True needs a Searcher opened from an index_path")
        dl = np.ascontiguousarray(np.asarray(doclens.cpu() if hasattr(doclens, "data_ptr") else doclens), dtype=np.int64)
        first = self.pid_offset + self.num_docs + 1
        if hasattr(codes, "data_ptr"):
            st = self._check_device_rows(codes, residuals)
            check(lib().clb_searcher_append_device(self._h, i64(dl.size), fptr(dl), i64(codes.numel()),
                                                   C.c_void_p(codes.data_ptr()), C.c_void_p(residuals.data_ptr()),
                                                   C.c_void_p(st)))
            if persist:
                co, r = self._rows_to_host(codes, residuals)
        else:
            co, r = self._check_host_rows(codes, residuals)
            check(lib().clb_searcher_append(self._h, i64(dl.size), fptr(dl), i64(co.size), fptr(co), fptr(r)))
        self.num_docs = int(lib().clb_searcher_num_docs(self._h))
        self.num_embeddings = int(lib().clb_searcher_num_embeddings(self._h))
        if persist and dl.size:
            storage.append_chunk(self.index_path, co, r, dl)
        return range(first, self.pid_offset + self.num_docs + 1)

    def remove_passages(self, pids, persist: bool = False) -> int:
        """Remove passages from the resident index without rebuilding it (clb_searcher_remove); returns how many lost
        embeddings.  `pids` as `search` returns them (1-based, this searcher's pid_offset included; any order, duplicates
        allowed; outside the searcher's passages: BoundsError).  Pids are stable: a removed passage stays in the numbering
        as an empty passage, `num_docs` does not change, and a later add numbers from `num_docs + 1` as before.  Afterwards
        every search answers as a Searcher made from the reduced index would; filters made before stay valid.  If the call
        raises, the searcher is unchanged.  `persist`: also rewrite the index directory the searcher was opened from
        (storage.remove_passages), after the device call has succeeded."""
        if persist and self.index_path is None:
            raise ColBERTError("persist=True needs a Searcher opened from an index_path")
        p = np.ascontiguousarray(np.asarray(pids).reshape(-1), dtype=np.int64)
        n = i64(0)
        check(lib().clb_searcher_remove(self._h, fptr(p), i64(p.size), C.byref(n)))
        self.num_embeddings = int(lib().clb_searcher_num_embeddings(self._h))
        if persist and n.value:
            storage.remove_passages(self.index_path, p - self.pid_offset)
        return int(n.value)

    def update_compressed(self, pids, codes, residuals, doclens, persist: bool = False) -> int:
        """Replace the content of passages in place, keeping their pids (clb_searcher_update): passage `pids[i]` loses its
        embeddings and receives the next `doclens[i]` columns of `codes` / `residuals` (compressed with the index's own
        codec; layouts and checks as in `add_compressed`: numpy arrays, or CUDA tensors on this searcher's device).  `pids`
        as `search` returns them, in any order, each at most once (twice: ArgumentError; outside the searcher's passages:
        BoundsError).  A doclen of 0 empties a passage as `remove_passages` does; an empty passage may be filled again.
        `num_docs` and every other pid are unchanged.  Returns how many named passages had or have embeddings.  Afterwards
        every search answers as a Searcher made from the changed index would; filters made before stay valid.  If the call
        raises, the searcher is unchanged.  `persist`: also rewrite the index directory the searcher was opened from
        (storage.update_passages), after the device call has succeeded."""
        if persist and self.index_path is None:
            raise ColBERTError("persist=True needs a Searcher opened from an index_path")
        p = np.ascontiguousarray(np.asarray(pids.cpu() if hasattr(pids, "data_ptr") else pids).reshape(-1), dtype=np.int64)
        dl = np.ascontiguousarray(np.asarray(doclens.cpu() if hasattr(doclens, "data_ptr") else doclens).reshape(-1), dtype=np.int64)
        if p.size != dl.size:
            raise ColBERTError(f"one doclen per pid: {p.size} pids, {dl.size} doclens")
        n = i64(0)
        if hasattr(codes, "data_ptr"):
            st = self._check_device_rows(codes, residuals)
            check(lib().clb_searcher_update_device(self._h, i64(p.size), fptr(p), fptr(dl), i64(codes.numel()),
                                                   C.c_void_p(codes.data_ptr()), C.c_void_p(residuals.data_ptr()),
                                                   C.c_void_p(st), C.byref(n)))
            if persist:
                co, r = self._rows_to_host(codes, residuals)
        else:
            co, r = self._check_host_rows(codes, residuals)
            check(lib().clb_searcher_update(self._h, i64(p.size), fptr(p), fptr(dl), i64(co.size), fptr(co), fptr(r),
                                            C.byref(n)))
        self.num_embeddings = int(lib().clb_searcher_num_embeddings(self._h))
        if persist and n.value:
            storage.update_passages(self.index_path, p - self.pid_offset, co, r, dl)
        return int(n.value)

    def update_embeddings(self, pids, embs, doclens, persist: bool = False) -> int:
        """Compress passage embeddings with the index's own codec on the device, as `add_embeddings` does, and put them in
        the place of the passages `pids` (update_compressed): `embs` numpy (dim, n) or a CUDA tensor (n, dim) float32."""
        codes, res = self._compress(embs)
        return self.update_compressed(pids, codes, res, doclens, persist=persist)

    def update_passages(self, pids, texts, persist: bool = False) -> int:
        """encode_passages (checkpoint.jl:159-189) with the attached encoder, then update_embeddings: texts[i] becomes the
        content of passage pids[i]."""
        if self.encoder is None:
            raise ColBERTError("no encoder attached: pass encoder=... or use update_embeddings(pids, embs, doclens)")
        embs, doclens = self.encoder.encode_passages(list(texts))
        return self.update_embeddings(pids, embs, doclens, persist=persist)

    def _index_codec(self):
        """The index's own codec, resident (codec.Codec): built on first use from the centroids and bucket_cutoffs the
        index dict or directory carries -- the codec stays fixed over appends."""
        if self._codec is None:
            from .codec import Codec
            cent, cut = self._codec_src
            if cut is None:
                raise ColBERTError("this index carries no bucket_cutoffs: embeddings cannot be compressed with its codec "
                                   "(pass an index with 'bucket_cutoffs', or use add_compressed)")
            cut = np.asarray(cut.cpu() if hasattr(cut, "data_ptr") else cut, dtype=np.float32)
            self._codec = Codec(cent, cut, self.dim, self.nbits, device=self.device)
        return self._codec

    def _compress(self, embs):
        """`embs` numpy (dim, n) or a CUDA tensor (n, dim) float32 -> (codes, residuals) on the device, by the index's codec"""
        import torch
        codec = self._index_codec()
        if hasattr(embs, "data_ptr"):
            x = embs
        else:
            e = colmajor(embs, np.float32)
            if e.ndim != 2 or e.shape[0] != self.dim:
                raise ColBERTError(f"embs must be (dim={self.dim}, n)")
            x = torch.from_numpy(np.ascontiguousarray(e.T)).to(torch.device("cuda", self.device))
        return codec.compress_device(x)

    def add_embeddings(self, embs, doclens, persist: bool = False) -> range:
        """Compress passage embeddings with the index's own codec on the device (compress, residual.jl:586-604) and append
        them: `embs` numpy (dim, n) or a CUDA tensor (n, dim) float32, `doclens` their passages' lengths.  -> the new pids."""
        codes, res = self._compress(embs)
        return self.add_compressed(codes, res, doclens, persist=persist)

    def add_passages(self, texts, persist: bool = False) -> range:
        """encode_passages (checkpoint.jl:159-189) with the attached encoder, then add_embeddings.  -> the new pids."""
        if self.encoder is None:
            raise ColBERTError("no encoder attached: pass encoder=... or use add_embeddings(embs, doclens)")
        embs, doclens = self.encoder.encode_passages(list(texts))
        return self.add_embeddings(embs, doclens, persist=persist)

    @property
    def device_bytes(self) -> int:
        return int(lib().clb_searcher_device_bytes(self._h))

    def set_mode(self, mode: int):
        check(lib().clb_searcher_set_mode(self._h, C.c_int(mode)))

    def set_wide_select(self, on: int):
        """-1: the selection step picks one or sixteen work-groups per query by the candidate capacity; 0 / 1 force it."""
        check(lib().clb_searcher_set_wide_select(self._h, C.c_int(on)))

    def set_pass1_gather(self, form: int):
        """-1: pass 1 picks its gather form from the index's code statistics; 0 / 1 force the VGPR / LDS-DMA form."""
        check(lib().clb_searcher_set_pass1_gather(self._h, C.c_int(form)))

    @property
    def pass1_gather(self):
        """(form in use: 0 VGPR / 1 LDS-DMA, code adjacency statistic of the index)"""
        adj = C.c_double(0)
        return int(lib().clb_searcher_get_pass1_gather(self._h, C.byref(adj))), adj.value

    def set_score_rows(self, form: int):
        """Batches of 16+ queries, two-pass mode: 0 = 64-byte fp16 score rows, 1 = 32-byte rows of 8-bit cells, -1 = default
        (0: the 8-bit format is faster in pass 1 only; set it alike on every shard of a group)."""
        check(lib().clb_searcher_set_score_rows(self._h, C.c_int(form)))

    @property
    def score_rows(self) -> int:
        """row format batches of 16+ queries take: 0 fp16 (64 B), 1 8-bit cells (32 B)"""
        return int(lib().clb_searcher_get_score_rows(self._h))

    def set_centroid_products(self, n: int):
        """Batches of 16+ queries, two-pass mode: 1 = score table from one fp16 product, 3 = the bf16 split, -1 = default (1 on a shard of a group, 3 on one GPU)."""
        check(lib().clb_searcher_set_centroid_products(self._h, C.c_int(n)))

    @property
    def centroid_products(self):
        """(products in use for batches of 16+ queries: 1 or 3, max ||c - fp16(c)|| over the centroids)"""
        dc = C.c_float(0)
        return int(lib().clb_searcher_get_centroid_products(self._h, C.byref(dc))), dc.value

    @property
    def mode(self) -> int:
        return int(lib().clb_searcher_get_mode(self._h))

    @property
    def bound_consts(self) -> np.ndarray:
        """The six constants of this handle's error bound (include/colbert_hip.h, clb_searcher_get_bound_consts)."""
        out = np.zeros(6, dtype=np.float32)
        check(lib().clb_searcher_get_bound_consts(self._h, fptr(out)))
        return out

    def raise_bound_consts(self, consts):
        """Element-wise maximum with `consts` (sharded search: one bound on every shard, distributed.sync_bound_consts)."""
        c = np.ascontiguousarray(consts, dtype=np.float32)
        assert c.shape == (6,)
        check(lib().clb_searcher_set_bound_consts(self._h, fptr(c)))

    # -- filters ----------------------------------------------------------------------------------
    def make_filter(self, pids=None, mask=None) -> PassageFilter:
        """A resident passage set for filtered search.  Exactly one of: `pids`, passage ids as `search` returns them
        (1-based, this searcher's pid_offset included; any order, duplicates allowed; outside the searcher's passages:
        BoundsError), or `mask`, a boolean array of `num_docs` entries (entry i = local passage i + 1)."""
        if (pids is None) == (mask is None):
            raise ColBERTError("make_filter takes exactly one of pids= and mask=")
        h = C.c_void_p()
        if pids is not None:
            p = np.ascontiguousarray(np.asarray(pids).reshape(-1), dtype=np.int64)
            check(lib().clb_filter_create_pids(self._h, fptr(p), i64(p.size), C.byref(h)))
        else:
            m = np.asarray(mask)
            if m.dtype != np.bool_ or m.shape != (self.num_docs,):
                raise ColBERTError(f"mask must be a boolean array of num_docs={self.num_docs} entries")
            words = np.ascontiguousarray(np.packbits(m, bitorder="little"))
            words = np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view("<u4")
            check(lib().clb_filter_create_bitmap(self._h, fptr(words), i64(words.size), C.byref(h)))
        return PassageFilter(self, h, lib().clb_filter_count(h))

    def _filter_handles(self, filters, B: int):
        """`filters` of a search call -> a ctypes array of B clb_filter handles (NULL = that query is unfiltered)."""
        if isinstance(filters, PassageFilter):
            filters = [filters] * B
        filters = list(filters)
        if len(filters) != B:
            raise ColBERTError(f"filters must be one PassageFilter or a sequence of B={B} entries (None = unfiltered)")
        arr = (C.c_void_p * B)()
        for j, f in enumerate(filters):
            if f is None:
                continue
            if not isinstance(f, PassageFilter) or not f._h:
                raise ColBERTError(f"filters[{j}] is not an open PassageFilter")
            arr[j] = f._h.value
        return arr

    def combine_filters(self, op: str, filters) -> PassageFilter:
        """A new filter from filters of this searcher, computed on the device (clb_filter_combine): `op` "and" (the
        intersection of all), "or" (their union), "andnot" (filters[0] minus the union of the rest) or "not" (the complement
        of the single filter).  1..16 filters, exactly one for "not"; "and" / "or" / "andnot" of one filter is a copy.  The
        operands are only read -- the same one may appear twice, and they may be closed once the call returns.  `a & b`,
        `a | b`, `a - b` and `~a` are the two-operand forms; this one avoids their temporaries."""
        from ._lib import ArgumentError
        if op not in _FILTER_OPS:
            raise ArgumentError(f"op must be 'and', 'or', 'andnot' or 'not', got {op!r}")
        filters = [filters] if isinstance(filters, PassageFilter) else list(filters)
        n = len(filters)
        if not 1 <= n <= MAX_FILTER_OPERANDS:
            raise ArgumentError(f"combine_filters takes 1..{MAX_FILTER_OPERANDS} filters, got {n}")
        if op == "not" and n != 1:
            raise ArgumentError(f"'not' takes exactly one filter, got {n}")
        for j, f in enumerate(filters):
            if f is None:           # (an unfiltered query to _filter_handles; no operand here)
                raise ColBERTError(f"filters[{j}] is not an open PassageFilter")
        arr = self._filter_handles(filters, n)
        h = C.c_void_p()
        check(lib().clb_filter_combine(self._h, C.c_int(_FILTER_OPS[op]), arr, i64(n), C.byref(h)))
        return PassageFilter(self, h, lib().clb_filter_count(h))

    def make_range_filter(self, prior, lo=None, hi=None, lo_open: bool = False, hi_open: bool = False) -> PassageFilter:
        """The passages whose value in `prior` (a PassagePrior of this searcher: the attribute, one fp32 value per passage)
        lies between `lo` and `hi`, computed on the device (clb_filter_create_range).  `None` is an open end; a bound is
        converted to float32 (integers are exact up to 2^24) and compared as IEEE does (-0 equals +0); `lo_open` / `hi_open`
        exclude the bound itself.  lo > hi, or lo == hi with an open end, is the empty filter; lo == hi is equality.  A bound
        that is not a real number is an ArgumentError."""
        if not isinstance(prior, PassagePrior) or not prior._h:
            raise ColBERTError("prior is not an open PassagePrior")
        lo32, hi32 = _range_bound(lo, "lo", -np.inf), _range_bound(hi, "hi", np.inf)
        flags = (1 if lo_open else 0) | (2 if hi_open else 0)           # CLB_RANGE_LO_OPEN / CLB_RANGE_HI_OPEN
        h = C.c_void_p()
        check(lib().clb_filter_create_range(self._h, prior._h, C.c_float(lo32), C.c_float(hi32), C.c_int(flags), C.byref(h)))
        return PassageFilter(self, h, lib().clb_filter_count(h))

    # -- groupings --------------------------------------------------------------------------------
    def make_grouping(self, group_ids=None, group_lens=None) -> PassageGrouping:
        """A resident passage -> document map for grouped search (`grouping=` of the search calls: the top-k DOCUMENTS, each
        by its best passage).  Exactly one of: `group_ids`, one integer per passage (`num_docs` entries, entry i = local
        passage i + 1), non-decreasing -- equal ids are one contiguous pid range, anything else is an ArgumentError naming the
        passage where the ids decrease -- or `group_lens`, the number of passages of every document in pid order (non-negative,
        summing to `num_docs`; document j gets id j, 0-based)."""
        if (group_ids is None) == (group_lens is None):
            raise ColBERTError("make_grouping takes exactly one of group_ids= and group_lens=")
        if group_lens is not None:
            lens = np.asarray(group_lens)
            if lens.ndim != 1 or lens.dtype.kind not in "iu" or (lens.size and int(lens.min()) < 0) or int(lens.sum()) != self.num_docs:
                raise ColBERTError(f"group_lens must be non-negative integers summing to num_docs={self.num_docs}")
            ids = np.repeat(np.arange(lens.size, dtype=np.int64), lens.astype(np.int64))
        else:
            ids = np.asarray(group_ids)
            if ids.ndim != 1 or ids.dtype.kind not in "iu":
                raise ColBERTError("group_ids must be a vector of integers, one per passage")
            ids = np.ascontiguousarray(ids, dtype=np.int64).copy()
        h = C.c_void_p()
        check(lib().clb_grouping_create(self._h, fptr(ids), i64(ids.size), C.byref(h)))
        return PassageGrouping(self, h, lib().clb_grouping_count(h), ids)

    def _grouping_handle(self, grouping):
        if not isinstance(grouping, PassageGrouping) or not grouping._h:
            raise ColBERTError("grouping is not an open PassageGrouping")
        return grouping._h

    # -- priors -----------------------------------------------------------------------------------
    def make_prior(self, values) -> PassagePrior:
        """A resident per-passage score term for `prior=` of the search calls: `values`, one finite number per passage
        (`num_docs` entries, entry i = local passage i + 1) as a numpy array (converted to float32) or a contiguous float32
        CUDA tensor on this searcher's device (clb_prior_create_device: checked on the device).  A wrong length or a value
        that is not finite in fp32 is an ArgumentError, naming the first offending passage."""
        from ._lib import ArgumentError
        h = C.c_void_p()
        if hasattr(values, "data_ptr"):
            import torch
            if not (values.is_cuda and values.is_contiguous() and values.device.index == self.device
                    and values.dtype == torch.float32 and values.dim() == 1):
                raise ArgumentError("a device prior must be a contiguous float32 CUDA vector on the searcher's device")
            if values.numel() != self.num_docs:
                raise ArgumentError(f"a prior holds one value per passage: {values.numel()} values, num_docs={self.num_docs}")
            torch.cuda.current_stream(values.device).synchronize()
            check(lib().clb_prior_create_device(self._h, C.c_void_p(values.data_ptr()), i64(values.numel()), C.byref(h)))
            n = values.numel()
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                v = np.ascontiguousarray(np.asarray(values), dtype=np.float32)
            if v.ndim != 1 or v.size != self.num_docs:
                raise ArgumentError(f"a prior holds one value per passage: shape {v.shape}, num_docs={self.num_docs}")
            bad = np.nonzero(~np.isfinite(v))[0]
            if bad.size:
                raise ArgumentError(f"the prior of passage {self.pid_offset + int(bad[0]) + 1} is not a finite number")
            check(lib().clb_prior_create(self._h, fptr(v), i64(v.size), C.byref(h)))
            n = v.size
        return PassagePrior(self, h, n, lib().clb_prior_max_abs(h))

    # -- search -----------------------------------------------------------------------------------
    def search_embeddings(self, Q, k: int, nprobe: Optional[int] = None, *, filter=None, scope="candidates", grouping=None,
                          per_group=None, prior=None, prior_weight=1.0, after=None, candidates=None,
                          return_candidate_scores=False, candidate_priors=None):
        """search() after encode_queries (searching.jl:102-127).  Q: (dim, T) Float32.
        Returns (pids Int64[k] 1-based, scores Float32[k]).
        `filter` (a PassageFilter of this searcher): search among its passages only -- scope "candidates": the query's
        candidates that are in the filter; "all": every passage of the filter (a re-rank of that list).  A filtered search
        never raises for a short result: the k-vectors come back padded, entries past min(k, last_num_candidates) are
        pid 0 / -Inf.
        `grouping` (a PassageGrouping of this searcher): the top-k GROUPS, each by its best passage (that passage's pid and
        score; `grouping.groups_of(pids)` gives the groups); last_num_candidates then counts the candidate groups, and fewer
        than k of them raise BoundsError as fewer than k candidates do without a grouping (never with a filter).
        `per_group` (an integer m, 1..16, with `grouping`): pids and scores are (m, k) -- column j the m best candidate
        passages of the j-th group, best first, padded with pid 0 / -Inf (Searcher.search_batch).
        `prior` (a PassagePrior of this searcher) with `prior_weight`: rank by score + prior_weight * value and return that
        sum as the score (Searcher.search_batch); short results as without a prior.
        `after` (a pair (score, pid), e.g. `next_cursor` of the previous page): the next k results past that cursor, always
        padded (Searcher.search_batch); not with `grouping`, `per_group` or `prior`.
        `candidates` (one array of pids): re-rank exactly these passages (Searcher.search_batch), always padded; with
        `return_candidate_scores=True` the call returns (pids, scores, candidate_scores), the third the score of every listed
        pid at its position.  Not with `filter`.
        `candidate_priors` (one array of values, one per listed pid) with `prior_weight`: rank the listed passages by score +
        prior_weight * value (Searcher.search_batch); not with `prior`, `per_group` > 1 or `after`."""
        return self._search_embeddings(Q, k, nprobe, SearchKeywords(
            filters=filter, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=True if return_candidate_scores else None, candidate_priors=candidate_priors))

    def _search_embeddings(self, Q, k: int, nprobe, kw: SearchKeywords):
        """search_embeddings with its keywords as the record of a ONE-QUERY call (`filters`: the filter)."""
        q = colmajor(Q, np.float32)
        if q.ndim != 2 or q.shape[0] != self.dim:
            raise ColBERTError(f"Q must be (dim={self.dim}, T)")
        kw.check()
        if kw.plain:                               # clb_search: the call the reference makes, short results included
            pids = np.zeros(k, dtype=np.int64); scores = np.zeros(k, dtype=np.float32)
            ncand = i64(0)
            check(lib().clb_search(self._h, fptr(q), i64(q.shape[1]), i64(nprobe or self.config.nprobe), i64(k), fptr(pids),
                                   fptr(scores), C.byref(ncand)))
            self.last_num_candidates = ncand.value
            return pids, scores
        out = self._search_batch(q.reshape(q.shape + (1,), order="F"), k, nprobe, False, kw.for_one_query())
        self.last_num_candidates = int(out[2][0])
        one = (np.asfortranarray(out[0][..., 0]), np.asfortranarray(out[1][..., 0]))
        return one + (out[3][0],) if kw.candidate_scores else one

    def search_batch(self, Q, k: int, nprobe: Optional[int] = None, pad_short: bool = False, *, filters=None,
                     scope="candidates", grouping=None, per_group=None, prior=None, prior_weight=1.0, after=None,
                     candidates=None, return_candidate_scores=False, candidate_priors=None):
        """B queries: Q (dim, T, B) -> (pids (k, B), scores (k, B), n_candidates[B]); one call of clb_search_batch_request.
        `filters`: one PassageFilter for every query, or a sequence of B entries (None = that query is unfiltered); with
        filters the results are always padded (pid 0 / -Inf past n_candidates[b], the count AFTER the filter) and `scope`
        is "candidates" (candidates that are in the filter) or "all" (the filter's passages themselves).
        `grouping`: one PassageGrouping for the whole batch -- every query returns its k best GROUPS, each by its best
        passage, and n_candidates counts the candidate groups (after any filter); short results as without a grouping.
        `per_group` (an integer m, 1..16; needs `grouping`): pids and scores are (m, k, B) -- [:, j, b] the m best CANDIDATE
        passages of query b's j-th group, score descending, the lower pid first among equal scores, padded with pid 0 / -Inf
        when the group has fewer; row 0 is what the call returns without per_group, and the
        groups, their order and n_candidates are unchanged.
        `prior`: one PassagePrior for the whole batch, with one finite `prior_weight` -- every candidate passage p (after any
        filter) is ranked by E = fl32(score + fl32(prior_weight * value[p])), the lower pid first among equal E, and the
        scores returned are E; with `grouping` a document is represented by its candidate with the largest E.  The candidates,
        n_candidates and short results are those of the call without a prior.  Not with `per_group` (Unsupported).
        `after`: a pair (scores float32[B], pids int64[B]) of cursors, one per query -- query b returns
        the first k of its candidates p (after any filter) with score < scores[b], or score == scores[b] and pid > pids[b], by
        (score descending, pid ascending): what its ranking continues with.  `after=next_cursor(pids, scores)` of the previous
        page walks the whole ranking in pieces of k, bit for bit.  A score of +Inf means no cursor for that query, -Inf an
        empty page, NaN is ArgumentError.  The result is always padded (pid 0 / -Inf; a page of padding alone is the end) and
        n_candidates is that of the call without cursors, the same on every page.  Composes with `filters` in both scopes;
        not with `grouping`, `per_group` or `prior` (Unsupported).
        `candidates`: re-rank given passages -- the candidate set of query b is the list the caller names, not the query's
        probes (`nprobe` is checked and otherwise unused).  A sequence of B integer arrays (ragged; any order, duplicates
        allowed; pids as search returns them), or a pair `(pids (L, B), lens [B])` whose column b holds query b's list in its
        first lens[b] rows.  The candidates are the distinct listed passages that hold embeddings; the result is bit for bit
        that of `filters=make_filter(pids=list), scope="all"` and is always padded.  A pid outside the searcher's range is
        BoundsError naming the query and the position.  Composes with `grouping`, `per_group`, `prior` and `after` as a
        scope="all" filter does; not with `filters` (Unsupported).
        `return_candidate_scores=True` (needs `candidates`): a fourth result, the exact score of every listed passage at its
        input position (with a prior: E), -Inf where the position holds no candidate -- a list of B float32 arrays of the
        input lengths for ragged lists, an (L, B) array for the pair form.  They are passage scores: a grouping or cursors
        do not change them.  Such a call scores every candidate exactly: it runs as the single exact pass whatever the mode.
        `candidate_priors` (needs `candidates`) with `prior_weight`: re-rank with first-stage scores -- one value per listed pid,
        a sequence of B arrays of the lists' lengths or an (L, B) block beside the pair form.  Candidate p of query b is ranked
        by E = fl32(e + fl32(prior_weight * v)), v the value at p's FIRST occurrence in query b's list, and E is the score
        returned (and the candidate score): bit for bit the one-query call with `prior=make_prior(dense)` whose dense vector
        holds v for the listed passages and 0 elsewhere, without a handle and per query.  Values must be finite and keep
        |prior_weight| * max|value| below FLT_MAX (ArgumentError, naming the query and the position).  Composes with
        `grouping` (`per_group=1` included); not with `prior`, `per_group` > 1 or `after` (Unsupported)."""
        return self._search_batch(Q, k, nprobe, pad_short, SearchKeywords(
            filters=filters, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=True if return_candidate_scores else None, candidate_priors=candidate_priors))

    def _search_batch(self, Q, k: int, nprobe, pad_short, kw: SearchKeywords):
        """search_batch with its keywords as the record."""
        q = colmajor(Q, np.float32)
        if q.ndim != 3 or q.shape[0] != self.dim:
            raise ColBERTError(f"Q must be (dim={self.dim}, T, B)")
        B = q.shape[2]
        req = search_request(self, B, keywords=kw, pad_short=pad_short)
        shape = (k, B) if kw.per_group is None else (int(req.per_group), k, B)
        pids = np.zeros(shape, dtype=np.int64, order="F"); scores = np.zeros(shape, dtype=np.float32, order="F")
        ncand = np.zeros(B, dtype=np.int64)
        check(request_entry("clb_search_batch_request")(self._h, fptr(q), q.shape[1], B, nprobe or self.config.nprobe, k, req,
                                                        fptr(pids), fptr(scores), fptr(ncand)))
        if not kw.candidate_scores:
            return pids, scores, ncand
        _, lens, _, cs, ragged = req.lists[:5]
        return pids, scores, ncand, ([cs[:int(n), b].copy() for b, n in enumerate(lens)] if ragged else cs)

    def retrieve(self, Q, nprobe: Optional[int] = None):
        """retrieve (src/search/ranking.jl:23-44): ascending candidate pids."""
        q = colmajor(Q, np.float32)
        out = np.zeros(max(self.num_docs, 1), dtype=np.int64)
        n = i64(0)
        check(lib().clb_retrieve(self._h, fptr(q), i64(q.shape[1]), i64(nprobe or self.config.nprobe), fptr(out), C.byref(n)))
        return out[: n.value].copy()

    def debug_scores(self, Q, k: int, nprobe: Optional[int] = None) -> dict:
        """Two-pass test hook: candidates with approximate and exact scores, tau, eps, #re-scored."""
        q = colmajor(Q, np.float32)
        cap = max(self.num_docs, 1)
        pids = np.zeros(cap, dtype=np.int64); ap = np.zeros(cap, dtype=np.float32); ex = np.zeros(cap, dtype=np.float32)
        n = i64(0); nr = i64(0); tau = C.c_float(0); eps = C.c_float(0)
        check(lib().clb_debug_scores(self._h, fptr(q), i64(q.shape[1]), i64(nprobe or self.config.nprobe), i64(k), i64(cap),
                                     fptr(pids), fptr(ap), fptr(ex), C.byref(n), C.byref(tau), C.byref(eps), C.byref(nr)))
        m = n.value
        return {"pids": pids[:m].copy(), "approx": ap[:m].copy(), "exact": ex[:m].copy(), "tau": tau.value,
                "eps": eps.value, "n_rescore": nr.value}

    def search(self, query: str, k: int, *, filter=None, scope="candidates", grouping=None, per_group=None, prior=None,
               prior_weight=1.0, after=None, candidates=None, return_candidate_scores=False, candidate_priors=None):
        """search(searcher, query::String, k) (searching.jl:93-128); `filter` / `scope` / `grouping` / `per_group` / `prior` /
        `prior_weight` / `after` / `candidates` / `return_candidate_scores` / `candidate_priors` as in search_embeddings.
        Keywords that conflict are answered before a missing encoder is."""
        kw = SearchKeywords(
            filters=filter, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=True if return_candidate_scores else None, candidate_priors=candidate_priors)
        kw.check()
        if self.encoder is None:
            raise ColBERTError("no query encoder attached: pass encoder=... or use search_embeddings(Q, k)")
        Q = self.encoder.encode_queries([query])
        assert Q.shape[2] == 1 and Q.shape[1] == self.config.query_maxlen, Q.shape
        return self._search_embeddings(Q[:, :, 0], k, None, kw)

    def text_search(self, k: int, nprobe: Optional[int] = None, graph: bool = True) -> "TextSearch":
        """A session for repeated `search(searcher, query::String, k)` calls with everything after the tokenizer on the
        device (TextSearch below).  A session takes no grouping and no per_group: grouped search and its hits are
        `search(..., grouping=, per_group=)`."""
        return TextSearch(self, k, nprobe, graph)

    # -- profiling (bench.py) -----------------------------------------------------------------------
    def profile_enable(self, on: bool = True, counters: bool = False):
        """Per-kernel HIP-event timing; `counters` additionally fills `last_batch_stats` (one extra kernel per
        batch -- not for timed regions)."""
        check(lib().clb_profile_enable(self._h, C.c_int((2 if counters else 1) if on else 0)))

    def profile_read(self) -> dict:
        cap = 16
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); cnt = (C.c_int64 * cap)()
        n = lib().clb_profile_read(self._h, names, ms, cnt, cap)
        if n < 0:
            check(10)
        return {names[i].decode(): {"ms": ms[i], "launches": cnt[i]} for i in range(n)}

    def last_batch_stats(self) -> dict:
        a, b, c, d = i64(0), i64(0), i64(0), i64(0)
        check(lib().clb_last_batch_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"cand_docs": a.value, "cand_embs": b.value, "rescored_docs": c.value, "rescored_embs": d.value}

    def last_batch_half_rows(self) -> dict:
        """Two-pass mode: the rows the exact pass multiplied against query tokens 0..15 and against tokens 16..31 in the
        last batch (needs `profile_enable(counters=True)`, like `last_batch_stats`)."""
        a, b = i64(0), i64(0)
        check(lib().clb_last_batch_half_rows(self._h, C.byref(a), C.byref(b)))
        return {"rows_lo": a.value, "rows_hi": b.value}


class TextSearch:
    """search(searcher, query::String, k) (src/searching.jl:93-128) for a serving loop: one text query per call --
    tokenize on the host, then encode_queries (1 x query_maxlen) -> search -> the k (pid, score) pairs, all on the device
    with no host round trip in between: the token ids go up in one 128-byte copy, the encoder writes the (1, T, dim) query
    tensor the search reads (clb_encode_queries_device -> clb_search_batch_device), the results come back in one copy.
    `graph=True`: the ~100 kernel launches of encoder + search are captured ONCE as a HIP graph over static buffers and
    replayed per query (the library only enqueues kernels and memsets on the stream it is handed).  Results are those of
    Searcher.search: BoundsError when the query has fewer than k candidates (searching.jl:127)."""

    def __init__(self, searcher: Searcher, k: int, nprobe: Optional[int] = None, graph: bool = True):
        import torch
        from .distributed import DeviceSearch
        if searcher.encoder is None or searcher.encoder.tokenizer is None:
            raise ColBERTError("text search needs an encoder with a tokenizer attached to the Searcher")
        self.s, self.enc, self.k = searcher, searcher.encoder, int(k)
        cfg = self.enc.config
        self.T = int(cfg.query_maxlen)
        self.dev = torch.device("cuda", searcher.device)
        tok = self.enc.tokenizer
        self.h_ids = torch.empty((1, self.T), dtype=torch.int32).pin_memory()
        self.h_mask = torch.empty((1, self.T), dtype=torch.uint8).pin_memory()
        self.d_ids = torch.zeros((1, self.T), dtype=torch.int32, device=self.dev)
        self.d_mask = torch.ones((1, self.T), dtype=torch.uint8, device=self.dev)
        self.d_skip = torch.tensor([tok.pad_id], dtype=torch.int64, device=self.dev)            # searching.jl:62
        self.d_q = torch.empty((1, self.T, searcher.dim), dtype=torch.float32, device=self.dev)
        self.run = DeviceSearch(searcher, self.T, 1, self.k, int(nprobe or searcher.config.nprobe))
        self.h_out = torch.empty(self.run.packed.numel(), dtype=torch.uint8).pin_memory()
        self.h_ncand = torch.empty(1, dtype=torch.int64).pin_memory()
        self.h_err = torch.zeros(1, dtype=torch.int32).pin_memory()
        # the encoder's sticky error flag (a 4-byte device word owned by the library) as a tensor view: copied back with every result
        flag = type("_Flag", (), {"__cuda_array_interface__": {"shape": (1,), "typestr": "<i4", "version": 2,
                                                                "data": (self.enc.error_flag_ptr(), False)}})()
        self.d_err = torch.as_tensor(flag, device=self.dev)
        self.stream = torch.cuda.Stream(self.dev)
        self.graph = None
        self.want_graph = bool(graph)
        self._prepare()

    def _prepare(self):
        """Size the workspaces and (graph=True) capture the graph, for the searcher as it is now.  Run again whenever the
        searcher's generation has moved: an append or a removal frees the arrays a captured graph points into and un-sizes the
        workspaces, so the stale graph is dropped before anything is enqueued."""
        import torch
        self.graph = None
        self.generation = self.s.generation
        # a first pass sizes every workspace (allocations cannot be captured)
        self.d_ids.fill_(self.enc.tokenizer.lookup("[MASK]"))
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.stream):
            self._enqueue()
        self.stream.synchronize()
        self.enc.check_last_ids()
        if self.want_graph:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self._enqueue()

    def _enqueue(self):
        self.enc.query_embeddings_device(self.d_ids, self.d_mask, self.d_skip, self.d_q)
        self.run(self.d_q)

    def __call__(self, query: str):
        """-> (pids Int64[k] 1-based, scores Float32[k])"""
        import torch
        from . import tokenization
        cfg = self.enc.config
        ids, mask = tokenization.tensorize_queries(cfg.query_token, cfg.attend_to_mask_tokens, self.enc.tokenizer, [query], self.T)
        self.h_ids.numpy()[0, :] = ids[:, 0]
        self.h_mask.numpy()[0, :] = mask[:, 0]
        if self.s.generation != self.generation:      # the searcher has grown or shrunk since the capture
            self._prepare()
        with torch.cuda.stream(self.stream):
            self.d_ids.copy_(self.h_ids, non_blocking=True)
            self.d_mask.copy_(self.h_mask, non_blocking=True)
            if self.graph is not None:
                self.graph.replay()
            else:
                self._enqueue()
            self.h_out.copy_(self.run.packed, non_blocking=True)
            self.h_ncand.copy_(self.run.ncand, non_blocking=True)
            self.h_err.copy_(self.d_err, non_blocking=True)
        self.stream.synchronize()
        if int(self.h_err[0]) != 0:       # id outside the vocabulary / non-finite embeddings: raises (and clears the flag)
            self.enc.check_last_ids()
        n = int(self.h_ncand[0])
        self.s.last_num_candidates = n
        if n < self.k:                                                            # searching.jl:127
            raise BoundsError(f"attempt to access {n}-element Vector at index [1:{self.k}] (the query has {n} candidate passages)")
        k = self.k
        out = self.h_out.numpy()
        return out[:k * 8].view(np.int64).copy(), out[k * 8:k * 12].view(np.float32).copy()

    def search_many(self, queries, group: int = 128, batch: int = 32):
        """Many text queries at the throughput shape (round 6): encode_queries (src/modelling/checkpoint.jl:271-301) on `group`
        queries per call -- at 128 x 32 rows the encoder's Linear layers fill the chip, at 32 x 32 they do not -- and search
        (src/searching.jl:102-127) on `batch` queries per call, the size the search kernels are tuned for; the encode of group
        g + 1 runs on its own stream beside the later search batches of group g (it starts once the first of them has
        finished).  Returns [(pids, scores)] in query order, each identical to what __call__ returns for that query; raises
        BoundsError for the first query with fewer than k candidates."""
        import torch
        from . import tokenization
        from .distributed import DeviceSearch
        if group % batch != 0:
            raise ValueError("group must be a multiple of batch")
        n = len(queries)
        if n == 0:
            return []
        cfg = self.enc.config
        ids, mask = tokenization.tensorize_queries(cfg.query_token, cfg.attend_to_mask_tokens, self.enc.tokenizer, list(queries), self.T)
        n_groups = -(-n // group)
        pad = n_groups * group - n
        ids_t = np.ascontiguousarray(np.concatenate([ids.T] + [ids.T[-1:]] * pad, axis=0), dtype=np.int32)        # (n + pad, T)
        mask_t = np.ascontiguousarray(np.concatenate([mask.T] + [mask.T[-1:]] * pad, axis=0), dtype=np.uint8)
        st = getattr(self, "_many", None)
        if st is None or st["group"] != group or st["batch"] != batch:
            nprobe = self.run.nprobe
            st = {"group": group, "batch": batch,
                  "runs": [DeviceSearch(self.s, self.T, batch, self.k, nprobe, slot=1 + i) for i in range(2)],
                  "enc_stream": torch.cuda.Stream(self.dev), "compute": [torch.cuda.Stream(self.dev) for _ in range(2)],
                  "d_ids": [torch.zeros((group, self.T), dtype=torch.int32, device=self.dev) for _ in range(2)],
                  "d_mask": [torch.ones((group, self.T), dtype=torch.uint8, device=self.dev) for _ in range(2)],
                  "d_q": [torch.empty((group, self.T, self.s.dim), dtype=torch.float32, device=self.dev) for _ in range(2)]}
            self._many = st
        per = group // batch
        nb = n_groups * per
        h_ids = torch.from_numpy(ids_t).pin_memory()
        h_mask = torch.from_numpy(mask_t).pin_memory()
        h_out = torch.empty((nb, st["runs"][0].packed.numel()), dtype=torch.uint8).pin_memory()
        h_nc = torch.empty((nb, batch), dtype=torch.int64).pin_memory()
        gate = None
        done = [[], []]                    # events of the search batches that read d_q[0] / d_q[1]
        torch.cuda.current_stream(self.dev).synchronize()
        for g in range(n_groups):
            b2 = g % 2
            es = st["enc_stream"]
            with torch.cuda.stream(es):
                for ev in done[b2]:        # the group that used these buffers two groups ago has been searched
                    es.wait_event(ev)
                done[b2] = []
                st["d_ids"][b2].copy_(h_ids[g * group:(g + 1) * group], non_blocking=True)
                st["d_mask"][b2].copy_(h_mask[g * group:(g + 1) * group], non_blocking=True)
                if gate is not None:
                    es.wait_event(gate)
                self.enc.query_embeddings_device(st["d_ids"][b2], st["d_mask"][b2], self.d_skip, st["d_q"][b2])
                encoded = torch.cuda.Event()
                encoded.record(es)
            for j in range(per):
                i = g * per + j
                cs, run = st["compute"][i % 2], st["runs"][i % 2]
                with torch.cuda.stream(cs):
                    cs.wait_event(encoded)
                    run(st["d_q"][b2][j * batch:(j + 1) * batch])
                    h_out[i].copy_(run.packed, non_blocking=True)
                    h_nc[i].copy_(run.ncand, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(cs)
                    done[b2].append(ev)
                    if j == 0:
                        gate = ev
        with torch.cuda.stream(st["enc_stream"]):
            self.h_err.copy_(self.d_err, non_blocking=True)
        for cs in st["compute"]:
            cs.synchronize()
        st["enc_stream"].synchronize()
        if int(self.h_err[0]) != 0:
            self.enc.check_last_ids()
        k, out = self.k, []
        raw, nc = h_out.numpy(), h_nc.numpy()
        for q in range(n):
            i, r = divmod(q, batch)
            if int(nc[i, r]) < k:                                                  # searching.jl:127
                self.s.last_num_candidates = int(nc[i, r])
                raise BoundsError(f"attempt to access {int(nc[i, r])}-element Vector at index [1:{k}] (query {q + 1} has {int(nc[i, r])} candidate passages)")
            pids = raw[i, :batch * k * 8].view(np.int64).reshape(batch, k)[r].copy()
            scores = raw[i, batch * k * 8:batch * k * 12].view(np.float32).reshape(batch, k)[r].copy()
            out.append((pids, scores))
        self.s.last_num_candidates = int(nc[(n - 1) // batch, (n - 1) % batch])
        return out

    def close(self):
        self.graph = None
        self._many = None


def search(searcher: Searcher, query, k: int, *, filter=None, scope="candidates", grouping=None, per_group=None, prior=None,
           prior_weight=1.0, after=None, candidates=None, return_candidate_scores=False, candidate_priors=None):
    """The reference's exported `search` (src/ColBERT.jl:40).  `query` may be a string (needs an
    encoder) or a (dim, T) Float32 matrix of query embeddings.  `filter` / `scope` / `grouping` / `per_group` / `prior` /
    `prior_weight` / `after` / `candidates` / `return_candidate_scores` / `candidate_priors`: Searcher.search_embeddings."""
    # `searcher` may be a ShardedSearcher or any object with these two methods: it always gets the four keywords below, and
    # each later one only when the caller gave it (a ShardedSearcher answers a cursor or candidate lists with Unsupported itself)
    more = {} if prior is None and prior_weight == 1.0 else {"prior": prior, "prior_weight": prior_weight}
    if after is not None:
        more.update(after=after)
    if candidates is not None or return_candidate_scores:
        more.update(candidates=candidates, return_candidate_scores=return_candidate_scores)
    if candidate_priors is not None:
        more.update(candidate_priors=candidate_priors)
    call = searcher.search if isinstance(query, str) else searcher.search_embeddings
    return call(query, k, filter=filter, scope=scope, grouping=grouping, per_group=per_group, **more)
