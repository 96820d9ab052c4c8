"""ShardedSearcher: one handle over a passage shard group, with `Searcher`'s calling conventions and GLOBAL pids.

The collection is cut into contiguous pid ranges (sharding.py), one `Searcher` per range.  A search runs on every shard and
the per-shard top-k lists are merged (distributed.py); filters, appends and removals are routed to the shards by pid range.
Two exchange protocols:
  * "two_phase": phase 1 on every shard (clb_search_shard_phase1_filtered_slot) -> all-gather of the shards' k largest
    approximate scores -> phase 2 at the global threshold -> all-gather of the packed per-shard top-k -> merge_packed;
  * "single": every shard searches with its own threshold (DeviceSearch.__call__) -> packed all-gather -> merge_packed.
A filter acts where phase 1 makes a shard's candidate list; everything after that reads only the list, so phase 2 takes
no filter.
Grouped search (`make_grouping`, `grouping=`): the group ids are cut at the shard boundaries, and a group that straddles a cut
keeps ONE global index on both sides (`group_base` of a shard + its local index).  Under "two_phase" the shards publish their
k best groups with those indices, the threshold counts a repeated index once, and the merge (merge_grouped_packed) keeps one
record per group and counts a straddling candidate group once; under "single" every shard runs its whole grouped search and
the same merge follows.  The hits of a grouped search (`per_group=` of `Searcher`) are not served across a shard group:
the search calls accept the keyword and raise Unsupported.  Candidate lists (`candidates=` / `return_candidate_scores=` /
`candidate_priors=` of `Searcher`) likewise.
Score priors (`make_prior`, `prior=`, `prior_weight=`): the values are cut at the shard boundaries, one PassagePrior per shard.
Under "two_phase" the shards publish their k largest BOOSTED approximate scores and, per query, the largest such score by
magnitude; the threshold of phase 2 is lowered by a rounding slack formed from the maximum of those magnitudes over ALL shards
(DESIGN.md section 5), and the usual merge follows -- it orders by (score, pid), which is the order of the boosted scores.
Under "single" every shard runs its whole search with the prior.  With a grouping both compose as above.

The shards live in one process (`group=None`; on one device, or one device each) or one or more per rank of a
torch.distributed process group: every method is then a COLLECTIVE -- all ranks call it with the same arguments -- and its
result is identical on every rank.  Over gloo the exchanges are staged through host memory.  Shards of one process on
SEVERAL devices are served by copying the gathered blocks to each shard's device; that path, like any run on more than
one physical GPU, is not covered by the test suite (its machines have one GPU)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from ._lib import ArgumentError, BoundsError, ColBERTError, Unsupported, check, colmajor, fptr, i64, lib
from .searcher import Owned, PassageFilter, SearchKeywords, _no_prior_hits, _range_bound, _scope_code, _weight_value

_PROTOCOLS = ("auto", "two_phase", "single")
_PIECE = 64          # queries per exchange: a filtered phase 1 carries at most 64 filter handles (include/colbert_hip.h)


# ---- host logic (no device): the pid tiling of a group ----------------------------------------------------------------
def check_tiling(ranges) -> np.ndarray:
    """ranges: (pid_offset, num_docs) per shard, in pid order -> boundaries [n_shards + 1] (passages before each shard, then
    the end), or ColBERTError when shard r + 1 does not start where shard r ends."""
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if r.shape[0] == 0:
        raise ColBERTError("a shard group needs at least one shard")
    for i in range(r.shape[0] - 1):
        if r[i + 1, 0] != r[i, 0] + r[i, 1]:
            raise ColBERTError(f"the shards do not tile a contiguous pid range: shard {i} ends at passage {r[i, 0] + r[i, 1]}, "
                               f"shard {i + 1} has pid_offset {r[i + 1, 0]}")
    return np.concatenate([r[:, 0], [r[-1, 0] + r[-1, 1]]])


def check_group_pids(pids, bounds) -> np.ndarray:
    """pids as a flat int64 array; BoundsError when one lies outside the group's passages bounds[0]+1 .. bounds[-1]."""
    p = np.ascontiguousarray(np.asarray(pids).reshape(-1), dtype=np.int64)
    bad = np.nonzero((p <= bounds[0]) | (p > bounds[-1]))[0]
    if bad.size:
        raise BoundsError(f"pid {int(p[bad[0]])} (entry {int(bad[0])}) outside {int(bounds[0]) + 1}..{int(bounds[-1])}, "
                          "the passages of the shard group")
    return p


def route_pids(pids, bounds):
    """Global pids -> one array per shard (the pids of that shard, in list order, duplicates kept)."""
    p = check_group_pids(pids, bounds)
    shard = np.searchsorted(bounds, p, side="left") - 1          # bounds[i] < p <= bounds[i + 1]
    return [p[shard == i] for i in range(len(bounds) - 1)]


def route_positions(pids, bounds):
    """Global pids -> one array per shard: the POSITIONS in the list of that shard's pids, ascending (what route_pids selects,
    for a caller that routes other per-pid data with them)."""
    p = check_group_pids(pids, bounds)
    shard = np.searchsorted(bounds, p, side="left") - 1
    return [np.nonzero(shard == i)[0] for i in range(len(bounds) - 1)]


def slice_mask(mask, bounds):
    """A boolean array over the group's passages -> one slice per shard."""
    m = np.asarray(mask)
    n = int(bounds[-1] - bounds[0])
    if m.dtype != np.bool_ or m.shape != (n,):
        raise ColBERTError(f"mask must be a boolean array of num_docs={n} entries")
    return [m[int(bounds[i] - bounds[0]):int(bounds[i + 1] - bounds[0])] for i in range(len(bounds) - 1)]


def slice_prior(values, bounds):
    """One finite number per passage of the group -> (the float32 array, one slice per shard).  ArgumentError for a wrong
    length or a value that is not finite in fp32, naming the first offending GLOBAL pid."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.ascontiguousarray(np.asarray(values), dtype=np.float32)
    first, n = int(bounds[0]), int(bounds[-1] - bounds[0])
    if v.ndim != 1:
        raise ArgumentError(f"a prior holds one value per passage of the shard group: shape {v.shape}, num_docs={n}")
    if v.size != n:
        what = "has no value" if v.size < n else "is not a passage of the shard group"
        raise ArgumentError(f"a prior holds one value per passage of the shard group: {v.size} values, num_docs={n} "
                            f"(pid {first + min(v.size, n) + 1} {what})")
    bad = np.nonzero(~np.isfinite(v))[0]
    if bad.size:
        raise ArgumentError(f"the prior of passage {first + int(bad[0]) + 1} is not a finite number")
    return v, [v[int(bounds[i]) - first:int(bounds[i + 1]) - first] for i in range(len(bounds) - 1)]


def dense_group_index(group_ids, n: int) -> np.ndarray:
    """The caller's group ids over the n passages of a shard group -> the dense 0-based index of every passage's group (the
    number of id changes before it; for non-decreasing ids this is np.unique's inverse).  ColBERTError for anything but one
    integer per passage, ArgumentError naming the first position at which the ids decrease."""
    ids = np.asarray(group_ids)
    if ids.ndim != 1 or ids.dtype.kind not in "iu" or ids.size != n:
        raise ColBERTError(f"group_ids must be a vector of integers, one per passage of the shard group (num_docs={n})")
    ids = ids.astype(np.int64)
    down = np.nonzero(ids[1:] < ids[:-1])[0]
    if down.size:
        i = int(down[0]) + 1
        raise ArgumentError(f"group ids must be non-decreasing in pid: they decrease at position {i} ({int(ids[i])} after {int(ids[i - 1])})")
    dense = np.zeros(n, dtype=np.int64)
    if n > 1:
        dense[1:] = np.cumsum(ids[1:] != ids[:-1])
    return dense


def slice_groups(group_ids, bounds):
    """Global group ids -> (one slice of the ids per shard, the group_base of every shard: the dense global index of the
    group of the shard's first passage -- 0 for a shard without passages)."""
    n = int(bounds[-1] - bounds[0])
    dense = dense_group_index(group_ids, n)
    ids = np.ascontiguousarray(np.asarray(group_ids), dtype=np.int64)
    cuts = [int(b - bounds[0]) for b in bounds]
    parts = [ids[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
    bases = [int(dense[cuts[i]]) if cuts[i] < cuts[i + 1] else 0 for i in range(len(cuts) - 1)]
    return parts, bases


class ShardedParts(Owned):
    """One resident handle per local shard (`parts`), owned by a handle over the whole shard group (`group`)."""

    def _release(self):
        for part in getattr(self, "parts", ()):
            part.close()


class ShardedGrouping(ShardedParts):
    """A passage -> group (document) map over a shard group: one resident PassageGrouping per local shard (`parts`), made
    from that shard's slice of the ids, and the `group_base` of each (`bases`).  Made by `ShardedSearcher.make_grouping`
    and refused by any other group.  `count` is the number of groups of the whole collection.  An append to the group
    invalidates it ("grouping made before an append; make another"); removals and updates do not."""

    def __init__(self, group: "ShardedSearcher", parts, bases, group_ids: np.ndarray, count: int):
        self.group, self.parts, self.bases, self.count = group, list(parts), [int(b) for b in bases], int(count)
        self._ids = group_ids                      # host copy of the caller's ids, entry i = global passage first + i
        self._first = int(group._bounds[0])        # passages before the group
        self.num_docs = int(group_ids.size)        # the group's passages when it was made

    def groups_of(self, pids) -> np.ndarray:
        """The caller's group ids of GLOBAL pids as a search returns them."""
        p = np.asarray(pids, dtype=np.int64) - self._first
        if p.size and (p.min() < 1 or p.max() > self._ids.size):
            raise BoundsError(f"pid outside {self._first + 1}..{self._first + self._ids.size} "
                              "(pid 0 pads a short result: cut the result at n_candidates first)")
        return self._ids[p - 1]


class ShardedPrior(ShardedParts):
    """One finite fp32 value per passage of a shard group: one resident PassagePrior per local shard (`parts`), made from that
    shard's slice of the values by `ShardedSearcher.make_prior` and refused by any other group.  `max_abs` is the largest
    |value| over ALL shards of the group (every rank holds the same number): the weight of a search is checked against it.
    An append to the group invalidates it ("prior made before an append; make another"); removals and updates do not."""

    def __init__(self, group: "ShardedSearcher", parts, max_abs: float, n: int):
        self.group, self.parts, self.max_abs, self.num_docs = group, list(parts), float(max_abs), int(n)
        self.count = self.num_docs                 # len(): the number of values


class ShardedFilter(ShardedParts):
    """A passage set over a shard group: one resident PassageFilter per local shard (`parts`), made by
    `ShardedSearcher.make_filter` and refused by any other group.  `count` is the population over the whole group.  An append
    to the group invalidates it (the library refuses it: "filter made before an append; make another"); a removal does not.
    Filters of one group compose part by part on the device (`ShardedSearcher.combine_filters`): `a & b`, `a | b`, `a - b`,
    `~a`.  Carrying a filter over an append (`PassageFilter.extended`) is not offered across a shard group: make another."""

    def __init__(self, group: "ShardedSearcher", parts, count: int):
        self.group, self.parts, self.count = group, list(parts), int(count)
        b = getattr(group, "_bounds", None)        # the group's passages when the filter was made
        self._first_pid, self.num_docs = (int(b[0]), int(b[-1] - b[0])) if b is not None else (0, 0)

    def __and__(self, other):
        return self.group.combine_filters("and", [self, other])

    def __or__(self, other):
        return self.group.combine_filters("or", [self, other])

    def __sub__(self, other):
        return self.group.combine_filters("andnot", [self, other])

    def __invert__(self):
        return self.group.combine_filters("not", [self])

    def to_mask(self) -> np.ndarray:
        """The set as a boolean array over the group's passages (entry i = global pid first + i + 1), read back from the
        device: the slices of THIS process's shards at their global positions.  With a process group every rank holds its
        own shards' slices and False elsewhere -- rank r the passages of shards r L .. r L + L - 1 (L shards per rank; their
        pids are `ShardedSearcher.shard_ranges` of those indices) -- and the element-wise OR over the ranks is the whole set;
        no collective runs here."""
        out = np.zeros(self.num_docs, dtype=np.bool_)
        for part in self.parts:
            at = int(part.searcher.pid_offset) - self._first_pid
            out[at:at + part.num_docs] = part.to_mask()
        return out


def _refuse_single_handle_keywords(kw: SearchKeywords):
    """What a single handle serves and a shard group does not: the hits of a grouped search, cursors, candidate lists.  The
    first thing every search call of a group answers (with a prior the `per_group` refusal is the single handle's:
    ShardedSearcher._check_prior)."""
    if kw.per_group is not None and kw.prior is None:
        raise Unsupported("per_group= (the best passages of every group) is not supported across a shard group: search "
                          "the unsharded Searcher, or the winners' passages with a filter and scope='all'")
    if kw.after is not None:
        raise Unsupported("after= (search after a cursor) is not supported across a shard group: search the unsharded "
                          "Searcher")
    if kw.candidates is not None or kw.candidate_scores or kw.candidate_priors is not None:
        raise Unsupported("candidates= (re-rank given passages) is not supported across a shard group: search the unsharded "
                          "Searcher, or hand every shard's Searcher the lists (its device route skips another shard's pids)")


class ShardedSearcher:
    """See the module docstring.  `shards`: this process's open `Searcher`s in pid order (with `group`: this rank's, and
    every rank holds the same number of them; rank r's pids come before rank r + 1's).  The handle takes the shards over:
    `close()` closes them."""

    def __init__(self, shards: Sequence, group=None, encoder=None):
        self.shards = list(shards)
        self.group, self.encoder = group, encoder
        if not self.shards:
            raise ColBERTError("a shard group needs at least one shard")
        desc = np.array([[s.pid_offset, s.num_docs, s.dim, s.nbits, s.num_centroids] for s in self.shards], dtype=np.int64)
        self.rank, self.world = 0, 1
        if group is not None:
            import torch.distributed as dist
            self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
            desc = self._gather(desc).reshape(-1, 5)          # every rank's shards, in rank order
        for name, col in (("dim", 2), ("nbits", 3), ("K", 4)):
            if np.any(desc[:, col] != desc[0, col]):
                raise ColBERTError(f"the shards of a group must agree on {name}: got {desc[:, col].tolist()}")
        self._bounds = check_tiling(desc[:, :2])
        self.dim = int(desc[0, 2])
        self._first = self.rank * len(self.shards)         # group index of this process's first shard
        self._runs = {}
        self.last_num_candidates = 0
        self._share_bounds()

    @classmethod
    def from_index(cls, index: dict, n_shards: int, devices=None, encoder=None):
        """Cut an in-memory index into `n_shards` contiguous shards (sharding.shard_index) in this process; `devices`: one
        device index per shard (default: all on device 0)."""
        from .searcher import Searcher
        from .sharding import shard_index
        devices = [0] * n_shards if devices is None else list(devices)
        if len(devices) != n_shards:
            raise ColBERTError("devices must name one device per shard")
        shards = []
        try:
            for r in range(n_shards):
                sub, off = shard_index(index, r, n_shards)
                shards.append(Searcher(index=sub, device=devices[r], pid_offset=off))
            return cls(shards, encoder=encoder)
        except Exception:
            for s in shards:
                s.close()
            raise

    # -- members ----------------------------------------------------------------------------------
    @property
    def num_docs(self) -> int:
        return int(self._bounds[-1] - self._bounds[0])

    @property
    def shard_ranges(self):
        """The global pids of every shard of the group, in order: a list of `range`s."""
        return [range(int(self._bounds[i]) + 1, int(self._bounds[i + 1]) + 1) for i in range(len(self._bounds) - 1)]

    def close(self):
        self._runs = {}
        for s in self.shards:
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- exchanges --------------------------------------------------------------------------------
    def _staged(self) -> bool:
        import torch.distributed as dist
        return dist.get_backend(self.group) != "nccl"        # gloo: through host memory

    def _gather_tensor(self, t, gather):
        """`gather` (all_gather_scores / all_gather_packed) of tensor t over the group, staged through the host where the
        backend has no device collectives; the result stays where the exchange left it."""
        return gather(t.cpu().contiguous() if self._staged() else t.contiguous(), self.group)

    def _gather(self, a: np.ndarray) -> np.ndarray:
        """host array (n, m) int64 -> (world, n, m) on every rank"""
        import torch
        from .distributed import all_gather_scores
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not self._staged():
            t = t.to(torch.device("cuda", self.shards[0].device))
        return self._gather_tensor(t, all_gather_scores).cpu().numpy()

    def _share_bounds(self):
        """One error bound on every shard of the group.  Set constants are only ever raised: get on every shard, element-wise
        maximum, set on every shard."""
        from .distributed import share_bound_consts, sync_bound_consts
        share_bound_consts(self.shards)
        if self.group is not None:
            sync_bound_consts(self.shards[0], self.group)
            share_bound_consts(self.shards)

    def _local_bounds(self, j: int):
        return int(self._bounds[self._first + j]), int(self._bounds[self._first + j + 1])

    # -- filters ----------------------------------------------------------------------------------
    def make_filter(self, pids=None, mask=None) -> ShardedFilter:
        """A resident passage set over the group.  Exactly one of: `pids`, GLOBAL passage ids (any order, duplicates allowed;
        outside 1..num_docs of the group: BoundsError before any shard is called) -- the list goes unchanged to every local
        shard (clb_filter_create_pids_global) -- or `mask`, a boolean array over the group's passages."""
        if (pids is None) == (mask is None):
            raise ColBERTError("make_filter takes exactly one of pids= and mask=")
        parts = []
        try:
            if pids is not None:
                p = check_group_pids(pids, self._bounds)
                for s in self.shards:
                    h, n_in = C.c_void_p(), i64(0)
                    check(lib().clb_filter_create_pids_global(s._h, fptr(p), i64(p.size), C.byref(h), C.byref(n_in)))
                    f = PassageFilter(s, h, lib().clb_filter_count(h))
                    f.n_inside = int(n_in.value)
                    parts.append(f)
            else:
                slices = slice_mask(mask, self._bounds)
                for j, s in enumerate(self.shards):
                    parts.append(s.make_filter(mask=np.ascontiguousarray(slices[self._first + j])))
            count = sum(f.count for f in parts)
            if self.group is not None:
                count = int(self._gather(np.array([[count]], dtype=np.int64)).sum())
        except Exception:
            for f in parts:
                f.close()
            raise
        return ShardedFilter(self, parts, count)

    def _filter_of_parts(self, make) -> ShardedFilter:
        """`make(j, shard)` -> the PassageFilter of local shard j; the group's count is summed over the ranks as make_filter
        sums it (the one collective)."""
        parts = []
        try:
            for j, s in enumerate(self.shards):
                parts.append(make(j, s))
            count = sum(f.count for f in parts)
            if self.group is not None:
                count = int(self._gather(np.array([[count]], dtype=np.int64)).sum())
        except Exception:
            for f in parts:
                f.close()
            raise
        return ShardedFilter(self, parts, count)

    def combine_filters(self, op: str, filters) -> ShardedFilter:
        """`Searcher.combine_filters` over the group: the filters' parts are combined shard by shard on the device -- part j of
        the result from part j of every operand, in the order given.  Operands of another group are refused."""
        filters = [filters] if isinstance(filters, ShardedFilter) else list(filters)
        for j, f in enumerate(filters):
            if not isinstance(f, ShardedFilter) or f.group is not self:
                raise ColBERTError(f"filters[{j}] is not a ShardedFilter of this shard group")
        return self._filter_of_parts(lambda j, s: s.combine_filters(op, [f.parts[j] for f in filters]))

    def make_range_filter(self, prior, lo=None, hi=None, lo_open: bool = False, hi_open: bool = False) -> ShardedFilter:
        """`Searcher.make_range_filter` over the group: `prior` a ShardedPrior of this group, every local shard takes the
        range over its own slice of the values.  The bounds are checked once, before any shard is called."""
        if not isinstance(prior, ShardedPrior) or prior.group is not self or prior.closed:
            raise ColBERTError("prior is not an open ShardedPrior of this shard group")
        if prior.num_docs != self.num_docs:
            raise ArgumentError("prior made before an append; make another")
        _range_bound(lo, "lo", -np.inf), _range_bound(hi, "hi", np.inf)
        return self._filter_of_parts(lambda j, s: s.make_range_filter(prior.parts[j], lo, hi, lo_open, hi_open))

    def _shard_filters(self, filters, B: int):
        """`filters` of a search call -> per local shard a list of B PassageFilters / None, or None when no query is filtered."""
        if filters is None:
            return None
        if isinstance(filters, ShardedFilter):
            filters = [filters] * B
        filters = list(filters)
        if len(filters) != B:
            raise ColBERTError(f"filters must be one ShardedFilter or a sequence of B={B} entries (None = unfiltered)")
        for j, f in enumerate(filters):
            if f is None:
                continue
            if not isinstance(f, ShardedFilter) or f.group is not self:
                raise ColBERTError(f"filters[{j}] is not a ShardedFilter of this shard group")
        if all(f is None for f in filters):
            return None
        return [[None if f is None else f.parts[i] for f in filters] for i in range(len(self.shards))]

    # -- groupings --------------------------------------------------------------------------------
    def make_grouping(self, group_ids=None, group_lens=None) -> ShardedGrouping:
        """A resident passage -> document map over the group, for `grouping=` of the search calls.  Exactly one of:
        `group_ids`, one integer per passage of the GROUP in pid order, non-decreasing (checked on the host before any shard
        is called: ArgumentError naming the position), or `group_lens`, the number of passages of every document in pid order
        (summing to num_docs; document j gets id j).  Every rank passes the same array, as with make_filter(mask=...).  The ids
        are cut at the shard boundaries; a document may straddle them."""
        if (group_ids is None) == (group_lens is None):
            raise ColBERTError("make_grouping takes exactly one of group_ids= and group_lens=")
        if group_lens is not None:
            lens = np.asarray(group_lens)
            if lens.ndim != 1 or lens.dtype.kind not in "iu" or (lens.size and int(lens.min()) < 0) or int(lens.sum()) != self.num_docs:
                raise ColBERTError(f"group_lens must be non-negative integers summing to num_docs={self.num_docs}")
            ids = np.repeat(np.arange(lens.size, dtype=np.int64), lens.astype(np.int64))
        else:
            ids = np.asarray(group_ids)
        slices, bases = slice_groups(ids, self._bounds)                 # raises before any shard is called
        ids = np.ascontiguousarray(ids, dtype=np.int64).copy()
        count = int(np.count_nonzero(ids[1:] != ids[:-1])) + 1 if ids.size else 0
        parts = []
        try:
            for j, s in enumerate(self.shards):
                parts.append(s.make_grouping(group_ids=np.ascontiguousarray(slices[self._first + j])))
        except Exception:
            for g in parts:
                g.close()
            raise
        L = len(self.shards)
        return ShardedGrouping(self, parts, bases[self._first:self._first + L], ids, count)

    def _check_grouping(self, grouping):
        if grouping is None:
            return None
        if not isinstance(grouping, ShardedGrouping) or grouping.group is not self:
            raise ColBERTError("grouping is not a ShardedGrouping of this shard group")
        if grouping.num_docs != self.num_docs:
            raise ArgumentError("grouping made before an append; make another")
        return grouping

    # -- priors -----------------------------------------------------------------------------------
    def make_prior(self, values) -> ShardedPrior:
        """A resident per-passage score term over the group, for `prior=` of the search calls: `values`, one finite number
        per passage of the GROUP (`num_docs` entries, entry i = global pid first + i + 1) as a numpy array (converted to
        float32).  Checked on the host before any shard is called: a wrong length or a value that is not finite in fp32 is an
        ArgumentError naming the first offending GLOBAL pid.  Every rank passes the same array, as with make_grouping."""
        v, slices = slice_prior(values, self._bounds)
        parts = []
        try:
            for j, s in enumerate(self.shards):
                parts.append(s.make_prior(np.ascontiguousarray(slices[self._first + j])))
            m = np.float32(max([p.max_abs for p in parts] + [0.0]))
            if self.group is not None:        # non-negative floats order as their bits
                m = self._gather(np.array([[int(m.view(np.int32))]], dtype=np.int64)).max().astype(np.int32).view(np.float32)
        except Exception:
            for p in parts:
                p.close()
            raise
        return ShardedPrior(self, parts, float(m), v.size)

    def _check_prior(self, kw: SearchKeywords):
        """`prior=` / `prior_weight=` of a search call -> (the ShardedPrior or None, the weight for every shard)."""
        prior = kw.prior
        if prior is None:
            return None, 1.0
        _no_prior_hits(kw.per_group)
        if not isinstance(prior, ShardedPrior) or prior.group is not self or prior.closed:
            raise ColBERTError("prior is not an open ShardedPrior of this shard group")
        if prior.num_docs != self.num_docs:
            raise ArgumentError("prior made before an append; make another")
        return prior, _weight_value(kw.prior_weight, prior.max_abs)      # against the GROUP's largest |value|

    # -- search -----------------------------------------------------------------------------------
    def _run(self, i: int, T: int, B: int, k: int, nprobe: int):
        from .distributed import DeviceSearch
        key = (i, T, B, k, nprobe)
        if key not in self._runs:
            self._runs[key] = DeviceSearch(self.shards[i], T, B, k, nprobe)
        return self._runs[key]

    def _two_pass(self, T: int) -> bool:
        """every local shard runs the two-pass mode for queries of T tokens (set the mode alike on all ranks)"""
        return all(s.mode == 1 for s in self.shards) and T <= 32

    def _gather_blocks(self, parts, dev0, cols: int):
        """One tensor per local shard -> the blocks of every shard of the group in shard order, as rows of `cols` entries: what
        travels between the phases (this process's blocks, then one all-gather)."""
        import torch
        from .distributed import all_gather_scores
        t = torch.stack([p.to(dev0) for p in parts]).view(-1, cols)
        return self._gather_tensor(t, all_gather_scores) if self.group is not None else t

    def _piece(self, q, k: int, nprobe: int, filters, scope: str, two_phase: bool, grouping=None, prior=None, weight=1.0):
        """One exchange for the queries q (dim, T, B <= 64) -> (pids (B, k), scores (B, k), n_cand [B]) as numpy.
        Two-phase: phase 1 on every local shard, then the shards' k largest approximate scores travel -- with a grouping they are
        those of its k best groups and their global group indices travel beside them, with a prior they are boosted and each
        shard's largest one by magnitude per query travels too -- and phase 2 takes exactly what travelled.  Single: every shard
        runs its whole search.  Then one block per process is gathered and merged: with a grouping the shards' packed grouped
        blocks (pids, scores, group indices, candidate groups, edge groups), merged with one record per group; without, the
        shards' packed top-k lists and the candidate counts."""
        import torch
        from .distributed import all_gather_packed, merge_grouped_packed, merge_packed, packed_grouped_bytes, packed_topk_bytes
        T, B = q.shape[1], q.shape[2]
        L = len(self.shards)
        host_q = torch.from_numpy(np.array(q.transpose(2, 1, 0), order="C"))            # (B, T, dim), a copy of the caller's
        runs = [self._run(i, T, B, k, nprobe) for i in range(L)]
        Qd = [host_q.to(r.dev) for r in runs]
        dev0 = runs[0].dev
        kws = [SearchKeywords(filters=None if filters is None else filters[i], scope=scope,
                              grouping=None if grouping is None else grouping.parts[i],
                              prior=None if prior is None else prior.parts[i], prior_weight=weight) for i in range(L)]
        bases = [0] * L if grouping is None else grouping.bases
        if two_phase:
            outs = [r._phase1_outputs(Qd[i], kws[i], bases[i]) for i, r in enumerate(runs)]
            top = self._gather_blocks([o[0] for o in outs], dev0, k).reshape(-1, B, k)
            gid = None if grouping is None else self._gather_blocks([o[1] for o in outs], dev0, k).reshape(-1, B, k)
            mabs = None if prior is None else self._gather_blocks([o[2] for o in outs], dev0, 1).reshape(-1, B)
            on = lambda t, r: None if t is None else t.to(r.dev).contiguous()
            blocks = [r.phase2(Qd[i], on(top, r), on(gid, r), kws[i].grouping, bases[i], kws[i].prior, weight, on(mabs, r))
                      for i, r in enumerate(runs)]
        elif grouping is not None:
            blocks = [r._grouped_shard(Qd[i], kws[i], bases[i]) for i, r in enumerate(runs)]
        else:
            for i, r in enumerate(runs):
                r._run(Qd[i], kws[i])
        if grouping is not None:
            block = torch.cat([x.to(dev0) for x in blocks])
        else:
            ncand = torch.stack([r.ncand.to(dev0) for r in runs]).sum(0)
            block = torch.cat([r.packed.to(dev0) for r in runs] + [ncand.view(torch.uint8)])
        g = (self._gather_tensor(block, all_gather_packed) if self.group is not None else block.view(1, -1)).to(dev0)
        if grouping is not None:
            mp, ms, n = merge_grouped_packed(g.contiguous().view(-1, packed_grouped_bytes(k, B)), B, k)
        else:
            nbytes = packed_topk_bytes(k, B)
            lists = g[:, :L * nbytes].contiguous().view(-1, nbytes)
            n = g[:, L * nbytes:].contiguous().view(torch.int64).view(-1, B).sum(0)
            mp, ms = merge_packed(lists, B, k)
        return mp.cpu().numpy(), ms.cpu().numpy(), n.cpu().numpy()

    def search_batch(self, Q, k: int, nprobe: Optional[int] = None, pad_short: bool = False, *, filters=None,
                     scope="candidates", protocol="auto", grouping=None, per_group=None, after=None, prior=None,
                     prior_weight=1.0, candidates=None, return_candidate_scores=False, candidate_priors=None):
        """B queries: Q (dim, T, B) -> (pids (k, B), scores (k, B), n_candidates[B]), GLOBAL pids, layouts and padding (pid 0 /
        -Inf) as `Searcher.search_batch`; n_candidates is the sum over the shards.  `filters`: one ShardedFilter or a sequence
        of B entries (None = that query is unfiltered); with filters the result is always padded.  Without, a query for which
        the whole group holds fewer than k candidates raises BoundsError unless `pad_short`.  Any B: batches of more than 64
        queries run as pieces of 64.  `protocol`: "two_phase", "single", or "auto" -- two-phase where every shard runs the
        two-pass mode for this query length, the single exchange otherwise (general-shape shards).
        `grouping`: one ShardedGrouping of this group for the whole batch -- every query returns its k best GROUPS, each by
        its best passage (`grouping.groups_of(pids)` names them), exactly as `Searcher.search_batch(grouping=)` on the
        unsharded index does; n_candidates counts the candidate groups, a group that straddles shards once.  Composes with
        `filters` in both scopes, under every protocol.
        `prior` (one ShardedPrior of this group for the whole batch) with `prior_weight`: rank by
        E = fl32(score + fl32(prior_weight * value)), the lower pid first among equal E, and return E -- exactly the result of
        `Searcher.search_batch(prior=)` on the unsharded index: pids, fp32 score bits, counts.  Composes with `filters` and
        with `grouping` (a group is represented by its candidate with the largest E), under every protocol.  The weight must be
        finite and keep |weight| * max|value| (over the whole group) below FLT_MAX: ArgumentError.
        `per_group`: anything but None raises Unsupported (the hits of a grouped search are a single handle's), and so does
        `after` (a cursor continues the ranking of a single handle), and so do `candidates` / `return_candidate_scores` /
        `candidate_priors` (candidate lists are a single handle's)."""
        return self._search_batch(Q, k, nprobe, pad_short, protocol, SearchKeywords(
            filters=filters, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=return_candidate_scores or None, candidate_priors=candidate_priors))

    def _search_batch(self, Q, k: int, nprobe, pad_short, protocol, kw: SearchKeywords):
        """search_batch with its keywords as the record."""
        _refuse_single_handle_keywords(kw)
        q = colmajor(Q, np.float32)
        if q.ndim != 3 or q.shape[0] != self.dim:
            raise ColBERTError(f"Q must be (dim={self.dim}, T, B)")
        if protocol not in _PROTOCOLS:
            raise ColBERTError(f"protocol must be one of {_PROTOCOLS}, got {protocol!r}")
        scope, filters = kw.scope, kw.filters
        _scope_code(scope)
        grouping = self._check_grouping(kw.grouping)
        prior, weight = self._check_prior(kw)
        k, B = int(k), q.shape[2]
        nprobe = int(nprobe or self.shards[0].config.nprobe)
        per_shard = self._shard_filters(filters, B)
        two_phase = protocol == "two_phase" or (protocol == "auto" and self._two_pass(q.shape[1]))
        pids = np.zeros((k, B), dtype=np.int64, order="F"); scores = np.zeros((k, B), dtype=np.float32, order="F")
        ncand = np.zeros(B, dtype=np.int64)
        for b0 in range(0, B, _PIECE):
            b1 = min(B, b0 + _PIECE)
            f = None if per_shard is None else [x[b0:b1] for x in per_shard]
            p, s, n = self._piece(q[:, :, b0:b1], k, nprobe, f, scope, two_phase, grouping, prior, weight)
            pids[:, b0:b1] = p.T; scores[:, b0:b1] = s.T; ncand[b0:b1] = n
        if filters is None and not pad_short:
            short = np.nonzero(ncand < k)[0]
            if short.size:                                                         # searching.jl:127
                b = int(short[0])
                what = "passages" if grouping is None else "groups"
                raise BoundsError(f"query {b} has {int(ncand[b])} candidate {what}, fewer than k={k}")
        return pids, scores, ncand

    def search_embeddings(self, Q, k: int, nprobe: Optional[int] = None, *, filter=None, scope="candidates", protocol="auto",
                          grouping=None, per_group=None, after=None, prior=None, prior_weight=1.0, candidates=None,
                          return_candidate_scores=False, candidate_priors=None):
        """One query, Q (dim, T) -> (pids Int64[k], scores Float32[k]) as `Searcher.search_embeddings`; the candidate count
        (with a grouping: the candidate groups) is left in `last_num_candidates`.  `prior` / `prior_weight`: search_batch."""
        return self._search_embeddings(Q, k, nprobe, protocol, SearchKeywords(
            filters=filter, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=return_candidate_scores or None, candidate_priors=candidate_priors))

    def _search_embeddings(self, Q, k: int, nprobe, protocol, kw: SearchKeywords):
        """search_embeddings with its keywords as the record of a ONE-QUERY call (`filters`: the filter)."""
        _refuse_single_handle_keywords(kw)
        q = colmajor(Q, np.float32)
        if q.ndim != 2 or q.shape[0] != self.dim:
            raise ColBERTError(f"Q must be (dim={self.dim}, T)")
        p, s, n = self._search_batch(q.reshape(q.shape + (1,), order="F"), k, nprobe, False, protocol, kw.for_one_query())
        self.last_num_candidates = int(n[0])
        return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(s[:, 0])

    def search(self, query: str, k: int, *, filter=None, scope="candidates", protocol="auto", grouping=None, per_group=None,
               after=None, prior=None, prior_weight=1.0, candidates=None, return_candidate_scores=False,
               candidate_priors=None):
        """search(searcher, query::String, k) over the group, with the attached encoder."""
        kw = SearchKeywords(
            filters=filter, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=return_candidate_scores or None, candidate_priors=candidate_priors)
        _refuse_single_handle_keywords(kw)
        self._check_prior(kw)                                     # before the encoder runs
        if self.encoder is None:
            raise ColBERTError("no query encoder attached: pass encoder=... or use search_embeddings(Q, k)")
        Q = self.encoder.encode_queries([query])
        return self._search_embeddings(Q[:, :, 0], k, None, protocol, kw)

    # -- append: to the LAST shard, the only range that can grow without colliding with a neighbour -------------------
    def _owns_last(self) -> bool:
        return self.rank == self.world - 1

    def _appended(self, n_new: int) -> range:
        first = int(self._bounds[-1]) + 1
        self._bounds[-1] += n_new
        self._share_bounds()          # the grown shard's constants may have risen: the next two-phase search needs one bound
        return range(first, int(self._bounds[-1]) + 1)

    def add_compressed(self, codes, residuals, doclens) -> range:
        """`Searcher.add_compressed` on the group's last shard; returns the GLOBAL pids of the new passages.  Afterwards the
        group's bound constants are shared again.  ShardedFilters made before are refused by the next search."""
        n_new = int(np.asarray(doclens.cpu() if hasattr(doclens, "data_ptr") else doclens).size)
        if self._owns_last():
            self.shards[-1].add_compressed(codes, residuals, doclens)
        return self._appended(n_new)

    def add_embeddings(self, embs, doclens) -> range:
        """`Searcher.add_embeddings` (compressed with the index's own codec) on the group's last shard."""
        n_new = int(np.asarray(doclens.cpu() if hasattr(doclens, "data_ptr") else doclens).size)
        if self._owns_last():
            self.shards[-1].add_embeddings(embs, doclens)
        return self._appended(n_new)

    def add_passages(self, texts) -> range:
        """encode_passages with the attached encoder, then add_embeddings."""
        if self.encoder is None:
            raise ColBERTError("no encoder attached: pass encoder=... or use add_embeddings(embs, doclens)")
        texts = list(texts)
        if self._owns_last():
            embs, doclens = self.encoder.encode_passages(texts)
            self.shards[-1].add_embeddings(embs, doclens)
        return self._appended(len(texts))

    # -- remove -----------------------------------------------------------------------------------
    def remove_passages(self, pids) -> int:
        """`Searcher.remove_passages` with GLOBAL pids routed to their shards by range (a pid outside the group: BoundsError
        before any shard is touched); returns the number of passages that lost embeddings, over the whole group.  Pids are
        stable and filters made before stay valid."""
        parts = route_pids(pids, self._bounds)
        n = 0
        for j, s in enumerate(self.shards):
            p = parts[self._first + j]
            if p.size:
                n += s.remove_passages(p)
        if self.group is not None:
            n = int(self._gather(np.array([[n]], dtype=np.int64)).sum())
        return n

    # -- update: every passage stays on the shard that owns its pid --------------------------------------------
    def _update(self, pids, doclens, call) -> int:
        """Route an update by pid range: call(shard, its pids, the positions of those pids in the caller's list) on every
        local shard that owns one; a pid outside the group raises BoundsError before any shard is touched.  -> the changed
        count over the whole group.  The group's bound constants are shared again, as after an append."""
        p = check_group_pids(pids, self._bounds)
        if p.size != np.asarray(doclens).size:
            raise ColBERTError(f"one doclen per pid: {p.size} pids, {np.asarray(doclens).size} doclens")
        if np.unique(p).size != p.size:             # a shard would refuse it, after the shards before it had changed
            raise ArgumentError("a pid is named twice: an update takes one new content per passage")
        where = route_positions(p, self._bounds)
        n = 0
        for j, s in enumerate(self.shards):
            at = where[self._first + j]
            if at.size:
                n += call(s, p[at], at)
        if self.group is not None:
            n = int(self._gather(np.array([[n]], dtype=np.int64)).sum())
        self._share_bounds()
        return n

    def update_compressed(self, pids, codes, residuals, doclens) -> int:
        """`Searcher.update_compressed` with GLOBAL pids: every passage and its rows go to the shard that owns the pid (numpy
        arrays, layouts as there).  Pids are stable, no passage changes its shard, and ShardedFilters made before stay valid.
        Returns the number of named passages that had or have embeddings, over the whole group."""
        dl = np.ascontiguousarray(np.asarray(doclens).reshape(-1), dtype=np.int64)
        co = np.ascontiguousarray(codes, dtype=np.uint32)
        r = colmajor(residuals, np.uint8)
        if co.ndim != 1 or r.ndim != 2 or r.shape[1] != co.size:
            raise ColBERTError("residuals must be (dim/8*nbits, n_emb)")
        if dl.size and (dl.min() < 0 or int(dl.sum()) != co.size):
            raise ColBERTError(f"doclens must be non-negative and sum to the {co.size} embeddings")
        off = np.concatenate([[0], np.cumsum(dl)])

        def call(s, p, at):
            cols = np.concatenate([np.arange(off[i], off[i + 1]) for i in at]) if at.size else np.zeros(0, np.int64)
            return s.update_compressed(p, co[cols], np.asfortranarray(r[:, cols]), dl[at])
        return self._update(pids, dl, call)

    def update_embeddings(self, pids, embs, doclens) -> int:
        """`Searcher.update_embeddings` with GLOBAL pids: `embs` numpy (dim, n), compressed on the owning shard with the
        index's own codec."""
        dl = np.ascontiguousarray(np.asarray(doclens).reshape(-1), dtype=np.int64)
        e = colmajor(embs, np.float32)
        if e.ndim != 2 or e.shape[0] != self.dim or (dl.size and dl.min() < 0) or int(dl.sum()) != e.shape[1]:
            raise ColBERTError(f"embs must be (dim={self.dim}, sum(doclens))")
        off = np.concatenate([[0], np.cumsum(dl)])

        def call(s, p, at):
            cols = np.concatenate([np.arange(off[i], off[i + 1]) for i in at]) if at.size else np.zeros(0, np.int64)
            return s.update_embeddings(p, np.asfortranarray(e[:, cols]), dl[at])
        return self._update(pids, dl, call)

    def update_passages(self, pids, texts) -> int:
        """encode_passages with the attached encoder on the owning shard's process, then update_embeddings: texts[i] becomes
        the content of passage pids[i]."""
        if self.encoder is None:
            raise ColBERTError("no encoder attached: pass encoder=... or use update_embeddings(pids, embs, doclens)")
        texts = list(texts)

        def call(s, p, at):
            embs, doclens = self.encoder.encode_passages([texts[i] for i in at])
            return s.update_embeddings(p, embs, doclens)
        return self._update(pids, np.zeros(len(texts), np.int64), call)
