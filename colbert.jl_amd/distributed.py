"""Multi-GPU search: one process per GPU, passages sharded across ranks (sharding.py), every rank runs
the whole search on its shard and one all-gather of the per-shard top-k (k (pid, score) records per
query, ~12 KB per rank at k = 1000) is the only exchange -- RCCL over xGMI through torch.distributed
(backend "nccl" is RCCL on ROCm).  The merged list is identical to the unsharded result because
candidates and scores are per passage.

On CPU (gloo, used by the tests) the same code runs with a caller-supplied local search function and a
host merge."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, i64, lib, request_entry
from .searcher import SearchKeywords, search_request
from .sharding import merge_topk_host


def all_gather_topk(pids, scores, group=None):
    """pids/scores: torch tensors (B, k) on this rank -> stacked (world, B, k) tensors on every rank."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    B, k = pids.shape
    gp = torch.empty((world * B, k), dtype=pids.dtype, device=pids.device)      # concatenation along dim 0
    gs = torch.empty((world * B, k), dtype=scores.dtype, device=scores.device)
    dist.all_gather_into_tensor(gp, pids.contiguous(), group=group)
    dist.all_gather_into_tensor(gs, scores.contiguous(), group=group)
    return gp.view(world, B, k), gs.view(world, B, k)


def packed_topk_bytes(k: int, B: int) -> int:
    """Bytes of one rank's packed (B, k) result block: [B*k int64 pids][B*k fp32 scores][pad to 8]."""
    return (B * k * 12 + 7) // 8 * 8


class LibraryComm:
    """The exchange step on the library's own RCCL communicator (clb_comm_*), for hosts without torch.distributed --
    the same calls the Julia shim makes.  Rank 0 creates the unique id (`LibraryComm.unique_id()`) and hands its bytes to
    the other ranks by any means; every rank then constructs `LibraryComm(device, rank, n_ranks, id_bytes)` (blocks until
    all ranks have joined).  Tensors are torch CUDA tensors here only because the Python driver keeps its device memory
    in torch; the entry points take bare device pointers."""

    def __init__(self, device: int, rank: int, n_ranks: int, id_bytes: bytes):
        self._h = C.c_void_p()
        self.device, self.rank, self.n_ranks = device, rank, n_ranks
        buf = C.create_string_buffer(bytes(id_bytes), len(id_bytes))
        check(lib().clb_comm_create(C.c_int(device), C.c_int(rank), C.c_int(n_ranks), buf, i64(len(id_bytes)), C.byref(self._h)))

    @staticmethod
    def unique_id() -> bytes:
        n = int(lib().clb_comm_unique_id_bytes())
        buf = C.create_string_buffer(n)
        check(lib().clb_comm_unique_id(buf, i64(n)))
        return buf.raw

    def close(self):
        if getattr(self, "_h", None):
            lib().clb_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def all_gather(self, t):
        """contiguous CUDA tensor -> (n_ranks, *t.shape) tensor of the same dtype, on torch's current stream"""
        import torch
        if not (t.is_cuda and t.is_contiguous() and t.device.index == self.device):
            raise ValueError("all_gather needs a contiguous CUDA tensor on the communicator's device")
        out = torch.empty((self.n_ranks,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        st = torch.cuda.current_stream(t.device).cuda_stream
        check(lib().clb_comm_all_gather(self._h, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()),
                                        i64(t.numel() * t.element_size()), C.c_void_p(st)))
        return out

    def all_reduce_max_(self, t):
        """in-place element-wise maximum of a contiguous float32 CUDA tensor over the ranks"""
        import torch
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.device.index == self.device):
            raise ValueError("all_reduce_max_ needs a contiguous float32 CUDA tensor on the communicator's device")
        st = torch.cuda.current_stream(t.device).cuda_stream
        check(lib().clb_comm_all_reduce_max_f32(self._h, C.c_void_p(t.data_ptr()), i64(t.numel()), C.c_void_p(st)))
        return t

    def sync_bound_consts(self, searcher):
        """one error bound on every shard (see sync_bound_consts below), over this communicator"""
        check(lib().clb_searcher_sync_bound_consts(searcher._h, self._h))     # the round trip inside the library
        return searcher.bound_consts


def all_gather_packed(packed, group=None):
    """ONE all-gather for a rank's whole result.  `packed`: the uint8 tensor of `packed_topk_bytes` bytes that
    DeviceSearch wrote its pids and scores into -> (world, nbytes) uint8 tensor on every rank."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    out = torch.empty(world * packed.numel(), dtype=torch.uint8, device=packed.device)   # concatenation along dim 0
    dist.all_gather_into_tensor(out, packed, group=group)
    return out.view(world, packed.numel())


def packed_grouped_bytes(k: int, B: int) -> int:
    """Bytes of one shard's packed GROUPED result block (clb_packed_grouped_bytes): the `packed_topk_bytes` block of pids and
    scores, then [B*k int64 global group indices][B int64 candidate groups][B*2 int64 edge groups]."""
    return packed_topk_bytes(k, B) + 8 * B * k + 8 * B + 16 * B


def merge_grouped_packed(gathered, B: int, k: int):
    """(n_lists, nbytes) gathered packed grouped blocks on a GPU -> (pids (B, k), scores (B, k), n_cand [B]): the merge that
    keeps one record per group and counts a group that straddles shards once (clb_merge_topk_grouped_packed_device), on
    torch's current stream."""
    import torch
    n_lists = gathered.shape[0]
    out_p = torch.empty((B, k), dtype=torch.int64, device=gathered.device)
    out_s = torch.empty((B, k), dtype=torch.float32, device=gathered.device)
    out_n = torch.empty(B, dtype=torch.int64, device=gathered.device)
    st = torch.cuda.current_stream(gathered.device).cuda_stream
    check(lib().clb_merge_topk_grouped_packed_device(gathered.device.index, C.c_void_p(gathered.data_ptr()), i64(k), i64(n_lists),
                                                     i64(B), C.c_void_p(out_p.data_ptr()), C.c_void_p(out_s.data_ptr()),
                                                     C.c_void_p(out_n.data_ptr()), C.c_void_p(st)))
    return out_p, out_s, out_n


def merge_packed(gathered, B: int, k: int, out_p=None, out_s=None):
    """(world, nbytes) gathered packed blocks -> (B, k) merged top-k via clb_merge_topk_packed_device on torch's
    current stream."""
    import torch
    world = gathered.shape[0]
    if not gathered.is_cuda:      # host merge (gloo tests): unpack the blocks and reuse the unpacked path
        gp = gathered[:, :B * k * 8].contiguous().view(torch.int64).view(world, B, k)
        gs = gathered[:, B * k * 8:B * k * 12].contiguous().view(torch.float32).view(world, B, k)
        return merge_gathered(gp, gs, k)
    if out_p is None:
        out_p = torch.empty((B, k), dtype=torch.int64, device=gathered.device)
        out_s = torch.empty((B, k), dtype=torch.float32, device=gathered.device)
    st = torch.cuda.current_stream(gathered.device).cuda_stream
    check(lib().clb_merge_topk_packed_device(gathered.device.index, C.c_void_p(gathered.data_ptr()), i64(k), i64(world),
                                             i64(B), C.c_void_p(out_p.data_ptr()), C.c_void_p(out_s.data_ptr()),
                                             C.c_void_p(st)))
    return out_p, out_s


def sync_bound_consts(searcher, group=None):
    """The two-phase sharded search cuts every shard at one global threshold tau - 2 eps, so eps must be the same
    (the largest) on every shard: all-reduce MAX of the three constants of the error bound, once, at load time.
    Without it a shard whose own embeddings give a smaller eps could skip a member of the global top-k."""
    import torch
    import torch.distributed as dist
    backend = dist.get_backend(group)
    dev = torch.device("cuda", searcher.device) if backend == "nccl" else torch.device("cpu")
    t = torch.from_numpy(searcher.bound_consts.copy()).to(dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    searcher.raise_bound_consts(t.cpu().numpy())
    return searcher.bound_consts


def share_bound_consts(searchers):
    """The same for several shards held by ONE process (tests, tools/shard_breakdown.py)."""
    m = np.max(np.stack([s.bound_consts for s in searchers]), axis=0)
    for s in searchers:
        s.raise_bound_consts(m)
    return m


def all_gather_scores(local_top, group=None):
    """(B, k) fp32 -> (world, B, k): the exchange between the two phases of the sharded search."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    B, k = local_top.shape
    out = torch.empty((world * B, k), dtype=local_top.dtype, device=local_top.device)
    dist.all_gather_into_tensor(out, local_top.contiguous(), group=group)
    return out.view(world, B, k)


def merge_gathered(gp, gs, k: int, device_index=None, out_p=None, out_s=None):
    """(world, B, k) gathered records -> (B, k) merged top-k.  GPU tensors go through the HIP merge
    kernel (clb_merge_topk_device) on torch's current stream; CPU tensors through the host merge."""
    import torch
    world, B, _ = gp.shape
    if gp.is_cuda:
        if out_p is None:
            out_p = torch.empty((B, k), dtype=torch.int64, device=gp.device)
            out_s = torch.empty((B, k), dtype=torch.float32, device=gp.device)
        st = torch.cuda.current_stream(gp.device).cuda_stream
        check(lib().clb_merge_topk_device(gp.device.index if device_index is None else device_index,
                                          C.c_void_p(gp.data_ptr()), C.c_void_p(gs.data_ptr()), i64(k), i64(world),
                                          i64(B), C.c_void_p(out_p.data_ptr()), C.c_void_p(out_s.data_ptr()),
                                          C.c_void_p(st)))
        return out_p, out_s
    P = gp.numpy(); S = gs.numpy()
    out_p = np.zeros((B, k), dtype=np.int64); out_s = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        mp, ms = merge_topk_host([P[r, b] for r in range(world)], [S[r, b] for r in range(world)], k)
        out_p[b, : mp.size] = mp; out_s[b, : ms.size] = ms
    return torch.from_numpy(out_p), torch.from_numpy(out_s)


def pack_topk(pids, scores):
    """(B, k) int64 pids + (B, k) fp32 scores -> the packed uint8 block of `packed_topk_bytes(k, B)` bytes."""
    import torch
    B, k = pids.shape
    buf = torch.zeros(packed_topk_bytes(k, B), dtype=torch.uint8, device=pids.device)
    buf[:B * k * 8].view(torch.int64).copy_(pids.reshape(-1))
    buf[B * k * 8:B * k * 12].view(torch.float32).copy_(scores.reshape(-1))
    return buf


def sharded_search(local_search, Q, k: int, group=None, packed: bool = False):
    """local_search(Q) -> (pids (B, k), scores (B, k)) torch tensors for this rank's shard, padded with
    (0, -inf).  Returns the merged (B, k) result, identical on every rank.  `packed`: move pids and scores in ONE
    all-gather of packed blocks (what bench.py does) instead of one collective each."""
    p, s = local_search(Q)
    if packed:
        return merge_packed(all_gather_packed(pack_topk(p, s), group), p.shape[0], k)
    gp, gs = all_gather_topk(p, s, group)
    return merge_gathered(gp, gs, k)


class DeviceSearch:
    """Device-resident batched search on one shard: queries and results stay in HBM (torch tensors),
    work is enqueued on torch's current stream."""

    def __init__(self, searcher, T: int, B: int, k: int, nprobe: int, slot: int = 0):
        import torch
        self.s, self.T, self.B, self.k, self.nprobe, self.slot = searcher, T, B, k, nprobe, slot
        self.dev = torch.device("cuda", searcher.device)
        # pids and scores live in one packed block so that a single all-gather can move both (all_gather_packed)
        self.packed = torch.empty(packed_topk_bytes(k, B), dtype=torch.uint8, device=self.dev)
        self.out_p = self.packed[:B * k * 8].view(torch.int64).view(B, k)
        self.out_s = self.packed[B * k * 8:B * k * 12].view(torch.float32).view(B, k)
        self.ncand = torch.zeros(B, dtype=torch.int64, device=self.dev)
        # the searcher's generation (Searcher.generation) at construction, then at the latest `capture`: an append un-sizes
        # the workspace slot and frees the index arrays a captured graph points into
        self.generation = searcher.generation
        # what every call needs, resolved once: the request entries of the device routes, the request of a call without
        # keywords, and torch's stream query
        self._search = request_entry("clb_search_batch_request_device_slot")
        self._phase1 = request_entry("clb_search_shard_phase1_request_slot")
        self._phase2 = request_entry("clb_search_shard_phase2_request_slot")
        self._plain = search_request(searcher, B)
        self._current_stream = torch.cuda.current_stream

    def graph_is_stale(self) -> bool:
        """True once the searcher has grown since the latest `capture`: that graph must not be replayed any more --
        `capture` again (it runs the sizing pass first), or go through `replay`."""
        return self.generation != self.s.generation

    def replay(self, graph, Qstatic, filters=None, scope="candidates", grouping=None, per_group=None, prior=None,
               prior_weight=1.0, after=None, candidates=None, candidate_scores=None, candidate_priors=None):
        """`graph.replay()` for a graph `capture` returned, made safe against appends: when the searcher has grown since
        the capture, the sizing pass runs again and the search is captured anew before anything is replayed.  Returns the
        graph that was replayed (keep it for the next call).  `after`: the cursor tensors the graph was captured with -- it
        reads their CONTENTS at every replay; `candidates` / `candidate_scores` / `candidate_priors` likewise."""
        kw = SearchKeywords(filters=filters, scope=scope, grouping=grouping, per_group=per_group, prior=prior,
                            prior_weight=prior_weight, after=after, candidates=candidates, candidate_scores=candidate_scores,
                            candidate_priors=candidate_priors)
        if self.graph_is_stale():
            graph = self._capture(Qstatic, kw)
        graph.replay()
        return graph

    def _fits(self, t, dtype, *shape) -> bool:
        """`t` may go to the kernels as a bare pointer: a contiguous tensor of `dtype` on this device -- and, where a shape is
        given, of that shape (None: any extent)."""
        import torch
        return (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.dev and t.is_contiguous()
                and (not shape or (t.dim() == len(shape) and all(n is None or n == m for n, m in zip(shape, t.shape)))))

    def _check_queries(self, Qdev):
        """The C ABI takes a bare pointer: a tensor with fewer than B x T x dim contiguous floats on this device would
        be read past its end by the kernels, so it is refused here."""
        import torch
        from ._lib import ArgumentError
        if not (self._fits(Qdev, torch.float32) and Qdev.numel() == self.B * self.T * int(self.s.dim)):
            raise ArgumentError(f"queries must be a contiguous float32 tensor of {self.B} x {self.T} x {int(self.s.dim)} "
                                f"elements on {self.dev}, got {getattr(Qdev, 'dtype', type(Qdev))} "
                                f"{tuple(getattr(Qdev, 'shape', ()))} on {getattr(Qdev, 'device', '?')}")

    def _check_cursors(self, after, _B=None):
        """The cursor arrays go to the kernels as bare pointers, like the queries: a pair of contiguous tensors, float32[B] and
        int64[B], on this device, or refused."""
        import torch
        from ._lib import ArgumentError
        if not (isinstance(after, (tuple, list)) and len(after) == 2 and self._fits(after[0], torch.float32, self.B)
                and self._fits(after[1], torch.int64, self.B)):
            raise ArgumentError(f"after must be a pair of contiguous tensors on {self.dev}: scores float32[{self.B}] and pids "
                                f"int64[{self.B}]")
        return tuple(after)

    def _check_lists(self, candidates, candidate_scores, _B=None):
        """The candidate lists go to the kernels as bare pointers, like the queries: a pair of contiguous tensors on this device,
        pids int64 [B, L] (L >= 1) and lens int64 [B] -- and, when given, candidate_scores float32 [B, L] -- or refused."""
        import torch
        from ._lib import ArgumentError
        if not (isinstance(candidates, (tuple, list)) and len(candidates) == 2 and self._fits(candidates[0], torch.int64, self.B, None)
                and candidates[0].shape[1] >= 1 and self._fits(candidates[1], torch.int64, self.B)):
            raise ArgumentError(f"candidates must be a pair of contiguous tensors on {self.dev}: pids int64[{self.B}, L] (L >= 1) "
                                f"and lens int64[{self.B}]")
        L = int(candidates[0].shape[1])
        if candidate_scores is not None and not self._fits(candidate_scores, torch.float32, self.B, L):
            raise ArgumentError(f"candidate_scores must be a contiguous float32[{self.B}, {L}] tensor on {self.dev}")
        return candidates[0], candidates[1], L, candidate_scores, False

    def _check_list_priors(self, candidate_priors, lists, _B=None):
        """The list priors go to the kernels as a bare pointer beside the lists: a contiguous float32 [B, L] tensor on this
        device, or refused.  Nothing is read back: the largest |value| the weight is checked against is 0 (a value whose
        product with the weight is not finite counts as 0 on the device)."""
        import torch
        from ._lib import ArgumentError
        if not self._fits(candidate_priors, torch.float32, self.B, lists[2]):
            raise ArgumentError(f"candidate_priors must be a contiguous float32[{self.B}, {lists[2]}] tensor on {self.dev}")
        return candidate_priors, 0.0

    def _request(self, kw: SearchKeywords, group_base: int = 0):
        """The clb_search_request of a call of this shard (searcher.search_request), its cursors and lists as device tensors.
        A call without keywords takes the request made at construction: it has nothing to check and nothing to point at."""
        if kw.plain:
            return self._plain
        return search_request(self.s, self.B, keywords=kw, group_base=group_base, cursor_arrays=self._check_cursors,
                              candidate_arrays=self._check_lists, candidate_prior_arrays=self._check_list_priors)

    def _stream(self) -> int:
        return self._current_stream(self.dev).cuda_stream

    def _grouped_block(self):
        """The packed grouped result block of this shard (packed_grouped_bytes) and the views the grouped calls write into."""
        import torch
        if not hasattr(self, "gpacked"):
            B, k = self.B, self.k
            self.gpacked = torch.zeros(packed_grouped_bytes(k, B), dtype=torch.uint8, device=self.dev)
            at_g = packed_topk_bytes(k, B); at_n = at_g + 8 * B * k; at_e = at_n + 8 * B
            self.g_out_p = self.gpacked[:B * k * 8].view(torch.int64).view(B, k)
            self.g_out_s = self.gpacked[B * k * 8:B * k * 12].view(torch.float32).view(B, k)
            self.g_out_g = self.gpacked[at_g:at_n].view(torch.int64).view(B, k)
            self.g_ncand = self.gpacked[at_n:at_e].view(torch.int64)
            self.g_edges = self.gpacked[at_e:].view(torch.int64).view(B, 2)
        return self.gpacked

    def search_grouped_shard(self, Qdev, filters, scope, grouping, group_base: int, prior=None, prior_weight=1.0):
        """The single exchange of a grouped sharded search on this shard: the whole grouped search
        (clb_search_batch_request_device_slot with the grouping; with `prior` / `prior_weight`, this shard's PassagePrior and
        the group's weight, in the same request), then the global group index of every result and the edge groups of every
        query (clb_search_result_groups_slot), all into the packed grouped block, which is returned.  B <= 64."""
        return self._grouped_shard(
            Qdev, SearchKeywords(filters=filters, scope=scope, grouping=grouping, prior=prior, prior_weight=prior_weight), group_base)

    def _grouped_shard(self, Qdev, kw: SearchKeywords, group_base: int):
        self._check_queries(Qdev)
        block = self._grouped_block()
        gh = self.s._grouping_handle(kw.grouping)
        req = self._request(kw)
        st = self._stream()
        check(self._search(
            self.s._h, self.slot, Qdev.data_ptr(), self.T, self.B, self.nprobe, self.k, req, self.g_out_p.data_ptr(),
            self.g_out_s.data_ptr(), self.g_ncand.data_ptr(), st))
        check(lib().clb_search_result_groups_slot(
            self.s._h, C.c_int(self.slot), gh, i64(group_base), C.c_void_p(self.g_out_p.data_ptr()), i64(self.B), i64(self.k),
            C.c_void_p(self.g_out_g.data_ptr()), C.c_void_p(self.g_edges.data_ptr()), C.c_void_p(st)))
        return block

    def phase1(self, Qdev, filters=None, scope="candidates", grouping=None, group_base: int = 0, prior=None, prior_weight=1.0):
        """Two-phase sharded search, first half (clb_search_shard_phase1_request_slot): everything up to pass 1 on this shard.
        Returns the (B, k) tensor of the shard's k largest approximate scores per query, to be all-gathered.
        `filters` / `scope` as in __call__ (at most 64 queries per call when one is filtered); phase2 takes none -- it continues on the filtered candidates phase 1 left on the slot.
        `grouping` (this shard's PassageGrouping) with `group_base` (the global index of the shard's first group): the grouped
        form -- returns (local_top, local_gid), the best approximate score of the
        shard's k best groups and their global group indices (int64), both (B, k) and both to be all-gathered.
        `prior` (this shard's PassagePrior) with `prior_weight` (the group's weight):
        the published scores are the BOOSTED approximate scores, and the call returns (local_top, local_gid or None,
        local_mabs): local_mabs [B] float32 is the shard's largest boosted approximate score by magnitude per query, to be
        all-gathered with the others (phase 2 forms its rounding slack from the maximum over the shards)."""
        top, gid, mabs = self._phase1_outputs(
            Qdev, SearchKeywords(filters=filters, scope=scope, grouping=grouping, prior=prior, prior_weight=prior_weight), group_base)
        if mabs is not None:
            return top, gid, mabs
        return top if gid is None else (top, gid)

    def _phase1_outputs(self, Qdev, kw: SearchKeywords, group_base: int = 0):
        """phase1 with its keywords as the record -> always (local_top, local_gid or None, local_mabs or None): gid with a
        grouping, mabs with a prior."""
        import torch
        self._check_queries(Qdev)
        req = self._request(kw, group_base)
        if not hasattr(self, "local_top"):
            self.local_top = torch.empty((self.B, self.k), dtype=torch.float32, device=self.dev)
        if kw.grouping is not None and not hasattr(self, "local_gid"):
            self.local_gid = torch.empty((self.B, self.k), dtype=torch.int64, device=self.dev)
        if kw.prior is not None and not hasattr(self, "local_mabs"):
            self.local_mabs = torch.zeros(self.B, dtype=torch.float32, device=self.dev)
        gid = self.local_gid if kw.grouping is not None else None
        mabs = self.local_mabs if kw.prior is not None else None
        check(self._phase1(
            self.s._h, self.slot, Qdev.data_ptr(), self.T, self.B, self.nprobe, self.k, req, self.local_top.data_ptr(),
            None if gid is None else gid.data_ptr(), None if mabs is None else mabs.data_ptr(), self._stream()))
        return self.local_top, gid, mabs

    def phase2(self, Qdev, all_top, all_gid=None, grouping=None, group_base: int = 0, prior=None, prior_weight=1.0,
               all_mabs=None):
        """Second half (clb_search_shard_phase2_request_slot).  all_top: (n_shards, B, k) gathered `local_top` blocks.
        With `grouping` / `group_base` as in phase1 and `all_gid`, the gathered `local_gid` blocks: the grouped form
        -- the result goes into the packed grouped block, which is returned (for
        merge_grouped_packed, after the all-gather).
        With `prior` / `prior_weight` as in phase1 and `all_mabs`, the gathered `local_mabs` blocks (n_shards, B): the form
        with a prior, with or without a grouping; it returns what the form without a
        prior returns."""
        import torch
        from ._lib import ArgumentError
        self._check_queries(Qdev)
        if not self._fits(all_top, torch.float32, None, self.B, self.k):
            raise ArgumentError(f"all_top must be a contiguous float32 (n_shards, {self.B}, {self.k}) tensor on {self.dev}")
        g = grouping is not None
        if g:
            if not self._fits(all_gid, torch.int64, *all_top.shape):
                raise ArgumentError(f"all_gid must be a contiguous int64 tensor of all_top's shape on {self.dev}")
            block = self._grouped_block()
        req = self._request(SearchKeywords(grouping=grouping, prior=prior, prior_weight=prior_weight), group_base)
        if prior is not None and not self._fits(all_mabs, torch.float32, all_top.shape[0], self.B):
            raise ArgumentError(f"all_mabs must be a contiguous float32 (n_shards, {self.B}) tensor on {self.dev}")
        out_p, out_s, ncand = (self.g_out_p, self.g_out_s, self.g_ncand) if g else (self.out_p, self.out_s, self.ncand)
        check(self._phase2(
            self.s._h, self.slot, Qdev.data_ptr(), self.T, self.B, self.nprobe, self.k, req, all_top.data_ptr(),
            all_gid.data_ptr() if g else None, None if prior is None else all_mabs.data_ptr(), all_top.shape[0], out_p.data_ptr(),
            out_s.data_ptr(), self.g_out_g.data_ptr() if g else None, ncand.data_ptr(), self.g_edges.data_ptr() if g else None,
            self._stream()))
        return block if g else (self.out_p, self.out_s)

    def capture(self, Qstatic, filters=None, scope="candidates", grouping=None, per_group=None, prior=None, prior_weight=1.0,
                after=None, candidates=None, candidate_scores=None, candidate_priors=None):
        """A HIP graph of one search over the STATIC query buffer `Qstatic` (B, T, dim): the library enqueues nothing but
        kernels and memsets on the stream it is handed, so the nine launches of a search can be captured once and
        replayed -- write the next queries into `Qstatic` (e.g. let the encoder write there), `graph.replay()`, read
        `out_p` / `out_s`.  Measured (one query, 1 M passages; bench.py `p50_latency_graph_replay_ms`, tools/graph_probe.py):
        no faster than the stream launches (0.171-0.184 against 0.171-0.179 ms with a new query per replay) -- the host
        enqueues the eleven launches ahead of the device either way; on a 10 M-passage index, where a search is ~20
        launches, the replay is faster (0.259 against 0.318 ms).  The
        search runs once on a side stream first, so that the workspace is sized outside the capture.
        `filters` / `scope` / `grouping` / `per_group` as in __call__: the graph holds the filters' and the grouping's device
        addresses -- keep them open while it is replayed; with `per_group` the results are in `hit_p` / `hit_s`.  `prior` /
        `prior_weight` likewise: the graph holds the prior's device address and the weight.  `after` (a pair of device
        tensors, as in __call__): the graph holds their ADDRESSES, not their values -- to page, copy the last row of `out_s` /
        `out_p` into them and replay.  `candidates` / `candidate_scores` (device tensors, as in __call__): the graph holds
        their ADDRESSES too -- to re-rank under a graph, write the next batch's pids and lengths into the same tensors and
        replay (the sizing pass grows the slot for this stride; a larger stride needs a new capture).  `candidate_priors`
        likewise: the graph holds the ADDRESS of the value block and the weight -- write the next batch's values beside its pids."""
        return self._capture(Qstatic, SearchKeywords(
            filters=filters, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=candidate_scores, candidate_priors=candidate_priors))

    def _capture(self, Qstatic, kw: SearchKeywords):
        import torch
        self._check_queries(Qstatic)
        self.generation = self.s.generation
        cur = torch.cuda.current_stream(self.dev)
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._run(Qstatic, kw)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._run(Qstatic, kw)
        return graph

    def __call__(self, Qdev, filters=None, scope="candidates", grouping=None, per_group=None, prior=None, prior_weight=1.0,
                 after=None, candidates=None, candidate_scores=None, candidate_priors=None):
        """Qdev: torch float32 tensor holding B queries laid out (B, T, dim) contiguous == Julia (dim, T, B).  One call of
        clb_search_batch_request_device_slot, whatever the keywords.
        `filters`: one PassageFilter or a sequence of B entries (None = unfiltered), `scope` "candidates" / "all"
        (Searcher.search_batch); `ncand` then holds the counts after the filter.
        `grouping`: one PassageGrouping for the batch (Searcher.search_batch): the k best groups of every query, short
        results padded with pid 0 / -inf, `ncand` the candidate groups.
        `per_group` (an integer m, 1..16; needs `grouping`): returns `hit_p` / `hit_s`, (B, k, m) tensors == Julia (m, k, B)
        -- the m best candidate passages of every group, best first, padded with pid 0 / -inf
        (the request's per_group); `out_p` / `out_s` are not written.
        `prior` (one PassagePrior for the batch) with `prior_weight`: rank by score + prior_weight * value
        (Searcher.search_batch); not with `per_group`.
        `after`: a pair of device tensors (scores float32[B], pids int64[B]) on the searcher's device, one cursor per query --
        the next k results past it, always padded (Searcher.search_batch; the cursors stay on the device); a NaN score
        gives an empty page here.  Not with `grouping`, `per_group` or `prior`.
        `candidates`: a pair of device tensors (pids int64[B, L], lens int64[B]) on the searcher's device -- row b's first
        lens[b] entries are query b's candidate set (Searcher.search_batch; the lists stay on the device, nothing is raised
        about their contents: a length is clamped to 0..L, a pid outside the searcher's range is skipped).  With
        `candidate_scores` (float32[B, L]) the call also writes every listed passage's exact score at its position, -Inf
        where the position holds no candidate, and runs as the single exact pass.  Not with `filters`.
        `candidate_priors` (float32[B, L] on the searcher's device, needs `candidates`) with `prior_weight`: rank by score +
        prior_weight * the value beside a passage's first occurrence (Searcher.search_batch).  Nothing is raised about the
        values: one that is not finite, or whose product with the weight is not finite, counts as 0.  Not with `prior`,
        `per_group` > 1 or `after`."""
        return self._run(Qdev, SearchKeywords(
            filters=filters, scope=scope, grouping=grouping, per_group=per_group, prior=prior, prior_weight=prior_weight, after=after,
            candidates=candidates, candidate_scores=candidate_scores, candidate_priors=candidate_priors))

    def _run(self, Qdev, kw: SearchKeywords):
        import torch
        self._check_queries(Qdev)
        req = self._request(kw)
        out_p, out_s = self.out_p, self.out_s
        if kw.per_group is not None:
            m = int(req.per_group)
            if getattr(self, "hit_p", None) is None or self.hit_p.shape[2] != m:
                self.hit_p = torch.zeros((self.B, self.k, m), dtype=torch.int64, device=self.dev)
                self.hit_s = torch.zeros((self.B, self.k, m), dtype=torch.float32, device=self.dev)
            out_p, out_s = self.hit_p, self.hit_s
        check(self._search(
            self.s._h, self.slot, Qdev.data_ptr(), self.T, self.B, self.nprobe, self.k, req, out_p.data_ptr(), out_s.data_ptr(),
            self.ncand.data_ptr(), self._stream()))
        return out_p, out_s
