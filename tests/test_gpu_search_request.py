"""Every named search entry point against its request form (clb_search_request, include/colbert_hip.h), through ctypes on the
same searcher and inputs: pids, scores, n_cand and -- on the phases of a shard group -- every exchange buffer are equal byte for
byte, and with profiling on the per-kernel launch counts are equal.  No tolerance is involved anywhere.

Shapes: the index of smoke() (2 000 passages, K = 256), T = 32, nprobe = 2, k = 10, modes 0 and 1.  The batch routes run at B = 3
and at B = 65 -- two sub-batches of 64 and 1 queries: the offsets of the filters, the cursors and the [B][k][m] hit outputs
of the second sub-batch are what a request could get wrong.  The phases keep the whole batch on the slot: B = 3."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd._lib import SearchRequest
from tests import util_general as ug
from tests.test_gpu_filtered_search import random_allowed
from tests.test_gpu_grouped_search import modes_of
from tests.util_group import random_lens

pytestmark = pytest.mark.gpu

T, NPROBE, K = 32, 2, 10
V, I, CI, F = C.c_void_p, C.c_int64, C.c_int, C.c_float
FILL = -7                                          # what every output holds before a call: an unwritten entry stays equal


def ptr(a):
    """numpy array / torch tensor / None as the pointer argument of an entry point with or without argtypes"""
    if a is None:
        return None
    return V(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def request(**fields):
    return SearchRequest(struct_bytes=C.sizeof(SearchRequest), **fields)


def launches(s):
    return {name: v["launches"] for name, v in s.profile_read().items()}


def raw(a):
    return (a.cpu().numpy() if hasattr(a, "data_ptr") else a).tobytes()


def assert_pair(s, named, by_request, buffers, what, written, image=lambda bufs: [raw(b) for b in bufs]):
    """named(bufs) and by_request(bufs), each on fresh buffers: both succeed, every buffer is equal byte for byte, the
    launch counts are equal; `written`: indices of the buffers that the call must have written; `image`: the bytes of the
    buffers that are compared"""
    import torch
    got = []
    for call in (named, by_request):
        bufs = buffers()
        rc = call(bufs)
        assert rc == 0, (what, rc, clb.lib().clb_last_error())
        torch.cuda.synchronize()
        got.append((image(bufs), launches(s)))
    (a, la), (b, lb) = got
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, (what, "buffer", i)
    assert la == lb, (what, la, lb)
    fresh = image(buffers())
    for i in written:
        assert a[i] != fresh[i], (what, "buffer", i, "was not written")
    return la


class World:
    """one searcher with a filter, a grouping and a prior, and the queries on the host and on the device"""

    def __init__(self, idx, Qs):
        import torch
        self.s = clb.Searcher(index=idx, device=0)
        self.s.profile_enable(True)
        n = self.s.num_docs
        self.Q = Qs
        self.dev = torch.device("cuda", self.s.device)
        self.Qd = torch.from_numpy(np.array(Qs.transpose(2, 1, 0), order="C")).to(self.dev)
        self.filt = self.s.make_filter(pids=random_allowed(n, 0.4, 3))
        self.grp = self.s.make_grouping(group_lens=random_lens(n, 1, 6, 4))
        self.pri = self.s.make_prior(np.random.default_rng(5).normal(0, 0.5, n).astype(np.float32))

    def handles(self, B):
        """a filter for every query but query 1"""
        return self.s._filter_handles([None if b == 1 else self.filt for b in range(B)], B)

    def cursors(self, B):
        """the cursors behind the first page of the filtered search, query 0 at +Inf (no cursor)"""
        p, sc, _ = self.s.search_batch(self.Q[:, :, :B], K, NPROBE, filters=[None if b == 1 else self.filt for b in range(B)])
        launches(self.s)
        cs, cp = clb.next_cursor(p, sc)
        cs[0] = np.inf
        return np.ascontiguousarray(cs, np.float32), np.ascontiguousarray(cp, np.int64)

    def close(self):
        for h in (self.filt, self.grp, self.pri, self.s):
            h.close()


@pytest.fixture(scope="module")
def world():
    idx = synthetic.make_index(seed=7, n_docs=2000, K=256)
    w = World(idx, synthetic.make_queries(idx, 8, 65, T=T))
    yield w
    w.close()


# name -> (request fields, named entry on the host route, named entry on the device route); f: the operands of the case
CASES = {
    "plain": (lambda f: {},
              lambda l, head, f, outs: l.clb_search_batch(*head, CI(1), *outs),
              lambda l, head, f, outs: l.clb_search_batch_device_slot(*head, *outs)),
    "filtered-candidates": (lambda f: dict(filters=f["handles"], scope=0),
                            lambda l, head, f, outs: l.clb_search_batch_filtered(*head, f["handles"], CI(0), *outs),
                            lambda l, head, f, outs: l.clb_search_batch_filtered_device_slot(*head, f["handles"], CI(0), *outs)),
    "filtered-all": (lambda f: dict(filters=f["handles"], scope=1),
                     lambda l, head, f, outs: l.clb_search_batch_filtered(*head, f["handles"], CI(1), *outs),
                     lambda l, head, f, outs: l.clb_search_batch_filtered_device_slot(*head, f["handles"], CI(1), *outs)),
    "grouped": (lambda f: dict(grouping=f["grp"]),
                lambda l, head, f, outs: l.clb_search_batch_grouped(*head, None, CI(0), f["grp"], CI(1), *outs),
                lambda l, head, f, outs: l.clb_search_batch_grouped_device_slot(*head, None, CI(0), f["grp"], *outs)),
    "hits": (lambda f: dict(filters=f["handles"], scope=0, grouping=f["grp"], per_group=3),
             lambda l, head, f, outs: l.clb_search_batch_grouped_hits(*head, f["handles"], CI(0), f["grp"], I(3), CI(1), *outs),
             lambda l, head, f, outs: l.clb_search_batch_grouped_hits_device_slot(*head, f["handles"], CI(0), f["grp"], I(3), *outs)),
    "prior": (lambda f: dict(prior=f["pri"], prior_weight=0.5),
              lambda l, head, f, outs: l.clb_search_batch_prior(*head, None, CI(0), None, f["pri"], F(0.5), CI(1), *outs),
              lambda l, head, f, outs: l.clb_search_batch_prior_device_slot(*head, None, CI(0), None, f["pri"], F(0.5), *outs)),
    "prior-grouped": (lambda f: dict(grouping=f["grp"], prior=f["pri"], prior_weight=0.5),
                      lambda l, head, f, outs: l.clb_search_batch_prior(*head, None, CI(0), f["grp"], f["pri"], F(0.5), CI(1), *outs),
                      lambda l, head, f, outs: l.clb_search_batch_prior_device_slot(*head, None, CI(0), f["grp"], f["pri"], F(0.5), *outs)),
    "after": (lambda f: dict(filters=f["handles"], scope=0, after_scores=f["cs"], after_pids=f["cp"]),
              lambda l, head, f, outs: l.clb_search_batch_after(*head, f["handles"], CI(0), V(f["cs"]), V(f["cp"]), *outs),
              lambda l, head, f, outs: l.clb_search_batch_after_device_slot(*head, f["handles"], CI(0), V(f["cs"]), V(f["cp"]), *outs)),
}


def batch_pair(w, name, route, B, what):
    """one case on one route at one batch size: the named entry against the request entry"""
    import torch
    l = clb.lib()
    s = w.s
    fields, host_named, device_named = CASES[name]
    m, Tq = 3 if name == "hits" else 1, w.Q.shape[1]
    f = dict(handles=w.handles(B), grp=w.grp._h, pri=w.pri._h)
    if name == "after":
        cs, cp = w.cursors(B)
        if route == "device":
            cs, cp = torch.from_numpy(cs).to(w.dev), torch.from_numpy(cp).to(w.dev)
        f.update(keep=(cs, cp), cs=ptr(cs).value, cp=ptr(cp).value)
    if route == "host":
        head = (s._h, ptr(w.Q[:, :, :B]), I(Tq), I(B), I(NPROBE), I(K))
        buffers = lambda: (np.full(B * K * m, FILL, np.int64), np.full(B * K * m, FILL, np.float32), np.full(B, FILL, np.int64))
        req = request(pad_short=1, **fields(f))
        return assert_pair(s, lambda o: host_named(l, head, f, [ptr(x) for x in o]),
                           lambda o: l.clb_search_batch_request(*head, req, *[ptr(x) for x in o]), buffers, what, (0, 1, 2))
    head = (s._h, CI(1), ptr(w.Qd[:B]), I(Tq), I(B), I(NPROBE), I(K))
    buffers = lambda: (torch.full((B * K * m,), FILL, dtype=torch.int64, device=w.dev),
                       torch.full((B * K * m,), FILL, dtype=torch.float32, device=w.dev),
                       torch.full((B,), FILL, dtype=torch.int64, device=w.dev))
    req = request(**fields(f))
    return assert_pair(s, lambda o: device_named(l, head, f, [ptr(x) for x in o] + [None]),
                       lambda o: l.clb_search_batch_request_device_slot(*head, req, *[ptr(x) for x in o], None), buffers, what, (0, 1, 2))


@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_named_entry_and_its_request_give_the_same_bytes(world, name, route, B):
    for mode in modes_of(world.s):
        counted = batch_pair(world, name, route, B, f"{name} {route} B={B} mode {mode}")
        assert sum(counted.values()) > 0, counted          # profiling is on: the equal counts are counts of something


def test_the_single_query_and_slot_0_shorthands(world):
    import torch
    l = clb.lib()
    s, B = world.s, 3
    for mode in modes_of(s):
        head = (s._h, ptr(world.Q[:, :, :1]), I(T))
        buffers = lambda: (np.full(K, FILL, np.int64), np.full(K, FILL, np.float32), np.full(1, FILL, np.int64))
        req = request()                         # clb_search does not pad: fewer than k candidates is BoundsError
        assert_pair(s, lambda o: l.clb_search(*head, I(NPROBE), I(K), *[ptr(x) for x in o]),
                    lambda o: l.clb_search_batch_request(*head, I(1), I(NPROBE), I(K), req, *[ptr(x) for x in o]), buffers,
                    f"clb_search mode {mode}", (0, 1, 2))
        tail = (ptr(world.Qd[:B]), I(T), I(B), I(NPROBE), I(K))
        buffers = lambda: (torch.full((B * K,), FILL, dtype=torch.int64, device=world.dev),
                           torch.full((B * K,), FILL, dtype=torch.float32, device=world.dev),
                           torch.full((B,), FILL, dtype=torch.int64, device=world.dev))
        assert_pair(s, lambda o: l.clb_search_batch_device(s._h, *tail, *[ptr(x) for x in o], None),
                    lambda o: l.clb_search_batch_request_device_slot(s._h, CI(0), *tail, req, *[ptr(x) for x in o], None), buffers,
                    f"clb_search_batch_device mode {mode}", (0, 1, 2))


def test_plain_and_grouped_on_a_general_shape_index():
    """dim 136, T = 17, K = 65 (tests/util_general.py): the general-shape path reads the same Batch"""
    idx, Qs, nprobe = ug.case_inputs(4)
    assert nprobe == NPROBE
    w = World(idx, Qs)
    try:
        for name in ("plain", "grouped"):
            for route in ("host", "device"):
                batch_pair(w, name, route, 3, f"general shape {name} {route}")
    finally:
        w.close()


# ---- the phases of a shard group: B = 3, mode 1, the shard's own records fed back as n_shards = 1 ---------------------------
BASE = 5                                           # group_base of the grouped phases


def phase_buffers(w, B):
    import torch
    full = lambda shape, dtype: torch.full(shape, FILL, dtype=dtype, device=w.dev)
    return lambda: (full((B, K), torch.float32), full((B, K), torch.int64), full((B,), torch.float32),      # local top / gid / mabs
                    full((B, K), torch.int64), full((B, K), torch.float32), full((B, K), torch.int64),      # out pids / scores / gids
                    full((B,), torch.int64), full((B, 2), torch.int64))                                     # n_cand, edge gids


def phase_image(bufs):
    """The bytes of the phase buffers that are compared.  Phase 1 publishes the RECORDS of a query -- (score, group index)
    pairs in d_local_top / d_local_gid -- "in no particular order" (include/colbert_hip.h): local_top_kernel and
    group_local_top_kernel hand out the k places of a query with an LDS atomicAdd, so which record lands in which place
    depends on the order its waves arrive in, and two runs of the SAME named entry need not agree place by place.  The
    records of every query are therefore put in the order of their own bits and then compared byte for byte; every other
    buffer -- d_local_mabs and all outputs of phase 2 -- is compared as it is."""
    top, gid = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    order = np.lexsort((gid, top.view(np.uint32)), axis=1)
    records = [np.take_along_axis(top, order, axis=1).tobytes(), np.take_along_axis(gid, order, axis=1).tobytes()]
    return records + [raw(b) for b in bufs[2:]]


def by_request(l, head, req1, req2):
    """both phases through the request entries: phase 2 reads what phase 1 wrote (n_shards = 1)"""
    def run(o):
        top, gid, mabs, op, os_, og, nc, eg = [ptr(x) for x in o]
        rc = l.clb_search_shard_phase1_request_slot(*head, req1, top, gid, mabs, None)
        return rc or l.clb_search_shard_phase2_request_slot(*head, req2, top, gid, mabs, I(1), op, os_, og, nc, eg, None)
    return run


def phase_cases(w, B):
    """name -> (fields of the request, both named phases as one call over the buffers, indices of the buffers written)"""
    l = clb.lib()
    s = w.s
    head = (s._h, CI(2), ptr(w.Qd[:B]), I(T), I(B), I(NPROBE), I(K))
    head0 = head[:1] + head[2:]                    # the shorthands without a slot
    fh, g, p = w.handles(B), w.grp._h, w.pri._h

    def named(phase1, phase2):
        def run(o):
            o = [ptr(x) for x in o]
            return phase1(*o[:3]) or phase2(*o)
        return run

    plain2 = lambda top, gid, mabs, op, os_, og, nc, eg: l.clb_search_shard_phase2_slot(*head, top, I(1), op, os_, nc, None)
    grouped2 = lambda top, gid, mabs, op, os_, og, nc, eg: l.clb_search_shard_phase2_grouped_slot(*head, top, gid, I(1), g, I(BASE), op,
                                                                                               os_, og, nc, eg, None)
    prior2 = lambda grp: (lambda top, gid, mabs, op, os_, og, nc, eg: l.clb_search_shard_phase2_prior_slot(
        *head, top, gid, mabs, I(1), grp, I(BASE), p, F(0.5), op, os_, og, nc, eg, None))
    return {
        "plain": ({}, named(lambda top, gid, mabs: l.clb_search_shard_phase1_slot(*head, top, None), plain2), (0, 3, 4, 6)),
        "filtered-candidates": (dict(filters=fh, scope=0),
                                named(lambda top, gid, mabs: l.clb_search_shard_phase1_filtered_slot(*head, fh, CI(0), top, None), plain2),
                                (0, 3, 4, 6)),
        "filtered-all": (dict(filters=fh, scope=1),
                         named(lambda top, gid, mabs: l.clb_search_shard_phase1_filtered_slot(*head, fh, CI(1), top, None), plain2),
                         (0, 3, 4, 6)),
        "grouped": (dict(filters=fh, scope=0, grouping=g, group_base=BASE),
                    named(lambda top, gid, mabs: l.clb_search_shard_phase1_grouped_slot(*head, fh, CI(0), g, I(BASE), top, gid, None),
                          grouped2), (0, 1, 3, 4, 5, 6, 7)),
        "prior": (dict(prior=p, prior_weight=0.5),
                  named(lambda top, gid, mabs: l.clb_search_shard_phase1_prior_slot(*head, None, CI(0), None, I(0), p, F(0.5), top, gid,
                                                                                    mabs, None), prior2(None)), (0, 2, 3, 4, 6)),
        "prior-grouped": (dict(grouping=g, group_base=BASE, prior=p, prior_weight=0.5),
                          named(lambda top, gid, mabs: l.clb_search_shard_phase1_prior_slot(*head, None, CI(0), g, I(BASE), p, F(0.5), top,
                                                                                            gid, mabs, None), prior2(g)),
                          (0, 1, 2, 3, 4, 5, 6, 7)),
        "slot-0": ({}, named(lambda top, gid, mabs: l.clb_search_shard_phase1(*head0, top, None),
                             lambda top, gid, mabs, op, os_, og, nc, eg: l.clb_search_shard_phase2(*head0, top, I(1), op, os_, nc, None)),
                   (0, 3, 4, 6)),
    }


@pytest.mark.parametrize("name", ["plain", "filtered-candidates", "filtered-all", "grouped", "prior", "prior-grouped", "slot-0"])
def test_the_named_phases_and_their_requests_give_the_same_bytes(world, name):
    l = clb.lib()
    s, B = world.s, 3
    s.set_mode(1)
    fields, named, written = phase_cases(world, B)[name]
    head = (s._h, CI(0 if name == "slot-0" else 2), ptr(world.Qd[:B]), I(T), I(B), I(NPROBE), I(K))
    req1 = request(**fields)
    req2 = request(**{k: v for k, v in fields.items() if k not in ("filters", "scope")})      # phase 2 takes no filters
    assert_pair(s, named, by_request(l, head, req1, req2), phase_buffers(world, B), f"phases {name}", written, phase_image)


def test_phase_1_by_a_named_entry_and_phase_2_by_the_request(world):
    """the pending record of phase 1 is compared against the request phase 2 is given: the two forms mix on one slot"""
    import torch
    l = clb.lib()
    s, B = world.s, 3
    s.set_mode(1)
    g = world.grp._h
    head = (s._h, CI(3), ptr(world.Qd[:B]), I(T), I(B), I(NPROBE), I(K))
    top, gid, mabs, op, os_, og, nc, eg = o = phase_buffers(world, B)()
    assert l.clb_search_shard_phase1_grouped_slot(*head, None, CI(0), g, I(BASE), ptr(top), ptr(gid), None) == 0
    req = request(grouping=g, group_base=BASE)
    assert l.clb_search_shard_phase2_request_slot(*head, req, ptr(top), ptr(gid), None, I(1), ptr(op), ptr(os_), ptr(og), ptr(nc),
                                                  ptr(eg), None) == 0, l.clb_last_error()
    torch.cuda.synchronize()
    assert torch.all(nc > 0) and torch.all(op[:, 0] > 0) and torch.all(og[:, 0] >= BASE)
    # ... and the other way round, against the same result
    o2 = phase_buffers(world, B)()
    assert l.clb_search_shard_phase1_request_slot(*head, req, ptr(o2[0]), ptr(o2[1]), None, None) == 0
    assert l.clb_search_shard_phase2_grouped_slot(*head, ptr(o2[0]), ptr(o2[1]), I(1), g, I(BASE), ptr(o2[3]), ptr(o2[4]), ptr(o2[5]),
                                                  ptr(o2[6]), ptr(o2[7]), None) == 0, l.clb_last_error()
    torch.cuda.synchronize()
    assert phase_image(o) == phase_image(o2)
    launches(s)


def test_phase_2_without_the_prior_of_phase_1_is_refused(world):
    l = clb.lib()
    s, B = world.s, 3
    s.set_mode(1)
    head = (s._h, CI(3), ptr(world.Qd[:B]), I(T), I(B), I(NPROBE), I(K))
    top, gid, mabs, op, os_, og, nc, eg = [ptr(x) for x in phase_buffers(world, B)()]
    with_prior = request(prior=world.pri._h, prior_weight=0.5)
    assert l.clb_search_shard_phase1_request_slot(*head, with_prior, top, None, mabs, None) == 0
    assert l.clb_search_shard_phase2_request_slot(*head, request(), top, None, None, I(1), op, os_, None, nc, None, None) == 4
    assert b"without a matching" in l.clb_last_error()
    other_weight = request(prior=world.pri._h, prior_weight=0.25)
    assert l.clb_search_shard_phase2_request_slot(*head, other_weight, top, None, mabs, I(1), op, os_, None, nc, None, None) == 4
    assert b"without a matching" in l.clb_last_error()
    assert l.clb_search_shard_phase2_request_slot(*head, with_prior, top, None, mabs, I(1), op, os_, None, nc, None, None) == 0
    launches(s)
