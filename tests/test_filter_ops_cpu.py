"""Composing filters on the device, the part that needs no GPU: the four new symbols of the C ABI with the argument checks
that need nothing of a searcher's state, what the Python operators and `combine_filters` hand the library (op code, operand
order), the conversion of range bounds, and the part-by-part work of a stubbed shard group."""
import ctypes as C

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import sharded
from tests.test_group_cpu import _NoDevice
from tests.test_sharded_searcher_cpu import SIZES, stub_group

NEW_SYMBOLS = ("clb_filter_combine", "clb_filter_create_range", "clb_filter_extend", "clb_filter_bitmap")
AND, OR, ANDNOT, NOT = 0, 1, 2, 3
EARG = 4
i64 = C.c_int64
NAN, INF = float("nan"), float("inf")


def fresh():
    return C.c_void_p(0xdead0)                 # an `out` that every failure must reset to NULL


def operands(*addresses):
    arr = (C.c_void_p * len(addresses))()
    for i, a in enumerate(addresses):
        arr[i] = a
    return arr


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_filter_op_symbols_are_declared_and_exported():
    l = clb.lib()
    declared = clb.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(l, name), name
    header = " ".join(open(clb._lib.HEADER).read().replace("*", " ").split())
    for text in ("CLB_FILTER_OP_AND = 0, CLB_FILTER_OP_OR = 1, CLB_FILTER_OP_ANDNOT = 2, CLB_FILTER_OP_NOT = 3",
                 "CLB_MAX_FILTER_OPERANDS = 16", "CLB_RANGE_LO_OPEN = 1, CLB_RANGE_HI_OPEN = 2", "exact up to 2^24"):
        assert text in header, text


def test_filter_combine_checks_its_arguments_first():
    """Nothing here reaches a device or reads the searcher: `s` and the operands are addresses that are never followed."""
    l = clb.lib()
    s, null = C.c_void_p(0xbeef0), C.c_void_p()
    two = operands(0xfee0, 0xfee8)

    def refused(what, *args):
        out = fresh()
        assert l.clb_filter_combine(*args, C.byref(out)) == EARG, what
        assert what.encode() in l.clb_last_error(), (what, l.clb_last_error())
        assert out.value is None, what         # a failed call leaves no handle

    refused("null searcher", null, AND, two, i64(2))
    assert l.clb_filter_combine(s, AND, two, i64(2), None) == EARG and b"out is null" in l.clb_last_error()
    for op in (-1, 4, 100):
        refused("op must be", s, op, two, i64(2))
    for n in (0, -1, 17, 1 << 40):
        for op in (AND, OR, ANDNOT):
            refused("n must be 1..16", s, op, two, i64(n))
    many = operands(*[0xfee0] * 17)
    refused("n must be 1..16", s, OR, many, i64(17))
    for n in (2, 3, 16):
        refused("CLB_FILTER_OP_NOT takes n = 1", s, NOT, many, i64(n))
    refused("n must be 1..16", s, NOT, many, i64(0))
    refused("operands is null", s, AND, None, i64(2))
    refused("operand 1 is null", s, ANDNOT, operands(0xfee0, None, 0xfee8), i64(3))
    refused("operand 0 is null", s, NOT, operands(None), i64(1))
    refused("operand 15 is null", s, OR, operands(*([0xfee0] * 15 + [None])), i64(16))


def test_filter_range_checks_its_arguments_first():
    l = clb.lib()
    s, null, prior = C.c_void_p(0xbeef0), C.c_void_p(), C.c_void_p(0xfee0)

    def refused(what, *args):
        out = fresh()
        assert l.clb_filter_create_range(*args, C.byref(out)) == EARG, what
        assert what.encode() in l.clb_last_error(), (what, l.clb_last_error())
        assert out.value is None, what

    refused("null searcher", null, prior, 0.0, 1.0, 0)
    assert l.clb_filter_create_range(s, prior, 0.0, 1.0, 0, None) == EARG and b"out is null" in l.clb_last_error()
    refused("values is null", s, null, 0.0, 1.0, 0)
    refused("lo is NaN", s, prior, NAN, 1.0, 0)
    refused("hi is NaN", s, prior, 0.0, NAN, 3)
    refused("lo is NaN", s, prior, NAN, NAN, 0)
    for flags in (4, 8, 7, -1, 1 << 20):
        refused("flags must be", s, prior, 0.0, 1.0, flags)
    refused("flags must be", s, prior, -INF, INF, 4)           # infinite bounds are fine; the flag is not


def test_filter_extend_and_bitmap_check_their_arguments_first():
    l = clb.lib()
    s, null, f = C.c_void_p(0xbeef0), C.c_void_p(), C.c_void_p(0xfee0)

    def refused(what, *args):
        out = fresh()
        assert l.clb_filter_extend(*args, C.byref(out)) == EARG, what
        assert what.encode() in l.clb_last_error(), (what, l.clb_last_error())
        assert out.value is None, what

    refused("null searcher", null, f, 0)
    assert l.clb_filter_extend(s, f, 0, None) == EARG and b"out is null" in l.clb_last_error()
    refused("f is null", s, null, 1)
    for fill in (2, -1, 255):
        refused("fill must be 0", s, f, fill)
    words = np.zeros(4, np.uint32)
    assert l.clb_filter_bitmap(null, words.ctypes.data_as(C.c_void_p), i64(4)) == EARG
    assert b"f is null" in l.clb_last_error()
    assert l.clb_filter_bitmap(null, None, i64(0)) == EARG and b"f is null" in l.clb_last_error()


# ---- Python: what the library is handed -----------------------------------------------------------------------------------
class Recorder:
    """stands in for one entry point of the loaded library: records the arguments, makes nothing (out stays NULL)"""

    def __init__(self):
        self.calls = []

    def combine(self, s, op, arr, n, out):
        self.calls.append((op.value, [arr[i] for i in range(n.value)]))
        return 0

    def range(self, s, prior, lo, hi, flags, out):
        self.calls.append((prior.value, lo.value, hi.value, flags.value))
        return 0

    def extend(self, s, f, fill, out):
        self.calls.append((f.value, fill.value))
        return 0


@pytest.fixture
def fakes():
    """a searcher without a device and filters a, b, c with addresses that are never followed nor destroyed"""
    s = _NoDevice()
    fs = [clb.PassageFilter(s, C.c_void_p(0x1000 * (i + 1)), 3) for i in range(3)]
    p = clb.PassagePrior(s, C.c_void_p(0x9000), 100, 2.0)
    yield s, fs, p
    for x in fs + [p]:
        x._h = None


def test_operators_hand_the_library_op_and_operand_order(fakes, monkeypatch):
    s, (a, b, c), _ = fakes
    rec = Recorder()
    monkeypatch.setattr(clb.lib(), "clb_filter_combine", rec.combine)
    A, B, Cc = 0x1000, 0x2000, 0x3000
    r = a & b
    assert isinstance(r, clb.PassageFilter) and r.searcher is s and r.num_docs == 100
    b & a, a | b, a - b, b - a, ~a, ~c
    assert rec.calls == [(AND, [A, B]), (AND, [B, A]), (OR, [A, B]), (ANDNOT, [A, B]), (ANDNOT, [B, A]), (NOT, [A]), (NOT, [Cc])]
    rec.calls.clear()
    s.combine_filters("and", [a, b, c]), s.combine_filters("or", (c, a)), s.combine_filters("andnot", [c, a, b, a])
    s.combine_filters("not", [b]), s.combine_filters("not", b), s.combine_filters("or", [a]), s.combine_filters("and", [a] * 16)
    assert rec.calls == [(AND, [A, B, Cc]), (OR, [Cc, A]), (ANDNOT, [Cc, A, B, A]), (NOT, [B]), (NOT, [B]), (OR, [A]),
                         (AND, [A] * 16)]
    rec.calls.clear()
    for op, fl in (("xor", [a, b]), ("AND", [a, b]), (0, [a]), (None, [a])):
        with pytest.raises(clb.ArgumentError, match="op must be"):
            s.combine_filters(op, fl)
    for op, fl in (("and", []), ("or", [a] * 17), ("not", [])):
        with pytest.raises(clb.ArgumentError, match="1..16 filters"):
            s.combine_filters(op, fl)
    with pytest.raises(clb.ArgumentError, match="'not' takes exactly one"):
        s.combine_filters("not", [a, b])
    closed = clb.PassageFilter(s, None, 3)
    for call, j in ((lambda: s.combine_filters("and", [a, closed]), 1), (lambda: a & closed, 1), (lambda: closed | a, 0),
                    (lambda: ~closed, 0), (lambda: a - np.ones(100, bool), 1), (lambda: s.combine_filters("or", [a, b, None]), 2),
                    (lambda: a & 1, 1)):
        with pytest.raises(clb.ColBERTError, match=rf"filters\[{j}\] is not an open PassageFilter"):
            call()
    assert rec.calls == []                     # refused on the host: the library was not called


def test_range_bounds_are_converted_and_checked(fakes, monkeypatch):
    s, _, p = fakes
    rec = Recorder()
    monkeypatch.setattr(clb.lib(), "clb_filter_create_range", rec.range)
    s.make_range_filter(p)
    s.make_range_filter(p, lo=0.5)
    s.make_range_filter(p, hi=3, hi_open=True)
    s.make_range_filter(p, 0.1, np.float64(0.7), lo_open=True)
    s.make_range_filter(p, np.int64(2), np.float32(2.0), True, True)
    s.make_range_filter(p, -INF, INF)
    f32 = lambda x: float(np.float32(x))
    assert rec.calls == [(0x9000, -INF, INF, 0), (0x9000, 0.5, INF, 0), (0x9000, -INF, 3.0, 2), (0x9000, f32(0.1), f32(0.7), 1),
                         (0x9000, 2.0, 2.0, 3), (0x9000, -INF, INF, 0)]
    rec.calls.clear()
    for bad in (NAN, np.float32("nan"), "1", b"1", "lo", True, [1.0], np.zeros(1), 1j):
        with pytest.raises(clb.ArgumentError, match="lo must be a real number or None"):
            s.make_range_filter(p, lo=bad)
        with pytest.raises(clb.ArgumentError, match="hi must be a real number or None"):
            s.make_range_filter(p, 0.0, bad)
    closed = clb.PassagePrior(s, None, 100, 1.0)
    for not_a_prior in (closed, None, np.zeros(100, np.float32), s):
        with pytest.raises(clb.ColBERTError, match="open PassagePrior"):
            s.make_range_filter(not_a_prior, 0.0, 1.0)
    assert rec.calls == []


def test_extended_and_to_mask_on_the_host(fakes, monkeypatch):
    s, (a, b, c), _ = fakes
    rec = Recorder()
    monkeypatch.setattr(clb.lib(), "clb_filter_extend", rec.extend)
    a.extended(), a.extended(True), b.extended(fill=False)
    assert rec.calls == [(0x1000, 0), (0x1000, 1), (0x2000, 0)]
    for bad in (2, "yes", None, 1.0):
        with pytest.raises(clb.ArgumentError, match="fill must be True or False"):
            a.extended(bad)
    closed = clb.PassageFilter(s, None, 3)
    with pytest.raises(clb.ColBERTError, match="not an open PassageFilter"):
        closed.extended()
    with pytest.raises(clb.ColBERTError, match="not an open PassageFilter"):
        closed.to_mask()
    assert len(rec.calls) == 3


# ---- a stubbed shard group ------------------------------------------------------------------------------------------------
class Part:
    """what a ShardedFilter / ShardedPrior holds per shard, with no device behind it"""

    def __init__(self, searcher, name, count=0, mask=None):
        self.searcher, self.name, self.count, self.closed, self.mask = searcher, name, count, False, mask
        self.num_docs = searcher.num_docs

    def close(self):
        self.closed = True

    def to_mask(self):
        return self.mask


def op_group():
    """tests/test_sharded_searcher_cpu's stub group whose shards record the filter calls they receive"""
    g = stub_group()
    for i, s in enumerate(g.shards):
        s.calls = []

        def combine(op, filters, s=s, i=i):
            s.calls.append(("combine", op, [f.name for f in filters]))
            assert all(f.searcher is s for f in filters)       # index by index: a shard sees only its own parts
            return Part(s, f"{op}{i}", count=i + 1)

        def make_range(prior, lo, hi, lo_open, hi_open, s=s, i=i):
            s.calls.append(("range", prior.name, lo, hi, lo_open, hi_open))
            assert prior.searcher is s
            return Part(s, f"range{i}", count=10 * (i + 1))

        s.combine_filters, s.make_range_filter = combine, make_range
    return g


def stub_filter(g, name):
    return sharded.ShardedFilter(g, [Part(s, f"{name}{i}") for i, s in enumerate(g.shards)], 0)


def test_a_shard_group_combines_part_by_part():
    g = op_group()
    n = len(SIZES)
    a, b, c = (stub_filter(g, x) for x in "abc")
    r = g.combine_filters("andnot", [a, b, c])
    assert isinstance(r, sharded.ShardedFilter) and r.group is g and [p.name for p in r.parts] == [f"andnot{i}" for i in range(n)]
    assert r.count == sum(range(1, n + 1)) and r.num_docs == sum(SIZES)
    for i, s in enumerate(g.shards):
        assert s.calls == [("combine", "andnot", [f"a{i}", f"b{i}", f"c{i}"])]
        s.calls.clear()
    a & b, b | a, a - c, c - a, ~b, g.combine_filters("or", a), g.combine_filters("and", [c, a, a])
    for i, s in enumerate(g.shards):
        assert s.calls == [("combine", "and", [f"a{i}", f"b{i}"]), ("combine", "or", [f"b{i}", f"a{i}"]),
                           ("combine", "andnot", [f"a{i}", f"c{i}"]), ("combine", "andnot", [f"c{i}", f"a{i}"]),
                           ("combine", "not", [f"b{i}"]), ("combine", "or", [f"a{i}"]), ("combine", "and", [f"c{i}", f"a{i}", f"a{i}"])]
        s.calls.clear()


def test_a_shard_group_refuses_operands_of_another_group():
    g, other = op_group(), op_group()
    a, foreign = stub_filter(g, "a"), stub_filter(other, "x")
    single = clb.PassageFilter(_NoDevice(), None, 3)
    for call, j in ((lambda: g.combine_filters("and", [a, foreign]), 1), (lambda: a & foreign, 1), (lambda: foreign | a, 1),   # asked of foreign's group
                    (lambda: a - single, 1), (lambda: g.combine_filters("or", [a, a, None]), 2), (lambda: g.combine_filters("not", [foreign]), 0)):
        with pytest.raises(clb.ColBERTError, match=rf"filters\[{j}\] is not a ShardedFilter of this shard group"):
            call()
    assert all(s.calls == [] for s in g.shards + other.shards)           # refused before any shard is called


def test_a_failing_shard_closes_the_parts_already_made():
    g = op_group()
    a = stub_filter(g, "a")
    made = []
    first = g.shards[0].combine_filters

    def keep(op, filters):
        made.append(first(op, filters))
        return made[-1]

    def fail(op, filters):
        raise clb.ArgumentError("the filter of operand 0: filter made before an append; make another")

    g.shards[0].combine_filters, g.shards[1].combine_filters = keep, fail
    with pytest.raises(clb.ArgumentError, match="made before an append"):
        ~a
    assert len(made) == 1 and made[0].closed


def test_a_shard_group_takes_ranges_part_by_part():
    g, other = op_group(), op_group()
    n = len(SIZES)
    prior = sharded.ShardedPrior(g, [Part(s, f"p{i}") for i, s in enumerate(g.shards)], 2.0, g.num_docs)
    r = g.make_range_filter(prior, 0.25, None, lo_open=True)
    assert isinstance(r, sharded.ShardedFilter) and r.count == sum(10 * (i + 1) for i in range(n))
    for i, s in enumerate(g.shards):
        assert s.calls == [("range", f"p{i}", 0.25, None, True, False)]
        s.calls.clear()
    for bad in (NAN, "3"):
        with pytest.raises(clb.ArgumentError, match="must be a real number or None"):
            g.make_range_filter(prior, bad, 1.0)
        with pytest.raises(clb.ArgumentError, match="must be a real number or None"):
            g.make_range_filter(prior, hi=bad)
    foreign = sharded.ShardedPrior(other, [Part(s, "q") for s in other.shards], 2.0, other.num_docs)
    closed = sharded.ShardedPrior(g, [Part(s, "c") for s in g.shards], 2.0, g.num_docs)
    closed.close()
    for not_ours in (foreign, closed, None, clb.PassagePrior(_NoDevice(), None, 100, 1.0)):
        with pytest.raises(clb.ColBERTError, match="not an open ShardedPrior of this shard group"):
            g.make_range_filter(not_ours, 0.0, 1.0)
    stale = sharded.ShardedPrior(g, [Part(s, "s") for s in g.shards], 2.0, g.num_docs - 1)
    with pytest.raises(clb.ArgumentError, match="prior made before an append; make another"):
        g.make_range_filter(stale, 0.0, 1.0)
    assert all(s.calls == [] for s in g.shards)


def test_a_sharded_mask_puts_every_slice_at_its_global_position():
    g = op_group()
    rng = np.random.default_rng(3)
    masks = [rng.random(n) < 0.5 for n in SIZES]
    f = sharded.ShardedFilter(g, [Part(s, f"m{i}", mask=masks[i]) for i, s in enumerate(g.shards)], 0)
    assert np.array_equal(f.to_mask(), np.concatenate(masks)) and f.to_mask().dtype == np.bool_
    # a rank that holds shards 1 and 2 of the four: its slices at their places, False elsewhere
    part = sharded.ShardedFilter(g, [Part(g.shards[i], f"m{i}", mask=masks[i]) for i in (1, 2)], 0)
    want = np.concatenate([np.zeros(SIZES[0], bool), masks[1], masks[2], np.zeros(SIZES[3], bool)])
    assert np.array_equal(part.to_mask(), want)
