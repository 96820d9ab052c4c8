"""Launch accounting of the search host path (csrc/search.hip): which profile row every launch lands in, how often, and the
work counters of the batch -- per request, compared for equality with tests/golden/search_launch_profile.json.

Bit-equal results do not show a launch that moved into another timed scope or one that now runs twice; the profile rows
(`profile_read()["..."]["launches"]`, counted per timed scope) and `last_batch_stats()` do.  The golden file holds what the
library gave at the commit named in its `recorded_from`; it is recorded by this same test with
COLBERT_RECORD_LAUNCH_PROFILE=<that commit> in the environment (and COLBERT_HIP_LIB naming that commit's library), which
writes the file and compares nothing.

One search per row, a few milliseconds each: the tuned index of tests/util_synth.py (dim 128, nbits 2, 300 passages) and a
general-shape index (dim 64).  The rows of two sub-batches (B = 65) also hold queries 64 and 0 against the same queries
searched alone, bit for bit: the one place a wrong offset of the second sub-batch would show."""
import json
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from colbert_jl_amd.distributed import DeviceSearch
from tests.util_synth import tiny_index

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_launch_profile.json")
RECORD = os.environ.get("COLBERT_RECORD_LAUNCH_PROFILE", "")
K = 10
K_SORT = 16384 + 1                      # just above kMaxTopK (csrc/search_kernels.hpp): the full sort per query
REQUESTS = ("plain", "filtered-candidates", "filtered-all", "grouped", "grouped-hits", "prior", "grouped-prior", "cursor",
            "listed", "listed-scores", "listed-priors")


class World:
    """one searcher with its operands; every per-query operand differs from query to query, so that a slice of it is
    that query's own"""

    def __init__(self, idx, n_queries, lengths):
        self.s = clb.Searcher(index=idx, device=0)
        n = self.s.num_docs
        rng = np.random.default_rng(11)
        self.Q = {T: synthetic.make_queries(idx, 2000 + T, n_queries, T=T) for T in lengths}
        self.filt = [self.s.make_filter(pids=1 + rng.choice(n, size=int(0.4 * n), replace=False)) for _ in range(2)]
        self.grp = self.s.make_grouping(group_lens=np.full(n // 3, 3))
        self.pri = self.s.make_prior(rng.normal(0, 0.5, n).astype(np.float32))
        self.lists = [1 + rng.choice(n, size=40 + b % 7, replace=True) for b in range(n_queries)]
        self.values = [rng.normal(0, 0.5, l.size).astype(np.float32) for l in self.lists]

    def keywords(self, name, T, nprobe, queries):
        """the keywords of request `name` for the queries `queries` (indices into the world's)"""
        g, p = self.grp, self.pri
        if name == "cursor":        # behind the first page of the plain search
            pids, scores, _ = self.s.search_batch(self.Q[T][:, :, queries], K, nprobe, pad_short=True)
            return dict(after=clb.next_cursor(pids, scores))
        return {"plain": {}, "grouped": dict(grouping=g), "grouped-hits": dict(grouping=g, per_group=2),
                "filtered-candidates": dict(filters=[self.filt[b % 2] for b in queries]),
                "filtered-all": dict(filters=[self.filt[b % 2] for b in queries], scope="all"),
                "prior": dict(prior=p, prior_weight=0.5), "grouped-prior": dict(grouping=g, prior=p, prior_weight=0.5),
                "listed": dict(candidates=[self.lists[b] for b in queries]),
                "listed-scores": dict(candidates=[self.lists[b] for b in queries], return_candidate_scores=True),
                "listed-priors": dict(candidates=[self.lists[b] for b in queries], prior_weight=0.5,
                                      candidate_priors=[self.values[b] for b in queries])}[name]

    def close(self):
        for h in self.filt + [self.grp, self.pri, self.s]:
            h.close()


def counted(s, run):
    """run() with profiling and counters on -> (what it returned, {"launches": per profile row, "stats": the batch's})"""
    s.profile_enable(True, counters=True)
    try:
        s.profile_read()
        out = run()
        launches = {name: int(v["launches"]) for name, v in s.profile_read().items()}
        return out, {"launches": launches, "stats": s.last_batch_stats()}
    finally:
        s.profile_enable(False)


def batch_row(w, name, mode, B, nprobe, T, k=K):
    s = w.s
    s.set_mode(mode)
    queries = list(range(B))
    kw = w.keywords(name, T, nprobe, queries)
    out, row = counted(s, lambda: s.search_batch(w.Q[T][:, :, :B], k, nprobe, pad_short=True, **kw))
    if B > 64:      # two sub-batches: the first query of each against the same query searched alone
        for b in (64, 0):
            alone = s.search_batch(w.Q[T][:, :, [b]], k, nprobe, pad_short=True, **w.keywords(name, T, nprobe, [b]))
            for got, want in zip(out, alone):
                got, want = (got[b], want[0]) if isinstance(got, list) or got.ndim == 1 else (got[..., b], want[..., 0])
                assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (name, mode, nprobe, T, b)
    return row


def phase_row(w, name, B, nprobe, T):
    """phase 1 then phase 2 on one shard, its own records gathered from n_shards = 1"""
    import torch
    s = w.s
    s.set_mode(1)
    dev = torch.device("cuda", s.device)
    Qd = torch.from_numpy(np.array(w.Q[T][:, :, :B].transpose(2, 1, 0), order="C")).to(dev)
    run = DeviceSearch(s, T, B, K, nprobe)
    kw = {"plain": {}, "grouped": dict(grouping=w.grp, group_base=0), "prior": dict(prior=w.pri, prior_weight=0.5)}[name]

    def both():
        records = run.phase1(Qd, **kw)          # local_top alone, or with local_gid, or with local_gid (or None) and local_mabs
        top, gid, mabs = ((records if isinstance(records, tuple) else (records,)) + (None, None))[:3]
        more = {} if gid is None else dict(all_gid=gid[None].contiguous())
        if mabs is not None:
            more["all_mabs"] = mabs[None].contiguous()
        run.phase2(Qd, top[None].contiguous(), **kw, **more)
        torch.cuda.synchronize()
    return counted(s, both)[1]


def tuned_rows(w):
    rows = {}
    for mode in (0, 1):
        for B in (1, 8, 16, 65):
            for nprobe in (2, 4):
                for T in (32, 40):
                    rows[f"plain mode{mode} B{B} nprobe{nprobe} T{T}"] = lambda a=(mode, B, nprobe, T): batch_row(w, "plain", *a)
        for name in REQUESTS[1:]:
            # one query, two sub-batches, and the batched kernels on the unfused centroid stage
            for B, nprobe in ((1, 2), (65, 2), (16, 4)):
                rows[f"{name} mode{mode} B{B} nprobe{nprobe} T32"] = lambda a=(name, mode, B, nprobe): batch_row(w, *a, 32)
        for name in ("plain", "grouped"):
            rows[f"{name} mode{mode} B2 nprobe2 T32 k{K_SORT}"] = lambda a=(name, mode): batch_row(w, *a, 2, 2, 32, k=K_SORT)
    for name in ("plain", "grouped", "prior"):
        rows[f"phases {name} B3 nprobe2 T32"] = lambda name=name: phase_row(w, name, 3, 2, 32)
    return rows


def general_rows(w):
    rows = {f"general {name} B3 nprobe2 T32": (lambda name=name: batch_row(w, name, 0, 3, 2, 32))
            for name in ("plain", "grouped", "cursor")}
    rows["general plain B1 nprobe2 T129"] = lambda: batch_row(w, "plain", 0, 1, 2, 129)
    return rows


@pytest.fixture(scope="module")
def measured():
    """every row of the matrix, run once"""
    out = {}
    idx, _ = tiny_index()
    for make, index, n_queries, lengths in ((tuned_rows, idx, 65, (32, 40)),
                                            (general_rows, synthetic.make_index(3, 300, K=64, dim=64), 3, (32, 129))):
        w = World(index, n_queries, lengths)
        try:
            for name, row in make(w).items():
                out[name] = row()
        finally:
            w.close()
    return out


def test_launches_and_counters_of_every_request_equal_the_recorded_ones(measured):
    if RECORD:
        with open(GOLDEN, "w") as f:
            json.dump({"recorded_from": RECORD, "rows": measured}, f, indent=0, sort_keys=True)
        return
    with open(GOLDEN) as f:
        golden = json.load(f)["rows"]
    assert sorted(measured) == sorted(golden)
    different = {name: (row, golden[name]) for name, row in measured.items() if row != golden[name]}
    assert not different, different


def test_the_matrix_reaches_every_timed_stage(measured):
    """the equal counts are counts of something: every profile row is launched by some request, and a two-pass row
    re-scores some of its candidates"""
    for stage in ("centroid_scores", "top_nprobe", "mark_candidates", "compact_candidates", "score_exact", "score_approx",
                  "select_margin", "rescore_rows", "topk"):
        assert any(row["launches"][stage] > 0 for row in measured.values()), stage
    row = measured["plain mode1 B65 nprobe2 T32"]
    assert 0 < row["stats"]["rescored_docs"] <= row["stats"]["cand_docs"], row
