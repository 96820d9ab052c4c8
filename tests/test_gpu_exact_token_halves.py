"""Pass 2 of the two-pass mode multiplies a passage's row only against the token half (tokens 0..15 / 16..31) whose window
selected it: the row sweep leaves one mask per half, and the exact kernel walks every chunk of a wave's passages twice, parking
the sum of tokens 0..15 between the walks.  Results stay bit-identical to the oracle; these tests aim at the new branches."""
import functools

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from test_gpu_parity import check_search
from test_gpu_pass1_packing import RAGGED, _with_doclens

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ragged_index():
    """3 000 short passages, 500 of them with the lengths of RAGGED: empty, one row, on and next to a 16-row step edge, and
    longer than the 256-row mask (the identity mapping in both halves) beside masked passages.  Returns (index with those
    lengths, the index the queries are drawn from)."""
    idx = synthetic.make_index(seed=61, n_docs=3000, K=64, doclen_mean=12, doclen_std=14, doclen_max=400)
    dl = idx["doclens"].copy()
    rng = np.random.default_rng(62)
    for j, pid in enumerate(rng.choice(3000, size=25 * len(RAGGED), replace=False)):
        dl[pid] = RAGGED[j % len(RAGGED)]
    return _with_doclens(idx, dl), idx


def _k_for(oracle, idx, Qs, nprobe, want):
    fewest = min(oracle.search(idx, Qs[:, :, j], nprobe=nprobe, k=1)[2] for j in range(Qs.shape[2]))
    assert fewest > 20, fewest
    return min(want, fewest)


@pytest.mark.parametrize("T", [1, 15, 16, 17, 31, 32])
def test_query_lengths_over_ragged_passages(oracle, T):
    """T <= 16: no hi half, the lo walk stores the score; T = 17: a one-token hi half; T = 32: a full one.  The listed passages
    are ragged, so half-passages end on and next to step edges and share steps within a half; both modes, single and batch."""
    idx2, idx = _ragged_index()
    Qs = synthetic.make_queries(idx, 63 + T, 3, T=T)
    check_search(oracle, idx2, Qs, k=_k_for(oracle, idx2, Qs, 4, 400), nprobe=4)


def test_chunk_ends_and_parked_sums_reused(oracle):
    """A sub-batch of 64 queries runs 768 / 64 = 12 work-groups of 4 waves per query, and a wave holds the headers of a chunk of
    its passages in registers (32 passages; 64 before the masks were split).  With k = 3 200 every query lists at least 3 200 >
    64 x 48 passages, so every wave walks more than two chunks: the lo -> hi switch, the end of a chunk and the reuse of the
    parked sums' lanes all happen inside a wave's run."""
    B, k = 64, 3200
    idx = synthetic.make_index(seed=71, n_docs=6000, K=32, doclen_mean=10, doclen_std=6, doclen_max=40)
    Qs = synthetic.make_queries(idx, 72, B)
    fewest = min(oracle.search(idx, Qs[:, :, j], nprobe=4, k=1)[2] for j in range(B))
    assert fewest > k > 64 * 4 * (768 // B), fewest
    check_search(oracle, idx, Qs, k=k, nprobe=4, modes=(1,))
    s = clb.Searcher(index=idx)
    try:
        s.set_mode(1)
        s.profile_enable(True, counters=True)
        s.search_batch(Qs, k, nprobe=4)
        assert s.last_batch_stats()["rescored_docs"] >= B * k       # (a list holds at least k passages)
    finally:
        s.close()


def test_one_half_selects_one_row_the_other_many(oracle):
    """Tokens 0..15 all copies of one passage row and tokens 16..31 of another: each half's windows select the few rows near
    that one maximum.  And the mixed forms: one half copies of a row, the other ordinary tokens (many rows), both ways round."""
    idx2, idx = _ragged_index()
    Qs = synthetic.make_queries(idx, 81, 3)
    rows = synthetic.decompress_numpy(idx, np.array([5, 4321 % idx["codes"].shape[0], 77])).astype(np.float32)
    Qs = np.array(Qs, order="F")
    Qs[:, :16, 0] = rows[:, 0:1]
    Qs[:, 16:, 0] = rows[:, 1:2]
    Qs[:, :16, 1] = rows[:, 2:3]
    Qs[:, 16:, 2] = rows[:, 0:1]
    Qs = np.asfortranarray(Qs)
    check_search(oracle, idx2, Qs, k=_k_for(oracle, idx2, Qs, 4, 400), nprobe=4)


@pytest.mark.parametrize("B", [1, 33])
def test_batch_sizes(oracle, B):
    idx2, idx = _ragged_index()
    Qs = synthetic.make_queries(idx, 90 + B, B)
    check_search(oracle, idx2, Qs, k=_k_for(oracle, idx2, Qs, 2, 300), modes=(1,))


def test_half_row_counters():
    """rows_lo / rows_hi: the rows multiplied against tokens 0..15 / 16..31; rescored_embs stays the rows in their union."""
    idx2, idx = _ragged_index()
    s = clb.Searcher(index=idx2)
    try:
        s.set_mode(1)
        s.profile_enable(True, counters=True)
        for T in (32, 17, 16, 1):
            Qs = synthetic.make_queries(idx, 100 + T, 5, T=T)
            s.search_batch(Qs, 200, nprobe=4)
            st, hr = s.last_batch_stats(), s.last_batch_half_rows()
            lo, hi, union = hr["rows_lo"], hr["rows_hi"], st["rescored_embs"]
            assert st["rescored_docs"] > 0 and lo > 0, (T, st, hr)
            assert max(lo, hi) <= union <= lo + hi, (T, st, hr)
            assert (hi == 0) == (T <= 16), (T, st, hr)
    finally:
        s.close()
