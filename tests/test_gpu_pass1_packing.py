"""Pass 1 pads a passage to a multiple of 8 rows and starts the wave's next passage in the free quads of a passage's
last 32-row step.  These tests walk ragged passage runs through those packed steps against the
oracle, and check directly that a passage's approximate score does not depend on where in a step it lands."""
import functools

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import synthetic
from test_gpu_parity import check_search

pytestmark = pytest.mark.gpu

# on and next to a quad edge (8) and a step edge (32), longer than the 256-row mask, and empty passages between them
RAGGED = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 255, 256, 257, 300, 0, 1, 0]


def _with_doclens(idx, dl):
    """`idx` with passage lengths `dl`: the embeddings are reused in order (repeated if more are needed) and the IVF rebuilt."""
    n_emb = int(dl.sum())
    reps = -(-n_emb // idx["codes"].shape[0])
    codes = np.concatenate([idx["codes"]] * reps)[:n_emb]
    res = np.asfortranarray(np.concatenate([idx["residuals"]] * reps, axis=1)[:, :n_emb])
    out = dict(idx, doclens=dl, codes=codes, residuals=res)
    out["ivf"], out["ivf_lengths"] = synthetic.build_ivf(codes, idx["centroids"].shape[1])
    return out


def test_pass1_packed_steps_ragged_runs(oracle):
    """Several passages end inside one step, a packed passage ends inside its head's step, boundaries fall on and next to
    quad and step edges, and wave ranges end mid-step (in the batch calls, 2-8 passages per wave): every mode, gather form and
    row format against the oracle's pids and exact scores.  Pass 1's own scores and 64-passage chunk ends: the test below."""
    idx = synthetic.make_index(seed=41, n_docs=3000, K=64, doclen_mean=12, doclen_std=14, doclen_max=400)
    dl = idx["doclens"].copy()
    rng = np.random.default_rng(42)
    for j, pid in enumerate(rng.choice(3000, size=25 * len(RAGGED), replace=False)):
        dl[pid] = RAGGED[j % len(RAGGED)]
    idx2 = _with_doclens(idx, dl)
    Qs = synthetic.make_queries(idx, 43, 32)                 # (from the unchanged index: idx2 has empty passages)
    fewest = min(oracle.search(idx2, Qs[:, :, j], nprobe=2, k=1)[2] for j in range(Qs.shape[2]))
    assert fewest > 600, fewest
    check_search(oracle, idx2, Qs, k=min(1500, fewest))


def _layout(base, fill_lens, targets, rng):
    """The target passages of `base` (same rows), each behind a filler passage of the given length.  The fillers are copies
    of rows of `base` and every passage of `base` is a target, so the index-wide inv_norm quantisation range is the same in
    every layout."""
    K = base["centroids"].shape[1]
    starts = np.concatenate([[0], np.cumsum(base["doclens"])])
    dl, codes, res = [], [], []
    for t, fl in zip(targets, fill_lens):
        if fl:
            rows = rng.integers(0, starts[-1], fl)
            dl.append(fl)
            codes.append(base["codes"][rows])
            res.append(base["residuals"][:, rows])
        dl.append(base["doclens"][t])
        codes.append(base["codes"][starts[t]:starts[t + 1]])
        res.append(base["residuals"][:, starts[t]:starts[t + 1]])
    codes = np.concatenate(codes)
    out = dict(base, doclens=np.array(dl, dtype=base["doclens"].dtype), codes=codes,
               residuals=np.asfortranarray(np.concatenate(res, axis=1)))
    out["ivf"], out["ivf_lengths"] = synthetic.build_ivf(codes, K)
    is_target = np.ones(len(dl), bool)
    pos = 0
    for fl in fill_lens:
        if fl:
            is_target[pos] = False
            pos += 1
        pos += 1
    return out, np.nonzero(is_target)[0]


# waves per query of the pass-1 launch behind debug_scores (grid 8 x 32 work-groups of 12 waves): one query is split over all
# eight groups (3 072 waves); with 8-bit score rows it runs as 16 copies, 32 work-groups each (384 waves)
DEBUG_WAVES = {0: 8 * 32 * 12, 1: 32 * 12}


@functools.lru_cache(maxsize=None)
def _invariance_layouts():
    """~29 600 passages (every one a candidate when all 32 centroids are probed): each wave walks ~10 passages per query in
    the fp16 form and ~78 -- more than one 64-passage chunk -- with 8-bit rows; below the 32 768 candidates of one selection
    work-group."""
    K = 32
    base = synthetic.make_index(seed=51, n_docs=15000, K=K, doclen_mean=16, doclen_std=12, doclen_max=60)
    Q = synthetic.make_queries(base, 52, 1)[:, :, 0]
    targets = np.arange(base["doclens"].size)
    rng = np.random.default_rng(53)
    layouts = []
    for shift in (0, 1, 5, 8, 13, 24, 31, 33):
        fill = [(shift + 7 * i) % 40 for i in range(len(targets))]
        layouts.append((shift,) + _layout(base, fill, targets, rng))
    return K, Q, layouts


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("gather", [0, 1])
def test_pass1_score_independent_of_step_position(rows, gather):
    """The same passages behind fillers of every length mod 8 and mod 32: their approximate scores (pass 1's own output, not
    absorbed by the exact re-score) are bit-identical in every layout.  Every wave walks several passages, so passages land
    in every quad of a step, as the head and as the tail of packed steps, and (8-bit rows) across 64-passage chunk ends."""
    K, Q, layouts = _invariance_layouts()
    ref = None
    for shift, idx, tpos in layouts:
        s = clb.Searcher(index=idx)
        s.set_mode(1)
        s.set_pass1_gather(gather)
        s.set_score_rows(rows)
        d = s.debug_scores(Q, k=10, nprobe=K)
        s.close()
        n = d["pids"].size
        assert n == idx["doclens"].size - np.count_nonzero(idx["doclens"] == 0), (shift, n)   # every passage a candidate
        assert n / DEBUG_WAVES[rows] >= (8 if rows == 0 else 65), (shift, n)                  # several passages per wave
        by_pid = dict(zip(d["pids"].tolist(), d["approx"].astype(np.float32).view(np.uint32).tolist()))
        got = [by_pid.get(int(p) + 1) for p in tpos]      # (pids are 1-based)
        assert None not in got, (shift, "a target is not a candidate")
        if ref is None:
            ref = got
        else:
            assert got == ref, (shift, sum(a != b for a, b in zip(got, ref)))
