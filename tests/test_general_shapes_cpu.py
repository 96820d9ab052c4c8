"""The oracle on the general shapes (every dim % 8 == 0, nbits 1/2/4/8, any query length) against the float64 restatement
of the exact score (tests/util_general.scores_float64), inside a bound derived from the fp32 arithmetic
(util_general.score_bound).  tests/test_gpu_general_shapes.py holds the device to the oracle bit for bit at the same shapes;
this file is what says the oracle itself is right there.  No kernel code runs here."""
import numpy as np
import pytest

from tests import util_general as ug


def test_expected_route_follows_the_case_table():
    for dim, nbits, T, _, route, _ in ug.CASES:
        assert ug.expected_route(dim, nbits, T) == route, (dim, nbits, T)
    assert {c[4] for c in ug.CASES} == set(ug.ROUTES)
    # the staged query passes 64 KB exactly where the table says it first does
    assert ug.lds_bytes(256, 4, 63) <= 64 * 1024 < ug.lds_bytes(256, 4, 64) < ug.lds_bytes(256, 8, 128)
    assert all(ug.lds_bytes(c[0], c[1], c[2]) <= 64 * 1024 for c in ug.CASES if c[4].startswith("batched") and c[0] < 256)
    for tuned in ((128, 2, 32), (128, 4, 128), (128, 1, 1)):
        with pytest.raises(ValueError):
            ug.expected_route(*tuned)
    assert ug.expected_route(128, 8, 32) == "batched32" and ug.expected_route(128, 2, 129) == "loop_mfma"


def test_default_fuzz_seeds_reach_every_route():
    """the 10 default seeds of test_general_search_random_configurations (tests/test_gpu_general_shapes.py)"""
    cfgs = [ug.fuzz_configuration(seed) for seed in range(10)]
    assert [ug.expected_route(c["dim"], c["nbits"], c["T"]) for c in cfgs] == ug.FUZZ_ROUTES
    assert set(ug.FUZZ_ROUTES) == set(ug.ROUTES)
    for c in cfgs:
        assert c["dim"] in ug.FUZZ_DIMS and c["T"] in ug.FUZZ_T and 1 <= c["nprobe"] <= min(c["K"], 8) and 1 <= c["k"] <= c["n_docs"]


def oracle_against_float64(oracle, idx, Q, nprobe, k):
    """-> (oracle pids, oracle scores, float64 scores of the same pids in the oracle's order, bound)"""
    pids, scores, n = oracle.search(idx, Q, nprobe=nprobe, k=k)
    assert n >= k
    return pids, scores.astype(np.float64), ug.scores_float64(idx, Q, pids), ug.score_bound(idx["dim"], Q.shape[1], Q)


@pytest.mark.parametrize("case", range(len(ug.CASES)), ids=ug.CASE_IDS)
def test_oracle_scores_and_order_within_the_float64_bound(oracle, case):
    """Scores within the bound; order as in float64 wherever two neighbours are further apart than twice the bound, and at most
    a tenth of the neighbouring pairs may be left out on that ground.  Neighbours whose float64 scores are EQUAL are not left
    out but held to the stable sort's rule: equal oracle scores, ascending pid.  (dim 8 / nbits 1 / K 1 has 256 distinct rows
    in the whole index and one token: the best row sits in some 50 passages, all of the first 30 scores are one number.)"""
    idx, Qs, nprobe = ug.case_inputs(case)
    Q = np.ascontiguousarray(Qs[:, :, 0])
    pids, got, want, bound = oracle_against_float64(oracle, idx, Q, nprobe, ug.CASE_K)
    err = np.abs(got - want).max()
    gaps = want[:-1] - want[1:]                       # neighbouring float64 scores in the oracle's order
    decided = np.abs(gaps) > 2 * bound
    tied = gaps == 0
    left_out = ~decided & ~tied
    print(f"{ug.CASE_IDS[case]}: max |oracle - float64| = {err:.3e} = {err / bound:.4f} of the bound {bound:.3e}; of {gaps.size} "
          f"neighbouring pairs {np.count_nonzero(tied)} tied, {np.count_nonzero(left_out)} closer than twice the bound")
    assert err <= bound, (err, bound)
    assert np.all(gaps[decided] > 0), np.nonzero(decided & (gaps <= 0))[0]
    assert np.all(got[:-1][tied] == got[1:][tied]) and np.all(pids[:-1][tied] < pids[1:][tied])
    assert np.count_nonzero(left_out) <= 0.10 * gaps.size


def fraction_outside(oracle, idx, wrong, Q, nprobe):
    """the share of the oracle's scores (on `idx`) that leave the bound when the float64 side reads `wrong` instead"""
    pids, scores, _ = oracle.search(idx, Q, nprobe=nprobe, k=ug.CASE_K)
    bound = ug.score_bound(idx["dim"], Q.shape[1], Q)
    assert np.abs(scores - ug.scores_float64(idx, Q, pids)).max() <= bound
    return float(np.mean(np.abs(scores - ug.scores_float64(wrong, Q, pids)) > bound))


@pytest.mark.parametrize("case", [ug.CASES.index(c) for c in ug.CASES if c[:2] in ((768, 1), (8, 1), (120, 4), (256, 4))],
                         ids=lambda i: ug.CASE_IDS[i])
def test_float64_check_sees_msb_first_bit_fields(oracle, case):
    """residual bit fields read MSB-first instead of LSB-first, at nbits 1 and at nbits 4"""
    idx, Qs, nprobe = ug.case_inputs(case)
    wrong = dict(idx, residuals=ug.msb_first_fields(idx["residuals"], idx["nbits"]))
    assert not np.array_equal(wrong["residuals"], idx["residuals"])
    assert np.array_equal(ug.msb_first_fields(wrong["residuals"], idx["nbits"]), idx["residuals"])
    assert fraction_outside(oracle, idx, wrong, np.ascontiguousarray(Qs[:, :, 0]), nprobe) > 0.5


@pytest.mark.parametrize("case", [ug.CASES.index(c) for c in ug.CASES if c[:3] in ((136, 2, 17), (8, 8, 600), (768, 1, 40))],
                         ids=lambda i: ug.CASE_IDS[i])
def test_float64_check_sees_doclens_shifted_by_one_passage(oracle, case):
    idx, Qs, nprobe = ug.case_inputs(case)
    wrong = dict(idx, doclens=np.roll(idx["doclens"], 1))
    assert fraction_outside(oracle, idx, wrong, np.ascontiguousarray(Qs[:, :, 0]), nprobe) > 0.5


def test_ragged_index_forces_the_lengths_and_keeps_the_index_consistent():
    idx = ug.case_inputs(4)[0]
    forced = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 0, 1, 16, 1]
    r = ug.ragged_index(idx, forced, seed=5, reps=10)
    changed = np.nonzero(r["doclens"] != idx["doclens"])[0]
    assert 140 <= changed.size <= 160 and set(r["doclens"][changed]) <= set(forced)
    for v in set(forced):
        assert np.count_nonzero(r["doclens"] == v) >= forced.count(v) * 10
    assert r["codes"].size == r["residuals"].shape[1] == int(r["doclens"].sum()) == r["ivf"].size == int(r["ivf_lengths"].sum())
    assert np.array_equal(np.sort(r["ivf"]), np.arange(1, r["codes"].size + 1))
    assert np.array_equal(idx["doclens"], ug.case_inputs(4)[0]["doclens"]) and idx["codes"].size == int(idx["doclens"].sum())
