"""The reference of a search with a score prior: the composed filtered reference of tests/util_filter.py, every candidate's
oracle score e boosted to E = fl32(e + fl32(weight * value)) with two separately rounded fp32 operations, and the candidates
ranked again -- E descending, the lower pid first among equal E.  The reference project has no prior; this re-ranking of
its full candidate ranking IS the specification.  No tests here."""
import numpy as np

from tests.util_filter import filtered_ranking, first_k
from tests.util_group import collapse


def boost(scores, values, weight):
    """E of candidates with fp32 scores `scores` and prior values `values` (same length): one rounded multiply, one rounded
    add (numpy rounds every fp32 operation on its own: nothing is contracted into an fma)."""
    e = np.asarray(scores, dtype=np.float32)
    pi = np.float32(weight) * np.asarray(values, dtype=np.float32)
    assert pi.dtype == np.float32 and np.all(np.isfinite(pi))
    E = e + pi
    assert E.dtype == np.float32
    return E


def boosted_ranking(ranking, values, weight=1.0):
    """`ranking` = (pids, scores) of every candidate (1-based local pids, any order) -> the same candidates ranked by E;
    values[p - 1] is the prior of passage p."""
    rp, rs = ranking
    rp = np.asarray(rp, dtype=np.int64)
    by_pid = np.argsort(rp, kind="stable")
    p = rp[by_pid]
    E = boost(np.asarray(rs)[by_pid], np.asarray(values)[p - 1], weight)
    order = np.argsort(-E, kind="stable")
    return p[order], E[order]


def prior_ranking(oracle, idx, Q, nprobe, values, weight=1.0, allowed=None, scope="candidates", group_ids=None):
    """the full ranking of a search with a prior; with `group_ids` its collapse (tests/util_group.collapse)"""
    r = boosted_ranking(filtered_ranking(oracle, idx, Q, nprobe, allowed, scope), values, weight)
    return r if group_ids is None else collapse(r, group_ids)


def prior_reference(oracle, idx, Q, nprobe, k, values, weight=1.0, allowed=None, scope="candidates", group_ids=None, pid_offset=0):
    """(pids[k], scores[k], n_cand) of a search with a prior, padded with pid 0 / -Inf"""
    return first_k(prior_ranking(oracle, idx, Q, nprobe, values, weight, allowed, scope, group_ids), k, pid_offset)
