"""The grouped-search reference: the composed filtered reference of tests/util_filter.py with every group kept once.
The reference project has no grouped search; its full stable ranking of a query's candidates, cut to the first occurrence
of every group, IS the specification (best passage per group, ties to the lower pid; groups by score descending, ties to
the lower representative pid).  No tests here."""
import numpy as np

from tests.util_filter import filtered_ranking, first_k


def collapse(ranking, group_ids):
    """Keep the first occurrence of every group in a `(pids, scores)` ranking.  pids are 1-based local passage ids;
    group_ids[p - 1] is the group of passage p."""
    rp, rs = ranking
    rp = np.asarray(rp, dtype=np.int64)
    if rp.size == 0:
        return rp, np.asarray(rs, dtype=np.float32)
    g = np.asarray(group_ids)[rp - 1]
    _, first = np.unique(g, return_index=True)
    keep = np.sort(first)
    return rp[keep], np.asarray(rs)[keep]


def grouped_ranking(oracle, idx, Q, nprobe, group_ids, allowed=None, scope="candidates"):
    return collapse(filtered_ranking(oracle, idx, Q, nprobe, allowed, scope), group_ids)


def grouped_reference(oracle, idx, Q, nprobe, k, group_ids, allowed=None, scope="candidates", pid_offset=0):
    """(pids[k], scores[k], n_cand) of a grouped search: n_cand = the number of groups among the candidates."""
    return first_k(grouped_ranking(oracle, idx, Q, nprobe, group_ids, allowed, scope), k, pid_offset)


def ids_from_lens(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return np.repeat(np.arange(lens.size, dtype=np.int64), lens)


def random_lens(n_docs, lo, hi, seed):
    """group lengths drawn from lo..hi that sum to n_docs exactly"""
    rng = np.random.default_rng(seed)
    lens = []
    left = n_docs
    while left > 0:
        n = int(min(left, rng.integers(lo, hi + 1)))
        lens.append(n)
        left -= n
    return np.asarray(lens, dtype=np.int64)
