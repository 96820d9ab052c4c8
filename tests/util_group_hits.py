"""The reference of the hits of a grouped search (`per_group=`): from the full stable ranking of a query's (filtered)
candidates -- tests/util_filter.filtered_ranking -- keep the first k distinct groups in order of first occurrence and, of
each, its first m occurrences.  Column j of the result is group j: row 0 its representative (what the grouped search
returns, tests/util_group.collapse), rows 1 .. m - 1 its next candidates in ranking order, pid 0 / -Inf where the group
has fewer.  No tests here."""
import numpy as np

from tests.util_filter import filtered_ranking


def hits_reference(ranking, group_ids, k, m, pid_offset=0):
    """-> (pids (m, k) int64, scores (m, k) float32, n_cand): n_cand = the number of groups among the candidates.
    ranking: (pids, scores) of every candidate, best first, 1-based local pids; group_ids[p - 1] = the group of passage p."""
    rp, rs = ranking
    rp = np.asarray(rp, dtype=np.int64); rs = np.asarray(rs, dtype=np.float32)
    pids = np.zeros((m, k), np.int64); scores = np.full((m, k), -np.inf, np.float32)
    if rp.size == 0:
        return pids, scores, 0
    g = np.asarray(group_ids)[rp - 1]
    by_group = np.argsort(g, kind="stable")                    # ranking positions, group by group, ranking order inside
    sg = g[by_group]
    head = np.concatenate([[True], sg[1:] != sg[:-1]])
    start = np.nonzero(head)[0]                                # where every group begins in by_group
    run = np.cumsum(head) - 1                                  # the group (in sorted order) of every entry
    nth = np.arange(rp.size) - start[run]                      # 0 for a group's best candidate, 1 for its second ...
    first_at = by_group[start]                                 # ranking position of every group's first occurrence
    place = np.empty(start.size, np.int64)
    place[np.argsort(first_at, kind="stable")] = np.arange(start.size)     # the group's rank among the groups
    col = place[run]
    keep = (nth < m) & (col < k)
    pids[nth[keep], col[keep]] = rp[by_group[keep]] + pid_offset
    scores[nth[keep], col[keep]] = rs[by_group[keep]]
    return pids, scores, int(start.size)


def hits_of(oracle, idx, Q, nprobe, group_ids, k, m, allowed=None, scope="candidates", pid_offset=0):
    return hits_reference(filtered_ranking(oracle, idx, Q, nprobe, allowed, scope), group_ids, k, m, pid_offset)


def assert_hits(got_p, got_s, got_n, ranking, group_ids, k, m, what, pid_offset=0):
    """One query's (pids (m, k), scores (m, k), n_cand) against hits_reference, bit for bit, padding included."""
    rp, rs, rn = hits_reference(ranking, group_ids, k, m, pid_offset)
    got_p = np.asarray(got_p); got_s = np.asarray(got_s, dtype=np.float32)
    assert got_p.shape == (m, k) and got_s.shape == (m, k), (what, got_p.shape, got_s.shape)
    assert int(got_n) == rn, (what, int(got_n), rn)
    if not np.array_equal(got_p, rp):
        bad = np.argwhere(got_p != rp)
        raise AssertionError(f"{what}: {bad.shape[0]} of {rp.size} pids differ, first at (hit, group) {tuple(bad[0])}: "
                             f"got {got_p[tuple(bad[0])]}, want {rp[tuple(bad[0])]}")
    gb = np.ascontiguousarray(got_s).view(np.uint32); rb = np.ascontiguousarray(rs).view(np.uint32)
    assert np.array_equal(gb, rb), f"{what}: {np.count_nonzero(gb != rb)} of {rb.size} score words differ"
