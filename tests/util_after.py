"""The reference of a search after a cursor: the oracle's full ranking of a query's candidates (tests/util_filter.
filtered_ranking: score descending, the lower pid first among equal scores) cut on the host behind the cursor (s*, p*) --
    after(p)  <=>  e(p) < s*  or  (e(p) == s* and pid(p) > p*)
with GLOBAL 1-based pids.  The reference project has no cursor; this cut of its full ranking IS the specification.  No tests
here."""
import numpy as np


def after_ranking(ranking, score, pid, pid_offset=0):
    """the members of `ranking` = (pids, scores) (1-based local pids, ranked) after the cursor (score, pid), in order; +Inf:
    all of them, -Inf or NaN: none"""
    rp, rs = np.asarray(ranking[0], dtype=np.int64), np.asarray(ranking[1], dtype=np.float32)
    s = np.float32(score)
    if np.isposinf(s):
        keep = np.ones(rp.size, bool)
    elif np.isnan(s) or np.isneginf(s):
        keep = np.zeros(rp.size, bool)
    else:
        keep = (rs < s) | ((rs == s) & (rp + pid_offset > int(pid)))
    return rp[keep], rs[keep]


def assert_page(got_p, got_s, got_n, ranking, cursor, k, what, pid_offset=0):
    """one query's page against the reference: pids equal, fp32 bits equal, pid 0 / -Inf past the last member, and the
    candidate count that of the FULL ranking"""
    ap, as_ = after_ranking(ranking, cursor[0], cursor[1], pid_offset)
    n = min(k, ap.size)
    got_p, got_s = np.asarray(got_p), np.ascontiguousarray(got_s, dtype=np.float32)
    assert got_p.shape == (k,) and got_s.shape == (k,), (what, got_p.shape, got_s.shape)
    assert np.array_equal(got_p[:n], ap[:n] + pid_offset), (what, cursor, got_p[:8], ap[:8] + pid_offset)
    assert np.array_equal(got_s[:n].view(np.uint32), np.ascontiguousarray(as_[:n]).view(np.uint32)), (what, cursor)
    assert np.all(got_p[n:] == 0) and np.all(np.isneginf(got_s[n:])), (what, cursor, n, got_p[n:][:8], got_s[n:][:8])
    assert int(got_n) == len(ranking[0]), (what, int(got_n), len(ranking[0]))
    return n
