"""The filtered-search reference: the oracle's own pipeline with the filter put where it belongs.  The oracle has no
filter argument; `retrieve` -> (restrict) -> gather -> decompress -> maxsim -> stable sort is composed here from its
pieces, and tests/test_filter_cpu.py pins the composition against `oracle.search` with no filter."""
import numpy as np


def filtered_ranking(oracle, idx, Q, nprobe, allowed=None, scope="candidates"):
    """Every candidate of query Q (dim, T) after the filter, fully ranked: (pids, scores), 1-based local pids.
    `allowed`: 1-based local pids (any order, duplicates fine) or None for no filter.  scope "candidates":
    retrieve(Q) restricted to `allowed`; "all": the candidates ARE sort(unique(allowed))."""
    dl = np.ascontiguousarray(idx["doclens"], dtype=np.int64)
    if scope == "all" and allowed is not None:
        c = np.unique(np.asarray(allowed, dtype=np.int64))
    else:
        c = oracle.retrieve(idx["ivf"], idx["ivf_lengths"], idx["centroids"], oracle.build_emb2pid(dl), nprobe, Q)
        if allowed is not None:
            c = c[np.isin(c, np.asarray(allowed, dtype=np.int64))]
    if c.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    co, re = oracle.collect_compressed_embs_for_pids(dl, idx["codes"], idx["residuals"], c)
    D = oracle.decompress(int(idx["dim"]), int(idx["nbits"]), idx["centroids"], idx["bucket_weights"], co, re)
    sc = oracle.maxsim(Q, D, c, dl)
    order = np.argsort(-sc, kind="stable")
    return c[order], sc[order]


def first_k(ranking, k, pid_offset=0):
    """What a filtered search returns for that ranking: (pids[k], scores[k], n_cand), padded with pid 0 / -Inf."""
    rp, rs = ranking
    n = min(k, rp.size)
    pids = np.zeros(k, np.int64); scores = np.full(k, -np.inf, np.float32)
    pids[:n] = rp[:n] + pid_offset
    scores[:n] = rs[:n]
    return pids, scores, int(rp.size)


def filtered_reference(oracle, idx, Q, nprobe, k, allowed=None, scope="candidates", pid_offset=0):
    return first_k(filtered_ranking(oracle, idx, Q, nprobe, allowed, scope), k, pid_offset)
