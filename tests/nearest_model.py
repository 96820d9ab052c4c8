"""A float64 model of the index build's nearest-centroid search (nearest_centroids<MODE> in csrc/codec.hip), in numpy alone.

What the build does, and what the model restates of it:

  groups   the list kernels score 32-centroid tiles on the MFMA; a lane keeps, per tile, the maximum over its 16 centroids.  That
           "group" is gid = 2 tile + h with the centroids 32 tile + (s & 3) + 8 (s >> 2) + 4 h, s < 16, c < K -- so h is bit 2 of
           c % 32, and each of a point's two lists (h = 0, 1) holds the kTopPartial = 4 best groups of its parity by approximate
           value, descending.
  scores   w(c) = x.c (MODE 0, compress_into_codes!) or x.c - ||c||^2 / 2 (MODE 1: the k-means distance is ||x||^2 - 2 w), and
           W(g) = max of w over the group.  The winner is the argmax of w, FIRST index on ties.
  margin   the exact pass re-scores every listed group with v >= g1 - margin, g1 = the best listed value, and hands a point on
           (second tier, then the exhaustive scan) when a full list's last entry still qualifies:
             margin = 2 * 1.25 * bound(xn, dq, cn, dc) + 4e-6 (1 + xn^2 + cn^2) + [dc > 0] 1.6e-5 cn^2
             bound  = max(7.4e-5 xn cn,  [dc > 0] (1.001 (1.0005 dq cn + xn dc) + 384 * 2^-24 xn cn))
           xn = 1.001 ||x||, dq = 1.001 ||x - fp16(x)||, cn = 1.001 max ||c||, dc = 1.0001 max ||c - fp16(c)|| (0 when the lists
           come from the three-product bf16 split, whose error is the first term alone).

The model takes nothing the kernels compute.  It cannot tell a list kernel that mixes up operands but stays inside margin / 2 from
a correct one; see DESIGN.md.  The generators below build the inputs tests/test_gpu_nearest_model.py runs on the device; the
properties each of them is built for are asserted without a device in tests/test_nearest_model_cpu.py.
"""
import numpy as np

DIM = 128
L = 4                      # kTopPartial
EMPTY = 0x7fffffff
U = 2.0 ** -24
EPS_SAFETY = 1.25          # kEpsSafety
B3 = 7.4e-5                # three bf16 products: |approx - canonical| / (xn cn)
TIER_LISTS, TIER_SECOND, TIER_EXHAUSTIVE = 0, 1, 2
SECOND_TIER_ABOVE = 64     # more undecided points than this in a chunk go through the second tier


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


# ---- groups ---------------------------------------------------------------------------------------------------------------------
def group_of(c):
    c = np.asarray(c)
    return 2 * (c // 32) + ((c % 32) >> 2 & 1)


def group_members(gid, K):
    tile, h = gid >> 1, gid & 1
    s = np.arange(16)
    c = 32 * tile + (s & 3) + 8 * (s >> 2) + 4 * h
    return c[c < K]


def n_groups(K):
    return 2 * ((K + 31) // 32)


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def scores(C, X, mode):
    """w (K, n) in float64.  Identical centroids get identical rows (a blocked matrix product need not give them that), so that
    the first-index rule applies to exact ties as it does on the device."""
    C = np.asarray(C, dtype=np.float64); X = np.asarray(X, dtype=np.float64)
    Cu, inv = np.unique(C, axis=1, return_inverse=True)
    with np.errstate(over="ignore", invalid="ignore"):
        W = Cu.T @ X
        if mode == 1:
            W = W - 0.5 * np.sum(Cu * Cu, axis=0)[:, None]
    return W[np.ravel(inv)]


def group_maxima(W, K):
    """W(g) (n_groups, n); a group without a centroid below K is -inf (the kernels never list it)"""
    G = np.full((n_groups(K), W.shape[1]), -np.inf)
    g = group_of(np.arange(K))
    np.maximum.at(G, g, W)
    return G


def winners(W):
    """0-based argmax, first index on ties"""
    return np.argmax(W, axis=0)


# ---- the margin -----------------------------------------------------------------------------------------------------------------
def cn_of(C):
    return 1.001 * float(np.linalg.norm(np.asarray(C, dtype=np.float64), axis=0).max())


def dc_of(C):
    """what max_row_f16_err_kernel reports: inf with a component beyond the fp16 range, never exactly 0"""
    C = np.asarray(C, dtype=np.float64)
    if np.abs(C).max() >= 6.0e4:
        return np.inf
    return max(1e-30, 1.0001 * float(np.linalg.norm(C - f16(C), axis=0).max()))


def product_bound(xn, dq, cn, dc):
    b3 = B3 * xn * cn
    if dc > 0:
        with np.errstate(invalid="ignore"):
            return np.maximum(b3, 1.001 * (dq * cn * 1.0005 + xn * dc) + 384.0 * U * xn * cn)
    return b3


def margin_of(xn, dq, cn, dc):
    return 2.0 * EPS_SAFETY * product_bound(xn, dq, cn, dc) + 4e-6 * (1.0 + xn * xn + cn * cn) + (1.6e-5 * cn * cn if dc > 0 else 0.0)


def point_norms(X):
    """xn, dq as the refine kernel measures them, and the largest dq the fp16 format allows for the same point"""
    X = np.asarray(X, dtype=np.float64)
    xn = 1.001 * np.linalg.norm(X, axis=0)
    with np.errstate(invalid="ignore"):
        d = np.where(np.abs(X) < 6.0e4, X - f16(X), np.inf)
    dq = 1.001 * np.sqrt(np.sum(d * d, axis=0))
    # a normal fp16 is within 2^-11 of the value, relatively; a subnormal within 2^-25, absolutely
    dq_worst = 1.001 * np.sqrt(np.sum(np.maximum(2.0 ** -11 * np.abs(X), 2.0 ** -25) ** 2, axis=0))
    dq_worst = np.where(np.isfinite(dq), dq_worst, np.inf)
    return xn, dq, dq_worst


def margins(X, cn, dc):
    """(the margin the kernel should have computed, its upper bound at the worst conversion error of the point)"""
    xn, dq, dq_worst = point_norms(X)
    return margin_of(xn, dq, cn, dc), margin_of(xn, dq_worst, cn, dc)


# ---- which points MUST and which CANNOT overflow their lists ------------------------------------------------------------------------
# A list overflows when it is full and its last value is >= g1 - margin.  With |listed value - W(g)| <= e(g) a point MUST overflow
# if some half has four groups with W - e >= max (W + e) - margin, and CANNOT if in both halves the fourth largest W + e is below
# max (W - e) - margin; a crafted tier input leaves no point between the two.  e(g), per point:
#   three products   7.4e-5 xn cn, the project's bound without its safety factor;
#   one product      the inequality the margin is built on, per centroid instead of with the maxima over all of them:
#                    1.001 (1.0005 dq ||c|| + xn ||c - fp16 c||) + 384 * 2^-24 xn ||c||, the largest over the group's centroids;
#   both             plus half of what the margin adds to 2 * 1.25 * bound (the exact pass's own rounding, the bias riding through
#                    the adds), counted here as list error in full.
def slack_of(xn, cn, dc):
    return 4e-6 * (1.0 + xn * xn + cn * cn) + (1.6e-5 * cn * cn if dc > 0 else 0.0)


def group_errors(C, X, cn, dc):
    """e (n_groups, n) of the lists the build would use for these centroids (dc > 0: one product)"""
    C = np.asarray(C, dtype=np.float64)
    K = C.shape[1]
    xn, dq, _ = point_norms(X)
    if dc > 0:
        cnorm = 1.001 * np.linalg.norm(C, axis=0)
        dcc = 1.0001 * np.linalg.norm(C - f16(C), axis=0)
        per_c = 1.001 * (1.0005 * dq[None, :] * cnorm[:, None] + xn[None, :] * dcc[:, None]) + 384.0 * U * xn[None, :] * cnorm[:, None]
        E = np.zeros((n_groups(K), X.shape[1]))
        np.maximum.at(E, group_of(np.arange(K)), per_c)
    else:
        E = np.broadcast_to(B3 * xn * cn, (n_groups(K), X.shape[1])).copy()
    return E + 0.5 * slack_of(xn, cn, dc)[None, :]


def _fourth(A):
    """the fourth largest per column, per half: (2, n); -inf where a half has fewer than four groups"""
    out = np.full((2, A.shape[1]), -np.inf)
    for h in (0, 1):
        Ah = A[h::2]
        if Ah.shape[0] >= L:
            out[h] = np.sort(Ah, axis=0)[-L]
    return out


def must_overflow(G, E, margin):
    return (_fourth(G - E) >= (G + E).max(axis=0) - margin).any(axis=0)


def cannot_overflow(G, E, margin):
    return (_fourth(G + E) < (G - E).max(axis=0) - margin).all(axis=0)


def predict_tiers(C, X, mode):
    """Per point TIER_LISTS / TIER_SECOND / TIER_EXHAUSTIVE for centroids the build scores with one product, given that the second
    tier runs, and -1 where the bounds cannot tell (a crafted input has none)."""
    cn, dc = cn_of(C), dc_of(C)
    G = group_maxima(scores(C, X, mode), np.asarray(C).shape[1])
    m1, _ = margins(X, cn, dc)
    m3, _ = margins(X, cn, 0.0)
    E1, E3 = group_errors(C, X, cn, dc), group_errors(C, X, cn, 0.0)
    tier = np.full(X.shape[1], -1)
    tier[cannot_overflow(G, E1, m1)] = TIER_LISTS
    over = must_overflow(G, E1, m1)
    tier[over & cannot_overflow(G, E3, m3)] = TIER_SECOND
    tier[over & must_overflow(G, E3, m3)] = TIER_EXHAUSTIVE
    return tier


# ---- checks shared by the device tests --------------------------------------------------------------------------------------------
def check_lists(vals, gids, margin, G):
    """(a): every listed value within margin / 2 of W(gid); each half descending, of its own parity, without repeats; no unlisted
    group of the half above the smallest listed value + margin / 2 (a list with an empty slot lists every group of its half).
    Points without a finite margin are skipped.  Returns the worst |v - W| / (margin / 2)."""
    n, ng = vals.shape[0], G.shape[0]
    ok = np.isfinite(margin.astype(np.float64))
    half_m = 0.5 * margin.astype(np.float64)
    rows = np.arange(n)[:, None]
    worst = 0.0
    for h in (0, 1):
        v, g = vals[:, h].astype(np.float64), gids[:, h].astype(np.int64)
        live = g != EMPTY
        k = live.sum(axis=1)
        assert np.all((live == (np.arange(L)[None, :] < k[:, None]))[ok]), h                  # filled from the front
        gl = np.where(live, g, h)                                                               # (an index that is valid)
        assert np.all(((gl % 2 == h) & (gl < ng))[ok]), h
        for i in range(L):
            for j in range(i + 1, L):
                assert not np.any(ok & live[:, i] & live[:, j] & (g[:, i] == g[:, j])), (h, i, j)   # no group twice
        both = live[:, :-1] & live[:, 1:] & ok[:, None]
        assert np.all(v[:, :-1][both] >= v[:, 1:][both]), h                                   # entry 0 the largest, the last the smallest
        err = np.where(live & ok[:, None], np.abs(v - G[gl, rows]), 0.0)
        bad = err > half_m[:, None]
        assert not bad.any(), (h, np.argwhere(bad)[:5], err[bad][:5], half_m[np.argwhere(bad)[:5, 0]])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(ok & (k > 0), err.max(axis=1) / half_m, 0.0)
        worst = max(worst, float(np.nanmax(ratio)) if n else 0.0)
        Gh = np.where(np.isfinite(G[h::2]), G[h::2], -np.inf).copy()                          # (ng / 2, n): the half's groups
        pp, ee = np.nonzero(live)
        Gh[g[pp, ee] // 2, pp] = -np.inf
        rest = Gh.max(axis=0)
        last = v[np.arange(n), np.maximum(k - 1, 0)]
        short = ok & (k < L)
        assert np.all(rest[short] == -np.inf), (h, np.flatnonzero(short & (rest > -np.inf))[:5])   # an open slot: nothing unlisted
        full = ok & (k == L)
        assert np.all(rest[full] <= last[full] + half_m[full]), (h, np.flatnonzero(full & (rest > last + half_m))[:5])
    return worst


def ideal_lists(G):
    """the lists an error-free list kernel would write: per half the L best groups by W, descending, empty slots behind"""
    n = G.shape[1]
    vals = np.full((n, 2, L), -np.inf, dtype=np.float32); gids = np.full((n, 2, L), EMPTY, dtype=np.int32)
    for h in (0, 1):
        Gh = G[h::2]
        order = np.argsort(-Gh, axis=0, kind="stable")[:L]
        for e in range(min(L, Gh.shape[0])):
            v = Gh[order[e], np.arange(n)]
            live = np.isfinite(v)
            vals[live, h, e] = v[live]; gids[live, h, e] = 2 * order[e][live] + h
    return vals, gids


def check_decisions(vals, gids, margin, tier, tied):
    """(c): a point its first lists decided has the group of every centroid in tied[p] listed with v >= g1 - margin"""
    for p in np.flatnonzero(tier == TIER_LISTS):
        g1 = max(vals[p, 0, 0], vals[p, 1, 0])
        for c in tied[p]:
            g = int(group_of(c))
            at = np.flatnonzero(gids[p, g & 1] == g)
            assert at.size == 1 and vals[p, g & 1, at[0]] >= g1 - margin[p], (p, c, g, gids[p], vals[p], margin[p])


def canonical_ties(orc, C, X, mode, W=None):
    """Per point the centroids whose CANONICAL fp32 score (the oracle's fmaf chain; MODE 1: fl(fl(-2 a + ||c||^2) + ||x||^2))
    equals the best one, ascending.  Only centroids within 4e-5 (||x||^2 + max ||c||^2) of the float64 best can tie -- the chain is
    within 128 * 2^-24 ||x|| ||c|| of the real product -- so only those are sent through the oracle."""
    C = np.asfortranarray(C, dtype=np.float32); X = np.asfortranarray(X, dtype=np.float32)
    W = scores(C, X, mode) if W is None else W
    cn2 = float(np.sum(C.astype(np.float64) ** 2, axis=0).max())
    out = []
    c2 = {}
    for p in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, p])
        win = 4e-5 * (float(np.sum(x.astype(np.float64) ** 2)) + cn2)
        cand = np.flatnonzero(W[:, p] >= W[:, p].max() - win)
        a = np.array([orc.dot(np.ascontiguousarray(C[:, c]), x) for c in cand], dtype=np.float32)
        if mode == 1:
            for c in cand:
                if c not in c2:
                    c2[c] = orc.sumsq(np.ascontiguousarray(C[:, c]))
            v = np.float32(-2.0) * a
            v = v + np.array([c2[c] for c in cand], dtype=np.float32)
            v = v + orc.sumsq(x)
            out.append(cand[v == v.min()])
        else:
            out.append(cand[a == a.max()])
    return out


def oracle_winners(orc, C, X, mode):
    """0-based winners by the CPU oracle: compress_into_codes! (MODE 0), the assignments of one k-means iteration from C (MODE 1)"""
    if mode == 0:
        return orc.compress_into_codes(C, X).astype(np.int64) - 1
    return orc.kmeans(X, C, max_iters=1)[1].astype(np.int64) - 1


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def unit(rng, n):
    a = rng.normal(size=(DIM, n))
    return np.asfortranarray((a / np.linalg.norm(a, axis=0)).astype(np.float32))


def near_ties(scale, K=512, n=1500, seed=211):
    """the construction of test_nearest_centroid_near_ties_below_the_fp16_product_error: points between two centroids with gaps
    1e-7 .. 1e-4, close centroid pairs, centroids x scale; scale 1e3 adds a centroid component beyond the fp16 range (three
    products whatever was asked for) and points beyond it"""
    rng = np.random.default_rng(seed)
    cent = unit(rng, K)
    cent[:, 100:140] = cent[:, 60:100] + np.float32(3e-4) * rng.normal(size=(DIM, 40)).astype(np.float32)
    a, b = rng.integers(0, K, n), rng.integers(0, K, n)
    gap = (10.0 ** rng.uniform(-7, -4, n)).astype(np.float32)
    pts = cent[:, a] * (1 + gap) + cent[:, b] + np.float32(1e-3) * rng.normal(size=(DIM, n)).astype(np.float32)
    pts = (pts / np.linalg.norm(pts.astype(np.float64), axis=0)).astype(np.float32)
    cent = cent * np.float32(scale)
    if scale == 1.0e3:
        cent[3, 11] = np.float32(7.0e4)
        pts[:, :50] *= np.float32(7.0e4)
    return np.asfortranarray(cent), np.asfortranarray(pts)


def _fillers(rng, K, norm):
    """fp16-exact random centroids of about `norm`: they add nothing to dc"""
    return np.asfortranarray(f16(unit(rng, K).astype(np.float64) * norm).astype(np.float32))


def _two_groups(rng, K):
    while True:
        a, b = (int(v) for v in rng.integers(0, K, 2))
        if group_of(a) != group_of(b):
            return a, b


def coherent_points(scale=1.0, K=512, pairs=8, per_pair=16, seed=5):
    """(b), the dq cn term.  Every centroid is fp16-exact (dc = its floor), so the whole list error is the points' conversion.
    A pair: c_a = S (alpha on A, -beta on B), c_b = S (-beta on A, alpha on B), S a sign pattern, A | B a split of the dims into
    64 + 64, alpha = 7/64, beta = 2/64.  A point: x = S t with t_d = g_d + h (1 - eta) on A -- just below the midpoint of two fp16
    neighbours, rounds DOWN -- and g + h (1 + eta) on B -- just above, rounds UP; g in [1/4, 1/2), h = 2^-13 its half ulp,
    eta = 2^-9; g_d = g everywhere but g + 2 h in ONE dim of A.  Then
        w(a) - w(b) = (alpha + beta) (sum_A t - sum_B t) = (alpha + beta) 2 h (1 - 64 eta)  > 0          (a wins, by 3.0e-5),
        fp16:         (alpha + beta) (sum_A g_d - sum_B (g + 2 h)) = (alpha + beta) 2 h (1 - 64)  < 0    (b leads, by 2.2e-3),
    and the error of a alone, (alpha + beta) 64 h (1 - eta) = 1.10e-3, is 0.87 of ||x - fp16 x|| ||c_a||: the rounding error
    vector is S (-1 on A, +1 on B) h, c_a is S (alpha on A, -beta on B).  ||c_a|| = ||c_b|| = 0.91 (the MODE 1 bias cancels in the
    gap); x.c_a = 5 g >= 1.25 stands 3.7 sigma above what a point scores against another pair's centroids; the fillers have
    norm 1/8.  scale: a power of two applied to points and centroids (exact; 64 gives MODE 1 centroid norms of 58)."""
    rng = np.random.default_rng(seed)
    C = _fillers(rng, K, 0.125).astype(np.float64)
    alpha, beta, h, eta = 7 / 64, 2 / 64, 2.0 ** -13, 2.0 ** -9
    X, a_of, b_of, used = [], [], [], set()
    for _ in range(pairs):
        while True:
            a, b = _two_groups(rng, K)
            if a not in used and b not in used:
                break
        used |= {a, b}
        S = rng.choice([-1.0, 1.0], DIM)
        inA = np.zeros(DIM, dtype=bool); inA[rng.permutation(DIM)[:64]] = True
        C[:, a] = S * np.where(inA, alpha, -beta)
        C[:, b] = S * np.where(inA, -beta, alpha)
        for j in range(per_pair):
            g = (1024 + int(rng.integers(0, 1000))) * 2.0 ** -12
            t = np.where(inA, g + h * (1 - eta), g + h * (1 + eta))
            t[rng.choice(np.flatnonzero(inA))] += 2 * h
            X.append(S * t); a_of.append(a); b_of.append(b)
    C = (C * scale).astype(np.float32); X = (np.array(X).T * scale).astype(np.float32)
    return np.asfortranarray(C), np.asfortranarray(X), np.array(a_of), np.array(b_of)


def coherent_centroids(K=512, pairs=8, seed=6):
    """(b) with the roles swapped, the xn dc term.  The points are fp16-exact (dq = 0): x = S q, q = 3/4.  A pair:
    c_a = S t_a with every component just BELOW a midpoint (g_d + h (1 - eta), rounds down), c_b = S t_b with every component just
    above (g + h (1 + eta), rounds up); g in [1/4, 1/2) per pair, h = 2^-13, eta = 2^-10, g_d = g but g + 2 h in one dim.
        w(a) - w(b) = (q - ~g) 2 h (1 - 128 eta) > 0   (MODE 0: q 2 h 0.875 = 1.6e-4; MODE 1 carries the -||c||^2 / 2 of each),
        fp16:         q 2 h (1 - 128) < 0,
    and the error of a, q 128 h (1 - eta), IS ||x|| ||c_a - fp16 c_a||: both are multiples of S.  Fillers: fp16-exact, norm 1/8."""
    rng = np.random.default_rng(seed)
    C = _fillers(rng, K, 0.125).astype(np.float64)
    q, h, eta = 0.75, 2.0 ** -13, 2.0 ** -10
    X, a_of, b_of, used = [], [], [], set()
    for _ in range(pairs):
        while True:
            a, b = _two_groups(rng, K)
            if a not in used and b not in used:
                break
        used |= {a, b}
        S = rng.choice([-1.0, 1.0], DIM)
        g = (1024 + int(rng.integers(0, 1000))) * 2.0 ** -12
        ta = np.full(DIM, g + h * (1 - eta)); ta[int(rng.integers(0, DIM))] += 2 * h
        C[:, a] = S * ta
        C[:, b] = S * (g + h * (1 + eta))
        X.append(S * q); a_of.append(a); b_of.append(b)
    return (np.asfortranarray(C.astype(np.float32)), np.asfortranarray(np.array(X).T.astype(np.float32)),
            np.array(a_of), np.array(b_of))


def well_spread(K=256, n=1000, seed=7):
    """unit centroids; points = a centroid + noise of 5 % of its length"""
    rng = np.random.default_rng(seed)
    C = unit(rng, K)
    X = C[:, rng.integers(0, K, n)] + np.float32(0.05) * unit(rng, n)
    return C, np.asfortranarray(X)


def _same_half_slots(rng, K, count, taken=()):
    """`count` centroid indices in `count` different tiles, all in half 0 (c % 32 < 4)"""
    tiles = [t for t in rng.permutation(K // 32) if not any(32 * t <= c < 32 * t + 32 for c in taken)][:count]
    return np.sort(32 * np.array(tiles) + rng.integers(0, 4, count))


def few_undecided(sitters=40, K=512, n=600, seed=8):
    """well-spread data + one centroid copied into five groups of half 0 + `sitters` points exactly on it: five equal group maxima
    overflow a four-entry list.  Returns C, X, the sitters' indices, the duplicate's centroid indices (ascending)."""
    rng = np.random.default_rng(seed)
    C, X = well_spread(K, n, seed + 100)
    dup = _same_half_slots(rng, K, 5)
    near = np.isin(winners(scores(C, X, 0)), dup)                  # points drawn around a slot that is overwritten: move them
    X[:, near] = C[:, (dup[0] + 5) % K][:, None] + np.float32(0.05) * unit(rng, int(near.sum()))
    C[:, dup] = unit(rng, 1)
    sit = np.sort(rng.permutation(n)[:sitters])
    X[:, sit] = C[:, dup[:1]]
    return C, X, sit, dup


def second_tier(mode, near=50, sitters=30, K=512, n=700, seed=9, where=None):
    """More than 64 undecided points of two kinds, in well-spread data (fillers of norm 1/2, fp16-exact):
      near ties   four fp16-exact centroids E - j m ulp e_d (j = 0 .. 3: E itself and three copies with ONE component lowered) in four
                  groups of half 0, and fp16-exact points 2 E + (a few ulps on other components): the four group maxima span
                  gap = w(j = 0) - w(j = 3), with m chosen so that gap sits in the middle of
                      (margin3 + 2 e3 ,  margin1 - 2 e1]
                  -- the single-product lists MUST overflow (their error for exact operands is the accumulation term e1 alone, and the
                  margin carries dc of the whole set: one decoy centroid with every component next to a midpoint keeps it large),
                  the three-product lists MUST NOT (e3 = 7.4e-5 xn cn) and decide the point: the winner is j = 0;
      sitters     a centroid copied into five groups of half 0 with points on it: no list can decide them.
    where: (near positions, sitter positions) or None for random places.  Returns C, X, near idx, sitter idx, info dict."""
    rng = np.random.default_rng(seed)
    C = _fillers(rng, K, 0.5)
    slots = _same_half_slots(rng, K, 4)
    dup = _same_half_slots(rng, K, 5, taken=slots)
    free = np.array([c for c in range(K) if c not in set(slots) | set(dup)])
    decoy = free[group_of(free) % 2 == 1][0]                       # in half 1: its conversion error is in no crafted group's bound
    X = C[:, free[free != decoy][rng.integers(0, free.size - 1, n)]] * np.float32(2) + np.float32(0.05) * unit(rng, n)     # around 2 x a filler
    S = rng.choice([-1.0, 1.0], DIM)
    C[:, decoy] = (S * (2.0 ** -4 + 2.0 ** -15 * (1 - 2.0 ** -6))).astype(np.float32)     # norm 0.71, ||c - fp16 c|| = 3.4e-4
    E = f16(unit(rng, 1)[:, 0].astype(np.float64))
    d = int(np.argmax(np.abs(E)))
    ulp = float(np.spacing(np.float16(abs(E[d])))) if abs(E[d]) >= 2.0 ** -14 else 2.0 ** -24
    D = unit(rng, 1)
    C[:, dup] = D

    def family(m):
        F = np.repeat(E[:, None], 4, axis=1)
        F[d, :] -= np.sign(E[d]) * m * ulp * np.arange(4)
        return F

    Cm = C.copy(); Cm[:, slots] = family(1).astype(np.float32)
    cn, dc = cn_of(Cm), dc_of(Cm)
    x0 = 2 * E
    xn = 1.001 * np.linalg.norm(x0)
    lo = margin_of(xn, 0.0, cn, 0.0) + 2 * B3 * xn * cn + slack_of(xn, cn, 0.0)           # see must_overflow / cannot_overflow
    hi = margin_of(xn, 0.0, cn, dc) - 2 * 384.0 * U * xn * cn - slack_of(xn, cn, dc)
    m = 1
    while True:                                                    # the smallest m whose gap passes the middle of the zone
        F = family(m)
        w = x0 @ F - (0.5 * np.sum(F * F, axis=0) if mode == 1 else 0.0)
        if w[0] - w[3] >= 0.5 * (lo + hi) or m > 4000:
            break
        m += 1
    C[:, slots] = family(m).astype(np.float32)
    assert np.array_equal(f16(C[:, slots]), C[:, slots].astype(np.float64))
    if where is None:
        order = rng.permutation(n)
        where = (np.sort(order[:near]), np.sort(order[near:near + sitters]))
    near_at, sit_at = (np.asarray(w_, dtype=np.int64) for w_ in where)
    ulp_x = [float(np.spacing(np.float16(abs(2 * E[k])))) for k in range(DIM)]
    for i, p in enumerate(near_at):
        x = x0.copy()
        k = [k_ for k_ in range(DIM) if k_ != d][i % (DIM - 1)]
        x[k] += (1 + i // (DIM - 1)) * ulp_x[k]
        X[:, p] = x.astype(np.float32)
    X[:, sit_at] = D
    return (np.asfortranarray(C), np.asfortranarray(X), near_at, sit_at,
            {"slots": slots, "dup": dup, "decoy": decoy, "zone": (lo, hi), "gap": float(w[0] - w[3]), "steps": m})


def chunked(mode, seed=10):
    """(e): n = 2 * 4096 + 37 points.  Undecided points in runs of 1 024: [0, 1 024) 45 near ties + 25 sitters, [1 024, 2 048) 10
    sitters, [2 048, 3 072) 45 + 25, [4 096, 8 192) 20 sitters, the 37-point tail 5 sitters.  Near ties only ever share a chunk
    with more than 64 undecided points, so their tier does not depend on the chunk size."""
    rng = np.random.default_rng(seed)
    n = 2 * 4096 + 37

    def pick(lo, hi, k):
        return lo + np.sort(rng.permutation(hi - lo)[:k])

    a0, a2 = pick(0, 1024, 70), pick(2048, 3072, 70)
    near = np.concatenate([a0[:45], a2[:45]])
    sit = np.concatenate([a0[45:], pick(1024, 2048, 10), a2[45:], pick(4096, 8192, 20), pick(8192, n, 5)])
    return second_tier(mode, K=512, n=n, seed=seed, where=(np.sort(near), np.sort(sit)))


def undecided_per_chunk(n, chunk_max, undecided_at):
    edges = np.arange(0, n, chunk_max)
    return np.array([np.count_nonzero((undecided_at >= e) & (undecided_at < e + chunk_max)) for e in edges])
