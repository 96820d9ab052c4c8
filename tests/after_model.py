"""A host model of the two-pass cut of a search after a cursor (csrc/after_kernels.hpp): what the selection
lists behind a cursor (s*, p*), against the true next k by (e descending, pid ascending).  fp32 values are numpy float32 and
`lo`, `hi`, the slack and the threshold are formed in the fp32 steps of the kernels; the inequalities are checked in float64.
Slot i is pid i + 1.  No tests here (tests/test_after_cpu.py)."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny


def step_down(x):
    """f32_step_down of after_kernels.hpp"""
    x = F32(x)
    if np.isneginf(x):
        return x
    if np.isposinf(x):
        return FLT_MAX
    if -FLT_MIN < x <= FLT_MIN:
        return F32(-FLT_MIN)
    u = x.view(np.uint32)
    return (u - np.uint32(1) if x > 0 else u + np.uint32(1)).view(np.float32)


def step_up(x):
    return F32(-step_down(F32(-F32(x))))


def bounds(s, eps, ulp_step=True):
    """(lo, hi) of a finite or -Inf cursor score: fl(s - eps) stepped down, fl(s + eps) stepped up (ulp_step False: unstepped)"""
    with np.errstate(over="ignore"):
        lo, hi = F32(F32(s) - F32(eps)), F32(F32(s) + F32(eps))
    return (step_down(lo), step_up(hi)) if ulp_step else (lo, hi)


def make_case(seed, n, eps, gap=None, ties_a=0, ties_e=0):
    """n candidates in pid order: exact scores e (fp32; `gap` None: uniform in 5 .. 30, else about `gap` apart on average),
    approximate scores a with |a - e| <= eps, a third of the draws pinned at e - 0.999 eps and a third at e + 0.999 eps.
    `ties_a` blocks of 6 consecutive candidates share one a (their e scattered within eps of it), `ties_e` blocks share one e
    (their a scattered within eps of it)."""
    rng = np.random.default_rng(seed)
    hi_e = 30.0 if gap is None else 5.0 + n * gap
    e = rng.uniform(5.0, hi_e, size=n).astype(np.float32)
    kind = rng.integers(0, 3, size=n)
    noise = np.where(kind == 0, -eps, np.where(kind == 1, eps, rng.uniform(-eps, eps, size=n))) * 0.999
    a = (e.astype(np.float64) + noise).astype(np.float32)
    starts = rng.choice(np.arange(0, n - 6), size=ties_a + ties_e, replace=False) if ties_a + ties_e else []
    for j, st in enumerate(starts):
        if j < ties_a:
            a[st:st + 6] = a[st]
            e[st:st + 6] = (np.float64(a[st]) + 0.999 * rng.uniform(-eps, eps, size=6)).astype(np.float32)
        else:
            e[st:st + 6] = e[st]
            a[st:st + 6] = (np.float64(e[st]) + 0.999 * rng.uniform(-eps, eps, size=6)).astype(np.float32)
    a = np.where(np.abs(a.astype(np.float64) - e) <= eps, a, e)       # (the fp32 rounding of a pinned draw may pass eps by an ulp)
    assert np.all(np.abs(a.astype(np.float64) - e.astype(np.float64)) <= eps)
    return dict(e=e, a=a.astype(np.float32), eps=float(F32(eps)))


def after_mask(case, s, p):
    e, pid = case["e"], np.arange(1, case["e"].size + 1)
    s = F32(s)
    if np.isposinf(s):
        return np.ones(e.size, bool)
    return (e < s) | ((e == s) & (pid > int(p)))


def true_next(case, s, p, k):
    """slots of the first k candidates after the cursor by (e descending, pid ascending)"""
    order = np.argsort(-case["e"], kind="stable")
    return order[after_mask(case, s, p)[order]][:k]


def listed(case, s, k, rule="sure", ulp_step=True, strict=True):
    """(list, passed): what after_cut_kernel and the unchanged selection list for the cursor score s, and the candidates
    masked as passed.  rule "sure": tau over {a < lo}; rule "below_cursor": the obvious and wrong tau over {a <= s*}.
    strict False: the comparisons a <= lo / a >= hi in place of a < lo / a > hi (where the ulp step is what keeps the proof)."""
    a, eps = case["a"], F32(case["eps"])
    s = F32(s)
    n = a.size
    if np.isposinf(s):
        sure, passed = np.ones(n, bool), np.zeros(n, bool)
    else:
        lo, hi = bounds(s, eps, ulp_step)
        sure = (a < lo) if strict else (a <= lo)
        passed = (a > hi) if strict else (a >= hi)
        if rule == "below_cursor":
            sure = a <= s
    masked = np.where(passed, F32(-np.inf), a)
    if np.count_nonzero(sure) < k:
        thr = F32(-np.inf) if np.isposinf(s) else F32(F32(-FLT_MAX) - F32(2.0) * eps)
    else:
        tau = np.sort(a[sure])[-k]
        delta = F32(2.0 ** -22) * F32(np.abs(tau) + F32(2.0) * eps)
        thr = F32(F32(tau - delta) - F32(2.0) * eps)
        assert float(thr) <= float(tau) - 2.0 * float(eps), (tau, eps, thr)        # the slack covers both roundings
    return ~(masked < thr), passed


def misses(case, s, p, k, **kw):
    """members of the true next k that the list does not hold"""
    L, _ = listed(case, s, k, **kw)
    return [int(i) for i in true_next(case, s, p, k) if not L[i]]


def cursors(case, seed=0, some=24):
    """(s*, p*) the issue names: members' own (e, pid); between two scores; every pid position of the tie blocks (and p* below /
    above them); within one ulp of a - eps and a + eps of some candidates; above the best and below the worst; none; -Inf"""
    e, a, eps = case["e"], case["a"], case["eps"]
    rng = np.random.default_rng(seed)
    n = e.size
    out = [(np.inf, 0), (-np.inf, 0), (F32(e.max() + 1), 0), (F32(e.min() - 1), 0), (e.max(), 0), (e.min(), n)]
    for i in rng.choice(n, size=min(some, n), replace=False):
        out.append((e[i], i + 1))
    srt = np.sort(e)
    for j in rng.choice(n - 1, size=min(some, n - 1), replace=False):
        out.append((F32(0.5 * (float(srt[j]) + float(srt[j + 1]))), 0))
    vals, counts = np.unique(e, return_counts=True)
    for v in vals[counts > 1][:8]:
        slots = np.nonzero(e == v)[0]
        out += [(v, 0), (v, n + 1)] + [(v, int(i) + 1) for i in slots]
    for i in rng.choice(n, size=min(some // 2, n), replace=False):
        for base in (F32(a[i] - F32(eps)), F32(a[i] + F32(eps))):             # s* - eps or s* + eps lands on a[i], give or take an ulp
            out += [(base, 0), (step_down(base), 0), (step_up(base), 0)]
    return out
