"""A host model of the two-pass cut of a search with a score prior (csrc/prior_kernels.hpp): what the
boosted selection lists, against the true top k by (E, pid).  fp32 values are numpy float32, the inequalities are checked in
float64.  No tests here (tests/test_prior_cpu.py)."""
import numpy as np

U = 2.0 ** -24                                                 # fp32 unit roundoff


def documented_delta(M, eps):
    """delta of prior_tau_kernel: 4 * 2^-24 * (M + eps), M = max |A| over the query's candidates"""
    return 4.0 * U * (float(M) + float(eps))


def make_case(seed, n, magnitude, eps, values="uniform", ties=0):
    """n candidates in pid order: exact scores e (fp32, 5 .. 30), approximate scores a = e + noise with |a - e| <= eps (a
    third of the draws pinned near -eps and near +eps), prior terms pi = fl32(weight * value) of size `magnitude`
    ("uniform": magnitude * U(-1, 1); "levels": magnitude * an integer 0 .. 3; "constant": magnitude), A = fl32(a + pi),
    E = fl32(e + pi).  `ties`: that many blocks of 8 consecutive candidates share one (a, pi), i.e. exactly tied A (blocks may overlap)."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(5.0, 30.0, size=n).astype(np.float32)
    kind = rng.integers(0, 3, size=n)
    noise = np.where(kind == 0, -eps, np.where(kind == 1, eps, rng.uniform(-eps, eps, size=n))) * 0.999
    a = (e.astype(np.float64) + noise).astype(np.float32)
    if values == "uniform":
        v = (magnitude * rng.uniform(-1.0, 1.0, size=n)).astype(np.float32)
    elif values == "levels":
        v = (magnitude * rng.integers(0, 4, size=n)).astype(np.float32)
    else:
        v = np.full(n, magnitude, np.float32)
    weight = np.float32(rng.choice([1.0, 0.75, -1.5]))
    pi = weight * v
    for start in rng.choice(np.arange(0, n - 8), size=ties, replace=False):
        a[start:start + 8] = a[start]                          # one A for the block; its exact scores lie around a, within eps
        e[start:start + 8] = (np.float64(a[start]) + 0.999 * rng.uniform(-eps, eps, size=8)).astype(np.float32)
        pi[start:start + 8] = pi[start]
    a = np.where(np.abs(a.astype(np.float64) - e) <= eps, a, e)       # (the fp32 rounding of a pinned draw may pass eps by an ulp)
    assert pi.dtype == np.float32 and np.all(np.abs(a.astype(np.float64) - e.astype(np.float64)) <= eps)
    A = a + pi
    E = e + pi
    assert A.dtype == np.float32 and E.dtype == np.float32
    return dict(e=e, a=a, pi=pi, A=A, E=E, eps=float(eps))


def true_top(case, k):
    """slots (= pid order) of the first k candidates by (E descending, pid ascending)"""
    return np.argsort(-case["E"], kind="stable")[:k]


def listed(case, k, delta=None, fp32_steps=False):
    """The list of the boosted selection: {A >= tau - 2 delta - 2 eps}, tau the k-th largest A (everything with fewer than k
    candidates).  delta None: the documented one.  fp32_steps: the threshold formed as the kernels form it, fl32(fl32(tau -
    2 delta) - 2 eps) with delta and eps rounded to fp32 first."""
    A, eps = case["A"], case["eps"]
    if A.size < k:
        return np.ones(A.size, bool)
    tau = np.sort(A)[-k]
    if delta is None:
        delta = documented_delta(np.max(np.abs(A.astype(np.float64))), eps)
    if fp32_steps:
        t_in = np.float32(tau) - np.float32(2.0) * np.float32(delta)
        thr = np.float32(t_in) - np.float32(2.0) * np.float32(eps)
        return ~(A < thr)
    return A.astype(np.float64) >= float(tau) - 2.0 * delta - 2.0 * eps


def misses(case, k, **kw):
    """members of the true top k that the list does not hold"""
    L = listed(case, k, **kw)
    return [int(i) for i in true_top(case, k) if not L[i]]
