"""Checker of the duration plans (include/summertts_hip.h sts_set_duration_plan): steps 3-4 of the definition restated with Python
integers, the float32 expressions with numpy float32 -- no shared code with the library.  ``fit`` is what sts_duration_fit, the plan
kernel (sts_duration_plan_apply) and an engine run with a plan must return, bit for bit."""
import math

import numpy as np

MAX_DUR = 100000          # the clamp of a call without a plan
MAX_TARGET = 1 << 20


def clamp_ceil(w):
    """step 3: min(ceilf(w), 100000), 0 for NaN or w <= 0"""
    w = np.float32(w)
    if not (w > 0):
        return 0
    if np.isinf(w):
        return MAX_DUR
    return min(int(math.ceil(float(w))), MAX_DUR)


def weight(w):
    """k = (int64) floorf(fminf(w, 4096.f) * 1048576.f); 0 when w is NaN or not above 0"""
    w = np.float32(w)
    if not (w > 0):
        return 0
    return int(np.floor(np.float32(min(w, np.float32(4096.0))) * np.float32(1048576.0)))


def feasible(fixed, n, target):
    """the rules of the set call for one utterance (fixed: None or n ints)"""
    fx = [-1] * n if fixed is None else [int(v) for v in fixed]
    if any(v < -1 or v > MAX_DUR for v in fx):
        return False
    if target == 0:
        return True
    if target < 1 or target > MAX_TARGET:
        return False
    sfix = sum(v for v in fx if v >= 0)
    nfree = sum(1 for v in fx if v < 0)
    return target - sfix >= nfree if nfree else sfix == target


def fit(w, fixed=None, target=0):
    """durations (int32 array) of one utterance with weights w"""
    w = np.asarray(w, np.float32).ravel()
    n = w.size
    fx = [-1] * n if fixed is None else [int(v) for v in fixed]
    assert feasible(fx, n, target)
    if target == 0:
        return np.asarray([fx[i] if fx[i] >= 0 else clamp_ceil(w[i]) for i in range(n)], np.int32)
    free = [i for i in range(n) if fx[i] < 0]
    d = list(fx)
    if not free:
        return np.asarray(d, np.int32)
    R = target - sum(v for v in fx if v >= 0) - len(free)
    k = {i: weight(w[i]) for i in free}
    K = sum(k.values())
    if K == 0:
        k = {i: 1 for i in free}
        K = len(free)
    a = {i: (R * k[i]) // K for i in free}
    r = {i: (R * k[i]) % K for i in free}
    assert all(R * k[i] < 1 << 54 for i in free)
    L = R - sum(a.values())
    assert 0 <= L < len(free)
    first = set(sorted(free, key=lambda i: (-r[i], i))[:L])
    for i in free:
        d[i] = 1 + a[i] + (1 if i in first else 0)
    return np.asarray(d, np.int32)


def exact_share(w, fixed, target):
    """(R', {i: R' k_i / K as a Fraction-free float pair}) for the property |d_i - 1 - R' k_i / K| < 1: returns per free phoneme the
    integers (R' k_i, K)"""
    w = np.asarray(w, np.float32).ravel()
    fx = [-1] * w.size if fixed is None else [int(v) for v in fixed]
    free = [i for i in range(w.size) if fx[i] < 0]
    R = target - sum(v for v in fx if v >= 0) - len(free)
    k = {i: weight(w[i]) for i in free}
    K = sum(k.values())
    if K == 0:
        k = {i: 1 for i in free}
        K = len(free)
    return {i: (R * k[i], K) for i in free}


def offsets(dur, lens, hop, P=1, Q=1):
    """start of every phoneme in output samples: ceil(f hop P / Q), f = the frames before it in its utterance"""
    out, o = [], 0
    for n in lens:
        f = 0
        for i in range(n):
            out.append(-((-f * hop * P) // Q))
            f += int(dur[o + i])
        o += n
    return np.asarray(out, np.int64)


# ---- the weights and targets both suites run
def weight_sets(n, seed):
    """name -> float32[n]: random weights and the adversarial ones"""
    rng = np.random.default_rng(seed)
    out = {"random": np.exp(rng.normal(0.5, 1.0, n)).astype(np.float32),
           "equal": np.full(n, 2.75, np.float32),
           "zero": np.zeros(n, np.float32),
           "tiny": np.full(n, 1e-3, np.float32)}
    out["tiny"][n // 2] = np.float32(1e5)
    bad = np.exp(rng.normal(0.0, 1.0, n)).astype(np.float32)
    bad[0] = np.inf
    if n > 1:
        bad[n - 1] = np.nan
    if n > 3:
        bad[n // 3] = np.nan; bad[2 * n // 3] = np.inf; bad[1] = np.float32(-3.0)
    out["inf_nan"] = bad
    return out


def targets(w, n_free, sfix):
    """the minimum, sum ceil(w) and three times that (each at least the minimum, at most 2^20)"""
    lo = sfix + n_free
    s = sum(clamp_ceil(v) for v in w)
    return sorted({lo, min(max(s, lo), MAX_TARGET), min(max(3 * s, lo), MAX_TARGET)})
