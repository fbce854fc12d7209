"""Pitch plans restated in NumPy (float64 and Python integers): steps 1-5 of include/summertts_hip.h sts_set_pitch_plan.  The tests compare
the library's host entries and the warp kernel against this file; nothing here calls the library."""
import numpy as np

from gain_ref import pcm_cast  # noqa: F401  (the reference's int16 cast, shared with the gain plan's restatement)

ZC, RES, BETA = 32, 512, 10.0
PROTO = ZC * RES
ONE = 1 << 32
MAX_CENTS = 600


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------------------
def design(cents):
    """cents [n] -> (ratio float32 [n], step int64 [n])"""
    c = np.asarray(cents, np.int64)
    r = np.power(2.0, c.astype(np.float64) / 1200.0)
    return r.astype(np.float32), np.floor(r * 4294967296.0 + 0.5).astype(np.int64)


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------------------
def layout(d, step, hop):
    """-> (o, e): Python-integer lists [n + 1]"""
    n = len(d)
    o, e = [0] * (n + 1), [0] * (n + 1)
    for i in range(n):
        L = (int(d[i]) * hop) << 32
        s = int(step[i])
        ni = -((-(L - e[i])) // s) if L > e[i] else 0
        e[i + 1] = e[i] + ni * s - L
        o[i + 1] = o[i] + ni
    return o, e


def rows(d, step, hop):
    """The phonemes as the warp sees them: (o, e, a, step) with the all-zero utterance's one frame as a single phoneme of step 2^32."""
    if int(np.sum(d)) == 0:
        d, step = [1], [ONE]
    o, e = layout(d, step, hop)
    a = [0] + [int(v) * hop for v in np.cumsum(np.asarray(d, np.int64))]
    return o, e, a, [int(s) for s in step]


def warped_length(d, step, hop):
    return rows(d, step, hop)[0][-1]


def positions(d, step, hop):
    """Q32 input position of every output, Python integers"""
    o, e, a, step = rows(d, step, hop)
    return [(a[i] << 32) + e[i] + (j - o[i]) * step[i] for i in range(len(step)) for j in range(o[i], o[i + 1])]


# ---- step 4 ---------------------------------------------------------------------------------------------------------------------------------
def window(u):
    u = np.asarray(u, np.float64)
    return np.where(u < ZC, np.i0(BETA * np.sqrt(np.clip(1.0 - (u / ZC) ** 2, 0.0, 1.0))) / np.i0(BETA), 0.0)


def table():
    """h0: float32 [16386]"""
    u = np.arange(PROTO + 2) / RES
    h = (np.sinc(u) * window(u)).astype(np.float32)
    h[PROTO:] = 0
    return h


_H0 = None


def coef(uabs):
    global _H0
    if _H0 is None:
        _H0 = table().astype(np.float64)
    t = uabs * RES
    k = np.floor(t).astype(np.int64)
    f = t - k
    k = np.minimum(k, PROTO)
    return _H0[k] + f * (_H0[k + 1] - _H0[k])


def reach(step):
    c = 0.9 * min(1.0, 1.0 / (int(step) / 4294967296.0))
    return c, int(np.ceil(ZC / c))


def warp(x, d, step, hop, exact=False):
    """One planned utterance: x float [max(1, sum d) hop] -> (y float64 [N'] before the rounding to float32, S [N'] =
    sum |g x| / |sum g|).  exact: the closed-form window instead of the interpolated prototype."""
    x = np.asarray(x, np.float64)
    N = x.size
    assert N == max(1, int(np.sum(d))) * hop
    o, e, a, step = rows(d, step, hop)
    y, S = np.zeros(o[-1]), np.zeros(o[-1])
    for i in range(len(step)):
        c, K = reach(step[i])
        m = np.arange(2 * K)
        for j in range(o[i], o[i + 1]):
            pos = (a[i] << 32) + e[i] + (j - o[i]) * step[i]
            n0, f = pos >> 32, (pos & 0xFFFFFFFF) / 4294967296.0
            dd = f + K - 1 - m
            idx = n0 - K + 1 + m
            u = np.abs(c * dd)
            g = np.sinc(u) * window(u) if exact else coef(u)
            ok = (idx >= 0) & (idx < N)
            xv = np.where(ok, x[np.clip(idx, 0, N - 1)], 0.0)
            y[j] = np.dot(g, xv) / g.sum()
            S[j] = np.dot(np.abs(g), np.abs(xv)) / abs(g.sum())
    return y, S


# ---- step 5 and the batch -------------------------------------------------------------------------------------------------------------------
def apply(x, d, hop, cents):
    """One utterance: -> (y float32, S float64, y64).  cents None: the copy."""
    x = np.asarray(x, np.float32)
    if cents is None:
        return x.copy(), np.abs(x.astype(np.float64)), x.astype(np.float64)
    y64, S = warp(x, d, design(cents)[1], hop)
    return y64.astype(np.float32), S, y64


def tolerance(y64, S):
    """|y - ref| <= 2^-23 |ref| + 2^-40 S (DESIGN.md 9l has the derivation)"""
    return 2.0 ** -23 * np.abs(y64) + 2.0 ** -40 * S
