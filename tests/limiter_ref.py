"""numpy checker of the look-ahead peak limiter (include/summertts_hip.h sts_set_limiter, steps 1-7).  `c` and `G` are passed in (tests
take them from sts_limiter_design so that a last-bit difference between libm and numpy pow cannot masquerade as a kernel error); H may be
computed here (design_H) or taken from the library."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ONE = 1 << 30


def design_H(rate, lookahead_ms):
    """step 1: H = floor(lookahead_ms fs / 1000 + 0.5), lookahead_ms as the float32 the C ABI receives, the arithmetic in float64"""
    return int(np.floor(float(np.float32(lookahead_ms)) * float(rate) / 1000.0 + 0.5))


def static_gain(G, g_loud=1.0):
    """step 2: g0 = float32(G * g_loud), one float64 product rounded once (g_loud: float32 loudness gain, or 1)"""
    return np.float32(float(G) * float(np.float32(g_loud)))


def limit(x, g0, H, c):
    """steps 3-7 for one utterance: x float32 [N], g0 float32, c float64 -> (y float32 [N], s float32 [N], S int64 [N])"""
    x = np.ascontiguousarray(x, np.float32)
    if x.size == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (x * np.float32(g0)).astype(np.float32)
    a = np.abs(v).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a > c, c / a, 1.0)
        q = np.floor(r * ONE)
    q[~np.isfinite(a)] = 0
    q = q.astype(np.int64)
    qp = np.full(x.size + 4 * H, ONE, np.int64)
    qp[2 * H:2 * H + x.size] = q
    m = sliding_window_view(qp, 2 * H + 1).min(axis=1)        # m[k], k = -H .. N+H-1
    S = sliding_window_view(m, 2 * H + 1).sum(axis=1)         # S[n], n = 0 .. N-1
    s = (S.astype(np.float64) / float((2 * H + 1) * ONE)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (v * s).astype(np.float32)
    return y, s, S


def pcm_cast(y):
    """the reference's cast (int16)(int32)(y * 32737): fp32 product, truncation, wrap-around (finite y)"""
    v = np.asarray(y, np.float32) * np.float32(32737.0)
    return np.trunc(v.astype(np.float64)).astype(np.int64).astype(np.int32).astype(np.int16)


def stats(y, s, S, g0, H):
    """sts_limiter_stats of one utterance: gain, min_gain (1.0 when untouched or empty), peak_out (NaN samples skipped), limited"""
    full = (2 * H + 1) * ONE
    return {"gain": np.float32(g0),
            "min_gain": np.float32(s.min()) if s.size else np.float32(1.0),
            "peak_out": np.float32(np.fmax.reduce(np.abs(y), initial=np.float32(0.0))),     # over the samples whose y is not NaN
            "limited": int((S < full).sum())}


def ceiling_pcm(c):
    """|pcm| never exceeds this"""
    return int(np.floor(32737.0 * c)) + 1
