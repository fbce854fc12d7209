"""NumPy restatement of the gain-plan definition (include/summertts_hip.h sts_set_gain_plan), steps 1-5, and of the reference's int16 cast.
Everything between the design and the envelope is integer arithmetic, so the engine's kernel must agree with this to the bit."""
import numpy as np

ONE = 1 << 20


def design(gain_db, n, ramp_ms=0.0):
    """step 1 -> (q int32 [n], h): float64 throughout"""
    if gain_db is None:
        q = np.full(n, ONE, np.int32)
    else:
        g = np.asarray(gain_db, np.float32).astype(np.float64)
        assert g.size == n
        with np.errstate(over="ignore"):
            q = np.where(np.isneginf(g), 0.0, np.floor(np.power(10.0, g / 20.0) * float(ONE) + 0.5)).astype(np.int32)
    h = int(np.floor(float(np.float32(ramp_ms)) * 8.0 + 0.5))
    return q, h


def step(q, dur, hop):
    """step 2 inside the utterance: Q int64 [max(1, sum d) * hop]"""
    d = np.asarray(dur, np.int64)
    Q = np.repeat(np.asarray(q, np.int64), d * hop)
    if Q.size == 0:                       # every duration is 0: one frame that nobody owns
        Q = np.full(hop, ONE, np.int64)
    return Q


def window_sums(Q, h):
    """step 3 from an int64 cumulative sum of Q padded with its edge values"""
    P = np.concatenate([[0], np.cumsum(np.pad(Q, h, mode="edge"), dtype=np.int64)])
    return P[2 * h + 1:] - P[:Q.size]


def window_sums_brute(Q, h):
    """step 3 as the definition writes it: one window sum per sample"""
    Qp = np.pad(Q, h, mode="edge")
    return np.asarray([int(Qp[t:t + 2 * h + 1].sum()) for t in range(Q.size)], np.int64)


def envelope(q, h, dur, hop):
    """steps 2-4 -> float32 [N]"""
    S = window_sums(step(q, dur, hop), h)
    return (S.astype(np.float64) / np.float64((2 * h + 1) * ONE)).astype(np.float32)


def apply(x, dur, hop, gain_db, ramp_ms=0.0):
    """steps 1-5 on one utterance's float wave -> y float32"""
    x = np.asarray(x, np.float32)
    q, h = design(gain_db, len(dur), ramp_ms)
    env = envelope(q, h, dur, hop)
    assert env.size == x.size, (env.size, x.size)
    return x * env


def pcm_cast(y):
    """the reference's cast (int16)(int32)(y * 32737): fp32 product, truncation toward zero, wrap-around modulo 2^16; beyond int32 (and NaN) 0"""
    v = np.asarray(y, np.float32) * np.float32(32737.0)
    ok = np.abs(v) < np.float32(2147483648.0)              # (False for NaN)
    q = np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64), -(1 << 31))
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)
