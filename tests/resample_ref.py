"""Float64 checker of the output sample-rate conversion (include/summertts_hip.h sts_set_output_rate): the filter table from its
definition, the output length and phase/base arithmetic, and the resampler itself.  Written from the definition, not from the library."""
from math import gcd

import numpy as np

NATIVE = 16000
BETA = 10.0


def design(out_rate, in_rate=NATIVE):
    """-> (P, Q, K, c, W)"""
    g = gcd(in_rate, out_rate)
    P, Q = out_rate // g, in_rate // g
    c = 0.9 * min(1.0, out_rate / in_rate)
    W = 32.0 / c
    return P, Q, int(np.ceil(W)), c, W


def valid(out_rate, in_rate=NATIVE):
    if not (8000 <= in_rate <= 48000 and 8000 <= out_rate <= 48000):
        return False
    return design(out_rate, in_rate)[0] <= 1024


def offsets(out_rate, in_rate=NATIVE):
    """d[phi, m] = phi / P + K - 1 - m: where tap m of phase phi sits relative to the output position, in input samples."""
    P, Q, K, c, W = design(out_rate, in_rate)
    return np.arange(P)[:, None] / P + (K - 1 - np.arange(2 * K))[None, :]


def table(out_rate, in_rate=NATIVE, normalise=True):
    """float64 [P][2K]; every phase sums to 1 (normalise=False: the raw windowed sinc)"""
    P, Q, K, c, W = design(out_rate, in_rate)
    d = offsets(out_rate, in_rate)
    inside = np.abs(d) < W
    r = np.where(inside, d / W, 0.0)
    h = np.where(inside, c * np.sinc(c * d) * np.i0(BETA * np.sqrt(1.0 - r * r)) / np.i0(BETA), 0.0)
    return h / h.sum(axis=1, keepdims=True) if normalise else h


def out_len(n_in, out_rate, in_rate=NATIVE):
    P, Q = design(out_rate, in_rate)[:2]
    return (n_in * P + Q - 1) // Q


def phase_base(j, out_rate, in_rate=NATIVE):
    P, Q = design(out_rate, in_rate)[:2]
    jq = np.asarray(j, np.int64) * Q
    return jq % P, jq // P


def resample(x, out_rate, in_rate=NATIVE, h=None):
    """y_j = sum_m h[phi_j, m] x[n0_j - K + 1 + m], x = 0 outside [0, len(x))."""
    x = np.asarray(x, np.float64).ravel()
    P, Q, K, c, W = design(out_rate, in_rate)
    h = table(out_rate, in_rate) if h is None else np.asarray(h, np.float64)
    n = out_len(x.size, out_rate, in_rate)
    phi, n0 = phase_base(np.arange(n), out_rate, in_rate)
    xp = np.concatenate([np.zeros(K), x, np.zeros(K + 1)])        # xp[i + K] = x[i]
    idx = (n0 - K + 1 + K)[:, None] + np.arange(2 * K)[None, :]
    return np.einsum("jm,jm->j", h[phi], xp[idx])


def pcm_cast(y):
    """The reference's (int16)(int32)(y * 32737) on x86-64: truncation toward zero, wrap-around, out-of-int32 -> 0 (devmath.hpp)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(y, np.float32) * np.float32(32737.0)).astype(np.float64)     # (the product in fp32, as on the device)
        v = np.nan_to_num(v, nan=2.0 ** 40)
    q = np.where(np.abs(v) < 2.0 ** 31, np.trunc(v), -2.0 ** 31).astype(np.int64)
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)


def prototype_response(out_rate, freqs_hz, in_rate=NATIVE):
    """|H(f)| of the prototype filter (the phases interleaved at P * in_rate), divided by P: 1 in the passband."""
    P = design(out_rate, in_rate)[0]
    h = table(out_rate, in_rate).ravel()
    d = offsets(out_rate, in_rate).ravel()            # tap positions in input samples (distinct multiples of 1 / P)
    f = np.asarray(freqs_hz, np.float64)
    out = np.empty(f.size)
    for i in range(0, f.size, 256):
        ph = np.exp(-2j * np.pi * np.outer(f[i:i + 256] / in_rate, d))
        out[i:i + 256] = np.abs(ph @ h) / P
    return out


def prototype_spectrum(out_rate, in_rate=NATIVE, nfft=1 << 20):
    """(freqs_hz, |H| / P) on an FFT grid up to the prototype's Nyquist P * in_rate / 2."""
    P, Q, K, c, W = design(out_rate, in_rate)
    h = table(out_rate, in_rate)
    d = offsets(out_rate, in_rate)
    k = np.rint(d * P).astype(np.int64)               # integer positions on the P * in_rate grid
    proto = np.zeros(k.max() - k.min() + 1)
    proto[(k - k.min()).ravel()] = h.ravel()
    nfft = max(nfft, 1 << int(np.ceil(np.log2(proto.size * 8))))
    H = np.abs(np.fft.rfft(proto, nfft)) / P
    return np.fft.rfftfreq(nfft, 1.0 / (P * in_rate)), H
