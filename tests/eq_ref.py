"""Float64 checker of the parametric equaliser (include/summertts_hip.h sts_set_eq): the Audio-EQ-Cookbook biquad of every band, the
validity rules, the sequential direct-form-I cascade that DEFINES the output (apply), the reference's int16 cast -- and scan(), a float64
restatement of the order in which eq.hip evaluates the same recurrence (chunks of R samples, tiles of THREADS chunks, carries composed
through powers of the chunk map).  Written from the definition, not from the library."""
import math

import numpy as np

try:
    from scipy.signal import sosfilt as _sosfilt
except Exception:          # (a plain float64 loop where scipy is absent)
    _sosfilt = None

from loudness_ref import pcm_cast  # noqa: F401  (the cast is the same one)

MAX_BANDS = 4
PEAK, LOWSHELF, HIGHSHELF, HIGHPASS, LOWPASS = 1, 2, 3, 4, 5
R, THREADS = 32, 256
TILE = R * THREADS
Q_RATIO_MAX = 6400.0


def check(rate, bands):
    """the validity rules; bands: sequence of (type, freq_hz, gain_db, q)"""
    if not 8000 <= int(rate) <= 48000 or not 0 <= len(bands) <= MAX_BANDS:
        return False
    for t, f, g, q in bands:
        f, g, q = float(np.float32(f)), float(np.float32(g)), float(np.float32(q))
        if t not in (1, 2, 3, 4, 5) or not all(math.isfinite(v) for v in (f, g, q)):
            return False
        if not (20.0 <= f <= 0.45 * rate and 0.1 <= q <= 8.0 and -24.0 <= g <= 24.0):
            return False
        if q * float(rate) / f > Q_RATIO_MAX:
            return False
    return True


def biquad(t, f0, gain_db, q, fs):
    """-> (b0, b1, b2, a1, a2) normalised by a0, float64, from the band's float32 values"""
    f0, gain_db, q, fs = float(np.float32(f0)), float(np.float32(gain_db)), float(np.float32(q)), float(fs)
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * f0 / fs
    cw, sw = math.cos(w0), math.sin(w0)
    al = sw / (2.0 * q)
    if t == PEAK:
        b = (1.0 + al * A, -2.0 * cw, 1.0 - al * A)
        a = (1.0 + al / A, -2.0 * cw, 1.0 - al / A)
    elif t == HIGHPASS:
        b = ((1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0)
        a = (1.0 + al, -2.0 * cw, 1.0 - al)
    elif t == LOWPASS:
        b = ((1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0)
        a = (1.0 + al, -2.0 * cw, 1.0 - al)
    elif t == LOWSHELF:
        s = 2.0 * math.sqrt(A) * al
        b = (A * ((A + 1.0) - (A - 1.0) * cw + s), 2.0 * A * ((A - 1.0) - (A + 1.0) * cw), A * ((A + 1.0) - (A - 1.0) * cw - s))
        a = ((A + 1.0) + (A - 1.0) * cw + s, -2.0 * ((A - 1.0) + (A + 1.0) * cw), (A + 1.0) + (A - 1.0) * cw - s)
    elif t == HIGHSHELF:
        s = 2.0 * math.sqrt(A) * al
        b = (A * ((A + 1.0) + (A - 1.0) * cw + s), -2.0 * A * ((A - 1.0) + (A + 1.0) * cw), A * ((A + 1.0) + (A - 1.0) * cw - s))
        a = ((A + 1.0) - (A - 1.0) * cw + s, 2.0 * ((A - 1.0) - (A + 1.0) * cw), (A + 1.0) - (A - 1.0) * cw - s)
    else:
        raise ValueError("unknown band type")
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def design(rate, bands):
    """-> [S][5] float64, the layout of sts_eq_design"""
    return np.array([biquad(t, f, g, q, rate) for t, f, g, q in bands], np.float64).reshape(len(bands), 5)


def apply(x, coeffs):
    """THE DEFINITION: float32 x -> float64 u_S, every section in direct form I from zero state (scipy's DF2T agrees to 1e-12)"""
    u = np.asarray(x, np.float32).astype(np.float64)
    coeffs = np.asarray(coeffs, np.float64).reshape(-1, 5)
    if u.size == 0 or coeffs.shape[0] == 0:
        return u
    if _sosfilt is not None:
        sos = np.array([[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in coeffs])
        return _sosfilt(sos, u)
    for b0, b1, b2, a1, a2 in coeffs:
        o = np.empty_like(u)
        x1 = x2 = y1 = y2 = 0.0
        for n, v in enumerate(u):
            w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, v, y1, w
            o[n] = w
        u = o
    return u


def apply_df1(x, coeffs):
    """the plain loop of the definition (slow; what the scan restatement is measured against)"""
    u = np.asarray(x, np.float32).astype(np.float64)
    for b0, b1, b2, a1, a2 in np.asarray(coeffs, np.float64).reshape(-1, 5):
        o = np.empty_like(u)
        x1 = x2 = y1 = y2 = 0.0
        for n in range(u.size):
            v = u[n]
            w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, v, y1, w
            o[n] = w
        u = o
    return u


def eq(x, rate, bands):
    """-> (y float32, pcm int16) of one utterance"""
    y = apply(x, design(rate, bands)).astype(np.float32)
    return y, pcm_cast(y)


# ---- the scan order of eq.hip ----------------------------------------------------------------------------------------------------
# State of the cascade between two samples, D = 2S values: per section s (y_s[n-1], y_s[n-1] - y_s[n-2]) -- the output history in
# the basis (value, difference), which keeps a pole pair near z = 1 well conditioned.  Section 1's input history is read from x.

def _cascade(coeffs, x0, x1, x2, y1, y2):
    """one sample of the cascade on arrays: x history (x1, x2), lists y1[s], y2[s]; returns the output, updates the lists in place"""
    v0, v1, v2 = x0, x1, x2
    for s, (b0, b1, b2, a1, a2) in enumerate(coeffs):
        w = b0 * v0 + b1 * v1 + b2 * v2 - a1 * y1[s] - a2 * y2[s]
        nv1, nv2 = y1[s], y2[s]
        y2[s] = y1[s]
        y1[s] = w
        v0, v1, v2 = w, nv1, nv2
    return v0


def chunk_map_powers(coeffs, npow=9):
    """Mp[d] = (A^R)^(2^d), d < npow, as float64 [npow][D][D]; A = one homogeneous step in the (value, difference) basis.  Built in the
    widest float the host has (x87 extended where there is one), as eq.hip builds it in long double, then rounded once."""
    L = np.longdouble
    cs = [tuple(L(v) for v in c) for c in np.asarray(coeffs, np.float64).reshape(-1, 5)]
    S = len(cs)
    D = 2 * S
    A = np.zeros((D, D), L)
    for j in range(D):
        y1 = [L(0)] * S
        y2 = [L(0)] * S
        s, k = divmod(j, 2)
        if k == 0:
            y1[s] = L(1); y2[s] = L(1)          # value 1, difference 0
        else:
            y2[s] = L(-1)                       # value 0, difference 1
        _cascade(cs, L(0), L(0), L(0), y1, y2)
        for i in range(S):
            A[2 * i, j] = y1[i]
            A[2 * i + 1, j] = y1[i] - y2[i]
    M = np.eye(D, dtype=L)
    for _ in range(R):
        M = A @ M
    out = []
    for _ in range(npow):
        out.append(M.astype(np.float64))
        M = M @ M
    return np.array(out)


def _mv(Mx, v):
    """o[..., i] = sum_j Mx[i][j] v[..., j], j ascending over the block-lower-triangular part (what the kernel's FMA chain does)"""
    D = Mx.shape[0]
    o = np.zeros_like(v)
    for i in range(D):
        acc = Mx[i, 0] * v[..., 0]
        for j in range(1, 2 * (i // 2) + 2):
            acc = acc + Mx[i, j] * v[..., j]
        o[..., i] = acc
    return o


def _run_chunks(coeffs, xs, xm1, xm2, st, out=None):
    """every chunk (rows of xs [n][R]) from its state st [n][D] with x history (xm1, xm2); returns the end states"""
    S = len(coeffs)
    y1 = [st[:, 2 * s].copy() for s in range(S)]
    y2 = [st[:, 2 * s] - st[:, 2 * s + 1] for s in range(S)]
    x1, x2 = xm1.copy(), xm2.copy()
    for i in range(xs.shape[1]):
        x0 = xs[:, i]
        w = _cascade(coeffs, x0, x1, x2, y1, y2)
        if out is not None:
            out[:, i] = w
        x2, x1 = x1, x0
    e = np.empty_like(st)
    for s in range(S):
        e[:, 2 * s] = y1[s]
        e[:, 2 * s + 1] = y1[s] - y2[s]
    return e


def scan(x, coeffs):
    """float64 restatement of eq.hip's evaluation order -> float64 u_S [N].  (Samples past N are zeros here and are not run in the
    kernel; they only feed states nothing reads.)"""
    xd = np.asarray(x, np.float32).astype(np.float64)
    coeffs = [tuple(c) for c in np.asarray(coeffs, np.float64).reshape(-1, 5)]
    N, S = xd.size, len(coeffs)
    if N == 0 or S == 0:
        return xd
    D = 2 * S
    Mp = chunk_map_powers(coeffs)
    nt = (N + TILE - 1) // TILE
    xp = np.zeros(nt * TILE)
    xp[:N] = xd
    xs = xp.reshape(nt * THREADS, R)
    h = np.concatenate([[0.0, 0.0], xp])
    xm1 = h[1:-1:R][: nt * THREADS].copy()          # x[n0 - 1]
    xm2 = h[0:-2:R][: nt * THREADS].copy()          # x[n0 - 2]
    # launch 1: zero-start end state of every chunk; inclusive scan within each wave of 64 chunks; the four waves in order
    e = _run_chunks(coeffs, xs, xm1, xm2, np.zeros((nt * THREADS, D)))
    P = e.reshape(nt, THREADS // 64, 64, D).copy()
    for d in range(6):
        o = 1 << d
        P[:, :, o:, :] = P[:, :, o:, :] + _mv(Mp[d], P[:, :, :-o, :].copy())
    Pex = np.zeros_like(P)
    Pex[:, :, 1:, :] = P[:, :, :-1, :]
    W = np.zeros((nt, D))
    Z = np.zeros((nt, THREADS // 64, 64, D))
    lane = np.arange(64)
    for w in range(THREADS // 64):
        Zw = np.repeat(W[:, None, :], 64, axis=1)
        for d in range(6):
            m = ((lane >> d) & 1).astype(bool)
            Zw[:, m, :] = _mv(Mp[d], Zw[:, m, :])
        Z[:, w] = Zw + Pex[:, w]
        W = _mv(Mp[6], W) + P[:, w, 63, :]
    E = W                                            # every tile's zero-start end state
    # launch 2: the tile carries in order, every chunk's carry-in, the true run
    St = np.zeros((nt, D))
    for t in range(1, nt):
        St[t] = _mv(Mp[8], St[t - 1]) + E[t - 1]
    C = np.repeat(St[:, None, :], THREADS, axis=1)
    tid = np.arange(THREADS)
    for d in range(8):
        m = ((tid >> d) & 1).astype(bool)
        C[:, m, :] = _mv(Mp[d], C[:, m, :])
    C = C + Z.reshape(nt, THREADS, D)
    y = np.empty((nt * THREADS, R))
    _run_chunks(coeffs, xs, xm1, xm2, C.reshape(nt * THREADS, D), y)
    return y.reshape(-1)[:N]


# the three filter sets of DESIGN.md 9j: (rate, bands)
FILTER_SETS = [
    (48000, [(HIGHPASS, 20.0, 0.0, 0.707), (PEAK, 100.0, 12.0, 8.0), (PEAK, 3000.0, -12.0, 8.0), (HIGHSHELF, 8000.0, 12.0, 0.707)]),
    (16000, [(PEAK, 20.0, 24.0, 8.0)]),
    (8000, [(HIGHPASS, 300.0, 0.0, 0.707), (LOWPASS, 3400.0, 0.0, 0.707), (PEAK, 1000.0, 24.0, 8.0), (LOWSHELF, 200.0, -24.0, 0.5)]),
]
