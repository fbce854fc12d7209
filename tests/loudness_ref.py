"""Float64 checker of loudness measurement and normalisation (include/summertts_hip.h sts_set_loudness): ITU-R BS.1770-4 integrated
loudness of one channel -- K-weighting from the analog prototypes, 400 ms blocks every 100 ms, absolute and relative gates -- the sample
peak, the gain rule and the reference's int16 cast.  Written from the definition with a plain sequential IIR, not from the library."""
import numpy as np

try:
    from scipy.signal import lfilter as _lfilter
except Exception:          # (a plain float64 loop where scipy is absent)
    _lfilter = None

ABS_GATE = -70.0


def kweight(fs):
    """-> (b_shelf[3], a_shelf[3], b_hp[3], a_hp[3]), float64"""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def coeffs10(fs):
    """the layout of sts_kweight_coeffs: {b0, b1, b2, a1, a2} of the shelf, then of the high-pass"""
    b1, a1, b2, a2 = kweight(fs)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def lfilter(b, a, x):
    x = np.asarray(x, np.float64)
    if _lfilter is not None:
        return _lfilter(b, a, x)
    y = np.zeros_like(x)
    x1 = x2 = y1 = y2 = 0.0
    for i, v in enumerate(x):
        o = b[0] * v + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
        x2, x1, y2, y1 = x1, v, y1, o
        y[i] = o
    return y


def k_filter(x, fs):
    b1, a1, b2, a2 = kweight(fs)
    return lfilter(b2, a2, lfilter(b1, a1, x))


def sub_block(fs):
    return int(np.floor(fs / 10.0 + 0.5))


def block_energies(x, fs):
    """z_j of every complete 400 ms block"""
    y = k_filter(x, fs)
    S = sub_block(fs)
    n = y.size
    if n < 4 * S:
        return np.zeros(0)
    nb = (n - 4 * S) // S + 1
    sq = y * y
    return np.array([sq[j * S: j * S + 4 * S].sum() / (4 * S) for j in range(nb)])


def _lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def measure(x, fs):
    """-> (L (float64, -inf when unmeasured), blocks in the final set)"""
    z = block_energies(x, fs)
    if z.size == 0:
        return -np.inf, 0
    l = _lufs(z)
    keep = l > ABS_GATE
    if not keep.any():
        return -np.inf, 0
    gr = _lufs(z[keep].mean()) - 10.0
    fin = keep & (l > gr)
    if not fin.any():
        return -np.inf, 0
    return float(_lufs(z[fin].mean())), int(fin.sum())


def peak(x):
    x = np.asarray(x, np.float32)
    return float(np.abs(x).max()) if x.size else 0.0


def gain(L, p, target, ceiling):
    """float64 gain rule, rounded to float32"""
    gl = 10.0 ** ((float(target) - L) / 20.0) if np.isfinite(L) else 1.0
    g = min(gl, 10.0 ** (float(ceiling) / 20.0) / p) if p > 0 else gl
    return np.float32(g)


def loudness(x, fs, target=-16.0, ceiling=-1.0):
    """-> dict(lufs, peak, gain, blocks) as sts_loudness reports them"""
    L, n = measure(x, fs)
    p = peak(x)
    return {"lufs": L, "peak": p, "gain": gain(L, p, np.float32(target), np.float32(ceiling)), "blocks": n}


def pcm_cast(y):
    """The reference's (int16)(int32)(y * 32737) on x86-64: truncation toward zero, wrap-around, out-of-int32 -> 0 (devmath.hpp)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(y, np.float32) * np.float32(32737.0)).astype(np.float64)
        v = np.nan_to_num(v, nan=2.0 ** 40)
    q = np.where(np.abs(v) < 2.0 ** 31, np.trunc(v), -2.0 ** 31).astype(np.int64)
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)


def normalize(x, g):
    """mode 2's PCM: one fp32 multiply in front of the cast"""
    return pcm_cast(np.asarray(x, np.float32) * np.float32(g))
