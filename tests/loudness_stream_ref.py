"""Float64 restatement of the TILED order in which loudness.hip measures: the K-weighting cascade of the definition run as
a scan over chunks of R samples, one per lane, 4 waves of 64 lanes per tile of TILE samples, tiles composed in order, everything anchored
at the utterance's first sample; y^2 summed per 100 ms sub-block into the slots of each tile with a fixed tree, max |x| per tile; then
the gate over the tiles' sums.  Two forms: `whole` evaluates a complete signal tile by tile; `Stream` is the CARRIED-STATE form of
sts_set_loudness_streaming -- between two steps it keeps only the position e up to which input has been consumed, the carry S_t of the
open tile (the tile that holds e), that tile's input so far with the two samples in front of it, and the sums and peak of every tile
(the open tile's provisional).  A step re-runs the open tile's prefix in the scan's order (a chunk's carry-in reads the chunks in front
of it only) and continues.  Written from the definition with loudness_ref's coefficients, not from the library."""
import numpy as np

import loudness_ref

R, THREADS, TILE, SLOTS = 32, 256, 8192, 16
WAVES = THREADS // 64


class Coef:
    """the filter of a rate, S = samples per 100 ms sub-block, Mp[d] = M^(2^d) for the chunk map M = A^R"""

    def __init__(self, fs):
        self.fs = fs
        self.c = loudness_ref.coeffs10(fs)
        self.S = loudness_ref.sub_block(fs)
        c = self.c
        A = np.array([[-c[3], -c[4], 0.0, 0.0],
                      [1.0, 0.0, 0.0, 0.0],
                      [c[6] - c[5] * c[3], c[7] - c[5] * c[4], -c[8], -c[9]],
                      [0.0, 0.0, 1.0, 0.0]])
        M = A.copy()
        for _ in range(R - 1):
            M = _mm(A, M)
        self.Mp = [M]
        for _ in range(8):
            self.Mp.append(_mm(self.Mp[-1], self.Mp[-1]))


def _mm(a, b):
    o = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += a[i, k] * b[k, j]
            o[i, j] = s
    return o


def _mv(M, v):
    """o = M v for v [..., 4], a fixed order per row (no BLAS: the bits must not depend on the batch's shape)"""
    v = np.asarray(v, np.float64)
    return np.stack([((M[i, 0] * v[..., 0] + M[i, 1] * v[..., 1]) + M[i, 2] * v[..., 2]) + M[i, 3] * v[..., 3] for i in range(4)], axis=-1)


def _mpow(k, n, v, bits):
    """v[i] = M^n[i] v[i], n's bits lowest first"""
    v = v.copy()
    for d in range(bits):
        m = ((n >> d) & 1).astype(bool)
        if m.any():
            v[m] = _mv(k.Mp[d], v[m])
    return v


def _run_chunks(k, xs, r, xm1, xm2, s, split=None):
    """The cascade over every lane's chunk xs[lane, :r[lane]] from state s [lanes, 4] with input history (xm1, xm2) -> (end states, acc0,
    acc1): with split, the squares of the K-weighted output are summed in order into acc0 for the chunk's first split[lane] samples, into
    acc1 for the rest."""
    c = k.c
    x1, x2 = xm1.astype(np.float64).copy(), xm2.astype(np.float64).copy()
    y1a, y1b, y2a, y2b = (s[:, i].copy() for i in range(4))
    acc0, acc1 = np.zeros(xs.shape[0]), np.zeros(xs.shape[0])
    for i in range(R):
        on = i < r
        if not on.any():
            break
        x0 = xs[:, i]
        y1 = c[0] * x0 + c[1] * x1 + c[2] * x2 - c[3] * y1a - c[4] * y1b
        y2 = c[5] * y1 + c[6] * y1a + c[7] * y1b - c[8] * y2a - c[9] * y2b
        if split is not None:
            sq = y2 * y2
            acc0 = np.where(on & (i < split), acc0 + sq, acc0)
            acc1 = np.where(on & (i >= split), acc1 + sq, acc1)
        x2, x1 = np.where(on, x1, x2), np.where(on, x0, x1)
        y1b, y1a = np.where(on, y1a, y1b), np.where(on, y1, y1a)
        y2b, y2a = np.where(on, y2a, y2b), np.where(on, y2, y2a)
    return np.stack([y1a, y1b, y2a, y2b], axis=1), acc0, acc1


def _tile(k, xt, prev, St, t):
    """Tile t holding its first n <= TILE samples xt (float64; zeros stand behind them), the two samples in front of it prev = (x[t0 - 1],
    x[t0 - 2]) and its carry St -> (E, tsum [SLOTS], tpeak): the scan's order; E, the tile's zero-start end state, means something
    only for n == TILE; the sums and the peak are those of an utterance that ends with xt's last sample."""
    n = xt.size
    assert 0 < n <= TILE
    xp = np.zeros(TILE)
    xp[:n] = xt
    xs = xp.reshape(THREADS, R)
    tid = np.arange(THREADS)
    r = np.clip(n - tid * R, 0, R)
    h = np.concatenate([[prev[1], prev[0]], xp])
    xm1 = np.where(r > 0, h[1:-1:R][:THREADS], 0.0)
    xm2 = np.where(r > 0, h[0:-2:R][:THREADS], 0.0)
    e, _, _ = _run_chunks(k, xs, r, xm1, xm2, np.zeros((THREADS, 4)))
    # inclusive scan within each wave, then the waves in order
    P = e.reshape(WAVES, 64, 4).copy()
    for d in range(6):
        o = 1 << d
        P[:, o:, :] = P[:, o:, :] + _mv(k.Mp[d], P[:, :-o, :].copy())
    Pex = np.zeros_like(P)
    Pex[:, 1:, :] = P[:, :-1, :]
    W = np.zeros(4)
    Z = np.zeros((WAVES, 64, 4))
    lane = np.arange(64)
    for w in range(WAVES):
        Z[w] = _mpow(k, lane, np.repeat(W[None, :], 64, axis=0), 6) + Pex[w]
        W = _mv(k.Mp[6], W) + P[w, 63, :]
    C = _mpow(k, tid, np.repeat(np.asarray(St, np.float64)[None, :], THREADS, axis=0), 8) + Z.reshape(THREADS, 4)
    # the true run, y^2 into the lane's two sub-blocks
    S = k.S
    t0 = t * TILE
    n0 = t0 + tid * R
    sb0 = t0 // S
    bin0 = n0 // S
    split = (bin0 + 1) * S - n0
    _, acc0, acc1 = _run_chunks(k, xs, r, xm1, xm2, C, split)
    tend = t0 + n - 1
    nslots = tend // S - sb0 + 1
    s0 = bin0 - sb0
    tsum = np.zeros(SLOTS)
    for s in range(min(nslots, SLOTS)):
        v = np.where(r > 0, np.where(s == s0, acc0, np.where(s == s0 + 1, acc1, 0.0)), 0.0).reshape(WAVES, 64)
        for o in (32, 16, 8, 4, 2, 1):                       # the butterfly of wave_sum: lane 0 holds the wave's sum
            v = v + v[:, lane ^ o]
        tsum[s] = ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]
    tpeak = np.float32(np.abs(xt.astype(np.float32)).max())
    return W, tsum, tpeak


def whole(x, k):
    """The whole signal -> (tsum [tiles][SLOTS], tpeak [tiles]) with tiles = ceil(N / TILE)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    N = x.size
    nt = (N + TILE - 1) // TILE
    tsum, tpeak = np.zeros((nt, SLOTS)), np.zeros(nt, np.float32)
    St = np.zeros(4)
    for t in range(nt):
        t0 = t * TILE
        prev = (x[t0 - 1] if t0 >= 1 else 0.0, x[t0 - 2] if t0 >= 2 else 0.0)
        E, tsum[t], tpeak[t] = _tile(k, x[t0:t0 + TILE], prev, St, t)
        St = _mv(k.Mp[8], St) + E
    return tsum, tpeak


class Stream:
    """The carried state of one utterance of N samples, its result tables and its steps."""

    def __init__(self, k, N):
        self.k = k
        self.e = 0
        self.St = np.zeros(4)
        self.prev = (0.0, 0.0)
        self.xt = np.zeros(0)            # the open tile's input so far: samples [e // TILE * TILE, e)
        nt = N // TILE + 1
        self.tsum, self.tpeak = np.full((nt, SLOTS), np.nan), np.full(nt, np.nan, np.float32)

    def step(self, xwin, u0, j1):
        """xwin: float32 input samples [u0, u0 + len) of the utterance.  Consumes [e, j1), each sample once."""
        xwin = np.asarray(xwin, np.float32).astype(np.float64)
        e = self.e
        assert u0 <= e <= j1 <= u0 + xwin.size
        t = e // TILE
        x = np.concatenate([self.xt, xwin[e - u0:j1 - u0]])        # samples [t TILE, j1)
        St, prev, pos = self.St, self.prev, 0
        while True:
            seg = x[pos:pos + TILE]
            if seg.size:
                E, self.tsum[t], self.tpeak[t] = _tile(self.k, seg, prev, St, t)
            if seg.size < TILE:
                break                    # the tile that holds j1: the open tile of the next step
            St = _mv(self.k.Mp[8], St) + E
            prev = (seg[-1], seg[-2])
            pos += TILE
            t += 1
        self.e, self.St, self.prev, self.xt = j1, St, prev, seg.copy()


def chunked(x, k, bounds, back=0):
    """One utterance through steps [bounds[i], bounds[i + 1]) (the last: to the end), each presenting the window widened by `back` on
    either side -> (tsum, tpeak) of the tiles ceil(N / TILE) the whole form has."""
    x = np.asarray(x, np.float32)
    N = x.size
    bounds = [int(b) for b in bounds]
    assert bounds and bounds[0] == 0 and all(b1 > b0 for b0, b1 in zip(bounds, bounds[1:]))
    st = Stream(k, N)
    for i, c0 in enumerate(bounds):
        if N <= c0:
            break
        last = i + 1 >= len(bounds)
        o0, o1 = max(0, c0 - back), N if last else min(N, bounds[i + 1] + back)
        st.step(x[o0:o1], o0, N if last else min(N, bounds[i + 1]))
    assert st.e == N
    nt = (N + TILE - 1) // TILE
    return st.tsum[:nt], st.tpeak[:nt]


def _lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def _reduce(v, n):
    """sum and count over the workgroup: lane tid takes the entries tid, tid + THREADS, ... in order, then a fixed tree"""
    sv, sn = np.zeros(THREADS), np.zeros(THREADS, np.int64)
    for j in range(v.size):
        sv[j % THREADS] += v[j]
        sn[j % THREADS] += n[j]
    o = THREADS // 2
    while o > 0:
        sv[:o] = sv[:o] + sv[o:2 * o]
        sn[:o] = sn[:o] + sn[o:2 * o]
        o //= 2
    return sv[0], int(sn[0])


def gate(tsum, tpeak, N, k, target=-16.0, ceiling=-1.0):
    """The blocks, both gates, L, the peak and the gain from the tiles' sums -> dict(lufs, peak, gain, blocks), lufs in float64."""
    S = k.S
    nsb = N // S
    nblk = nsb - 3 if nsb >= 4 else 0

    def sub(j):
        v = 0.0
        for t in range((j * S) // TILE, ((j + 1) * S - 1) // TILE + 1):
            v += tsum[t][j - (t * TILE) // S]
        return v
    z = np.array([(((sub(j) + sub(j + 1)) + sub(j + 2)) + sub(j + 3)) / (4.0 * S) for j in range(nblk)])
    L, n2 = -np.inf, 0
    if nblk:
        l = _lufs(z)
        keep = l > -70.0
        s1, n1 = _reduce(np.where(keep, z, 0.0), keep.astype(np.int64))
        if n1 > 0:
            gr = _lufs(s1 / n1) - 10.0
            fin = keep & (l > gr)
            s2, n2 = _reduce(np.where(fin, z, 0.0), fin.astype(np.int64))
            if n2 > 0:
                L = float(_lufs(s2 / n2))
    p = float(np.max(tpeak[:(N + TILE - 1) // TILE])) if N > 0 else 0.0
    return {"lufs": L, "peak": p, "gain": loudness_ref.gain(L, p, np.float32(target), np.float32(ceiling)),
            "blocks": n2 if np.isfinite(L) else 0}
