"""Float64 restatement of the equaliser's CARRIED-STATE evaluation (include/summertts_hip.h sts_set_eq_streaming): the
signal of an utterance is eq_ref.scan's -- the definition's cascade evaluated in chunks of R samples and tiles of TILE, anchored at
the first sample -- but produced step by step.  Between two steps only this is kept: the position e up to which input has been
consumed, the carry S_t of the open tile (the tile that holds e), that tile's input so far with the two samples in front of it, and
the last HIST samples of y.  A step re-runs the open tile's prefix in the scan's order (a chunk's carry-in reads the chunks in front of
it only) and continues; a tile that completes hands S_{t+1} = M^256 S_t + E_t on.  Written from that definition with eq_ref's helpers,
not from the library."""
import numpy as np

import eq_ref
from eq_ref import R, THREADS, TILE, _mv, _run_chunks

HIST = 4096          # y samples kept behind e (a step's range may reach back that far)


def _tile(coeffs, Mp, xt, prev, St):
    """One tile holding its first n <= TILE samples xt (float64), the two samples in front of it prev = (x[t0 - 1], x[t0 - 2]) and its
    carry St -> (y [n], E): the scan's order on the chunks that hold samples; E, the tile's zero-start end state, means something only
    for n == TILE."""
    n, D = xt.size, 2 * len(coeffs)
    if n == 0:
        return np.zeros(0), np.zeros(D)
    nc = (n + R - 1) // R
    xp = np.zeros(TILE)
    xp[:n] = xt
    xs = xp.reshape(THREADS, R)
    h = np.concatenate([[prev[1], prev[0]], xp])
    xm1 = h[1:-1:R][:THREADS].copy()
    xm2 = h[0:-2:R][:THREADS].copy()
    e = np.zeros((THREADS, D))          # (chunks without samples feed only states nothing reads)
    e[:nc] = _run_chunks(coeffs, xs[:nc], xm1[:nc], xm2[:nc], np.zeros((nc, D)))
    P = e.reshape(THREADS // 64, 64, D).copy()
    for d in range(6):
        o = 1 << d
        P[:, o:, :] = P[:, o:, :] + _mv(Mp[d], P[:, :-o, :].copy())
    Pex = np.zeros_like(P)
    Pex[:, 1:, :] = P[:, :-1, :]
    W = np.zeros(D)
    Z = np.zeros((THREADS // 64, 64, D))
    lane = np.arange(64)
    for w in range(THREADS // 64):
        Zw = np.repeat(W[None, :], 64, axis=0)
        for d in range(6):
            m = ((lane >> d) & 1).astype(bool)
            Zw[m, :] = _mv(Mp[d], Zw[m, :])
        Z[w] = Zw + Pex[w]
        W = _mv(Mp[6], W) + P[w, 63, :]
    C = np.repeat(np.asarray(St, np.float64)[None, :], THREADS, axis=0)
    tid = np.arange(THREADS)
    for d in range(8):
        m = ((tid >> d) & 1).astype(bool)
        C[m, :] = _mv(Mp[d], C[m, :])
    C = C + Z.reshape(THREADS, D)
    y = np.empty((nc, R))
    _run_chunks(coeffs, xs[:nc], xm1[:nc], xm2[:nc], C[:nc], y)
    return y.reshape(-1)[:n], W


class Stream:
    """The carried state of one utterance and its steps."""

    def __init__(self, coeffs, Mp=None):
        self.coeffs = [tuple(c) for c in np.asarray(coeffs, np.float64).reshape(-1, 5)]
        self.Mp = eq_ref.chunk_map_powers(self.coeffs) if Mp is None else Mp
        D = 2 * len(self.coeffs)
        self.e = 0
        self.St = np.zeros(D)
        self.prev = (0.0, 0.0)
        self.xt = np.zeros(0)            # the open tile's input so far: samples [e // TILE * TILE, e)
        self.yh = np.zeros(0)            # y of [e - yh.size, e), at most HIST samples

    def step(self, xwin, u0, o0, o1):
        """xwin: float32 input samples [u0, u0 + len) of the utterance; -> y [o0, o1) (float64).  Consumes [e, o1), each sample once."""
        xwin = np.asarray(xwin, np.float32).astype(np.float64)
        e = self.e
        assert u0 <= e <= o1 <= u0 + xwin.size and 0 <= o0 <= e and e - o0 <= HIST and o0 <= o1
        t0e = e // TILE * TILE
        x = np.concatenate([self.xt, xwin[e - u0:o1 - u0]])        # samples [t0e, o1)
        St, prev, pos, out = self.St, self.prev, 0, []
        while True:
            seg = x[pos:pos + TILE]
            y, E = _tile(self.coeffs, self.Mp, seg, prev, St)
            out.append(y)
            if seg.size < TILE:
                break                    # the tile that holds o1: the open tile of the next step
            St = _mv(self.Mp[8], St) + E
            prev = (seg[-1], seg[-2])
            pos += TILE
        ynew = np.concatenate(out)                                  # y of [t0e, o1)
        hs = e - self.yh.size                                       # the history's first sample
        redo = self.yh[max(0, t0e - hs):]                           # the open tile's prefix, evaluated again: the same bits
        assert np.array_equal(redo.view(np.int64), ynew[max(0, hs - t0e):e - t0e].view(np.int64))
        if t0e > hs:
            ynew = np.concatenate([self.yh[:t0e - hs], ynew])
            first = hs
        else:
            first = t0e
        assert o0 >= first
        res = ynew[o0 - first:o1 - first].copy()
        self.e, self.St, self.prev, self.xt = o1, St, prev, seg.copy()
        self.yh = ynew[-HIST:].copy() if ynew.size > HIST else ynew
        return res


def chunked(x, coeffs, bounds, back=0, Mp=None):
    """One utterance through steps [bounds[k], bounds[k + 1]) (the last: to the end), each presenting the window widened by `back` on
    either side -> (y [N] float64 assembled from the steps' own ranges, [(start, y of the whole window)] per step that takes part)."""
    x = np.asarray(x, np.float32)
    N = x.size
    bounds = [int(b) for b in bounds]
    assert bounds and bounds[0] == 0 and all(b1 > b0 for b0, b1 in zip(bounds, bounds[1:]))
    st = Stream(coeffs, Mp)
    y = np.full(N, np.nan)
    wins = []
    for k, c0 in enumerate(bounds):
        if N <= c0:
            break
        c1 = min(N, bounds[k + 1]) if k + 1 < len(bounds) else N
        o0, o1 = max(0, c0 - back), min(N, (bounds[k + 1] + back) if k + 1 < len(bounds) else N)
        w = st.step(x[o0:o1], o0, o0, o1)
        wins.append((o0, w))
        y[c0:c1] = w[c0 - o0:c1 - o0]
    return y, wins
