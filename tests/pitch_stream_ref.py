"""A stream through the pitch warp restated in Python integers (DESIGN.md 9l "Streamed"; summertts_amd/csrc/pitch_stream.hpp and the warped
step of stream_step.hpp): which warped outputs a chunk of decoder frames owns, what the stages behind the warp and the warp itself read
for them, the halo, and the rows of a step.  Built on pitch_ref: nothing here calls the library."""
import bisect

import pitch_ref as pr

MAX_K = 51
STEP_MIN, STEP_MAX = 3037000500, 6074001000


class Utt:
    """One utterance as the warp sees it.  cents None: the member without a plan (N' = N, pos(j) = j << 32)."""

    def __init__(self, d, cents, hop):
        self.d, self.hop = [int(v) for v in d], hop
        self.F = max(1, sum(self.d))
        self.N = self.F * hop
        self.planned = cents is not None
        if self.planned:
            self.step_in = pr.design(cents)[1]
            self.o, self.e, self.a, self.step = pr.rows(self.d, self.step_in, hop)
            self.Nw = self.o[-1]
        else:
            self.Nw = self.N

    def pos(self, j):
        if not self.planned:
            return j << 32
        i = bisect.bisect_right(self.o, j, 1) - 1           # the phoneme with o[i] <= j < o[i + 1] (one that emits nothing is never it)
        return (self.a[i] << 32) + self.e[i] + (j - self.o[i]) * self.step[i]

    def Y(self, s):
        """outputs j with pos(j) < s << 32"""
        if not self.planned:
            return min(s, self.N)
        lo, hi, lim = 0, self.Nw, s << 32
        while lo < hi:
            mid = (lo + hi) >> 1
            if self.pos(mid) < lim:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def Y_slow(self, s):
        """the definition, from every output's position (small utterances)"""
        if not self.planned:
            return min(s, self.N)
        return sum(1 for p in pr.positions(self.d, self.step_in, self.hop) if p < (s << 32))


def out_count(n, P, Q):
    return n if P == Q else -((-n * P) // Q)


def extra(K, H, P, Q):
    """what the stages behind the warp read beyond a chunk, in warped samples: the resampler's K (0: off) and the limiter's reach"""
    return K + ((2 * H * Q + P - 1) // P + 1 if H > 0 else 0)


def halo(dec_halo, ext, hop):
    reach = -((-ext * STEP_MAX) >> 32) + MAX_K + 1
    return dec_halo + -(-reach // hop)


def cap(wmax, hop):
    return ((wmax * hop) << 32) // STEP_MIN + 2


def window(u, f0, C, hl, P, Q, H, K):
    hop, F = u.hop, u.F
    w = {"f0": f0, "f1": min(F, f0 + C)}
    w["w0"], w["w1"] = max(0, f0 - hl), min(F, w["f1"] + hl)
    w["y0"], w["y1"] = u.Y(f0 * hop), u.Y(w["f1"] * hop)
    w["j0"], w["j1"], w["Nout"] = out_count(w["y0"], P, Q), out_count(w["y1"], P, Q), out_count(u.Nw, P, Q)
    w["jl0"] = max(0, w["j0"] - 2 * H) if H > 0 else w["j0"]
    w["jl1"] = min(w["Nout"], w["j1"] + 2 * H) if H > 0 else w["j1"]
    yl0 = yl1 = w["y0"]
    if w["jl1"] > w["jl0"]:
        if K > 0:
            a, b = max(0, w["jl0"] * Q // P - K + 1), min(u.Nw, (w["jl1"] - 1) * Q // P + K + 1)
        else:
            a, b = w["jl0"], w["jl1"]
        if b > a:
            yl0, yl1 = a, b
    w["yl0"], w["yl1"] = yl0, yl1
    w["c0"], w["c1"] = staged(u, yl0, yl1)
    return w


def staged(u, yl0, yl1):
    """the input samples the warp reads for [yl0, yl1), clipped to the utterance"""
    if yl1 <= yl0:
        return 0, 0
    if not u.planned:
        return yl0, yl1
    return max(0, (u.pos(yl0) >> 32) - MAX_K + 1), min(u.N, (u.pos(yl1 - 1) >> 32) + MAX_K + 1)


def chunk_starts(u, C):
    """Y(k C) for every chunk and N'"""
    return [u.Y(k * C * u.hop) for k in range(-(-u.F // C))] + [u.Nw]


def chunks(u, C, P, Q):
    """(first output, count) of every chunk at the output rate, empty ones included"""
    ys = chunk_starts(u, C)
    js = [out_count(y, P, Q) for y in ys]
    return [(js[k], js[k + 1] - js[k]) for k in range(len(js) - 1)]


def step_rows(utts, live, k, C, hl, hop, P, Q, H, K, srs, slim, zoff, sid):
    """The words of step k over the utterances `live`, as step_build_warped writes them: per window (ints6, RsRow, LimRow, PsRow, seg2),
    and the step's totals (Wtot, maxW, dsum, ysum, max_rs, max_out, max_yl)"""
    rsum = dsum = ysum = Wtot = 0
    rows, mx = [], [0, 0, 0, 0]
    for b in live:
        u = utts[b]
        g = window(u, k * C, C, hl, P, Q, H, K if srs else 0)
        wlen = g["w1"] - g["w0"]
        nrs, nout, nyl = g["jl1"] - g["jl0"], g["j1"] - g["j0"], g["yl1"] - g["yl0"]
        ints = [zoff[b] + g["w0"], Wtot, wlen, sid[b], 0, dsum]
        rs = [g["yl0"], u.Nw, g["jl0"], g["jl1"], rsum if slim else dsum]
        lim = [rsum if srs else ysum, g["jl0"] if srs else g["yl0"], nrs if srs else nyl, g["Nout"], g["j0"], g["j1"], dsum]
        ps = [Wtot * hop, g["w0"] * hop, wlen * hop, b, g["yl0"], g["yl1"], ysum, g["y0"], g["y1"], dsum]
        rows.append((ints, rs, lim, ps, [ysum, nyl], g))
        rsum += nrs
        dsum += nout
        ysum += nyl
        Wtot += wlen
        mx = [max(mx[0], wlen), max(mx[1], nrs), max(mx[2], nout), max(mx[3], nyl)]
    return rows, [Wtot, mx[0], dsum, ysum, mx[1], mx[2], mx[3]]


def cut_ranges(u, edges):
    """[0, N') cut at `edges` -> the windows (u0, xlen, y0, y1) that hold exactly each range's staged span"""
    e = sorted(set([0, u.Nw] + [int(v) for v in edges if 0 <= v <= u.Nw]))
    out = []
    for y0, y1 in zip(e[:-1], e[1:]):
        c0, c1 = staged(u, y0, y1)
        out.append((c0, c1 - c0, y0, y1))
    return out
