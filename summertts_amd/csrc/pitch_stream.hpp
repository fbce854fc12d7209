// pitch_stream.hpp -- the geometry of a stream through the pitch warp (sts_set_pitch_streaming; DESIGN.md 9l "Streamed"): which warped
// outputs a chunk of decoder frames owns, which warped samples the stages behind the warp read for them, which input samples the warp
// stages for those, and the halo that keeps all of them inside the decode window.  Exact 64-bit integers on the rows pitch_tables
// computes per utterance.  Plain C++: no HIP, no engine type (tests/pitch_stream_check.cpp compiles it alone).
//
// pos(j) is the Q32 input position of warped output j; it increases strictly over the utterance, and consecutive outputs are at most
// kPitchStepMax / 2^32 < 1.4143 samples apart.  Y(s) = #{j : pos(j) < s << 32}: the outputs in front of input sample s; Y(N) = N'.
// Chunk k of an utterance of F frames (the chunk grid stays the decoder's) owns the warped outputs [y0, y1) = [Y(k C hop),
// Y(min(F, (k + 1) C) hop)) and, at the output rate P / Q, [j0, j1) = [ceil(y0 P / Q), ceil(y1 P / Q)) of Nout = ceil(N' P / Q): the
// chunks partition [0, Nout) in order.  [jl0, jl1) is the limiter's widening by 2H; [yl0, yl1) the warped samples the stages behind the
// warp read for [jl0, jl1): the resampler's K taps on either side, or [jl0, jl1) itself; the warp stages the input samples
// [n0(yl0) - kPitchMaxK + 1, n0(yl1 - 1) + kPitchMaxK], n0 = pos >> 32.
//
// The halo.  Let extra = the resampler's K plus the limiter's reach in native samples (Engine::stream_halo) -- what [yl0, yl1) lies beyond
// [y0, y1) at most, in WARPED samples.  pos(y0) >= f0 hop and pos(y1 - 1) < f1 hop by the definition of Y, and going back (forward) by
// extra outputs moves pos by at most extra kPitchStepMax; the taps reach kPitchMaxK further, and the floor of n0 one more.  So with
//   halo = dec_halo + ceil((ceil(extra kPitchStepMax / 2^32) + kPitchMaxK + 1) / hop)
// every staged input sample lies at least dec_halo frames inside the decode window [w0, w1) or outside the utterance: it is the one-pass
// decode's sample, bit for bit under a pinned conv mode.  pitch_window_check proves it per window.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "live_stream.hpp"
#include "pitch_layout.hpp"

namespace sts {

// one utterance as the warp's tables hold it (kernels.hpp PitchTables::words): rows == 0 is a member without a plan (N' = N, pos(j) = j << 32)
struct PsUtt { const long long *oend, *pos0, *step; int rows; long long N, Nw; };
static inline PsUtt ps_utt(const long long* words, int B, long long TT, int b) {
    const long long* m = words + 6 * (size_t)b; const long long* oend = words + 6 * (size_t)B;
    return PsUtt{oend + m[4], oend + TT + m[4], oend + 2 * TT + m[4], (int)m[5], m[1], m[3]};
}
// pos(j), 0 <= j < N'
static inline long long ps_pos(const PsUtt& u, long long j) {
    if (u.rows == 0) return j << 32;
    int l = 0, r = u.rows - 1;
    while (l < r) { const int mid = (l + r) >> 1; if (u.oend[mid] > j) r = mid; else l = mid + 1; }
    return u.pos0[l] + (j - (l ? u.oend[l - 1] : 0)) * u.step[l];
}
// Y(s): the outputs in front of input sample s (0 <= s <= N)
static inline long long ps_Y(const PsUtt& u, long long s) {
    if (u.rows == 0) return std::min(s, u.N);
    const long long lim = s << 32;
    long long lo = 0, hi = u.Nw;        // the first j with pos(j) >= lim
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (ps_pos(u, mid) < lim) lo = mid + 1; else hi = mid; }
    return lo;
}

// the halo of a warped stream, in frames (the derivation above); extra as Engine::stream_halo sums it
static inline long pitch_stream_halo(long dec_halo, long long extra, long hop) {
    const long long reach = (long long)(((__int128)extra * kPitchStepMax + (kPitchOne - 1)) >> 32) + kPitchMaxK + 1;
    return dec_halo + (long)((reach + hop - 1) / hop);
}
// the most warped samples one window of at most wmax frames emits (sizing of the step's warped buffer); clip to N' where it is known
static inline long long pitch_stream_cap(long long wmax, long hop) {
    return (long long)((((__int128)wmax * hop) << 32) / kPitchStepMin) + 2;
}

// the window of chunk frames [f0, min(F, f0 + C)): stream_window's with Y in place of f hop.  K: the resampler's reach (0: it is off).
// [s0, s1): the staged input samples, not clipped (empty with [yl0, yl1))
struct PsWin { long f0, f1, w0, w1; long long y0, y1, j0, j1, jl0, jl1, yl0, yl1, Nw, Nout, s0, s1; };
static inline PsWin pitch_window(const PsUtt& u, long F, long f0, long C, long halo, long hop, long long P, long long Q, long long H, long long K) {
    PsWin w{};
    w.f0 = f0; w.f1 = std::min<long>(F, f0 + C);
    w.w0 = std::max<long>(0, f0 - halo); w.w1 = std::min<long>(F, w.f1 + halo);
    w.Nw = u.Nw;
    w.y0 = ps_Y(u, (long long)f0 * hop); w.y1 = ps_Y(u, (long long)w.f1 * hop);
    w.j0 = stream_out_count(w.y0, P, Q); w.j1 = stream_out_count(w.y1, P, Q);
    w.Nout = stream_out_count(u.Nw, P, Q);
    w.jl0 = H > 0 ? std::max<long long>(0, w.j0 - 2 * H) : w.j0; w.jl1 = H > 0 ? std::min<long long>(w.Nout, w.j1 + 2 * H) : w.j1;
    if (w.jl1 <= w.jl0) { w.yl0 = w.yl1 = w.y0; return w; }
    if (K > 0) { w.yl0 = std::max<long long>(0, w.jl0 * Q / P - K + 1); w.yl1 = std::min<long long>(u.Nw, (w.jl1 - 1) * Q / P + K + 1); }
    else { w.yl0 = w.jl0; w.yl1 = w.jl1; }
    if (w.yl1 <= w.yl0) { w.yl0 = w.yl1 = w.y0; return w; }
    w.s0 = (ps_pos(u, w.yl0) >> 32) - kPitchMaxK + 1; w.s1 = (ps_pos(u, w.yl1 - 1) >> 32) + kPitchMaxK + 1;
    if (u.rows == 0) { w.s0 = w.yl0; w.s1 = w.yl1; }      // (a copy reads its own sample)
    return w;
}
// the staged span [s0, s1) of the outputs [yl0, yl1), clipped to the utterance
static inline void pitch_staged(const PsUtt& u, long long yl0, long long yl1, long long* c0, long long* c1) {
    if (yl1 <= yl0) { *c0 = *c1 = 0; return; }
    if (u.rows == 0) { *c0 = yl0; *c1 = yl1; return; }
    *c0 = std::max<long long>(0, (ps_pos(u, yl0) >> 32) - kPitchMaxK + 1);
    *c1 = std::min<long long>(u.N, (ps_pos(u, yl1 - 1) >> 32) + kPitchMaxK + 1);
}
// Null, or why the window cannot run: every staged sample inside the utterance lies at least dec_halo frames inside [w0, w1) (an edge
// of the utterance needs no margin)
static inline const char* pitch_window_check(const PsUtt& u, const PsWin& w, long F, long hop, long dec_halo) {
    if (w.yl1 > w.yl0) {
        const long long c0 = std::max<long long>(0, w.s0), c1 = std::min<long long>(u.N, w.s1);
        const long long lo = w.w0 > 0 ? (long long)(w.w0 + dec_halo) * hop : 0, hi = w.w1 < F ? (long long)(w.w1 - dec_halo) * hop : u.N;
        if (c0 < lo || c1 > hi) return "pitch stream: the warp's input span leaves the decoded window's interior (the halo is too small)";
    }
    return nullptr;
}

// a window as the range warp reads it (PitchArgs::rows): x[xbase ..) holds the native samples [u0, u0 + xlen) of member `mem`; the
// outputs [yl0, yl1) go to y[ybase ..), and of them [y0, y1) as int16 to pcm[pbase ..) when the warp writes the PCM.  (The gain kernel
// reads u0 of this row in a warped step: the window's RsRow then describes the warped window.)
struct PsRow { long long xbase, u0, xlen, mem, yl0, yl1, ybase, y0, y1, pbase; };
static_assert(sizeof(PsRow) == 10 * 8, "table row");

}  // namespace sts
