// join_stream.hpp -- the step geometry of a joined stream (sts_infer_ids_joined_stream).  Plain C++: no HIP, no engine type.
//
// The joined signal J has F_J frames of hop samples; sentence b holds the frames [s_b, s_b + F_b) of it.  With C = chunk_frames, step k
// delivers the frames [f0, f1) = [k C, min((k + 1) C, F_J)) of J.  The resampler and the limiter reach Ho frames beyond a chunk's edges, the
// decoder Hd frames beyond whatever it is asked for, so a step
//   joins the J window [g0, g1) = [max(0, f0 - Ho), min(F_J, f1 + Ho)), and
//   decodes, of every sentence that meets it, the local frames [max(0, g0 - s_b - Hd), min(F_b, g1 - s_b + Hd)),
// the windows packed back to back in sentence order.  A step whose J window meets no sentence has no window: nothing is decoded.
// The output ranges are those of one utterance of N_J = F_J hop samples: the kept outputs [j0, j1) = [ceil(f0 hop P / Q), ceil(f1 hop P / Q))
// and, with a limiter of look-ahead H, the float range [jl0, jl1) = [j0 - 2H, j1 + 2H) clipped to [0, L_out).
#pragma once

#include <algorithm>
#include <vector>

namespace sts {

// one decode window: sentence b's local frames [w0, w1) at frame coff of the step's compact decode
struct JsWin { int b; long long w0, w1, coff; };
// a row of the windowed join's table, in samples: J[st, en) is sentence samples [st - S, en - S) of N, read from x[xoff + (i - S)]
struct JsRow { long long st, en, S, N, xoff; };

struct JsStep {
    long long f0 = 0, f1 = 0, g0 = 0, g1 = 0;
    long long j0 = 0, j1 = 0, jl0 = 0, jl1 = 0;
    long long Wtot = 0, maxW = 0;       // summed and longest window, in frames
    std::vector<JsWin> win;
};

struct JsPlan {
    std::vector<long long> s, F;        // sentence b: first frame in J, frames
    long long FJ = 0;                   // frames of J
    int hop = 1;
    long long C = 1;                    // chunk frames
    int Hd = 0, Ho = 0;                 // decoder halo; the resampler's and the limiter's reach, in frames
    long long P = 1, Q = 1;             // output rate / native rate in lowest terms (1 / 1: native)
    int H = 0;                          // limiter look-ahead in output samples (0: no limiter)

    // the layout of sts_join_layout in frames: sil[b] = silence in front of sentence b, total_sil = lead + every gap + trail
    void layout(int B, const int* frames, const long long* sil, long long total_sil) {
        s.resize((size_t)B); F.resize((size_t)B);
        long long acc = 0;
        for (int b = 0; b < B; b++) { s[b] = acc + sil[b]; F[b] = frames[b]; acc += frames[b]; }
        FJ = acc + total_sil;
    }
    long long out_count(long long native) const { return (native * P + Q - 1) / Q; }
    long long steps() const { return (FJ + C - 1) / C; }
    // the windows of the J frames [g0, g1) with a decoder halo of hd frames, appended to `out` (sentence ends ascend: a binary search
    // finds the first sentence that ends behind g0)
    void windows(long long g0, long long g1, int hd, std::vector<JsWin>& out, long long* Wtot, long long* maxW) const {
        const int B = (int)s.size();
        int lo = 0, hi = B;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s[mid] + F[mid] > g0) hi = mid; else lo = mid + 1;
        }
        long long tot = 0, mx = 0;
        for (int b = lo; b < B && s[b] < g1; b++) {
            const long long w0 = std::max<long long>(0, g0 - s[b] - hd), w1 = std::min<long long>(F[b], g1 - s[b] + hd);
            out.push_back(JsWin{b, w0, w1, tot});
            tot += w1 - w0; mx = std::max(mx, w1 - w0);
        }
        if (Wtot) *Wtot = tot;
        if (maxW) *maxW = mx;
    }
    void step(long long k, JsStep& t) const {
        t.f0 = k * C; t.f1 = std::min(FJ, t.f0 + C);
        t.g0 = std::max<long long>(0, t.f0 - Ho); t.g1 = std::min(FJ, t.f1 + Ho);
        const long long Nout = out_count(FJ * hop);
        t.j0 = out_count(t.f0 * hop); t.j1 = out_count(t.f1 * hop);
        t.jl0 = H ? std::max<long long>(0, t.j0 - 2LL * H) : t.j0; t.jl1 = H ? std::min(Nout, t.j1 + 2LL * H) : t.j1;
        t.win.clear();
        windows(t.g0, t.g1, Hd, t.win, &t.Wtot, &t.maxW);
    }
    // the decoder's frame workspace: the most frames one step decodes.  Host cost: one pass over the steps that decode anything (a run of
    // silent steps is skipped in one move) with a binary search and its windows each -- with C = 1 that is one iteration per frame of
    // every sentence and its reach, before the first chunk leaves
    long long workspace() const {
        JsStep t;
        long long w = 0;
        const int B = (int)s.size();
        for (long long k = 0, n = steps(); k < n; k++) {
            step(k, t);
            w = std::max(w, t.Wtot);
            if (!t.win.empty()) continue;
            // silence: on to the first step whose J window reaches the next sentence (none: done)
            int b = 0;
            while (b < B && s[b] < t.g1) b++;
            if (b == B) break;
            k = std::max(k, (s[b] - Ho) / C - 1);
        }
        return w;
    }
    // frames of the J window buffer: a chunk and the reach on both sides (never more than J)
    long long window_frames() const { return std::min(FJ, std::min(C, FJ) + 2LL * Ho); }
    // the join's table for the J frames [g0, g1) and their windows
    void rows(long long g0, long long g1, const std::vector<JsWin>& win, std::vector<JsRow>& out) const {
        out.clear();
        for (const JsWin& w : win) {
            const long long a = std::max(g0, s[w.b]), e = std::min(g1, s[w.b] + F[w.b]);
            out.push_back(JsRow{a * hop, e * hop, s[w.b] * hop, F[w.b] * hop, (w.coff - w.w0) * hop});
        }
    }
};

}  // namespace sts
