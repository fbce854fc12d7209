// stream_step.hpp -- the tables of one step of a stream (Engine::run_stream_steps): the one definition of their layout, the
// rows the host writes, and the builders that fill a step's tables from its windows.  Plain C++: no HIP, no engine type
// (tests/stream_step_check.cpp compiles it alone).
//
// One step decodes nw windows and uploads one table for them (RunCtx::d_win points at it).  Its sections, in order:
//   ints  [zoff nw | coff nw | wlen nw | sid nw | pack source nw | packed destination nw + 1]   (the last word: the step's samples in all)
//   from the next 8-byte boundary: the resampler's rows, RsRow [nw]; behind them the limiter's, LimRow [nw]
//   a run with a gain plan: each window's utterance, ints [nw] (GainArgs::utt; the gain kernel takes u0 from the window's RsRow) -- in a
//   planned open stream its slot, as the sid column then holds it (StepWin::tab)
//   a plain stream, from the next 8-byte boundary each: the EQ's rows, EqsRow [nw]; loudness' rows, LdsRow [nw]
//   a joined stream, from the next 8-byte boundary: the ONE window of J for the resampler (RsRow) and the limiter (LimRow), the windowed
//   join's rows, JsRow [nw], the one EqsRow of J, the one LdsRow of J
//   a stream through the pitch warp (pitch_stream.hpp), from the next 8-byte boundary: the range warp's rows, PsRow [nw]; behind them the
//   windows' places in the step's warped float buffer, ints [offset nw | length nw] (the SegView at scale 1 of everything behind the warp)
// A section exists only in a run that reads it (gain, eq, loud, pitch); the sections in front of it lie where they lie without it.
#pragma once
#include <stddef.h>
#include <string.h>

#include "eq_stream.hpp"
#include "join_stream.hpp"
#include "live_stream.hpp"
#include "loud_stream.hpp"
#include "out_chain.hpp"
#include "pitch_stream.hpp"

namespace sts {

// a window as the resampler reads it (ResampleArgs::wtab): it holds the utterance's native samples [u0, u0 + len) of L, and its outputs
// [j0, j1) go to the packed destination from obase on.  (The gain kernel reads u0 of the same row.)
struct RsRow { long long u0, L, j0, j1, obase; };
static_assert(sizeof(RsRow) == 5 * 8, "table row");
// a window as the limiter reads it (LimArgs::wtab): x[xbase .. xbase + xlen) holds the samples [u0, u0 + xlen) of an utterance of N,
// and the outputs [j0, j1) go to y / pcm[dst ..)
struct LimRow { long long xbase, u0, xlen, N, j0, j1, dst; };
static_assert(sizeof(LimRow) == 7 * 8, "table row");
static_assert(sizeof(JsRow) == 5 * 8, "table row");

// the layout: byte offsets of every section from the table's start, and the table's size
struct StepTab {
    int nw;
    bool gain, eq, loud, joined;
    size_t rs, lim, utt;            // every stream
    size_t j_rs, j_lim, j_rows;     // a joined stream only (0 otherwise)
    size_t eq_rows, loud_rows;      // nw rows each; a joined stream: one row each
    size_t ps_rows = 0, ps_seg = 0; // a warped stream only (0 otherwise): PsRow [nw], then ints [offset nw | length nw]
    bool pitch = false;
    size_t bytes;
    static size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
    // the int block's columns, in ints from the table's start
    static int zoff(int) { return 0; }
    static int coff(int nw) { return nw; }
    static int wlen(int nw) { return 2 * nw; }
    static int sid(int nw) { return 3 * nw; }
    static int pack_src(int nw) { return 4 * nw; }
    static int pack_dst(int nw) { return 5 * nw; }
    static int ints(int nw) { return 6 * nw + 1; }

    StepTab(int nw_, bool gain_, bool eq_, bool loud_, bool joined_, bool pitch_ = false) : nw(nw_), gain(gain_), eq(eq_), loud(loud_), joined(joined_), pitch(pitch_) {
        const size_t n = (size_t)nw;
        rs = up8((size_t)ints(nw) * 4);
        lim = rs + n * sizeof(RsRow);
        utt = lim + n * sizeof(LimRow);
        size_t end = utt + (gain ? n * 4 : 0);
        j_rs = j_lim = j_rows = 0;
        if (joined) {
            j_rs = up8(end); j_lim = j_rs + sizeof(RsRow); j_rows = j_lim + sizeof(LimRow);
            eq_rows = j_rows + n * sizeof(JsRow);
            loud_rows = eq_rows + (eq ? sizeof(EqsRow) : 0);
            bytes = loud_rows + (loud ? sizeof(LdsRow) : 0);
        } else {
            eq_rows = up8(end);
            if (eq) end = eq_rows + n * sizeof(EqsRow);
            loud_rows = up8(end);
            bytes = loud ? loud_rows + n * sizeof(LdsRow) : end;
        }
        if (pitch) { ps_rows = up8(bytes); ps_seg = ps_rows + n * sizeof(PsRow); bytes = ps_seg + 2 * n * 4; }
    }
};

// the constants of the call: the window geometry's facts (stream_window; P = Q = 1 without the resampler, H = 0 without the limiter),
// which stages run on a step's windows, and the stage loudness reads (OutChain::src[OS_LOUD])
struct StepCall {
    long C = 1, halo = 0; int hop = 1; long long P = 1, Q = 1, H = 0;
    bool srs = false, slim = false, seq = false, sld = false, gain = false, mix = false;
    int lsrc = -1;
    // a stream through the pitch warp (null otherwise): the host copy of the warp's tables over the call's B utterances, the decoder's own
    // halo in frames (`halo` is pitch_stream_halo's) and the resampler's reach K (0: off)
    const long long* pitch_words = nullptr; int pitch_B = 0; long long pitch_TT = 0; long dec_halo = 0; long long K = 0;
};
// one window of a plain step: utterance b of F frames at z offset `zoff` speaks as `sid`; its chunk starts at frame f0.  tab: the row of
// the run's per-utterance tables it reads (the gain kernel's utt[m]; with `mix` the column of the conditioning table in the sid column)
// -- < 0: b itself, utterance b of a closed call; a planned open stream: its SLOT (live_stream.hpp: the pools are indexed by slot).
// st: whose carried EQ / loudness state and consumed position its rows name -- < 0: b itself; an open stream: its SLOT (the state pools)
struct StepWin { int b; long F, f0; int zoff, sid; int tab = -1; int st = -1; };

// what the step loop needs of a built step.  (Its vectors keep their storage from step to step.)
struct StepOut {
    StepTab tab{0, false, false, false, false};
    int nw = 0; long Wtot = 0; int maxW = 0;            // the decode: windows, their frames in all, the longest
    int zoff0 = 0, wlen0 = 0, src0 = 0;                 // window 0 by value: its place in z, its frames, its pack source
    long long max_rs = 0, max_out = 0, etiles = 1, ltiles = 1;      // launch dimensions of the output side
    long long dsum = 0;                                 // samples of the step's chunks, packed
    long long ysum = 0, max_yl = 0;                     // a warped step: the warped samples of its windows in all, the most of one
    std::vector<long long> j0, n, dst;                  // each delivered chunk: first output, count, offset in the packed buffer
    JsStep jt; std::vector<JsRow> jrows;                // a joined step: its geometry and the join's rows
    void begin(const StepTab& t, int chunks) {
        tab = t; nw = t.nw; Wtot = 0; maxW = 0; zoff0 = wlen0 = src0 = 0;
        max_rs = max_out = 0; etiles = ltiles = 1; dsum = 0; ysum = max_yl = 0;
        j0.assign((size_t)chunks, 0); n.assign((size_t)chunks, 0); dst.assign((size_t)chunks, 0);
    }
};

template <class Row> static inline void step_put(char* ht, size_t off, int i, const Row& r) { memcpy(ht + off + (size_t)i * sizeof(Row), &r, sizeof(Row)); }

// decode window i of a step: its ints, its resampler and limiter rows, its utterance for the gain kernel
static inline void step_put_window(char* ht, const StepTab& t, int i, int b, int zoff, int coff, int wlen, int sid, int pack_src, int pack_dst,
                                   const RsRow& r, const LimRow& m) {
    int* const ti = (int*)ht;
    const int nw = t.nw;
    ti[StepTab::zoff(nw) + i] = zoff; ti[StepTab::coff(nw) + i] = coff; ti[StepTab::wlen(nw) + i] = wlen; ti[StepTab::sid(nw) + i] = sid;
    ti[StepTab::pack_src(nw) + i] = pack_src; ti[StepTab::pack_dst(nw) + i] = pack_dst;
    step_put(ht, t.rs, i, r); step_put(ht, t.lim, i, m);
    if (t.gain) ((int*)(ht + t.utt))[i] = b;
}

// A step of a closed or an open stream (they differ in where f0 comes from): window i is the chunk of w[i] at f0 with its halo, the
// windows packed in the order given.  The resampler writes each window's widened outputs [jl0, jl1) back to back (rsum) when the
// limiter follows, else its kept ones [j0, j1) (dsum); the EQ reads the resampler's outputs (native rate: the decode window) and writes
// what the limiter reads; loudness reads the stage the chain names.  Null, or why a row cannot run.
static inline const char* step_build_warped(const StepCall& c, const StepWin* w, int nw, char* ht, StepOut& o);
static inline const char* step_build(const StepCall& c, const StepWin* w, int nw, EqsTrack& eqt, LdsTrack& ldt, char* ht, StepOut& o) {
    if (c.pitch_words) return step_build_warped(c, w, nw, ht, o);
    const StepTab t(nw, c.gain, c.seq, c.sld, false);
    o.begin(t, nw);
    const long long hop = c.hop;
    const bool wide = c.srs || c.seq;       // the limiter reads widened outputs at the output rate, else the decode window
    long long rsum = 0, dsum = 0;
    long Wtot = 0;
    for (int i = 0; i < nw; i++) {
        const StepWin& u = w[i];
        const StreamWin g = stream_window(u.F, u.f0, c.C, c.halo, c.hop, c.P, c.Q, c.H);
        const int row = u.tab >= 0 ? u.tab : u.b, sb = u.st >= 0 ? u.st : u.b;
        const long wlen = g.w1 - g.w0;
        const long long nrs = g.jl1 - g.jl0, nout = g.j1 - g.j0;
        const long long xnat = Wtot * hop, unat = g.w0 * hop, lnat = wlen * hop;        // the decode window's samples: where, from, how many
        step_put_window(ht, t, i, row, u.zoff + (int)g.w0, (int)Wtot, (int)wlen, c.mix ? row : u.sid, (int)((Wtot + (u.f0 - g.w0)) * hop), (int)dsum,
                        RsRow{unat, u.F * hop, g.jl0, g.jl1, c.slim ? rsum : dsum},
                        LimRow{wide ? rsum : xnat, wide ? g.jl0 : unat, wide ? nrs : lnat, g.Nout, g.j0, g.j1, dsum});
        if (c.seq) {
            const EqsRow r = c.srs ? eqt.row(sb, rsum, g.jl0, nrs, g.jl0, g.jl1, rsum, g.j0, g.j1, dsum)
                                   : eqt.row(sb, xnat, unat, lnat, g.jl0, g.jl1, rsum, g.j0, g.j1, dsum);
            if (const char* bad = eqs_row_check(r, g.Nout)) return bad;
            step_put(ht, t.eq_rows, i, r);
            o.etiles = std::max(o.etiles, eqs_tiles(r.e, r.o1));
        }
        if (c.sld) {
            const LdsRow r = c.lsrc == OS_EQ ? ldt.row(sb, rsum, g.jl0, nrs, g.j1)
                             : c.lsrc == OS_RESAMPLE ? ldt.row(sb, c.slim ? rsum : dsum, g.jl0, nrs, g.j1)
                                                     : ldt.row(sb, xnat, unat, lnat, g.j1);
            if (const char* bad = lds_row_check(r, g.Nout)) return bad;
            step_put(ht, t.loud_rows, i, r);
            o.ltiles = std::max(o.ltiles, lds_tiles(r.e, r.j1));
        }
        if (i == 0) { o.zoff0 = u.zoff + (int)g.w0; o.wlen0 = (int)wlen; o.src0 = (int)((u.f0 - g.w0) * hop); }
        o.j0[(size_t)i] = g.j0; o.n[(size_t)i] = nout; o.dst[(size_t)i] = dsum;
        rsum += nrs; o.max_rs = std::max(o.max_rs, nrs);
        dsum += nout; o.max_out = std::max(o.max_out, nout);
        Wtot += wlen; o.maxW = std::max(o.maxW, (int)wlen);
    }
    ((int*)ht)[StepTab::pack_dst(nw) + nw] = (int)dsum;
    o.Wtot = Wtot; o.dsum = dsum;
    return nullptr;
}

// A step of a closed stream through the pitch warp: window i decodes the frames pitch_window gives (the larger halo), the range warp turns
// it into the warped samples [yl0, yl1) of utterance b at ysum in the step's warped buffer, and the resampler's and the limiter's rows
// describe THAT window of an utterance of N' samples.  At the native rate without the limiter the warp writes the kept [y0, y1) itself.
// The EQ's and loudness' stream modes do not run (the engine refuses them with a plan).  A chunk may own no output (C hop = 1): n = 0.
static inline const char* step_build_warped(const StepCall& c, const StepWin* w, int nw, char* ht, StepOut& o) {
    if (c.seq || c.sld) return "pitch stream: the streamed EQ and streamed loudness do not run behind the warp";
    const StepTab t(nw, c.gain, false, false, false, true);
    o.begin(t, nw);
    const long long hop = c.hop;
    long long rsum = 0, dsum = 0, ysum = 0;
    long Wtot = 0;
    int* const seg = (int*)(ht + t.ps_seg);
    for (int i = 0; i < nw; i++) {
        const StepWin& u = w[i];
        if (u.b < 0 || u.b >= c.pitch_B) return "pitch stream: a window of an utterance the warp's tables do not hold";
        const PsUtt pu = ps_utt(c.pitch_words, c.pitch_B, c.pitch_TT, u.b);
        if (pu.N != (long long)u.F * hop) return "pitch stream: the warp's tables were laid out for another frame count";
        const PsWin g = pitch_window(pu, u.F, u.f0, c.C, c.halo, c.hop, c.P, c.Q, c.H, c.srs ? c.K : 0);
        if (const char* bad = pitch_window_check(pu, g, u.F, c.hop, c.dec_halo)) return bad;
        const int row = u.tab >= 0 ? u.tab : u.b;
        const long wlen = g.w1 - g.w0;
        const long long nrs = g.jl1 - g.jl0, nout = g.j1 - g.j0, nyl = g.yl1 - g.yl0;
        if (ysum + nyl > 0x7fffffffll) return "pitch stream: a step's warped samples exceed 2^31";
        step_put_window(ht, t, i, row, u.zoff + (int)g.w0, (int)Wtot, (int)wlen, c.mix ? row : u.sid, 0, (int)dsum,
                        RsRow{g.yl0, g.Nw, g.jl0, g.jl1, c.slim ? rsum : dsum},
                        LimRow{c.srs ? rsum : ysum, c.srs ? g.jl0 : g.yl0, c.srs ? nrs : nyl, g.Nout, g.j0, g.j1, dsum});
        step_put(ht, t.ps_rows, i, PsRow{Wtot * hop, g.w0 * hop, wlen * hop, u.b, g.yl0, g.yl1, ysum, g.y0, g.y1, dsum});
        seg[i] = (int)ysum; seg[nw + i] = (int)nyl;
        if (i == 0) { o.zoff0 = u.zoff + (int)g.w0; o.wlen0 = (int)wlen; o.src0 = 0; }
        o.j0[(size_t)i] = g.j0; o.n[(size_t)i] = nout; o.dst[(size_t)i] = dsum;
        rsum += nrs; o.max_rs = std::max(o.max_rs, nrs);
        dsum += nout; o.max_out = std::max(o.max_out, nout);
        ysum += nyl; o.max_yl = std::max(o.max_yl, nyl);
        Wtot += wlen; o.maxW = std::max(o.maxW, (int)wlen);
    }
    ((int*)ht)[StepTab::pack_dst(nw) + nw] = (int)dsum;
    o.Wtot = Wtot; o.dsum = dsum; o.ysum = ysum;
    return nullptr;
}

// Step k of a joined stream: the decode windows are the plan's (sentence b at z offset zoff[b] speaks as sid[b]); nothing packs them and
// no stage runs on them but the decoder and the gain kernel, so their pack words and rows are zero but for the gain kernel's u0 and L.
// The output side sees the ONE window of J: its resampler and limiter rows, the join's rows, its EQ and loudness row -- a silence-only
// step (nw == 0) too: the EQ and the measurement advance over the join's zeros.
static inline const char* step_build_joined(const StepCall& c, const JsPlan& js, long long k, const int* zoff, const int* sid, EqsTrack& eqt,
                                            LdsTrack& ldt, char* ht, StepOut& o) {
    JsStep& jt = o.jt;
    js.step(k, jt);
    js.rows(jt.g0, jt.g1, jt.win, o.jrows);
    const int nw = (int)jt.win.size();
    const StepTab t(nw, c.gain, c.seq, c.sld, true);
    o.begin(t, 1);
    const long long hop = c.hop;
    for (int i = 0; i < nw; i++) {
        const JsWin& w = jt.win[(size_t)i];
        step_put_window(ht, t, i, w.b, zoff[w.b] + (int)w.w0, (int)w.coff, (int)(w.w1 - w.w0), c.mix ? w.b : sid[w.b], 0, 0,
                        RsRow{w.w0 * hop, js.F[(size_t)w.b] * hop, 0, 0, 0}, LimRow{});
        step_put(ht, t.j_rows, i, o.jrows[(size_t)i]);
    }
    ((int*)ht)[StepTab::pack_dst(nw) + nw] = 0;
    const long long NJ = js.FJ * hop, Nout = stream_out_count(NJ, c.P, c.Q);
    const long long u0 = jt.g0 * hop, ulen = (jt.g1 - jt.g0) * hop, nrs = jt.jl1 - jt.jl0, nout = jt.j1 - jt.j0;
    const bool wide = c.srs || c.seq;
    step_put(ht, t.j_rs, 0, RsRow{u0, NJ, jt.jl0, jt.jl1, 0});
    step_put(ht, t.j_lim, 0, LimRow{0, wide ? jt.jl0 : u0, wide ? nrs : ulen, Nout, jt.j0, jt.j1, 0});
    if (c.seq) {
        const EqsRow r = eqt.row(0, 0, c.srs ? jt.jl0 : u0, c.srs ? nrs : ulen, jt.jl0, jt.jl1, 0, jt.j0, jt.j1, 0);
        if (const char* bad = eqs_row_check(r, Nout)) return bad;
        step_put(ht, t.eq_rows, 0, r);
        o.etiles = eqs_tiles(r.e, r.o1);
    }
    if (c.sld) {
        const bool at_out = c.lsrc == OS_EQ || c.lsrc == OS_RESAMPLE;       // (the window of J at the output rate, else the join's native one)
        const LdsRow r = ldt.row(0, 0, at_out ? jt.jl0 : u0, at_out ? nrs : ulen, jt.j1);
        if (const char* bad = lds_row_check(r, Nout)) return bad;
        step_put(ht, t.loud_rows, 0, r);
        o.ltiles = lds_tiles(r.e, r.j1);
    }
    if (nw > 0) { o.zoff0 = zoff[jt.win[0].b] + (int)jt.win[0].w0; o.wlen0 = (int)(jt.win[0].w1 - jt.win[0].w0); }
    o.Wtot = (long)jt.Wtot; o.maxW = (int)jt.maxW;
    o.max_rs = nrs; o.max_out = nout; o.dsum = nout;
    o.j0[0] = jt.j0; o.n[0] = nout; o.dst[0] = 0;
    return nullptr;
}

}  // namespace sts
