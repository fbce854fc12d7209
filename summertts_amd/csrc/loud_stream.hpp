// loud_stream.hpp -- the host side of loudness measurement in a stream (loudness.hip's stream mode, DESIGN.md 9d "streamed"): the
// per-window table rows of a step, the carried state's layout, the per-call result tables, and the bookkeeping of how far each utterance
// has been consumed.  Plain C++: no HIP, no engine type (tests/loud_stream_check.cpp compiles it alone).
//
// The whole call K-weights in tiles of 8192 samples anchored at the utterance's first sample; the carry-in of a chunk depends on its
// tile's carry S_t and on the chunks in front of it in the same tile only, and a tile's sub-block sums and peak are a function of the
// tile's samples and S_t.  A stream therefore keeps, per utterance: the position e up to which input has been consumed, S_t of the open
// tile (the tile that holds e), the open tile's input so far with the two samples in front of the tile -- and, per call, the sums and the
// peak of every tile, the open one's provisional.  A step re-runs the open tile's prefix in the whole call's order and continues it.
// Nothing reads the K-weighted signal back: there is no ring of outputs.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sts {

constexpr int kLdsTile = 8192;            // == LD_TILE (loudness.hip asserts it)
constexpr int kLdsSlots = 16;             // == LD_SLOTS
constexpr int kLdsRow = 8;                // long long words per table row

// one window of a step as the kernels read it (LoudStreamArgs::wtab[kLdsRow w ..])
struct LdsRow {
    long long b;                // the utterance (its carried state)
    long long xbase, u0, xlen;  // x[xbase .. xbase + xlen) holds the utterance's input samples [u0, u0 + xlen)
    long long j1;               // the step consumes [e, j1)
    long long e;                // input consumed before this step (0: the step starts the utterance from zero state, no state is read)
    long long tbase;            // the utterance's first tile in the call's result tables
    long long pad;
};
static_assert(sizeof(LdsRow) == kLdsRow * 8, "table row");

// carried state of one utterance, one of its two slots: S_t [4] doubles | the two samples in front of the open tile (x[t0 - 1], x[t0 - 2])
// padded to 256 bytes | the open tile's input so far [kLdsTile] floats
constexpr size_t kLdsOffPrev = 4 * 8, kLdsOffX = 256;
constexpr size_t kLdsSlotBytes = kLdsOffX + (size_t)kLdsTile * 4;
static_assert(kLdsSlotBytes % 256 == 0, "slots keep 256-byte alignment");
// two slots per utterance: a step reads slot s and writes slot 1 - s, and the host flips s only behind a step that will not run again
static inline size_t lds_state_bytes(int B) { return (size_t)B * 2 * kLdsSlotBytes; }
// tiles a step over [e, j1) touches: the open tile through the tile that holds j1 (the new open tile, possibly still empty)
static inline long long lds_tiles(long long e, long long j1) { return j1 / kLdsTile - e / kLdsTile + 1; }
// workspace of a step: every touched tile's zero-start end state
static inline size_t lds_ws_bytes(int nw, long long max_tiles) { return (size_t)nw * (size_t)max_tiles * 4 * 8; }
// the most tiles one step of at most max_new new samples can touch
static inline long long lds_max_tiles(long long max_new) { return max_new / kLdsTile + 2; }
// tiles of an utterance of N samples in the result tables (the tile that holds N included: a step that ends on a tile's edge owns it)
static inline long long lds_utt_tiles(long long N) { return N / kLdsTile + 1; }
// the call's result tables for `tiles` tiles in all and B utterances: [utab B x 3 long long | tsum tiles x kLdsSlots double | tpeak
// tiles float | gain B float], as loud_gate_kernel reads them
static inline size_t lds_res_bytes(int B, long long tiles) {
    return (size_t)B * 3 * 8 + (size_t)tiles * kLdsSlots * 8 + (size_t)tiles * 4 + (size_t)B * 4 + 256;
}

// why a row cannot run (null: it can).  The kernels trust these: every address they form follows from them.
static inline const char* lds_row_check(const LdsRow& r, long long N) {
    if (r.b < 0 || r.xbase < 0 || r.u0 < 0 || r.xlen < 0 || r.tbase < 0) return "loudness stream: negative geometry";
    if (r.e < 0 || r.e > r.j1 || r.j1 > N) return "loudness stream: the consumed position lies outside [0, j1], or j1 beyond the utterance";
    if (r.u0 > r.e || r.u0 + r.xlen < r.j1) return "loudness stream: the window does not hold the input [e, j1)";
    return nullptr;
}

// The steps of B utterances: consumed positions and the slot flip.  begin() before step 0; row() fills a window's row from its geometry
// and the utterance's position; commit() behind a step that succeeded (a step that is run again simply is not committed).
struct LdsTrack {
    std::vector<long long> e, pend, tbase; int slot = 0;
    void begin(int B) { e.assign((size_t)B, 0); pend.assign((size_t)B, -1); tbase.assign((size_t)B, 0); slot = 0; }
    // the utterances' places in the result tables from their lengths; returns the tiles in all
    long long layout(const long long* N) {
        long long t = 0;
        for (size_t b = 0; b < tbase.size(); b++) { tbase[b] = t; t += lds_utt_tiles(N[b]); }
        return t;
    }
    LdsRow row(int b, long long xbase, long long u0, long long xlen, long long j1) {
        pend[(size_t)b] = j1;
        return LdsRow{b, xbase, u0, xlen, j1, e[(size_t)b], tbase[(size_t)b], 0};
    }
    void commit() {
        bool any = false;
        for (size_t b = 0; b < e.size(); b++) if (pend[b] >= 0) { e[b] = pend[b]; pend[b] = -1; any = true; }
        if (any) slot ^= 1;
    }
    void drop() { std::fill(pend.begin(), pend.end(), -1); }      // the step will run again from the same state
};

}  // namespace sts
