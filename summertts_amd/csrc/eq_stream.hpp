// eq_stream.hpp -- the host side of the equaliser's stream mode (eq.hip, DESIGN.md 9j "streamed"): the per-window table rows of a step,
// the carried state's layout, and the bookkeeping of how far each utterance has been consumed.  Plain C++: no HIP, no engine type
// (tests/eq_stream_check.cpp compiles it alone).
//
// The whole call evaluates the cascade in tiles of 8192 samples anchored at the utterance's first sample; the carry-in of a chunk depends
// on its tile's carry S_t and on the chunks in front of it in the same tile only.  A stream therefore keeps, per utterance: the position e
// up to which input has been consumed, S_t of the open tile (the tile that holds e), the open tile's input so far with the two samples in
// front of the tile, and the last kEqsHist samples of y (a step's range may reach back before e: the limiter's window does).  A step
// re-runs the open tile's prefix in the whole call's order and continues it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sts {

constexpr int kEqsTile = 8192;            // == EQ_TILE (eq.hip asserts it)
constexpr int kEqsHist = 4096;            // ring of the last y samples, indexed by the sample's position & (kEqsHist - 1)
constexpr int kEqsDim = 8;                // == kEqDim
constexpr int kEqsRow = 12;               // long long words per table row

// one window of a step as the kernels read it (EqArgs::wtab[kEqsRow w ..])
struct EqsRow {
    long long b;                // the utterance (its carried state)
    long long xbase, u0, xlen;  // x[xbase .. xbase + xlen) holds the utterance's input samples [u0, u0 + xlen)
    long long o0, o1;           // y to produce: [o0, o1) at ydst[ybase ..)
    long long ybase;
    long long j0, j1, pdst;     // with a PCM destination: int16 of [j0, j1) (inside [o0, o1)) at pcm[pdst ..)
    long long e;                // input consumed before this step (0: the step starts the utterance from zero state, no state is read)
    long long pad;
};
static_assert(sizeof(EqsRow) == kEqsRow * 8, "table row");

// carried state of one utterance, one of its two slots: S_t [8] doubles | the two samples in front of the open tile (x[t0 - 1], x[t0 - 2])
// padded to 256 bytes | the open tile's input so far [kEqsTile] floats | the y ring [kEqsHist] floats
constexpr size_t kEqsOffPrev = kEqsDim * 8, kEqsOffX = 256, kEqsOffY = kEqsOffX + (size_t)kEqsTile * 4;
constexpr size_t kEqsSlotBytes = kEqsOffY + (size_t)kEqsHist * 4;
static_assert(kEqsSlotBytes % 256 == 0, "slots keep 256-byte alignment");
// two slots per utterance: a step reads slot s and writes slot 1 - s, and the host flips s only behind a step that will not run again
static inline size_t eqs_state_bytes(int B) { return (size_t)B * 2 * kEqsSlotBytes; }
// tiles a step over [e, o1) touches: the open tile through the tile that holds o1 (the new open tile, possibly still empty)
static inline long long eqs_tiles(long long e, long long o1) { return o1 / kEqsTile - e / kEqsTile + 1; }
// workspace of a step: every touched tile's zero-start end state
static inline size_t eqs_ws_bytes(int nw, long long max_tiles) { return (size_t)nw * (size_t)max_tiles * kEqsDim * 8; }
// the most tiles one step of at most max_new new samples can touch
static inline long long eqs_max_tiles(long long max_new) { return max_new / kEqsTile + 2; }

// why a row cannot run (null: it can).  The kernels trust these: every address they form follows from them.
static inline const char* eqs_row_check(const EqsRow& r, long long N) {
    if (r.b < 0 || r.xbase < 0 || r.ybase < 0 || r.u0 < 0 || r.xlen < 0) return "eq stream: negative geometry";
    if (r.e < 0 || r.e > r.o1 || r.o1 > N) return "eq stream: the consumed position lies outside [0, o1], or o1 beyond the utterance";
    if (r.o0 < 0 || r.o0 > r.o1) return "eq stream: empty or negative output range";
    if (r.u0 > r.e || r.u0 + r.xlen < r.o1) return "eq stream: the window does not hold the input [e, o1)";
    if (r.o0 > r.e) return "eq stream: a gap between the consumed input and the output range";
    if (r.e - r.o0 > kEqsHist) return "eq stream: the output range reaches further back than the carried history";
    if (r.j0 < r.o0 || r.j1 > r.o1 || r.j0 > r.j1 || r.pdst < 0) return "eq stream: the kept range lies outside the output range";
    return nullptr;
}

// The steps of B utterances: consumed positions and the slot flip.  begin() before step 0; row() fills a window's row from its geometry
// and the utterance's position; commit() behind a step that succeeded (a step that is run again simply is not committed).
struct EqsTrack {
    std::vector<long long> e, pend; int slot = 0;
    void begin(int B) { e.assign((size_t)B, 0); pend.assign((size_t)B, -1); slot = 0; }
    EqsRow row(int b, long long xbase, long long u0, long long xlen, long long o0, long long o1, long long ybase, long long j0, long long j1,
               long long pdst) {
        pend[(size_t)b] = o1;
        return EqsRow{b, xbase, u0, xlen, o0, o1, ybase, j0, j1, pdst, e[(size_t)b], 0};
    }
    void commit() {
        bool any = false;
        for (size_t b = 0; b < e.size(); b++) if (pend[b] >= 0) { e[b] = pend[b]; pend[b] = -1; any = true; }
        if (any) slot ^= 1;
    }
    void drop() { std::fill(pend.begin(), pend.end(), -1); }      // the step will run again from the same state
};

}  // namespace sts
