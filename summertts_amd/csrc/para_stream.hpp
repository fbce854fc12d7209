// para_stream.hpp -- the host side of an OPEN PARAGRAPH (Engine::para_open / para_append / para_finish / para_step / para_close, DESIGN.md 9i
// "Open paragraphs"): a joined stream (join_stream.hpp) whose right end grows between its steps, its sentences' latents resident in a
// pool of column ranges (live_stream.hpp's allocator).  Plain C++: no HIP, no engine type (tests/para_stream_check.cpp compiles it alone).
//
// The paragraph is ONE joined signal J on one chunk grid: chunk k = the frames [k C, (k + 1) C) of J.  Sentence i (a global index that
// only ever grows) starts at s_i = s_{i-1} + F_{i-1} + gap_i (s_0 = lead) -- sts_join_layout's rule, continued -- and E = s_n + F_n is
// the end of the last sentence appended so far.
//
// The frontier.  Before finish nobody knows F_J, but a step of a joined stream looks at J only through its window [f0 - Ho, f1 + Ho)
// (JsPlan::step): so chunk k is deliverable iff (k + 1) C + Ho <= E.  Everything behind E is still open -- the next sentence may start
// there -- and everything in front of it is fixed for good: a later sentence starts at or behind E and so never meets that window.  For
// such a chunk none of JsPlan::step's clips against F_J or N_out binds (f1 + Ho <= E <= F_J, and j1 + 2H <= ceil((f1 + Ho) hop P / Q)
// because Ho hop covers the limiter's 2H outputs), so the step computed with the provisional F_J = E is the step the closed stream over
// the finished paragraph computes: the same chunk, J window, output ranges, decode windows and join rows.  After finish F_J is known and
// every remaining chunk is deliverable, the short last one included.
//
// Residency.  Sentence i holds F_i columns of the pool from its append until no later step reads it: a step reads a sentence only when
// its J window meets it, so once the next undelivered chunk k has k C - Ho - Hd >= s_i + F_i the sentence retires (the decoder's halo Hd
// never leaves a sentence; it is kept in the rule as slack).  Sentences retire in order.
#pragma once

#include "join_stream.hpp"
#include "live_stream.hpp"

namespace sts {

constexpr long long kParaMaxNative = 2000000000LL;      // N_J, as for every joined call
constexpr long long kParaMaxOut = 2147483647LL;         // L_out

struct ParaStream {
    // the growing plan: s / F of EVERY sentence appended so far (24 bytes per sentence for the paragraph's life); FJ = E until finish
    JsPlan js;
    // the latent pool's slots and free column ranges, the step count and the form-0 flag (and the engine's device pointers)
    LiveStream pool;
    // per sentence (global index): its z offset in the pool, its speaker, its slot (-1: retired)
    std::vector<int> zoff, sid, slot;
    long long lead = 0, E = 0;          // E: end of the last sentence, frames of J (0: no sentence yet)
    long long k = 0;                    // the next undelivered chunk
    int first_live = 0;                 // the first sentence that has not retired
    bool finished = false, stopped = false;
    int fade_h = 0;                     // the join's fade in samples (join_design)

    void open(long long C, int max_resident, long long capacity, long long lead_frames, int hop, int Hd, int Ho, long long P, long long Q, int H) {
        js = JsPlan();
        js.hop = hop; js.C = C; js.Hd = Hd; js.Ho = Ho; js.P = P; js.Q = Q; js.H = H;
        pool.open((int)std::min<long long>(C, 2147483647LL), max_resident, capacity);
        pool.halo = Hd + Ho; pool.hop = hop; pool.P = P; pool.Q = Q; pool.H = H;
        zoff.clear(); sid.clear(); slot.clear();
        lead = lead_frames; E = 0; k = 0; first_live = 0; finished = stopped = false;
    }
    int sentences() const { return (int)js.s.size(); }
    int resident() const { return pool.live_count(); }
    // would a joined signal of `frames` frames be one call's?  (N_J <= 2 10^9 native samples, L_out <= 2^31 - 1)
    bool fits(long long frames) const {
        const long long N = frames * js.hop;
        return frames >= 0 && frames <= kParaMaxNative && N <= kParaMaxNative && js.out_count(N) <= kParaMaxOut;
    }
    // frames of J whose content is known for good
    long long frames_known() const { return finished ? js.FJ : E; }
    long long frames_delivered() const { return std::min(k * js.C, js.FJ); }
    // chunks deliverable now without a further append
    long long ready() const {
        if (stopped) return 0;
        if (finished) return std::max<long long>(0, js.steps() - k);
        const long long reach = E - js.Ho;
        return reach < js.C ? 0 : std::max<long long>(0, reach / js.C - k);
    }
    // Appends B sentences of F[b] >= 1 frames, gap[b] frames of silence in front of each (the paragraph's first: 0; null: zeros).
    // 1: done, start[b] = its first frame in J; 0: slots or columns do not suffice now; -1: J would be too long for one call.  0 and -1
    // change nothing.
    int append(int B, const long* F, const int* sids, const long long* gap, long long* start) {
        long long e = E;
        std::vector<long long> st((size_t)B);
        for (int b = 0; b < B; b++) {
            st[(size_t)b] = (sentences() == 0 && b == 0) ? lead : e + (gap ? gap[b] : 0);
            e = st[(size_t)b] + F[b];
            if (F[b] < 1 || !fits(e)) return -1;
        }
        std::vector<int> sl((size_t)B, -1);
        if (!pool.admit(B, F, sids, sl.data())) return 0;
        for (int b = 0; b < B; b++) {
            js.s.push_back(st[(size_t)b]); js.F.push_back(F[b]);
            slot.push_back(sl[(size_t)b]); sid.push_back(sids ? sids[b] : 0);
            zoff.push_back((int)pool.slots[(size_t)sl[(size_t)b]].off);
            if (start) start[b] = st[(size_t)b];
        }
        E = e; js.FJ = E;
        return 1;
    }
    // takes the last B sentences back (an append whose device work failed): the state in front of that append
    void undo(int B) {
        for (int b = 0; b < B; b++) {
            if (slot.back() >= 0) { pool.retire(slot.back()); pool.admitted--; pool.retired--; }
            js.s.pop_back(); js.F.pop_back(); slot.pop_back(); sid.pop_back(); zoff.pop_back();
        }
        E = sentences() ? js.s.back() + js.F.back() : 0;
        js.FJ = E;
    }
    // no more sentences: F_J = E + trail.  False: no sentence, or J would be too long
    bool finish(long long trail) {
        if (finished || sentences() == 0 || trail < 0 || !fits(E + trail)) return false;
        js.FJ = E + trail; finished = true;
        return true;
    }
    // The plan a step runs on: the sentences that have not retired alone, sentence first_live as its index 0 (the caller shifts zoff and
    // sid likewise).  No step from chunk k on meets a retired sentence, so its step k is js's with every window's b lower by first_live
    // -- and a step's host cost follows the resident sentences, not every sentence of the paragraph's life
    JsPlan resident_plan() const {
        JsPlan p;
        p.FJ = js.FJ; p.hop = js.hop; p.C = js.C; p.Hd = js.Hd; p.Ho = js.Ho; p.P = js.P; p.Q = js.Q; p.H = js.H;
        p.s.assign(js.s.begin() + first_live, js.s.end()); p.F.assign(js.F.begin() + first_live, js.F.end());
        return p;
    }
    // sentence i is no longer read by chunk k or any later one
    bool behind(int i) const { return k * js.C - js.Ho - js.Hd >= js.s[(size_t)i] + js.F[(size_t)i]; }
    void retire_front() {
        const bool all = stopped || (finished && k >= js.steps());
        while (first_live < sentences() && (all || behind(first_live))) {
            if (slot[(size_t)first_live] >= 0) pool.retire(slot[(size_t)first_live]);
            slot[(size_t)first_live] = -1;
            first_live++;
        }
    }
    // chunk k has left (stop: its callback ended the paragraph)
    void delivered(bool stop) {
        k++;
        if (stop) stopped = true;
        retire_front();
    }
};

}  // namespace sts
