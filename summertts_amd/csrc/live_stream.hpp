// live_stream.hpp -- the host side of an OPEN stream (Engine::stream_open / stream_admit / stream_step / stream_close, DESIGN.md 9c
// "Open streams"): the geometry of one chunk's window, the slot table of the live utterances, and the first-fit allocator over column
// ranges of the persistent latent pool.  Plain C++: no HIP, no engine type (tests/live_stream_check.cpp compiles it alone).
//
// A closed stream (sts_infer_ids_batch_stream) keeps z of its B utterances in the frame arena for the length of the one call and walks
// all of them with one step counter.  An open stream keeps z of every live utterance in a pool [inter_channels][capacity] of its own,
// one column range per utterance, and a frame position PER utterance: utterances are admitted between steps, each starts at frame 0
// whenever it arrives, and a retired one gives its slot and its columns back.  What a slot's chunks are does not depend on who else is
// live: the window of a chunk is a function of (F, f0, C, halo, hop, P, Q, H) alone (stream_window below, the one every stream uses).
//
// A PLANNED open stream (sts_stream_open_ex with capacity_phonemes > 0; DESIGN.md 9c "Planned open streams") also admits utterances with
// the per-call tables of a closed stream: a duration plan or forced durations (used by the admission's duration stage and nothing else), a
// speaker mix and a gain plan.  What a step reads of them survives the admission's arenas in pools of the stream's own, indexed by SLOT:
// the conditioning vector of every slot (gpool [gin][max_live]), the phoneme pool [cum | q][capacity_phonemes + 1] with one column range
// per gain-planned utterance -- first fit over a second free list, the same take / give as the frame ranges -- and the slot words
// [off | n | h][max_live] the gain kernel indexes by slot.  The pool's last column is the shared neutral row (cum 0, q 2^20): a slot
// without a gain plan points its words at it {capacity_phonemes, 1, 0}, for which the gain kernel's envelope is 1.0f at every sample.
//
// PER-SLOT FILTER STATE (open_filters; DESIGN.md 9c "Per-slot filter state"): an open stream runs the streamed EQ (sts_set_eq_streaming)
// and measures loudness (mode 1 with sts_set_loudness_streaming) from states that survive the arenas in pools of the stream's own,
// indexed by SLOT as the kernels index them by the row's utterance: the EQ's and loudness' two state slots per stream slot, and the
// loudness result tables tsum / tpeak over a TILE pool -- a slot of N output samples owns lds_utt_tiles(N) tiles, first fit over a third
// free list.  The consumed positions (EqsTrack / LdsTrack, sized max_live) persist between steps; an admission sets its slot's to 0, and
// the kernels read no state at e == 0, so a retired slot's stale state is never read and nothing is cleared.  The tracks' ONE parity
// suffices: every live slot has a window in every step, so every live slot's state was written by the last committed step, into the
// slot the global flip then names (a newcomer reads none and writes where the others write).
//
// Not admitted (the open stream refuses them when it is opened): loudness normalization (mode 2: the gain needs the whole utterance),
// record taps, and the EQ or loudness without their stream modes.  An unplanned stream (capacity_phonemes == 0) refuses the per-call
// tables too, as it always has.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "eq_stream.hpp"
#include "loud_stream.hpp"

namespace sts {

// The window of chunk frames [f0, f1) = [f0, min(F, f0 + C)) of an utterance of F frames: frames [w0, w1) = the chunk and `halo` frames
// on either side, clipped to the utterance.  Its native samples [f0 hop, f1 hop) are, at the output rate P / Q, the outputs j with
// ceil(f0 hop P / Q) <= j < ceil(f1 hop P / Q) = [j0, j1) of Nout.  With the limiter (H > 0: its look-ahead in output samples) they are
// produced from the float signal over [jl0, jl1) = [j0 - 2H, j1 + 2H) clipped to the utterance; without it [jl0, jl1) = [j0, j1).
struct StreamWin { long f0, f1, w0, w1; long long j0, j1, jl0, jl1, Nout; };
static inline long long stream_out_count(long long native, long long P, long long Q) { return P == Q ? native : (native * P + Q - 1) / Q; }
static inline StreamWin stream_window(long F, long f0, long C, long halo, long hop, long long P, long long Q, long long H) {
    StreamWin w{};
    w.f0 = f0; w.f1 = std::min<long>(F, f0 + C);
    w.w0 = std::max<long>(0, f0 - halo); w.w1 = std::min<long>(F, w.f1 + halo);
    w.j0 = stream_out_count((long long)f0 * hop, P, Q); w.j1 = stream_out_count((long long)w.f1 * hop, P, Q);
    w.Nout = stream_out_count((long long)F * hop, P, Q);
    w.jl0 = H > 0 ? std::max<long long>(0, w.j0 - 2 * H) : w.j0; w.jl1 = H > 0 ? std::min<long long>(w.Nout, w.j1 + 2 * H) : w.j1;
    return w;
}

// one live utterance: its columns [off, off + F) of the pool, its speaker, the first frame of its next chunk
// (a planned stream: its columns [poff, poff + pn) of the phoneme pool when it carries a gain plan, has_gain)
// (a measuring stream: its tiles [toff, toff + tn) of the result tables)
struct LiveSlot { bool live = false; long long off = 0; long F = 0; int sid = 0; long f = 0; long long poff = 0; int pn = 0; bool has_gain = false; long long toff = 0, tn = 0; };
struct LiveRange { long long off, len; };

// The capacity a group of `max_live` utterances needs when none is longer than `longest` frames: every slot can hold the longest one.
// (sts_pool sizes its streams with it: longest = kLivePoolFrames, 16.4 s of speech at 256 samples per frame and 16 kHz -- 0.8 MB of
// pool per slot at 192 channels.  Requests that do not fit an EMPTY pool run as a closed stream, as without admission.)
constexpr long long kLivePoolFrames = 1024;
static inline long long live_capacity_rule(int max_live, long long longest) { return (long long)max_live * longest; }
// The phoneme capacity by the same rule: every slot can hold the gain plan of the longest utterance.  Nothing ties phonemes to frames (a
// phoneme may own no frame), so the longest is a constant of its own: kLivePoolPhonemes = 1024 phonemes, 8 KB of pool per slot.  (A
// gain-planned request with more phonemes than the EMPTY pool holds runs as a closed stream, as for frames.)
constexpr long long kLivePoolPhonemes = 1024;
static inline long long live_phoneme_rule(int max_live, long long longest) { return (long long)max_live * longest; }
// The tile capacity of a measuring stream: an utterance of F <= capacity_frames frames owns out(F hop) / 8192 + 1 tiles, so any ONE
// utterance that fits the EMPTY frame pool fits the empty tile pool.  (Several that fill the frame pool together usually fit too, but the
// output count rounds up per utterance: their tiles may exceed the pool's by one -- the outcome is "no room now".)
static inline long long live_tile_rule(long long capacity_frames, long hop, long long P, long long Q, int max_live) {
    return stream_out_count(capacity_frames * hop, P, Q) / kLdsTile + max_live;
}

struct LiveStream {
    // fixed when the stream is opened
    int chunk = 0, max_live = 0; long long capacity = 0;
    long long capacity_phonemes = 0;                            // > 0: a planned stream
    int halo = 0, hop = 0; long long P = 1, Q = 1, H = 0;       // the window geometry's facts: stream_halo, samples per frame, rate, limiter
    // the pool and the adoption table (engine-owned device / pinned memory; plain pointers: this header knows no HIP)
    float* zpool = nullptr; void* tab_dev = nullptr; void* tab_host = nullptr;
    // a planned stream's pools, one allocation [gpool | ppool | swords] (null otherwise; gpool: a multi-speaker model with a conditioned
    // decoder only)
    void* tables_dev = nullptr; float* gpool = nullptr; int* ppool = nullptr; int* swords = nullptr;
    // per-slot filter state (open_filters): which stages carry one, the tile pool's size, and the pools -- one allocation
    // [eqst | ldst | tsum | tpeak], each only if its stage is on (null otherwise)
    bool eq_on = false, loud_on = false; long long capacity_tiles = 0;
    void* filters_dev = nullptr; char* eqst = nullptr; char* ldst = nullptr; double* tsum = nullptr; float* tpeak = nullptr;
    // state between steps
    EqsTrack eqt; LdsTrack ldt;     // consumed positions by slot and the one parity (begun by open_filters, kept from step to step)
    std::vector<LiveRange> free_tiles;                                     // the tile pool's free tiles, kept as the two lists below
    std::vector<LiveSlot> slots; std::vector<LiveRange> free_ranges;      // free_ranges: ascending, never adjacent (coalesced)
    std::vector<LiveRange> free_phonemes;                                  // the phoneme pool's free columns, kept the same way
    long long steps = 0;            // stream_step calls since open (STS_DBG_STREAM_RETRY_STEP counts them)
    bool form0 = false;             // conv math 3: an overflow was raised in a step -- split-bf16 until the stream is closed
    long long admitted = 0, retired = 0;

    void open(int chunk_frames, int max_live_, long long capacity_frames, long long capacity_phonemes_ = 0) {
        chunk = chunk_frames; max_live = max_live_; capacity = capacity_frames; capacity_phonemes = capacity_phonemes_;
        slots.assign((size_t)max_live, LiveSlot());
        free_ranges.assign(1, LiveRange{0, capacity});
        free_phonemes.clear();
        if (capacity_phonemes > 0) free_phonemes.push_back(LiveRange{0, capacity_phonemes});
        steps = 0; form0 = false; admitted = retired = 0;
        eq_on = loud_on = false; capacity_tiles = 0; free_tiles.clear();
    }
    // behind open() and the window geometry's facts (hop, P, Q): the stream carries EQ state (eq) and measures loudness (loud) per slot
    void open_filters(bool eq, bool loud) {
        eq_on = eq; loud_on = loud;
        if (eq) eqt.begin(max_live);
        if (loud) {
            ldt.begin(max_live);
            capacity_tiles = live_tile_rule(capacity, hop, P, Q, max_live);
            free_tiles.assign(1, LiveRange{0, capacity_tiles});
        }
    }
    long long tiles_of(long F) const { return loud_on ? lds_utt_tiles(stream_out_count((long long)F * hop, P, Q)) : 0; }
    long long free_tile_count() const { long long n = 0; for (const LiveRange& r : free_tiles) n += r.len; return n; }
    int live_count() const { int n = 0; for (const LiveSlot& s : slots) n += s.live; return n; }
    int free_slots() const { return max_live - live_count(); }
    long long free_frames() const { long long n = 0; for (const LiveRange& r : free_ranges) n += r.len; return n; }
    bool planned() const { return capacity_phonemes > 0; }
    long long free_phoneme_count() const { long long n = 0; for (const LiveRange& r : free_phonemes) n += r.len; return n; }
    bool any_gain() const { for (const LiveSlot& s : slots) if (s.live && s.has_gain) return true; return false; }

    // first fit: the lowest free range that holds `len` columns gives its first `len`; -1: none does
    static long long take(std::vector<LiveRange>& fr, long long len) {
        for (size_t i = 0; i < fr.size(); i++)
            if (fr[i].len >= len) {
                const long long off = fr[i].off;
                fr[i].off += len; fr[i].len -= len;
                if (fr[i].len == 0) fr.erase(fr.begin() + (long)i);
                return off;
            }
        return -1;
    }
    // columns [off, off + len) become free again; neighbours coalesce
    static void give(std::vector<LiveRange>& fr, long long off, long long len) {
        if (len <= 0) return;
        size_t i = 0;
        while (i < fr.size() && fr[i].off < off) i++;
        fr.insert(fr.begin() + (long)i, LiveRange{off, len});
        if (i + 1 < fr.size() && fr[i].off + fr[i].len == fr[i + 1].off) { fr[i].len += fr[i + 1].len; fr.erase(fr.begin() + (long)i + 1); }
        if (i > 0 && fr[i - 1].off + fr[i - 1].len == fr[i].off) { fr[i - 1].len += fr[i].len; fr.erase(fr.begin() + (long)i); }
    }

    // All or nothing: utterance b of the admission (F[b] frames, speaker sid[b]) takes the lowest free slot and the first fit of F[b]
    // columns, in the order b = 0 .. B - 1; slot_out[b] = its slot (-1: an utterance without frames takes none and is never stepped).
    // False: slots or columns do not suffice, and nothing has changed.
    bool admit(int B, const long* F, const int* sid, int* slot_out) { return admit(B, F, sid, nullptr, slot_out); }
    // ... and over phonemes too: utterance b with n_phonemes[b] > 0 carries a gain plan and takes the first fit of that many columns of
    // the phoneme pool (0, or n_phonemes == null: it takes none; an utterance without frames takes none either).  False: slots, frame
    // columns or phoneme columns do not suffice, and nothing has changed.
    // ... and, in a measuring stream, over tiles: every utterance with frames takes the first fit of tiles_of(F[b]) tiles.  Its slot's
    // consumed positions start at 0 (no state is read at e == 0: whatever the slot's last tenant left is never seen).
    bool admit(int B, const long* F, const int* sid, const int* n_phonemes, int* slot_out) {
        std::vector<LiveRange> fr = free_ranges, fp = free_phonemes, ft = free_tiles;
        std::vector<long long> off((size_t)B, 0), poff((size_t)B, 0), toff((size_t)B, 0);
        int need = 0;
        for (int b = 0; b < B; b++) {
            if (F[b] < 0 || (n_phonemes && n_phonemes[b] < 0)) return false;
            if (F[b] == 0) continue;
            need++;
            if ((off[(size_t)b] = take(fr, F[b])) < 0) return false;
            if (n_phonemes && n_phonemes[b] > 0 && (poff[(size_t)b] = take(fp, n_phonemes[b])) < 0) return false;
            if (loud_on && (toff[(size_t)b] = take(ft, tiles_of(F[b]))) < 0) return false;
        }
        if (need > free_slots()) return false;
        size_t s = 0;
        for (int b = 0; b < B; b++) {
            if (F[b] == 0) { slot_out[b] = -1; continue; }
            while (slots[s].live) s++;
            const int pn = n_phonemes ? n_phonemes[b] : 0;
            slots[s] = LiveSlot{true, off[(size_t)b], F[b], sid ? sid[b] : 0, 0, poff[(size_t)b], pn, pn > 0, toff[(size_t)b], tiles_of(F[b])};
            if (eq_on) { eqt.e[s] = 0; eqt.pend[s] = -1; }
            if (loud_on) { ldt.e[s] = 0; ldt.pend[s] = -1; ldt.tbase[s] = toff[(size_t)b]; }
            slot_out[b] = (int)s;
            admitted++;
        }
        free_ranges.swap(fr); free_phonemes.swap(fp); free_tiles.swap(ft);
        return true;
    }
    void retire(int s) {
        LiveSlot& sl = slots[(size_t)s];
        if (!sl.live) return;
        give(free_ranges, sl.off, sl.F);
        give(free_phonemes, sl.poff, sl.pn);
        give(free_tiles, sl.toff, sl.tn);
        sl = LiveSlot();
        retired++;
    }
    // the live slots of the next step, ascending
    void step_slots(std::vector<int>& out) const {
        out.clear();
        for (size_t s = 0; s < slots.size(); s++) if (slots[s].live) out.push_back((int)s);
    }
    StreamWin window(int s) const { const LiveSlot& sl = slots[(size_t)s]; return stream_window(sl.F, sl.f, chunk, halo, hop, P, Q, H); }
    // slot s has delivered the chunk of window(s): it moves on, and retires behind its last chunk or when its callback stopped it.
    // True: it retired.
    bool delivered(int s, bool stop) {
        LiveSlot& sl = slots[(size_t)s];
        sl.f = std::min<long>(sl.F, sl.f + chunk);
        if (stop || sl.f >= sl.F) { retire(s); return true; }
        return false;
    }
    void drop_all() { for (size_t s = 0; s < slots.size(); s++) retire((int)s); }
};

}  // namespace sts
