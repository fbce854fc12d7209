// live_filters_check.cpp -- the host side of an open stream with PER-SLOT FILTER STATE (summertts_amd/csrc/live_stream.hpp, stream_step.hpp):
// slots, frame ranges, phoneme ranges and the TILE pool, the consumed positions by slot and the one parity, driven through seeded random
// schedules of admit / step / repeat / stop / retire against brute force, alone: no HIP, no engine.  Built with
// -fsanitize=address,undefined by tests/test_live_filters_cpu.py and run directly.
// Prints "ok <schedules> <admissions> <refused> <refused for tiles alone> <steps> <repeated steps> <rows>" or the first violated property.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "stream_step.hpp"

using namespace sts;

#define REQUIRE(cond, ...)                                                  \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);      \
            printf(__VA_ARGS__);                                            \
            printf("\n");                                                   \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

namespace {

enum { R_FRAMES, R_PHONEMES, R_TILES, R_COUNT };

long long r_off(const LiveSlot& s, int r) { return r == R_FRAMES ? s.off : r == R_PHONEMES ? s.poff : s.toff; }
long long r_len(const LiveSlot& s, int r) { return r == R_FRAMES ? (long long)s.F : r == R_PHONEMES ? (long long)s.pn : s.tn; }
long long r_cap(const LiveStream& L, int r) { return r == R_FRAMES ? L.capacity : r == R_PHONEMES ? L.capacity_phonemes : L.capacity_tiles; }
const std::vector<LiveRange>& r_free(const LiveStream& L, int r) { return r == R_FRAMES ? L.free_ranges : r == R_PHONEMES ? L.free_phonemes : L.free_tiles; }
const char* r_name(int r) { return r == R_FRAMES ? "frames" : r == R_PHONEMES ? "phonemes" : "tiles"; }

std::vector<char> occupancy(const LiveStream& L, int r) {
    std::vector<char> used((size_t)r_cap(L, r), 0);
    for (const LiveSlot& s : L.slots) {
        if (!s.live) continue;
        for (long long c = r_off(s, r); c < r_off(s, r) + r_len(s, r); c++) {
            REQUIRE(c >= 0 && c < r_cap(L, r), "%s: a live range leaves [0, capacity)", r_name(r));
            REQUIRE(!used[(size_t)c], "%s: two live ranges overlap at %lld", r_name(r), c);
            used[(size_t)c] = 1;
        }
    }
    return used;
}

// live ranges never overlap (occupancy), free ones ascend and never touch, the two kinds cover [0, capacity) exactly
void check_state(const LiveStream& L) {
    for (int r = 0; r < R_COUNT; r++) {
        std::vector<char> used = occupancy(L, r);
        long long prev_end = -1;
        for (const LiveRange& f : r_free(L, r)) {
            REQUIRE(f.len > 0 && f.off > prev_end && f.off + f.len <= r_cap(L, r), "%s: free ranges are not ascending, not coalesced or leave the pool", r_name(r));
            for (long long c = f.off; c < f.off + f.len; c++) { REQUIRE(!used[(size_t)c], "%s: a free range overlaps a live one at %lld", r_name(r), c); used[(size_t)c] = 2; }
            prev_end = f.off + f.len;
        }
        for (size_t c = 0; c < used.size(); c++) REQUIRE(used[c] != 0, "%s: column %zu leaked", r_name(r), c);
    }
    for (const LiveSlot& s : L.slots) {
        if (!s.live) { REQUIRE(s.tn == 0 && s.toff == 0 && s.pn == 0, "a free slot keeps tiles or phonemes"); continue; }
        REQUIRE(s.tn == lds_utt_tiles(stream_out_count((long long)s.F * L.hop, L.P, L.Q)), "a slot's tiles are not lds_utt_tiles of its output samples");
    }
    REQUIRE(L.live_count() + L.free_slots() == L.max_live, "the counters disagree with the tables");
}

long long first_fit(const std::vector<char>& used, long long len) {
    long long run = 0;
    for (size_t c = 0; c < used.size(); c++) {
        run = used[c] ? 0 : run + 1;
        if (run == len) return (long long)c + 1 - len;
    }
    return -1;
}
bool place_all(std::vector<char> used, const std::vector<long long>& len, std::vector<long long>& want) {
    want.assign(len.size(), -1);
    for (size_t b = 0; b < len.size(); b++) {
        if (len[b] == 0) continue;
        if ((want[b] = first_fit(used, len[b])) < 0) return false;
        for (long long c = want[b]; c < want[b] + len[b]; c++) used[(size_t)c] = 1;
    }
    return true;
}

bool same_ranges(const std::vector<LiveRange>& a, const std::vector<LiveRange>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].off != b[i].off || a[i].len != b[i].len) return false;
    return true;
}
bool same(const LiveStream& a, const LiveStream& b) {
    if (a.admitted != b.admitted || a.retired != b.retired || a.slots.size() != b.slots.size()) return false;
    for (int r = 0; r < R_COUNT; r++) if (!same_ranges(r_free(a, r), r_free(b, r))) return false;
    for (size_t s = 0; s < a.slots.size(); s++) {
        const LiveSlot &x = a.slots[s], &y = b.slots[s];
        if (x.live != y.live || x.off != y.off || x.F != y.F || x.f != y.f || x.sid != y.sid || x.poff != y.poff || x.pn != y.pn || x.toff != y.toff || x.tn != y.tn) return false;
    }
    return a.eqt.e == b.eqt.e && a.eqt.pend == b.eqt.pend && a.eqt.slot == b.eqt.slot && a.ldt.e == b.ldt.e && a.ldt.pend == b.ldt.pend &&
           a.ldt.tbase == b.ldt.tbase && a.ldt.slot == b.ldt.slot;
}

struct Tally { long admissions = 0, refused = 0, refused_tiles = 0, steps = 0, repeats = 0, rows = 0; };
struct Geo { long long P, Q, H; };

// The brute-force model of the carried state: for every stream slot, which of its two state slots holds its state (-1: none yet) and up
// to where that state has consumed the utterance -- what the kernels do with a row (read slot `slot` unless e == 0, write slot 1 - slot).
struct Model { std::vector<int> where; std::vector<long long> upto; };

void run_schedule(unsigned seed, int chunk, int max_live, long long cap, long long capP, const Geo& geo, const std::vector<long>& F, const std::vector<int>& N,
                  double p_stop, Tally& t) {
    std::mt19937 rng(seed);
    auto coin = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
    LiveStream L;
    L.open(chunk, max_live, cap, capP);
    L.halo = 2; L.hop = 256; L.P = geo.P; L.Q = geo.Q; L.H = geo.H;
    L.open_filters(true, true);
    REQUIRE(L.eq_on && L.loud_on && L.capacity_tiles == stream_out_count(cap * L.hop, geo.P, geo.Q) / kLdsTile + max_live, "the tile pool's capacity rule");
    REQUIRE((long long)L.eqt.e.size() == max_live && (long long)L.ldt.e.size() == max_live && L.free_tile_count() == L.capacity_tiles, "open_filters");
    check_state(L);
    // the chain of such a stream, as the engine plans it
    const OutChain oc = plan_out_chain(OutFacts{true, max_live, geo.P != geo.Q, false, false, true, 1, geo.H > 0, false, false, true, true});
    REQUIRE(oc.eqst && oc.lst && oc.src[OS_LOUD] == OS_EQ, "the planner runs both stages in a stream");
    StepCall call;
    call.C = chunk; call.halo = L.halo; call.hop = L.hop; call.P = geo.P; call.Q = geo.Q; call.H = geo.H;
    call.srs = oc.run[OS_RESAMPLE]; call.slim = oc.run[OS_LIMIT]; call.seq = true; call.sld = true; call.lsrc = oc.src[OS_LOUD];
    Model me{std::vector<int>((size_t)max_live, -1), std::vector<long long>((size_t)max_live, 0)}, ml = me;
    size_t next = 0;
    bool one = false;
    std::vector<char> ht, ht2;
    StepOut st, st2;
    while (next < F.size() || L.live_count() > 0) {
        if (next < F.size() && (L.live_count() == 0 || coin(0.45))) {
            const int B = one ? 1 : (int)std::min<size_t>(F.size() - next, 1 + rng() % 3);
            one = false;
            std::vector<long> Fb(F.begin() + (long)next, F.begin() + (long)next + B);
            std::vector<int> Nb(N.begin() + (long)next, N.begin() + (long)next + B), sid((size_t)B), slots((size_t)B, -7);
            std::vector<long long> len[R_COUNT], want[R_COUNT];
            int need = 0;
            for (int b = 0; b < B; b++) {
                sid[(size_t)b] = (int)next + b;
                const bool has = Fb[(size_t)b] > 0;
                len[R_FRAMES].push_back(Fb[(size_t)b]); len[R_PHONEMES].push_back(has ? Nb[(size_t)b] : 0);
                len[R_TILES].push_back(has ? stream_out_count((long long)Fb[(size_t)b] * L.hop, geo.P, geo.Q) / kLdsTile + 1 : 0);
                need += has;
            }
            const LiveStream before = L;
            bool fit[R_COUNT];
            for (int r = 0; r < R_COUNT; r++) fit[r] = place_all(occupancy(L, r), len[r], want[r]);
            const bool fit_s = need <= L.free_slots();
            const bool ok = L.admit(B, Fb.data(), sid.data(), Nb.data(), slots.data());
            REQUIRE(ok == (fit_s && fit[0] && fit[1] && fit[2]), "admit answered %d where brute force says slots %d frames %d phonemes %d tiles %d", (int)ok,
                    (int)fit_s, (int)fit[0], (int)fit[1], (int)fit[2]);
            if (!ok) {
                REQUIRE(same(L, before), "a refused admission changed the state (ranges, slots, positions or parity)");
                for (int b = 0; b < B; b++) REQUIRE(slots[(size_t)b] == -7, "a refused admission wrote a slot");
                t.refused++;
                if (fit_s && fit[0] && fit[1]) t.refused_tiles++;
                REQUIRE(L.live_count() > 0 || B > 1, "one utterance does not fit the empty pools: the empty-pool rule");
                one = L.live_count() == 0;
            } else {
                REQUIRE(L.eqt.slot == before.eqt.slot && L.ldt.slot == before.ldt.slot, "an admission moved the parity");
                for (int b = 0; b < B; b++) {
                    if (Fb[(size_t)b] == 0) { REQUIRE(slots[(size_t)b] == -1, "an utterance without frames took a slot"); continue; }
                    const int s = slots[(size_t)b];
                    REQUIRE(s >= 0 && s < max_live && L.slots[(size_t)s].live && !before.slots[(size_t)s].live, "slot out of range, or taken from a live one");
                    const LiveSlot& sl = L.slots[(size_t)s];
                    for (int r = 0; r < R_COUNT; r++)
                        if (len[r][(size_t)b] > 0) REQUIRE(r_off(sl, r) == want[r][(size_t)b] && r_len(sl, r) == len[r][(size_t)b], "%s: not first fit, or not what was admitted", r_name(r));
                    REQUIRE(L.eqt.e[(size_t)s] == 0 && L.ldt.e[(size_t)s] == 0 && L.eqt.pend[(size_t)s] < 0 && L.ldt.pend[(size_t)s] < 0, "an admitted slot does not start at position 0");
                    REQUIRE(L.ldt.tbase[(size_t)s] == sl.toff, "the slot's first tile is not its range's");
                    me.where[(size_t)s] = ml.where[(size_t)s] = -1; me.upto[(size_t)s] = ml.upto[(size_t)s] = 0;     // (whatever is there is stale)
                }
                // the other slots keep their positions
                for (int s = 0; s < max_live; s++)
                    if (before.slots[(size_t)s].live) REQUIRE(L.eqt.e[(size_t)s] == before.eqt.e[(size_t)s] && L.ldt.e[(size_t)s] == before.ldt.e[(size_t)s], "an admission moved another slot's position");
                next += (size_t)B;
                t.admissions++;
            }
            check_state(L);
            continue;
        }
        // one step: every live slot's window, rows by slot
        std::vector<int> order;
        L.step_slots(order);
        std::vector<StepWin> win;
        for (size_t i = 0; i < order.size(); i++) {
            const LiveSlot& sl = L.slots[(size_t)order[i]];
            win.push_back(StepWin{(int)i, sl.F, sl.f, (int)sl.off, sl.sid, -1, order[i]});
        }
        const int nw = (int)win.size();
        const StepTab tab(nw, false, true, true, false);
        ht.assign(tab.bytes, 0x5a); ht2.assign(tab.bytes, 0x5a);
        const bool repeat = coin(0.2);
        if (repeat) {       // the step's first attempt: built, then dropped -- the second builds the same rows from the same positions
            const LiveStream before = L;
            const char* bad = step_build(call, win.data(), nw, L.eqt, L.ldt, ht2.data(), st2);
            REQUIRE(!bad, "a row of an open step cannot run: %s", bad);
            L.eqt.drop(); L.ldt.drop();
            REQUIRE(same(L, before), "a dropped step left a trace");
            t.repeats++;
        }
        const char* bad = step_build(call, win.data(), nw, L.eqt, L.ldt, ht.data(), st);
        REQUIRE(!bad, "a row of an open step cannot run: %s", bad);
        if (repeat) REQUIRE(memcmp(ht.data(), ht2.data(), tab.bytes) == 0 && st.etiles == st2.etiles && st.ltiles == st2.ltiles && st.dsum == st2.dsum, "the repeated step built other rows");
        for (int i = 0; i < nw; i++) {
            const int s = order[(size_t)i];
            const LiveSlot& sl = L.slots[(size_t)s];
            const StreamWin g = L.window(s);
            EqsRow er; LdsRow lr;
            memcpy(&er, ht.data() + tab.eq_rows + (size_t)i * sizeof(EqsRow), sizeof(EqsRow));
            memcpy(&lr, ht.data() + tab.loud_rows + (size_t)i * sizeof(LdsRow), sizeof(LdsRow));
            REQUIRE(!eqs_row_check(er, g.Nout) && !lds_row_check(lr, g.Nout), "row checks");
            REQUIRE(er.b == s && lr.b == s && er.b < max_live, "a row does not name its slot");
            // the row continues where the slot's state ends, and that state lies in the state slot the step reads (the parity invariant)
            REQUIRE(er.e == me.upto[(size_t)s] && lr.e == ml.upto[(size_t)s], "slot %d: the row starts at %lld / %lld, its state ends at %lld / %lld", s, er.e, lr.e, me.upto[(size_t)s], ml.upto[(size_t)s]);
            if (er.e > 0) REQUIRE(me.where[(size_t)s] == L.eqt.slot, "slot %d: the EQ reads state slot %d, its state lies in %d", s, L.eqt.slot, me.where[(size_t)s]);
            if (lr.e > 0) REQUIRE(ml.where[(size_t)s] == L.ldt.slot, "slot %d: loudness reads state slot %d, its state lies in %d", s, L.ldt.slot, ml.where[(size_t)s]);
            REQUIRE(er.o1 == g.jl1 && lr.j1 == g.j1 && er.j0 == g.j0 && er.j1 == g.j1, "the rows' ranges are not the window's");
            // every tile the step writes is the slot's own
            REQUIRE(lr.tbase == sl.toff && lr.j1 / kLdsTile < sl.tn && lr.e / kLdsTile + lds_tiles(lr.e, lr.j1) <= sl.tn, "slot %d writes tiles outside its range", s);
            REQUIRE(eqs_tiles(er.e, er.o1) <= st.etiles && lds_tiles(lr.e, lr.j1) <= st.ltiles, "the launch dimensions do not cover a row");
            t.rows++;
        }
        // the kernels ran: every window's state now lies in the other state slot
        for (int i = 0; i < nw; i++) {
            const int s = order[(size_t)i];
            EqsRow er; LdsRow lr;
            memcpy(&er, ht.data() + tab.eq_rows + (size_t)i * sizeof(EqsRow), sizeof(EqsRow));
            memcpy(&lr, ht.data() + tab.loud_rows + (size_t)i * sizeof(LdsRow), sizeof(LdsRow));
            me.where[(size_t)s] = 1 - L.eqt.slot; me.upto[(size_t)s] = er.o1;
            ml.where[(size_t)s] = 1 - L.ldt.slot; ml.upto[(size_t)s] = lr.j1;
        }
        const int pe = L.eqt.slot, pl = L.ldt.slot;
        L.eqt.commit(); L.ldt.commit();
        REQUIRE(L.eqt.slot == 1 - pe && L.ldt.slot == 1 - pl, "a step with windows did not flip the parity");
        for (const int s : order) {
            const LiveSlot sl = L.slots[(size_t)s];
            const bool stop = coin(p_stop), last = sl.f + chunk >= sl.F;
            const long long ft = L.free_tile_count(), ff = L.free_frames();
            const bool retired = L.delivered(s, stop);
            REQUIRE(retired == (stop || last), "slot %d retired %d, stop %d last %d", s, (int)retired, (int)stop, (int)last);
            if (retired) REQUIRE(L.free_tile_count() == ft + sl.tn && L.free_frames() == ff + sl.F && !L.slots[(size_t)s].live, "a retirement did not return its ranges");
            else REQUIRE(L.free_tile_count() == ft && L.free_frames() == ff, "a step moved ranges");
            if (last && !stop) REQUIRE(ml.upto[(size_t)s] == stream_out_count((long long)sl.F * L.hop, geo.P, geo.Q), "a slot retired behind its last chunk before loudness consumed all of it");
        }
        t.steps++;
        check_state(L);
    }
    for (int r = 0; r < R_COUNT; r++)
        REQUIRE(r_free(L, r).size() == 1 && r_free(L, r)[0].off == 0 && r_free(L, r)[0].len == r_cap(L, r), "%s: a full drain does not leave one free range", r_name(r));
    REQUIRE(L.admitted == L.retired, "admitted %lld, retired %lld", L.admitted, L.retired);
}

}  // namespace

int main() {
    Tally t;
    long schedules = 0;
    const Geo geos[4] = {{1, 1, 0}, {441, 320, 110}, {1, 2, 0}, {1, 1, 80}};        // native; 22 050 Hz with the limiter; 8 000 Hz; native with the limiter
    for (unsigned set = 0; set < 32; set++) {
        std::mt19937 rng(977 + set);
        const int max_live = 3 + (int)(rng() % 5);
        const Geo& geo = geos[set % 4];
        std::vector<long> F(36); std::vector<int> N(36);
        // (up to 150 frames = 38 400 native samples: utterances of one tile and of five, some without frames, half of them short, half without a gain plan)
        for (size_t u = 0; u < F.size(); u++) { F[u] = rng() % 2 == 0 ? (long)(rng() % 12) : (long)(rng() % 150); N[u] = rng() % 2 ? 0 : 1 + (int)(rng() % 30); }
        F[2] = 1; F[6] = 0; F[9] = 32; F[11] = 64;      // (32 and 64 frames: 8192 and 16 384 samples -- an utterance that ends on a tile's edge owns the next tile)
        // frames are scarce enough to fragment both pools: short utterances hold a whole tile each
        const long long cap = 150 + (long long)(rng() % 200), capP = 200;
        for (unsigned sched = 0; sched < 4; sched++) {
            run_schedule(131 * sched + set, 1 + (int)(rng() % 24), max_live, cap, capP, geo, F, N, 0.03 * sched, t);
            schedules++;
        }
    }
    // the empty-pool rule: ONE utterance of any length up to the capacity fits the empty tile pool.  (Several that fill the frame pool
    // together may need a tile more than it has -- the output count rounds up per utterance -- and then find no room: not a rule)
    for (const Geo& geo : geos)
        for (long long cap = 1; cap <= 400; cap += 7)
            for (int max_live = 1; max_live <= 5; max_live += 2) {
                for (long f = 1; f <= cap; f += std::max<long>(1, (long)cap / 9)) {
                    LiveStream L;
                    L.open(8, max_live, cap, 0);
                    L.halo = 2; L.hop = 256; L.P = geo.P; L.Q = geo.Q; L.H = geo.H;
                    L.open_filters(false, true);
                    int slot = -1;
                    REQUIRE(L.admit(1, &f, nullptr, &slot) && slot == 0, "an utterance of %ld frames fits the empty frame pool of %lld but not the tile pool", f, cap);
                    L.drop_all();
                    REQUIRE(L.free_tiles.size() == 1 && L.free_tiles[0].len == L.capacity_tiles && L.free_ranges.size() == 1, "drop_all");
                }
            }
    // without open_filters nothing of this exists: no tiles are taken, and the stream is the one it was
    {
        LiveStream U;
        U.open(4, 3, 100);
        const long F[2] = {10, 20}; int slots[2];
        REQUIRE(!U.eq_on && !U.loud_on && U.capacity_tiles == 0 && U.free_tiles.empty() && U.admit(2, F, nullptr, slots), "the plain stream");
        REQUIRE(U.slots[0].tn == 0 && U.slots[1].tn == 0 && U.free_tiles.empty() && U.tiles_of(50) == 0, "a plain stream took tiles");
        // a re-opened stream forgets its filters
        U.open(4, 3, 100);
        U.hop = 256;
        U.open_filters(false, true);
        REQUIRE(U.loud_on && !U.eq_on && U.capacity_tiles == 100 * 256 / kLdsTile + 3, "open_filters");
        U.open(4, 3, 100);
        REQUIRE(!U.loud_on && U.capacity_tiles == 0 && U.free_tiles.empty(), "open() keeps the filters of the stream before");
    }
    printf("ok %ld %ld %ld %ld %ld %ld %ld\n", schedules, t.admissions, t.refused, t.refused_tiles, t.steps, t.repeats, t.rows);
    return 0;
}
