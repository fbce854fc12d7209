// live_tables_check.cpp -- the host side of a PLANNED open stream (summertts_amd/csrc/live_stream.hpp): slots, frame ranges and phoneme
// ranges driven through seeded random schedules of admit / step / stop / retire against brute force, alone: no HIP, no engine.  Built with
// -fsanitize=address,undefined by tests/test_live_tables_cpu.py and run directly.
// Prints "ok <schedules> <admissions> <refused> <refused for phonemes alone> <steps>" or the first violated property.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "live_stream.hpp"

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

// one resource's ranges: live ones never overlap and stay inside [0, cap); free ones ascend, never touch, never overlap a live one; the
// two kinds cover [0, cap) exactly
void check_ranges(const char* what, long long cap, const std::vector<LiveRange>& live, const std::vector<LiveRange>& free_) {
    std::vector<char> used((size_t)cap, 0);
    long long nlive = 0, nfree = 0, prev_end = -1;
    for (const LiveRange& r : live) {
        REQUIRE(r.off >= 0 && r.len > 0 && r.off + r.len <= cap, "%s: a live range leaves [0, capacity): off %lld len %lld", what, r.off, r.len);
        for (long long c = r.off; c < r.off + r.len; c++) { REQUIRE(!used[(size_t)c], "%s: two live ranges overlap at column %lld", what, c); used[(size_t)c] = 1; }
        nlive += r.len;
    }
    for (const LiveRange& r : free_) {
        REQUIRE(r.len > 0 && r.off >= 0 && r.off + r.len <= cap, "%s: a free range leaves [0, capacity)", what);
        REQUIRE(r.off > prev_end, "%s: free ranges are not ascending, or two adjacent ones did not coalesce", what);
        for (long long c = r.off; c < r.off + r.len; c++) { REQUIRE(!used[(size_t)c], "%s: a free range overlaps a live one at column %lld", what, c); used[(size_t)c] = 2; }
        nfree += r.len; prev_end = r.off + r.len;
    }
    REQUIRE(nlive + nfree == cap, "%s: columns leaked: %lld live + %lld free of %lld", what, nlive, nfree, cap);
}

void check_state(const LiveStream& L) {
    std::vector<LiveRange> fl, pl;
    for (const LiveSlot& s : L.slots) {
        if (!s.live) { REQUIRE(s.pn == 0 && !s.has_gain && s.poff == 0, "a free slot keeps phonemes"); continue; }
        REQUIRE(s.F > 0 && s.f >= 0 && s.f < s.F, "a live slot has delivered everything");
        fl.push_back(LiveRange{s.off, s.F});
        REQUIRE(s.has_gain == (s.pn > 0), "has_gain disagrees with the count");
        if (s.pn > 0) pl.push_back(LiveRange{s.poff, s.pn});
    }
    check_ranges("frames", L.capacity, fl, L.free_ranges);
    check_ranges("phonemes", L.capacity_phonemes, pl, L.free_phonemes);
    long long fp = 0;
    for (const LiveRange& r : L.free_phonemes) fp += r.len;
    REQUIRE(L.free_phoneme_count() == fp && L.live_count() + L.free_slots() == L.max_live, "the counters disagree with the tables");
    bool any = false;
    for (const LiveSlot& s : L.slots) any = any || (s.live && s.has_gain);
    REQUIRE(L.any_gain() == any, "any_gain disagrees with the slots");
}

std::vector<char> occupancy(long long cap, const LiveStream& L, bool phonemes) {
    std::vector<char> used((size_t)cap, 0);
    for (const LiveSlot& s : L.slots) {
        if (!s.live) continue;
        const long long o = phonemes ? s.poff : s.off, n = phonemes ? s.pn : s.F;
        for (long long c = o; c < o + n; c++) used[(size_t)c] = 1;
    }
    return used;
}
// the lowest offset at which `len` free columns start, by brute force over the occupancy (-1: nowhere)
long long first_fit(const std::vector<char>& used, long long len) {
    long long run = 0;
    for (size_t c = 0; c < used.size(); c++) {
        run = used[c] ? 0 : run + 1;
        if (run == len) return (long long)c + 1 - len;
    }
    return -1;
}
// an admission's placements in one resource, in order b = 0 .. B - 1 (len 0: takes none); false: some utterance finds no room
bool place_all(std::vector<char> used, const std::vector<long long>& len, std::vector<long long>& want) {
    want.assign(len.size(), -1);
    for (size_t b = 0; b < len.size(); b++) {
        if (len[b] == 0) continue;
        if ((want[b] = first_fit(used, len[b])) < 0) return false;
        for (long long c = want[b]; c < want[b] + len[b]; c++) used[(size_t)c] = 1;
    }
    return true;
}

bool same(const LiveStream& a, const LiveStream& b) {
    if (a.slots.size() != b.slots.size() || a.free_ranges.size() != b.free_ranges.size() || a.free_phonemes.size() != b.free_phonemes.size() ||
        a.admitted != b.admitted || a.retired != b.retired) return false;
    for (size_t s = 0; s < a.slots.size(); s++) {
        const LiveSlot &x = a.slots[s], &y = b.slots[s];
        if (x.live != y.live || x.off != y.off || x.F != y.F || x.f != y.f || x.sid != y.sid || x.poff != y.poff || x.pn != y.pn || x.has_gain != y.has_gain) return false;
    }
    for (size_t r = 0; r < a.free_ranges.size(); r++) if (a.free_ranges[r].off != b.free_ranges[r].off || a.free_ranges[r].len != b.free_ranges[r].len) return false;
    for (size_t r = 0; r < a.free_phonemes.size(); r++) if (a.free_phonemes[r].off != b.free_phonemes[r].off || a.free_phonemes[r].len != b.free_phonemes[r].len) return false;
    return true;
}

struct Tally { long admissions = 0, refused = 0, refused_phonemes = 0, steps = 0; };

// utterance u: F[u] frames, N[u] phonemes in its gain plan (0: it carries none)
void run_schedule(unsigned seed, int chunk, int max_live, long long cap, long long capP, const std::vector<long>& F, const std::vector<int>& N, double p_stop, Tally& t) {
    std::mt19937 rng(seed);
    auto coin = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
    LiveStream L;
    L.open(chunk, max_live, cap, capP);
    L.halo = 2; L.hop = 256;
    REQUIRE(L.planned() && L.free_phoneme_count() == capP, "open");
    check_state(L);
    size_t next = 0;
    bool one = false;
    while (next < F.size() || L.live_count() > 0) {
        if (next < F.size() && (L.live_count() == 0 || coin(0.45))) {
            const int B = one ? 1 : (int)std::min<size_t>(F.size() - next, 1 + rng() % 3);
            one = false;
            std::vector<long> Fb(F.begin() + (long)next, F.begin() + (long)next + B);
            std::vector<int> Nb(N.begin() + (long)next, N.begin() + (long)next + B), sid((size_t)B), slots((size_t)B, -7);
            std::vector<long long> lenF((size_t)B), lenP((size_t)B), wantF, wantP;
            int need = 0;
            for (int b = 0; b < B; b++) {
                sid[(size_t)b] = (int)next + b;
                lenF[(size_t)b] = Fb[(size_t)b]; lenP[(size_t)b] = Fb[(size_t)b] > 0 ? Nb[(size_t)b] : 0;    // (no frames: no slot, no phonemes)
                need += Fb[(size_t)b] > 0;
            }
            const LiveStream before = L;
            const bool fit_s = need <= L.free_slots();
            const bool fit_f = place_all(occupancy(cap, L, false), lenF, wantF);
            const bool fit_p = place_all(occupancy(capP, L, true), lenP, wantP);
            const bool ok = L.admit(B, Fb.data(), sid.data(), Nb.data(), slots.data());
            REQUIRE(ok == (fit_s && fit_f && fit_p), "admit answered %d where brute force says slots %d frames %d phonemes %d", (int)ok, (int)fit_s, (int)fit_f, (int)fit_p);
            if (!ok) {
                REQUIRE(same(L, before), "a refused admission changed the state");
                for (int b = 0; b < B; b++) REQUIRE(slots[(size_t)b] == -7, "a refused admission wrote a slot");
                t.refused++;
                if (fit_s && fit_f) t.refused_phonemes++;
                REQUIRE(L.live_count() > 0 || B > 1, "one utterance does not fit the empty pools (test set-up)");
                one = L.live_count() == 0;
            } else {
                std::vector<char> taken((size_t)max_live, 0);
                for (size_t s = 0; s < before.slots.size(); s++) taken[s] = before.slots[s].live;
                for (int b = 0; b < B; b++) {
                    if (Fb[(size_t)b] == 0) { REQUIRE(slots[(size_t)b] == -1, "an utterance without frames took a slot"); continue; }
                    const int s = slots[(size_t)b];
                    REQUIRE(s >= 0 && s < max_live && L.slots[(size_t)s].live, "slot out of range");
                    const int lowest = (int)(std::find(taken.begin(), taken.end(), 0) - taken.begin());
                    REQUIRE(s == lowest, "slot %d taken, the lowest free one is %d", s, lowest);
                    taken[(size_t)s] = 1;
                    const LiveSlot& sl = L.slots[(size_t)s];
                    REQUIRE(sl.off == wantF[(size_t)b] && sl.F == Fb[(size_t)b] && sl.f == 0 && sl.sid == sid[(size_t)b], "frames: not first fit, or not what was admitted");
                    REQUIRE(sl.pn == Nb[(size_t)b] && sl.has_gain == (Nb[(size_t)b] > 0), "phonemes: not what was admitted");
                    if (sl.pn > 0) REQUIRE(sl.poff == wantP[(size_t)b], "phonemes: at %lld, first fit is %lld", sl.poff, wantP[(size_t)b]);
                }
                next += (size_t)B;
                t.admissions++;
            }
            check_state(L);
            continue;
        }
        std::vector<int> order;
        L.step_slots(order);
        for (const int s : order) {
            const LiveSlot sl = L.slots[(size_t)s];
            const bool stop = coin(p_stop), last = sl.f + chunk >= sl.F;
            const long long fp = L.free_phoneme_count(), ff = L.free_frames();
            const bool retired = L.delivered(s, stop);
            REQUIRE(retired == (stop || last), "slot %d retired %d, stop %d last %d", s, (int)retired, (int)stop, (int)last);
            if (retired) REQUIRE(L.free_phoneme_count() == fp + sl.pn && L.free_frames() == ff + sl.F && !L.slots[(size_t)s].live, "a retirement did not return its ranges");
            else REQUIRE(L.free_phoneme_count() == fp && L.free_frames() == ff, "a step moved ranges");
        }
        t.steps++;
        check_state(L);
    }
    REQUIRE(L.free_ranges.size() == 1 && L.free_ranges[0].off == 0 && L.free_ranges[0].len == cap, "a full drain does not leave one free frame range");
    REQUIRE(L.free_phonemes.size() == 1 && L.free_phonemes[0].off == 0 && L.free_phonemes[0].len == capP, "a full drain does not leave one free phoneme range");
    REQUIRE(L.admitted == L.retired, "admitted %lld, retired %lld", L.admitted, L.retired);
}

}  // namespace

int main() {
    Tally t;
    long schedules = 0;
    for (unsigned set = 0; set < 30; set++) {
        std::mt19937 rng(4242 + set);
        const int max_live = 3 + (int)(rng() % 5);
        std::vector<long> F(40); std::vector<int> N(40);
        for (size_t u = 0; u < F.size(); u++) { F[u] = (long)(rng() % 60); N[u] = rng() % 3 == 0 ? 0 : 1 + (int)(rng() % 40); }   // (some without frames, a third without a plan)
        F[2] = 1; N[2] = 1; F[6] = 0; N[6] = 9;
        // frames are plentiful (every slot can hold the longest), phonemes are scarce: the phoneme pool decides most refusals
        const long long cap = (long long)max_live * 60, capP = 40 + (long long)(rng() % 30);
        for (unsigned sched = 0; sched < 4; sched++) {
            run_schedule(31 * sched + set, 1 + (int)(rng() % 20), max_live, cap, capP, F, N, 0.02 * sched, t);
            schedules++;
        }
    }
    // drop_all leaves one range in each list, and the unplanned form takes no phonemes
    {
        LiveStream L;
        L.open(4, 3, 100, 50);
        const long F[2] = {10, 20}; const int sid[2] = {0, 1}, n[2] = {7, 0}; int slots[2];
        REQUIRE(L.admit(2, F, sid, n, slots) && L.free_phoneme_count() == 43 && L.any_gain(), "admit");
        L.drop_all();
        REQUIRE(L.free_ranges.size() == 1 && L.free_ranges[0].len == 100 && L.free_phonemes.size() == 1 && L.free_phonemes[0].off == 0 && L.free_phonemes[0].len == 50, "drop_all");
        LiveStream U;
        U.open(4, 3, 100);
        REQUIRE(!U.planned() && U.free_phonemes.empty() && U.admit(2, F, sid, slots) && !U.any_gain(), "the unplanned stream");
        REQUIRE(!U.admit(1, F, sid, n, slots) && U.live_count() == 2, "an unplanned stream has no phoneme columns to give");
    }
    printf("ok %ld %ld %ld %ld %ld\n", schedules, t.admissions, t.refused, t.refused_phonemes, t.steps);
    return 0;
}
