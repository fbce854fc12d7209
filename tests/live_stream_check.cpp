// live_stream_check.cpp -- the host side of an open stream (summertts_amd/csrc/live_stream.hpp) driven through seeded random schedules of
// admit / step / stop, alone: no HIP, no engine.  Built with -fsanitize=address,undefined by tests/test_live_stream_cpu.py and run directly.
// Prints "ok <schedules> <admissions> <refused> <steps>" or the first violated property.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <random>
#include <tuple>
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

struct Facts { int C, halo, hop; long long P, Q, H; };
using WinKey = std::tuple<long, long, long, long, long long, long long>;      // (f0, f1, w0, w1, j0, j1)

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// what a slot of F frames must see, written out independently of stream_window: chunk k = frames [k C, min(F, (k + 1) C))
std::vector<WinKey> expected_windows(long F, const Facts& f) {
    std::vector<WinKey> out;
    for (long f0 = 0; f0 < F; f0 += f.C) {
        const long f1 = f0 + f.C < F ? f0 + f.C : F;
        const long w0 = f0 - f.halo > 0 ? f0 - f.halo : 0, w1 = f1 + f.halo < F ? f1 + f.halo : F;
        out.emplace_back(f0, f1, w0, w1, ceil_div((long long)f0 * f.hop * f.P, f.Q), ceil_div((long long)f1 * f.hop * f.P, f.Q));
    }
    return out;
}

// every property of the state that must hold between any two operations
void check_state(const LiveStream& L) {
    std::vector<char> used((size_t)L.capacity, 0);
    long long live_cols = 0;
    for (const LiveSlot& s : L.slots) {
        if (!s.live) continue;
        REQUIRE(s.off >= 0 && s.F > 0 && s.off + s.F <= L.capacity, "a live range leaves [0, capacity): off %lld F %ld", s.off, s.F);
        REQUIRE(s.f >= 0 && s.f < s.F, "a live slot has delivered everything: f %ld F %ld", s.f, s.F);
        for (long long c = s.off; c < s.off + s.F; c++) { REQUIRE(!used[(size_t)c], "two live ranges overlap at column %lld", c); used[(size_t)c] = 1; }
        live_cols += s.F;
    }
    long long free_cols = 0, prev_end = -1;
    for (const LiveRange& r : L.free_ranges) {
        REQUIRE(r.len > 0 && r.off >= 0 && r.off + r.len <= L.capacity, "a free range leaves [0, capacity)");
        REQUIRE(r.off > prev_end, "free ranges are not ascending, or two adjacent ones did not coalesce (off %lld after end %lld)", r.off, prev_end);
        for (long long c = r.off; c < r.off + r.len; c++) { REQUIRE(!used[(size_t)c], "a free range overlaps a live one at column %lld", c); used[(size_t)c] = 2; }
        free_cols += r.len; prev_end = r.off + r.len;
    }
    REQUIRE(live_cols + free_cols == L.capacity, "columns leaked: %lld live + %lld free of %lld", live_cols, free_cols, L.capacity);
    REQUIRE(L.free_frames() == free_cols && L.live_count() + L.free_slots() == L.max_live, "the counters disagree with the tables");
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

struct Tally { long admissions = 0, refused = 0, steps = 0; };

// One schedule over the utterances F[]: admissions of 1..3 utterances in order, steps, stops.  Returns every utterance's window sequence
// (only of utterances that were never stopped) and its placement (slot, offset), and checks every property on the way.
void run_schedule(unsigned seed, const Facts& f, int max_live, long long capacity, const std::vector<long>& F, double p_stop,
                  std::map<int, std::vector<WinKey>>& seen, std::vector<std::pair<int, long long>>& placed, Tally& t) {
    std::mt19937 rng(seed);
    auto coin = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
    LiveStream L;
    L.open(f.C, max_live, capacity);
    L.halo = f.halo; L.hop = f.hop; L.P = f.P; L.Q = f.Q; L.H = f.H;
    check_state(L);
    std::vector<int> utt_of((size_t)max_live, -1);
    std::vector<char> stopped(F.size(), 0);
    placed.assign(F.size(), std::make_pair(-2, -1LL));
    size_t next = 0;
    bool one = false;               // the last admission did not fit the EMPTY pool: its first utterance alone does
    while (next < F.size() || L.live_count() > 0) {
        const bool can_admit = next < F.size();
        if (can_admit && (L.live_count() == 0 || coin(0.4))) {
            const int B = one ? 1 : (int)std::min<size_t>(F.size() - next, 1 + rng() % 3);
            one = false;
            std::vector<long> Fb(F.begin() + (long)next, F.begin() + (long)next + B);
            std::vector<int> sid((size_t)B), slots((size_t)B, -7);
            for (int b = 0; b < B; b++) sid[(size_t)b] = (int)(next + (size_t)b);
            const LiveStream before = L;
            // what first fit must give, from the occupancy alone
            std::vector<char> used((size_t)capacity, 0);
            for (const LiveSlot& s : L.slots) if (s.live) for (long long c = s.off; c < s.off + s.F; c++) used[(size_t)c] = 1;
            std::vector<long long> want((size_t)B, -1);
            bool fits = true; int need = 0;
            for (int b = 0; b < B && fits; b++) {
                if (Fb[(size_t)b] == 0) continue;
                need++;
                want[(size_t)b] = first_fit(used, Fb[(size_t)b]);
                if (want[(size_t)b] < 0) { fits = false; break; }
                for (long long c = want[(size_t)b]; c < want[(size_t)b] + Fb[(size_t)b]; c++) used[(size_t)c] = 1;
            }
            fits = fits && need <= L.free_slots();
            const bool ok = L.admit(B, Fb.data(), sid.data(), slots.data());
            REQUIRE(ok == fits, "admit answered %d where brute force says %d", (int)ok, (int)fits);
            if (!ok) {
                // nothing may have changed
                REQUIRE(L.slots.size() == before.slots.size() && L.free_ranges.size() == before.free_ranges.size() && L.admitted == before.admitted &&
                        L.retired == before.retired, "a refused admission changed the tables' sizes or the counters");
                for (size_t s = 0; s < L.slots.size(); s++)
                    REQUIRE(L.slots[s].live == before.slots[s].live && L.slots[s].off == before.slots[s].off && L.slots[s].F == before.slots[s].F &&
                            L.slots[s].f == before.slots[s].f && L.slots[s].sid == before.slots[s].sid, "a refused admission changed slot %zu", s);
                for (size_t r = 0; r < L.free_ranges.size(); r++)
                    REQUIRE(L.free_ranges[r].off == before.free_ranges[r].off && L.free_ranges[r].len == before.free_ranges[r].len, "a refused admission changed a free range");
                for (int b = 0; b < B; b++) REQUIRE(slots[(size_t)b] == -7, "a refused admission wrote a slot");
                t.refused++;
                REQUIRE(L.live_count() > 0 || B > 1, "one utterance does not fit the empty pool (test set-up)");
                one = L.live_count() == 0;
            } else {
                std::vector<char> taken((size_t)max_live, 0);
                for (size_t s = 0; s < before.slots.size(); s++) taken[s] = before.slots[s].live;
                for (int b = 0; b < B; b++) {
                    const int u = (int)next + b;
                    if (Fb[(size_t)b] == 0) { REQUIRE(slots[(size_t)b] == -1, "an utterance without frames took a slot"); placed[(size_t)u] = {-1, -1}; continue; }
                    const int s = slots[(size_t)b];
                    REQUIRE(s >= 0 && s < max_live && L.slots[(size_t)s].live, "slot out of range");
                    const int lowest = (int)(std::find(taken.begin(), taken.end(), 0) - taken.begin());
                    REQUIRE(s == lowest, "utterance %d took slot %d, the lowest free one is %d", u, s, lowest);
                    taken[(size_t)s] = 1;
                    REQUIRE(L.slots[(size_t)s].off == want[(size_t)b], "utterance %d lies at %lld, first fit is %lld", u, L.slots[(size_t)s].off, want[(size_t)b]);
                    REQUIRE(L.slots[(size_t)s].F == Fb[(size_t)b] && L.slots[(size_t)s].f == 0 && L.slots[(size_t)s].sid == u, "the slot does not hold what was admitted");
                    utt_of[(size_t)s] = u;
                    placed[(size_t)u] = {s, L.slots[(size_t)s].off};
                }
                next += (size_t)B;
                t.admissions++;
            }
            check_state(L);
            continue;
        }
        // one step: every live slot, ascending, at its own frame
        std::vector<int> order;
        L.step_slots(order);
        REQUIRE(std::is_sorted(order.begin(), order.end()) && (int)order.size() == L.live_count(), "a step does not walk the live slots in ascending order");
        for (const int s : order) {
            const int u = utt_of[(size_t)s];
            const StreamWin w = L.window(s);
            REQUIRE(w.jl0 <= w.j0 && w.j1 <= w.jl1 && w.jl1 <= w.Nout && w.jl0 >= 0 && w.w0 <= w.f0 && w.f1 <= w.w1, "window out of order");
            REQUIRE(w.jl0 == (f.H > 0 ? std::max<long long>(0, w.j0 - 2 * f.H) : w.j0) && w.jl1 == (f.H > 0 ? std::min<long long>(w.Nout, w.j1 + 2 * f.H) : w.j1),
                    "the limiter's widened range");
            seen[u].emplace_back(w.f0, w.f1, w.w0, w.w1, w.j0, w.j1);
            const bool stop = coin(p_stop);
            if (stop) stopped[(size_t)u] = 1;
            const bool last = w.f1 >= F[(size_t)u];
            const bool retired = L.delivered(s, stop);
            REQUIRE(retired == (stop || last), "slot %d retired %d, stop %d last %d", s, (int)retired, (int)stop, (int)last);
            if (retired) utt_of[(size_t)s] = -1;
        }
        t.steps++;
        check_state(L);
    }
    REQUIRE(L.live_count() == 0 && L.free_ranges.size() == 1 && L.free_ranges[0].off == 0 && L.free_ranges[0].len == capacity,
            "a full drain does not leave one free range");
    REQUIRE(L.admitted == L.retired, "admitted %lld, retired %lld", L.admitted, L.retired);
    for (size_t u = 0; u < F.size(); u++) if (stopped[u]) seen.erase((int)u);
}

}  // namespace

int main() {
    const Facts facts[] = {{7, 3, 256, 1, 1, 0}, {1, 5, 256, 441, 160, 0}, {16, 9, 256, 3, 1, 48}, {5, 2, 64, 1, 2, 8}, {100000, 4, 256, 147, 80, 0}};
    Tally t;
    long schedules = 0;
    for (const Facts& f : facts)
        for (unsigned set = 0; set < 6; set++) {
            std::mt19937 rng(1000 * set + (unsigned)f.C);
            const int max_live = 1 + (int)(rng() % 6);
            std::vector<long> F(24);
            for (long& v : F) v = (long)(rng() % 70);            // (0 frames among them)
            F[3] = 1; F[5] = 0;
            const long long capacity = 70 + (long long)(rng() % 140);
            // the same utterances through different schedules: what a slot sees may not depend on them; the same schedule twice: the same placement
            std::map<int, std::vector<WinKey>> first;
            for (unsigned sched = 0; sched < 5; sched++) {
                std::map<int, std::vector<WinKey>> seen, again;
                std::vector<std::pair<int, long long>> placed, placed2;
                const double p_stop = sched == 0 ? 0.0 : 0.03 * sched;
                run_schedule(77 * sched + set, f, max_live, capacity, F, p_stop, seen, placed, t);
                run_schedule(77 * sched + set, f, max_live, capacity, F, p_stop, again, placed2, t);
                REQUIRE(placed == placed2 && seen == again, "the same schedule placed or stepped differently the second time");
                for (const auto& kv : seen) {
                    REQUIRE(kv.second == expected_windows(F[(size_t)kv.first], f), "utterance %d of F %ld saw a window sequence that depends on the schedule", kv.first,
                            F[(size_t)kv.first]);
                    if (sched == 0) first[kv.first] = kv.second; else if (first.count(kv.first)) REQUIRE(first[kv.first] == kv.second, "two schedules, two sequences");
                }
                schedules += 2;
            }
        }
    printf("ok %ld %ld %ld %ld\n", schedules, t.admissions, t.refused, t.steps);
    return 0;
}
