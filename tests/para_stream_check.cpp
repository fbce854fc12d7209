// para_stream_check.cpp -- the host side of an open paragraph (summertts_amd/csrc/para_stream.hpp) driven through seeded random schedules
// of append / step / finish, alone: no HIP, no engine.  Built plain and with -fsanitize=address,undefined by tests/test_para_stream_cpu.py.
//
// stdin, one case per line:  hop C Hd Ho P Q H lead trail max_resident capacity seed n F_0 .. F_{n-1} gap_0 .. gap_{n-1}   (gap_0 = 0)
// stdout, per case: "case n", then one line per operation and a "state" line behind each:
//   A B ok first            an append of B sentences from global index `first`: ok = 1 taken, 0 no room now (nothing changed)
//   S k f0 f1 g0 g1 j0 j1 jl0 jl1 Wtot maxW nw {b w0 w1 coff zoff st en S N xoff}*      a delivered step, as step_build_joined sees it
//   T i                     sentence i retired (behind the S that let it go)
//   F trail                 finish
//   state ready sentences resident free_slots free_frames E
// and "end steps".  Every property that needs no second opinion is checked here (REQUIRE); tests/para_stream_ref.py replays the log.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "para_stream.hpp"

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

struct Kept { JsStep t; std::vector<JsRow> rows; };

void state(const ParaStream& P) {
    printf("state %lld %d %d %d %lld %lld\n", P.ready(), P.sentences(), P.resident(), P.pool.free_slots(), P.pool.free_frames(), P.E);
}

// the resident sentences' column ranges lie inside the pool and do not overlap; the counters agree
void check_pool(const ParaStream& P) {
    std::vector<char> used((size_t)P.pool.capacity, 0);
    long long cols = 0;
    int res = 0;
    for (int i = 0; i < P.sentences(); i++) {
        if (P.slot[(size_t)i] < 0) { REQUIRE(i < P.first_live, "sentence %d lost its slot out of order", i); continue; }
        REQUIRE(i >= P.first_live, "sentence %d is retired and holds a slot", i);
        const LiveSlot& s = P.pool.slots[(size_t)P.slot[(size_t)i]];
        REQUIRE(s.live && s.off == P.zoff[(size_t)i] && s.F == P.js.F[(size_t)i], "sentence %d and its slot disagree", i);
        REQUIRE(s.off >= 0 && s.off + s.F <= P.pool.capacity, "sentence %d leaves the pool", i);
        for (long long c = s.off; c < s.off + s.F; c++) { REQUIRE(!used[(size_t)c], "two resident sentences overlap at column %lld", c); used[(size_t)c] = 1; }
        cols += s.F; res++;
    }
    REQUIRE(res == P.resident() && cols + P.pool.free_frames() == P.pool.capacity, "columns or slots leaked");
}

bool same(const JsStep& a, const JsStep& b) {
    if (a.f0 != b.f0 || a.f1 != b.f1 || a.g0 != b.g0 || a.g1 != b.g1 || a.j0 != b.j0 || a.j1 != b.j1 || a.jl0 != b.jl0 || a.jl1 != b.jl1 ||
        a.Wtot != b.Wtot || a.maxW != b.maxW || a.win.size() != b.win.size()) return false;
    for (size_t i = 0; i < a.win.size(); i++)
        if (a.win[i].b != b.win[i].b || a.win[i].w0 != b.win[i].w0 || a.win[i].w1 != b.win[i].w1 || a.win[i].coff != b.win[i].coff) return false;
    return true;
}

long run_case(long idx) {
    int hop, Hd, Ho, H, max_res, n;
    long long C, P_, Q_, lead, trail, cap;
    unsigned seed;
    if (scanf("%d %lld %d %d %lld %lld %d %lld %lld %d %lld %u %d", &hop, &C, &Hd, &Ho, &P_, &Q_, &H, &lead, &trail, &max_res, &cap, &seed, &n) != 13) return -1;
    std::vector<long> F((size_t)n); std::vector<long long> gap((size_t)n);
    for (long& v : F) REQUIRE(scanf("%ld", &v) == 1, "input");
    for (long long& v : gap) REQUIRE(scanf("%lld", &v) == 1, "input");
    printf("case %d\n", n);
    std::mt19937 rng(seed);
    auto coin = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
    ParaStream P;
    P.open(C, max_res, cap, lead, hop, Hd, Ho, P_, Q_, H);
    check_pool(P);
    std::vector<Kept> kept;
    int next = 0;
    bool one = false;                   // the last append found no room: try a single sentence next
    const double p_append = 0.2 + 0.15 * (double)(seed % 5), p_finish = (seed % 3) == 0 ? 1.0 : 0.3;
    while (true) {
        const bool more = next < n;
        if (P.finished && P.ready() == 0) break;
        const bool must_append = more && P.ready() == 0;
        if (more && (must_append || coin(p_append))) {
            const int B = one ? 1 : (int)std::min<long>(n - next, 1 + (long)(rng() % 3));
            std::vector<int> sid((size_t)B);
            for (int b = 0; b < B; b++) sid[(size_t)b] = 100 + next + b;
            std::vector<long long> st((size_t)B, -1);
            const ParaStream before = P;
            const int ok = B > max_res ? 0 : P.append(B, F.data() + next, sid.data(), gap.data() + next, st.data());
            REQUIRE(ok == 0 || ok == 1, "append answered %d", ok);
            printf("A %d %d %d\n", B, ok, next);
            if (ok) {
                for (int b = 0; b < B; b++) {
                    const int i = next + b;
                    const long long want = i == 0 ? lead : P.js.s[(size_t)i - 1] + P.js.F[(size_t)i - 1] + gap[(size_t)i];
                    REQUIRE(st[(size_t)b] == want && P.js.s[(size_t)i] == want && P.js.F[(size_t)i] == F[(size_t)i] && P.sid[(size_t)i] == 100 + i, "sentence %d is not where the layout puts it", i);
                }
                next += B; one = false;
            } else {
                REQUIRE(P.sentences() == before.sentences() && P.E == before.E && P.js.FJ == before.js.FJ && P.resident() == before.resident() &&
                        P.pool.free_frames() == before.pool.free_frames() && P.pool.free_ranges.size() == before.pool.free_ranges.size(), "a refused append changed the paragraph");
                REQUIRE(!(must_append && one), "stuck: one sentence does not fit and nothing is deliverable (test set-up: pool too small for C + reach)");
                one = true;
            }
            check_pool(P); state(P);
            continue;
        }
        if (!more && !P.finished && (P.ready() == 0 || coin(p_finish))) {
            REQUIRE(P.finish(trail), "finish refused");
            REQUIRE(!P.finish(trail), "a second finish was taken");
            printf("F %lld\n", trail);
            state(P);
            continue;
        }
        if (P.ready() == 0) continue;
        // one step, as Engine::para_step takes it
        const long long k = P.k;
        if (!P.finished) REQUIRE((k + 1) * C + Ho <= P.E, "chunk %lld is delivered while its reach passes E = %lld", k, P.E);
        Kept kp;
        P.js.step(k, kp.t);
        P.js.rows(kp.t.g0, kp.t.g1, kp.t.win, kp.rows);
        if (!P.finished) REQUIRE(kp.t.g1 <= P.E && kp.t.f1 == kp.t.f0 + C, "a clip against the provisional F_J binds");
        {   // the plan the engine's step runs on -- the resident sentences alone -- gives the same step, its windows' b lower by first_live
            const JsPlan rp = P.resident_plan();
            REQUIRE((int)rp.s.size() == P.sentences() - P.first_live && rp.F.size() == rp.s.size() && rp.FJ == P.js.FJ, "the resident plan's sentences");
            JsStep rt; std::vector<JsRow> rrows;
            rp.step(k, rt);
            rp.rows(rt.g0, rt.g1, rt.win, rrows);
            for (JsWin& w : rt.win) w.b += P.first_live;
            REQUIRE(same(rt, kp.t) && rrows.size() == kp.rows.size(), "step %lld of the resident plan differs from the whole plan's", k);
            for (size_t i = 0; i < rrows.size(); i++) {
                const JsRow &a = rrows[i], &b = kp.rows[i];
                REQUIRE(a.st == b.st && a.en == b.en && a.S == b.S && a.N == b.N && a.xoff == b.xoff, "step %lld row %zu of the resident plan differs", k, i);
            }
        }
        printf("S %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %zu", k, kp.t.f0, kp.t.f1, kp.t.g0, kp.t.g1, kp.t.j0, kp.t.j1, kp.t.jl0, kp.t.jl1, kp.t.Wtot,
               kp.t.maxW, kp.t.win.size());
        for (size_t i = 0; i < kp.t.win.size(); i++) {
            const JsWin& w = kp.t.win[i];
            REQUIRE(w.b >= P.first_live && P.slot[(size_t)w.b] >= 0, "step %lld reads sentence %d, which has retired", k, w.b);
            const JsRow& r = kp.rows[i];
            printf(" %d %lld %lld %lld %d %lld %lld %lld %lld %lld", w.b, w.w0, w.w1, w.coff, P.zoff[(size_t)w.b], r.st, r.en, r.S, r.N, r.xoff);
        }
        printf("\n");
        kept.push_back(kp);
        const int fl = P.first_live;
        P.delivered(false);
        for (int i = fl; i < P.first_live; i++) printf("T %d\n", i);
        check_pool(P); state(P);
    }
    // the finished paragraph as a closed plan: every delivered step is its step k, word for word
    JsPlan closed;
    closed.hop = hop; closed.C = C; closed.Hd = Hd; closed.Ho = Ho; closed.P = P_; closed.Q = Q_; closed.H = H;
    std::vector<int> fr(F.begin(), F.end()); std::vector<long long> sil((size_t)n);
    long long acc = lead;
    for (int b = 0; b < n; b++) { acc += gap[(size_t)b]; sil[(size_t)b] = acc; }
    closed.layout(n, fr.data(), sil.data(), acc + trail);
    REQUIRE(closed.FJ == P.js.FJ && closed.s == P.js.s && closed.F == P.js.F, "the finished paragraph is not the closed layout");
    REQUIRE((long long)kept.size() == closed.steps() && P.k == closed.steps(), "%zu chunks left, the closed stream has %lld", kept.size(), closed.steps());
    JsStep t; std::vector<JsRow> rows;
    for (long long k = 0; k < closed.steps(); k++) {
        closed.step(k, t); closed.rows(t.g0, t.g1, t.win, rows);
        REQUIRE(same(t, kept[(size_t)k].t), "step %lld differs from the closed plan's", k);
        REQUIRE(rows.size() == kept[(size_t)k].rows.size(), "step %lld: rows", k);
        for (size_t i = 0; i < rows.size(); i++) {
            const JsRow &a = rows[i], &b = kept[(size_t)k].rows[i];
            REQUIRE(a.st == b.st && a.en == b.en && a.S == b.S && a.N == b.N && a.xoff == b.xoff, "step %lld row %zu differs from the closed plan's", k, i);
        }
    }
    REQUIRE(P.resident() == 0 && P.first_live == n && P.pool.free_ranges.size() == 1 && P.pool.free_ranges[0].off == 0 && P.pool.free_ranges[0].len == cap &&
            P.pool.admitted == P.pool.retired, "the pool does not return to empty");
    printf("end %zu\n", kept.size());
    (void)idx;
    return (long)kept.size();
}

}  // namespace

int main() {
    long cases = 0, steps = 0;
    for (;; cases++) {
        const long s = run_case(cases);
        if (s < 0) break;
        steps += s;
    }
    // a stopped paragraph, the undo of an append, the limits
    ParaStream P;
    P.open(4, 3, 64, 2, 256, 3, 1, 1, 1, 0);
    const long F[3] = {10, 5, 7}; const int sid[3] = {0, 1, 2}; const long long gap[3] = {0, 2, 0};
    REQUIRE(!P.finish(0), "finish without a sentence");
    REQUIRE(P.append(3, F, sid, gap, nullptr) == 1 && P.E == 2 + 10 + 2 + 5 + 7 && P.resident() == 3, "append");
    P.undo(2);
    REQUIRE(P.sentences() == 1 && P.E == 12 && P.resident() == 1 && P.pool.free_frames() == 54 && P.pool.admitted == 1 && P.pool.retired == 0, "undo");
    const long big[1] = {60};
    REQUIRE(P.append(1, big, sid, gap + 2, nullptr) == 0 && P.sentences() == 1, "no room");
    const long huge[1] = {(long)(kParaMaxNative / 256)};
    REQUIRE(P.append(1, huge, sid, gap + 2, nullptr) == -1 && P.sentences() == 1 && P.E == 12, "too long");
    REQUIRE(P.ready() == 2, "ready %lld", P.ready());              // (k + 1) 4 + 1 <= 12: chunks 0 and 1
    P.delivered(true);
    REQUIRE(P.stopped && P.ready() == 0 && P.resident() == 0 && P.pool.free_frames() == 64, "a stopped paragraph drops its sentences");
    // 44.1 kHz from 16 kHz (P / Q = 441 / 160 > 1): the output count passes 2^31 - 1 while N_J is far below 2 10^9, and it alone refuses
    ParaStream Q;
    Q.open(4, 2, 64, 0, 256, 3, 2, 441, 160, 0);
    REQUIRE(Q.fits(3000000) && !Q.fits(3100000) && 3100000LL * 256 < kParaMaxNative && P.fits(3100000), "the output count's limit");
    REQUIRE(Q.js.out_count(3000000LL * 256) <= kParaMaxOut && Q.js.out_count(3100000LL * 256) > kParaMaxOut, "the output count's limit, by hand");
    const long five[1] = {5}; const long long none[1] = {0}, far[1] = {3100000}, near[1] = {2900000};
    REQUIRE(Q.append(1, five, sid, none, nullptr) == 1 && Q.E == 5, "append");
    REQUIRE(Q.append(1, five, sid, far, nullptr) == -1 && Q.sentences() == 1 && Q.E == 5 && Q.resident() == 1, "an append whose output count alone is too long");
    REQUIRE(Q.append(1, five, sid, near, nullptr) == 1 && Q.E == 2900010, "an append below the limit");
    REQUIRE(!Q.finish(150000) && !Q.finished && Q.js.FJ == Q.E, "a trail whose output count alone is too long");
    REQUIRE(Q.finish(50000) && Q.js.FJ == 2950010, "finish below the limit");
    printf("ok %ld %ld\n", cases, steps);
    return 0;
}
