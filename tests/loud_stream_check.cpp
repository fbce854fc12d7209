// loud_stream_check.cpp -- the host side of streamed loudness (summertts_amd/csrc/loud_stream.hpp) as a stand-alone program: walks
// utterances through step lists the way the engine and sts_loudness_measure_chunked do and checks every row's invariants -- each input
// sample consumed exactly once and in order, the window covering [e, j1), the tiles touched and their place in the result tables, a
// repeated step starting from the same position and slot.  Prints "ok <rows>" or the first violation.  (Plain C++: tests build it with
// the address and undefined-behaviour sanitizers.)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loud_stream.hpp"

using namespace sts;

static int fail(const char* what, long long a, long long b) { std::printf("FAIL %s %lld %lld\n", what, a, b); return 1; }

int main() {
    static_assert(kLdsOffPrev + 8 <= kLdsOffX && kLdsOffX % 16 == 0, "state layout");
    const long long T = kLdsTile;
    long long rows = 0;
    const long long lens[] = {1, 2, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5, 3 * T + 5};
    const long long steps[] = {1, 7, 32, 1000, T, 3 * T + 100};
    const long long backs[] = {0, 7, 960, 2048};
    for (long long N : lens) for (long long st : steps) for (long long back : backs) for (int retry = 0; retry < 2; retry++) {
        LdsTrack tr; tr.begin(2);
        const long long Ns[2] = {5 * T, N};
        const long long all = tr.layout(Ns);
        if (tr.tbase[0] != 0 || tr.tbase[1] != 6 || all != 6 + N / T + 1) return fail("layout", tr.tbase[1], all);
        std::vector<char> written((size_t)all, 0);
        long long consumed = 0; int slot = 0; long long k = 0;
        for (long long c0 = 0; c0 < N; c0 += st, k++) {
            const long long c1 = std::min(N, c0 + st), o0 = std::max(0LL, c0 - back), o1 = std::min(N, c0 + st + back);
            for (int attempt = 0; attempt <= (retry && k == 1 ? 1 : 0); attempt++) {
                if (attempt) tr.drop();
                if (tr.slot != slot) return fail("slot", tr.slot, slot);
                const LdsRow r = tr.row(1, 100 + o0, o0, o1 - o0, c1);
                if (const char* bad = lds_row_check(r, N)) { std::printf("FAIL %s (N %lld step %lld back %lld)\n", bad, N, st, back); return 1; }
                if (r.e != consumed) return fail("each sample once, in order", r.e, consumed);
                const long long tiles = lds_tiles(r.e, r.j1);
                if (tiles < 1 || tiles > lds_max_tiles(r.j1 - r.e)) return fail("tiles", tiles, lds_max_tiles(r.j1 - r.e));
                if ((r.e / T + tiles - 1) * T > r.j1 || (r.e / T + tiles) * T <= r.j1) return fail("the last tile holds j1", tiles, r.j1);
                // every touched tile has its entry in the tables, inside the utterance's own range
                for (long long t = r.e / T; t < r.e / T + tiles; t++) {
                    if (r.tbase + t < tr.tbase[1] || r.tbase + t >= all) return fail("a tile outside the utterance's tables", t, all);
                    written[(size_t)(r.tbase + t)] = 1;
                }
                rows++;
            }
            tr.commit();
            consumed = c1; slot ^= 1;
            if (tr.e[1] != consumed || tr.e[0] != 0) return fail("commit", tr.e[1], consumed);
        }
        if (consumed != N) return fail("the whole utterance", consumed, N);
        // the gate reads the tiles [0, ceil(N / T)): a step wrote each of them
        for (long long t = 0; t < (N + T - 1) / T; t++) if (!written[(size_t)(tr.tbase[1] + t)]) return fail("a tile the gate reads was never written", t, N);
    }
    // rows the check must refuse
    LdsRow g{0, 0, 0, 100, 100, 0, 0, 0};
    if (lds_row_check(g, 100)) return fail("a good row", 0, 0);
    LdsRow b1 = g; b1.e = 50; b1.u0 = 60;                    // the window starts behind the consumed position
    LdsRow b2 = g; b2.j1 = 101; b2.xlen = 200;               // beyond the utterance
    LdsRow b3 = g; b3.xlen = 99;                             // the window ends before j1
    LdsRow b4 = g; b4.e = 101; b4.j1 = 100;                  // consumed past the step's end
    LdsRow b5 = g; b5.tbase = -1;
    LdsRow b6 = g; b6.xbase = -1;
    for (const LdsRow* r : {&b1, &b2, &b3, &b4, &b5, &b6})
        if (!lds_row_check(*r, 100)) return fail("a bad row passed", r - &b1, 0);
    if (lds_state_bytes(3) != 6 * kLdsSlotBytes || lds_ws_bytes(2, 3) != 2 * 3 * 4 * 8) return fail("sizes", 0, 0);
    if (lds_res_bytes(2, 5) < 2 * 24 + 5 * 16 * 8 + 5 * 4 + 2 * 4) return fail("result tables", 0, 0);
    std::printf("ok %lld\n", rows);
    return 0;
}
