// eq_stream_check.cpp -- the host side of the streamed equaliser (summertts_amd/csrc/eq_stream.hpp) as a stand-alone program: walks
// utterances through step lists the way the engine and sts_eq_apply_chunked do and checks every row's invariants -- each input sample
// consumed exactly once and in order, the window covering [e, o1), the re-presented part inside the carried history, the tiles touched,
// a repeated step starting from the same position and slot.  Prints "ok <rows>" or the first violation.  (Plain C++: tests build it with
// the address and undefined-behaviour sanitizers.)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eq_stream.hpp"

using namespace sts;

static int fail(const char* what, long long a, long long b) { std::printf("FAIL %s %lld %lld\n", what, a, b); return 1; }

int main() {
    static_assert(kEqsOffPrev + 16 <= kEqsOffX && kEqsOffX % 16 == 0 && kEqsOffY % 16 == 0, "state layout");
    const long long T = kEqsTile;
    long long rows = 0;
    const long long lens[] = {1, 2, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5, 3 * T + 5};
    const long long steps[] = {1, 7, 32, 1000, T, 3 * T + 100};
    const long long backs[] = {0, 7, 960, 2048};
    for (long long N : lens) for (long long st : steps) for (long long back : backs) for (int retry = 0; retry < 2; retry++) {
        EqsTrack tr; tr.begin(2);
        long long consumed = 0; int slot = 0; long long k = 0;
        for (long long c0 = 0; c0 < N; c0 += st, k++) {
            const long long c1 = std::min(N, c0 + st), o0 = std::max(0LL, c0 - back), o1 = std::min(N, c0 + st + back);
            for (int attempt = 0; attempt <= (retry && k == 1 ? 1 : 0); attempt++) {
                if (attempt) tr.drop();
                if (tr.slot != slot) return fail("slot", tr.slot, slot);
                const EqsRow r = tr.row(1, 100 + o0, o0, o1 - o0, o0, o1, 0, c0, c1, c0);
                if (const char* bad = eqs_row_check(r, N)) { std::printf("FAIL %s (N %lld step %lld back %lld)\n", bad, N, st, back); return 1; }
                if (r.e != consumed) return fail("each sample once, in order", r.e, consumed);
                const long long tiles = eqs_tiles(r.e, r.o1);
                if (tiles < 1 || tiles > eqs_max_tiles(r.o1 - r.e)) return fail("tiles", tiles, eqs_max_tiles(r.o1 - r.e));
                if ((r.e / T + tiles - 1) * T > r.o1 || (r.e / T + tiles) * T <= r.o1) return fail("the last tile holds o1", tiles, r.o1);
                rows++;
            }
            tr.commit();
            consumed = o1; slot ^= 1;
            if (tr.e[1] != consumed || tr.e[0] != 0) return fail("commit", tr.e[1], consumed);
        }
        if (consumed != N) return fail("the whole utterance", consumed, N);
    }
    // rows the check must refuse
    EqsRow g{0, 0, 0, 100, 0, 100, 0, 0, 100, 0, 0, 0};
    if (eqs_row_check(g, 100)) return fail("a good row", 0, 0);
    EqsRow b1 = g; b1.e = 50; b1.u0 = 60;                    // the window starts behind the consumed position
    EqsRow b2 = g; b2.o1 = 101;                              // beyond the utterance
    EqsRow b3 = g; b3.e = 5000; b3.o1 = 5000 + 10; b3.xlen = 6000; b3.j0 = b3.j1 = 900; b3.o0 = 5000 - kEqsHist - 1;   // history too short
    EqsRow b4 = g; b4.j1 = 101;
    EqsRow b5 = g; b5.o0 = 10;                               // a gap in front of the range
    EqsRow b6 = g; b6.xlen = 99;
    for (const EqsRow* r : {&b1, &b2, &b3, &b4, &b5, &b6})
        if (!eqs_row_check(*r, r == &b3 ? 6000 : 100)) return fail("a bad row passed", r - &b1, 0);
    if (eqs_state_bytes(3) != 6 * kEqsSlotBytes || eqs_ws_bytes(2, 3) != 2 * 3 * 8 * 8) return fail("sizes", 0, 0);
    std::printf("ok %lld\n", rows);
    return 0;
}
