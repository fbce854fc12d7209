// pitch_layout_check.cpp -- the pitch plan's layout arithmetic (summertts_amd/csrc/pitch_layout.hpp) as a stand-alone program:
// tests/test_pitch_plan_cpu.py builds it with -fsanitize=undefined (a signed 64-bit overflow ends it) and compares every printed line
// with tests/pitch_ref.py.  One line per case: "hop n | d .. | cents .. | step .. | o .. | e .." or "hop n | d .. | cents .. | refused".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pitch_layout.hpp"

using namespace sts;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

static void run(int hop, const std::vector<int32_t>& d, const std::vector<int32_t>& cents) {
    const int n = (int)d.size();
    std::vector<int64_t> step(n), o(n + 1), e(n + 1);
    for (int i = 0; i < n; i++) step[i] = pitch_step(cents[i]);
    printf("%d %d |", hop, n);
    for (int i = 0; i < n; i++) printf(" %d", d[i]);
    printf(" |");
    for (int i = 0; i < n; i++) printf(" %d", cents[i]);
    if (!pitch_layout(d.data(), step.data(), n, hop, o.data(), e.data())) { printf(" | refused\n"); return; }
    printf(" |");
    for (int i = 0; i < n; i++) printf(" %lld", (long long)step[i]);
    printf(" |");
    for (int i = 0; i <= n; i++) printf(" %lld", (long long)o[i]);
    printf(" |");
    for (int i = 0; i <= n; i++) printf(" %lld", (long long)e[i]);
    printf("\n");
}

int main() {
    // the largest signals the layout admits, at both ends of the step range and mixed: N just below 2^30
    for (int c : {-600, -1, 0, 1, 600}) {
        run(1 << 20, {1023}, {c});
        run(1 << 20, {1000, 0, 23}, {c, -c, 600});
        run(10737, {100000}, {c});
        run(1, {100000, 100000, 100000, 100000, 100000}, {c, 600, -600, c, 0});
        run(16384, {65535}, {c});
    }
    // ... and just past it: refused, not wrapped
    run(1 << 20, {1024}, {0});
    run(1 << 20, {1000, 24}, {600, -600});
    run(10738, {100000}, {0});
    run(16384, {65536}, {-600});
    // hop 1, one-frame phonemes at +600: stepped over
    run(1, std::vector<int32_t>(64, 1), std::vector<int32_t>(64, 600));
    // all durations 0; runs of empty phonemes
    run(256, {0, 0, 0}, {600, -600, 0});
    run(6, {0, 0, 5, 0, 0, 0, 3, 0, 0}, {600, -600, 37, 600, 600, -1, -600, 0, 600});
    // seeded random cases
    for (int k = 0; k < 200; k++) {
        const int hops[] = {1, 2, 6, 16, 256, 300, 4096};
        const int hop = hops[rnd() % 7], n = 1 + (int)(rnd() % 24);
        std::vector<int32_t> d(n), cents(n);
        for (int i = 0; i < n; i++) {
            const uint32_t r = rnd() % 8;
            d[i] = r < 2 ? 0 : (r < 4 ? 1 : (int)(rnd() % 40));
            const uint32_t q = rnd() % 6;
            cents[i] = q == 0 ? 600 : q == 1 ? -600 : q == 2 ? 0 : (int)(rnd() % 1201) - 600;
        }
        run(hop, d, cents);
    }
    return 0;
}
