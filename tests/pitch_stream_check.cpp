// pitch_stream_check.cpp -- the geometry of a stream through the pitch warp (summertts_amd/csrc/pitch_stream.hpp) and the warped step of
// stream_step.hpp as a stand-alone program: tests/test_pitch_stream_cpu.py builds it with -fsanitize=address,undefined, and compares every
// printed word with tests/pitch_stream_ref.py.  It walks whole closed streams through step_build and prints
//   C hop C P Q H K dec_halo halo srs slim B            one stream
//   U b F zoff sid planned n | d .. | cents ..           its utterances
//   S k nw Wtot maxW dsum ysum max_rs max_out max_yl packed_end
//   W k i b | ints 6 | RsRow 5 | LimRow 7 | PsRow 10 | seg 2 | j0 n dst
//   E steps                                              the stream's end
// and "R reason" where the builder refuses a step.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "stream_step.hpp"

using namespace sts;

struct U { std::vector<int32_t> d, cents; bool planned; };

// the warp's tables as pitch_tables lays them out (kernels.hpp PitchTables::words): [member x 6 | oend | pos0 | step | c | K]
static bool tables(const std::vector<U>& us, int hop, std::vector<long long>& words, long long* TTo) {
    const int B = (int)us.size();
    long long TT = 0;
    for (const U& u : us) TT += u.planned ? (long long)u.d.size() : 0;
    words.assign((size_t)6 * B + 5 * (size_t)TT, 0);
    long long *oend = words.data() + 6 * (size_t)B, *pos0 = oend + TT, *st = pos0 + TT;
    long long toff = 0, yoff = 0, xoff = 0;
    for (int b = 0; b < B; b++) {
        const U& u = us[(size_t)b];
        const int n = (int)u.d.size();
        long long frames = 0;
        for (int v : u.d) frames += v;
        const long long N = (frames > 0 ? frames : 1) * hop;
        long long nout = N, np = 0;
        if (u.planned) {
            std::vector<int64_t> step((size_t)n), o((size_t)n + 1), e((size_t)n + 1);
            for (int i = 0; i < n; i++) step[(size_t)i] = pitch_step(u.cents[(size_t)i]);
            if (frames > 0) {
                if (!pitch_layout(u.d.data(), step.data(), n, hop, o.data(), e.data())) return false;
                long long a = 0;
                for (int i = 0; i < n; i++) {
                    oend[toff + i] = o[(size_t)i + 1]; pos0[toff + i] = ((a * hop) << 32) + e[(size_t)i]; st[toff + i] = step[(size_t)i];
                    a += u.d[(size_t)i];
                }
                nout = o[(size_t)n]; np = n;
            } else { oend[toff] = hop; pos0[toff] = 0; st[toff] = kPitchOne; nout = hop; np = 1; }
        }
        long long* m = words.data() + 6 * (size_t)b;
        m[0] = xoff; m[1] = N; m[2] = yoff; m[3] = nout; m[4] = toff; m[5] = np;
        xoff += N; yoff += nout; toff += u.planned ? n : 0;
    }
    *TTo = TT;
    return true;
}

static void words_of(const char* p, int n) { for (int i = 0; i < n; i++) { long long v; memcpy(&v, p + 8 * i, 8); printf(" %lld", v); } }

static void stream(int hop, long C, long long P, long long Q, long long H, long long K, long dec_halo, const std::vector<U>& us) {
    const int B = (int)us.size();
    std::vector<long long> words; long long TT = 0;
    if (!tables(us, hop, words, &TT)) { printf("R layout refused\n"); return; }
    const bool srs = K > 0, slim = H > 0;
    long long extra = srs ? K : 0;
    if (slim) extra += (2 * H * Q + P - 1) / P + 1;
    StepCall call;
    call.C = C; call.halo = pitch_stream_halo(dec_halo, extra, hop); call.hop = hop; call.P = P; call.Q = Q; call.H = H;
    call.srs = srs; call.slim = slim;
    call.pitch_words = words.data(); call.pitch_B = B; call.pitch_TT = TT; call.dec_halo = dec_halo; call.K = K;
    printf("C %d %ld %lld %lld %lld %lld %ld %ld %d %d %d\n", hop, C, P, Q, H, K, dec_halo, call.halo, (int)srs, (int)slim, B);
    std::vector<long> F((size_t)B); std::vector<int> zoff((size_t)B);
    long ztot = 0;
    for (int b = 0; b < B; b++) {
        const U& u = us[(size_t)b];
        const PsUtt pu = ps_utt(words.data(), B, TT, b);
        F[(size_t)b] = (long)(pu.N / hop); zoff[(size_t)b] = (int)ztot; ztot += F[(size_t)b];
        printf("U %d %ld %d %d %d %d |", b, F[(size_t)b], zoff[(size_t)b], 10 + b, (int)u.planned, (int)u.d.size());
        for (int v : u.d) printf(" %d", v);
        printf(" |");
        if (u.planned) for (int v : u.cents) printf(" %d", v);
        printf("\n");
    }
    EqsTrack eqt; LdsTrack ldt;
    StepOut o;
    std::vector<char> ht;
    std::vector<StepWin> win;
    long k = 0;
    for (;; k++) {
        win.clear();
        for (int b = 0; b < B; b++) if (k * C < F[(size_t)b]) win.push_back(StepWin{b, F[(size_t)b], k * C, zoff[(size_t)b], 10 + b});
        const int nw = (int)win.size();
        if (nw == 0) break;
        ht.assign(StepTab(nw, false, false, false, false, true).bytes, (char)0x5A);
        if (const char* bad = step_build(call, win.data(), nw, eqt, ldt, ht.data(), o)) { printf("R %s\n", bad); return; }
        const StepTab& t = o.tab;
        const int* ti = (const int*)ht.data();
        printf("S %ld %d %ld %d %lld %lld %lld %lld %lld %d\n", k, nw, o.Wtot, o.maxW, o.dsum, o.ysum, o.max_rs, o.max_out, o.max_yl, ti[StepTab::pack_dst(nw) + nw]);
        for (int i = 0; i < nw; i++) {
            printf("W %ld %d %d |", k, i, win[(size_t)i].b);
            printf(" %d %d %d %d %d %d |", ti[StepTab::zoff(nw) + i], ti[StepTab::coff(nw) + i], ti[StepTab::wlen(nw) + i], ti[StepTab::sid(nw) + i],
                   ti[StepTab::pack_src(nw) + i], ti[StepTab::pack_dst(nw) + i]);
            words_of(ht.data() + t.rs + (size_t)i * sizeof(RsRow), 5); printf(" |");
            words_of(ht.data() + t.lim + (size_t)i * sizeof(LimRow), 7); printf(" |");
            words_of(ht.data() + t.ps_rows + (size_t)i * sizeof(PsRow), 10); printf(" |");
            const int* seg = (const int*)(ht.data() + t.ps_seg);
            printf(" %d %d | %lld %lld %lld\n", seg[i], seg[nw + i], o.j0[(size_t)i], o.n[(size_t)i], o.dst[(size_t)i]);
        }
    }
    printf("E %ld\n", k);
}

static U planned(std::vector<int32_t> d, std::vector<int32_t> c) { return U{std::move(d), std::move(c), true}; }
static U plain(std::vector<int32_t> d) { return U{std::move(d), {}, false}; }

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

int main() {
    // a StepTab without the warp is what it was: the warped sections trail
    {
        const StepTab a(5, true, false, false, false), b(5, true, false, false, false, true);
        if (a.bytes > b.ps_rows || b.rs != a.rs || b.lim != a.lim || b.utt != a.utt || b.ps_rows % 8 || a.ps_rows || a.ps_seg) { printf("R layout moved\n"); return 1; }
    }
    const std::vector<int32_t> mixed_c = {600, -600, 1, -1, 0, 600, 600, 600, -600, 37, 0, -1};
    const std::vector<int32_t> mixed_d = {3, 2, 0, 0, 1, 1, 1, 0, 4, 1, 0, 5};
    struct Rate { long long P, Q, K; };
    const Rate rates[] = {{1, 1, 0}, {3, 1, 36}, {1, 2, 72}, {441, 320, 36}};
    for (const int hop : {1, 6, 256})
        for (const long C : {1L, 4L, 32L})
            for (const Rate& r : rates)
                for (const long long H : {0LL, 5LL}) {
                    // mixed cents with runs of empty and one-frame phonemes; the all-zero utterance; a member without a plan; F < C, = C, = k C + 1
                    std::vector<U> us;
                    us.push_back(planned(mixed_d, mixed_c));
                    us.push_back(planned({0, 0, 0}, {600, -600, 0}));
                    us.push_back(plain({2, 0, 5, 1}));
                    us.push_back(planned({(int32_t)C}, {600}));
                    us.push_back(planned({(int32_t)(2 * C), 1}, {-600, 600}));
                    us.push_back(planned(std::vector<int32_t>(40, 1), std::vector<int32_t>(40, 600)));
                    stream(hop, C, r.P, r.Q, H, r.K, 3, us);
                }
    // seeded random streams
    for (int k = 0; k < 40; k++) {
        const int hops[] = {1, 2, 6, 16, 256};
        const int hop = hops[rnd() % 5];
        const long C = 1 + (long)(rnd() % 9);
        const Rate& r = rates[rnd() % 4];
        std::vector<U> us;
        const int B = 1 + (int)(rnd() % 3);
        for (int b = 0; b < B; b++) {
            const int n = 1 + (int)(rnd() % 16);
            std::vector<int32_t> d((size_t)n), c((size_t)n);
            for (int i = 0; i < n; i++) {
                const uint32_t q = rnd() % 8;
                d[(size_t)i] = q < 2 ? 0 : (q < 4 ? 1 : (int)(rnd() % 12));
                const uint32_t s = rnd() % 6;
                c[(size_t)i] = s == 0 ? 600 : s == 1 ? -600 : s == 2 ? 0 : (int)(rnd() % 1201) - 600;
            }
            us.push_back(rnd() % 5 == 0 ? plain(d) : planned(d, c));
        }
        stream(hop, C, r.P, r.Q, (rnd() & 1) ? 7 : 0, r.K, (long)(rnd() % 4), us);
    }
    // the largest admitted signal: N just under 2^30, at both ends of the step range and mixed
    for (const int c : {-600, 600, 1}) {
        stream(1 << 20, 32, 1, 1, 0, 0, 3, {planned({1023}, {c})});
        stream(1 << 20, 32, 3, 1, 5, 36, 3, {planned({1000, 0, 23}, {c, -c, 600})});
        stream(16384, 4096, 1, 2, 0, 72, 3, {planned({65535}, {c})});
    }
    return 0;
}
