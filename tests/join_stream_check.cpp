// join_stream_check.cpp -- prints what summertts_amd/csrc/join_stream.hpp and out_chain.hpp decide for a joined stream;
// tests/test_join_stream_cpu.py compares the lines against tests/join_stream_ref.py and its own plan table.
//   join_stream_check steps < cases   one case per line: hop C Hd Ho P Q H B  frames[B]  sil[B]  total_sil
//       -> "case FJ steps workspace window_frames", then per step
//          "k f0 f1 g0 g1 j0 j1 jl0 jl1 Wtot maxW nw" and per window " b w0 w1 coff st en S N xoff"
//   join_stream_check plan            the output chain of the 64 streaming joined combinations, in out_chain_check.cpp's format
#include <cstdio>
#include <cstring>
#include <vector>

#include "join_stream.hpp"
#include "out_chain.hpp"

using namespace sts;

static int plans() {
    static const char* const name[OS_COUNT] = {"tail", "gain", "join", "resample", "pack", "eq", "loud", "limit"};
    for (int B = 1; B <= 3; B += 2) for (int R = 0; R < 2; R++) for (int G = 0; G < 2; G++) for (int M = 0; M < 2; M++)
    for (int T = 0; T < 2; T++) for (int D = 0; D < 2; D++) {
        const OutChain p = plan_out_chain(OutFacts{true, B, R != 0, G != 0, true, false, 0, M != 0, T != 0, D != 0});
        std::printf("S=1 B=%d R=%d G=%d J=1 E=0 L=0 M=%d T=%d D=%d |", B, R, G, M, T, D);
        for (int s = 0; s < OS_COUNT; s++)
            std::printf(" %s=%d:%s:%d", name[s], (int)p.run[s], p.src[s] < 0 ? "-" : name[p.src[s]], (int)p.wave[s]);
        std::printf(" | writer=%s pcm_nat=%d pcm_rs=%d loud_cast=%d no_clamp=%d gloud=%d lws=%d limws=%d spack=%d stab=%d in_place=%d\n",
                    name[p.writer], (int)p.pcm_nat, (int)p.pcm_rs, (int)p.loud_cast, (int)p.loud_no_clamp, (int)p.lim_gloud, (int)p.lws,
                    (int)p.limws, (int)p.spack, (int)p.stab, (int)p.chunk_in_place);
    }
    return 0;
}

static int steps() {
    long long hop, C, Hd, Ho, P, Q, H, B;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &hop, &C, &Hd, &Ho, &P, &Q, &H, &B) == 8) {
        std::vector<int> frames((size_t)B);
        std::vector<long long> sil((size_t)B);
        long long total_sil = 0;
        for (auto& f : frames) if (std::scanf("%d", &f) != 1) return 2;
        for (auto& s : sil) if (std::scanf("%lld", &s) != 1) return 2;
        if (std::scanf("%lld", &total_sil) != 1) return 2;
        JsPlan js;
        js.layout((int)B, frames.data(), sil.data(), total_sil);
        js.hop = (int)hop; js.C = C; js.Hd = (int)Hd; js.Ho = (int)Ho; js.P = P; js.Q = Q; js.H = (int)H;
        std::printf("case %lld %lld %lld %lld\n", js.FJ, js.steps(), js.workspace(), js.window_frames());
        JsStep t;
        std::vector<JsRow> rows;
        for (long long k = 0, n = js.steps(); k < n; k++) {
            js.step(k, t);
            js.rows(t.g0, t.g1, t.win, rows);
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %zu", k, t.f0, t.f1, t.g0, t.g1, t.j0, t.j1, t.jl0, t.jl1, t.Wtot, t.maxW,
                        t.win.size());
            for (size_t i = 0; i < t.win.size(); i++)
                std::printf(" %d %lld %lld %lld %lld %lld %lld %lld %lld", t.win[i].b, t.win[i].w0, t.win[i].w1, t.win[i].coff, rows[i].st, rows[i].en,
                            rows[i].S, rows[i].N, rows[i].xoff);
            std::printf("\n");
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "plan")) return plans();
    if (argc == 2 && !std::strcmp(argv[1], "steps")) return steps();
    std::fprintf(stderr, "usage: join_stream_check steps < cases | join_stream_check plan\n");
    return 1;
}
