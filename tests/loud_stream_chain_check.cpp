// loud_stream_chain_check.cpp -- prints the output-chain plan (summertts_amd/csrc/out_chain.hpp) with the trailing fact loud_stream, one
// line per admissible combination of a run's facts; tests/test_loudness_stream_cpu.py reads the lines.  With "base" as its argument:
// out_chain_check.cpp's enumeration with both trailing facts given as false, in that program's format (the lines must be the same ones).
// Otherwise every combination of the ten older facts with eq_stream (ES) and loud_stream (LS); a stream is admissible with bands only
// under ES, under loudness mode 1 only with LS, under mode 2 never.
#include <cstdio>
#include <cstring>

#include "out_chain.hpp"

using namespace sts;

static const char* const name[OS_COUNT] = {"tail", "gain", "join", "resample", "pack", "eq", "loud", "limit"};

static void line(const OutFacts& f, int S, int B, int R, int G, int J, int E, int L, int M, int T, int D, bool ext) {
    const OutChain p = plan_out_chain(f);
    std::printf("S=%d B=%d R=%d G=%d J=%d E=%d L=%d M=%d T=%d D=%d", S, B, R, G, J, E, L, M, T, D);
    if (ext) std::printf(" ES=%d LS=%d", (int)f.eq_stream, (int)f.loud_stream);
    std::printf(" |");
    for (int s = 0; s < OS_COUNT; s++)
        std::printf(" %s=%d:%s:%d", name[s], (int)p.run[s], p.src[s] < 0 ? "-" : name[p.src[s]], (int)p.wave[s]);
    std::printf(" | writer=%s pcm_nat=%d pcm_rs=%d loud_cast=%d no_clamp=%d gloud=%d lws=%d limws=%d spack=%d stab=%d in_place=%d",
                name[p.writer], (int)p.pcm_nat, (int)p.pcm_rs, (int)p.loud_cast, (int)p.loud_no_clamp, (int)p.lim_gloud, (int)p.lws,
                (int)p.limws, (int)p.spack, (int)p.stab, (int)p.chunk_in_place);
    if (ext) std::printf(" eqws=%d eqst=%d lst=%d", (int)p.eqws, (int)p.eqst, (int)p.lst);
    std::printf("\n");
}

int main(int argc, char** argv) {
    const bool base = argc > 1 && !std::strcmp(argv[1], "base");
    for (int S = 0; S < 2; S++) for (int B = 1; B <= 3; B += 2) for (int R = 0; R < 2; R++) for (int G = 0; G < 2; G++)
    for (int J = 0; J < 2; J++) for (int E = 0; E < 2; E++) for (int L = 0; L < 3; L++) for (int M = 0; M < 2; M++)
    for (int T = 0; T < 2; T++) for (int D = 0; D < 2; D++) {
        if (base) {
            if (S && (J || E || L)) continue;       // (out_chain_check.cpp's own rule)
            line(OutFacts{S != 0, B, R != 0, G != 0, J != 0, E != 0, L, M != 0, T != 0, D != 0, false, false}, S, B, R, G, J, E, L, M, T, D, false);
            continue;
        }
        for (int ES = 0; ES < 2; ES++) for (int LS = 0; LS < 2; LS++) {
            if (S && ((E && !ES) || (L == 1 && !LS) || L == 2)) continue;
            line(OutFacts{S != 0, B, R != 0, G != 0, J != 0, E != 0, L, M != 0, T != 0, D != 0, ES != 0, LS != 0}, S, B, R, G, J, E, L, M, T, D, true);
        }
    }
    return 0;
}
