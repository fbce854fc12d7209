// out_chain_check.cpp -- prints the output-chain plan (summertts_amd/csrc/out_chain.hpp) of every admissible combination of a run's
// facts, one line each; tests/test_out_chain_cpu.py compares the lines against its own table.
#include <cstdio>

#include "out_chain.hpp"

using namespace sts;

int main() {
    static const char* const name[OS_COUNT] = {"tail", "gain", "join", "resample", "pack", "eq", "loud", "limit"};
    for (int S = 0; S < 2; S++) for (int B = 1; B <= 3; B += 2) for (int R = 0; R < 2; R++) for (int G = 0; G < 2; G++)
    for (int J = 0; J < 2; J++) for (int E = 0; E < 2; E++) for (int L = 0; L < 3; L++) for (int M = 0; M < 2; M++)
    for (int T = 0; T < 2; T++) for (int D = 0; D < 2; D++) {
        if (S && (J || E || L)) continue;       // refused at the top of a run
        const OutChain p = plan_out_chain(OutFacts{S != 0, B, R != 0, G != 0, J != 0, E != 0, L, M != 0, T != 0, D != 0});
        std::printf("S=%d B=%d R=%d G=%d J=%d E=%d L=%d M=%d T=%d D=%d |", S, B, R, G, J, E, L, M, T, D);
        for (int s = 0; s < OS_COUNT; s++)
            std::printf(" %s=%d:%s:%d", name[s], (int)p.run[s], p.src[s] < 0 ? "-" : name[p.src[s]], (int)p.wave[s]);
        std::printf(" | writer=%s pcm_nat=%d pcm_rs=%d loud_cast=%d no_clamp=%d gloud=%d lws=%d limws=%d spack=%d stab=%d in_place=%d\n",
                    name[p.writer], (int)p.pcm_nat, (int)p.pcm_rs, (int)p.loud_cast, (int)p.loud_no_clamp, (int)p.lim_gloud, (int)p.lws,
                    (int)p.limws, (int)p.spack, (int)p.stab, (int)p.chunk_in_place);
    }
    return 0;
}
