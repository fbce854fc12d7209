// stream_step_check.cpp -- walks whole streams through summertts_amd/csrc/stream_step.hpp and prints every table of every step;
// tests/test_stream_step_cpu.py compares the lines against tests/stream_step_ref.py and checks the tables' invariants.
//   stream_step_check < cases     one case per line, all integers:
//       form hop C halo P Q H srs slim seq sld gain mix retry B  F[B] f0[B] zoff[B] sid[B]   and, form 2:  sil[B] total_sil Hd Ho
//       form 0: a closed stream (step k: chunk k of every utterance that has one; f0 is not read), 1: an open stream (every slot at its
//       own frame, f0 the first), 2: a joined stream.  retry: the step that runs twice (the first attempt is dropped, not committed)
//   -> "case lsrc", then per attempt
//      "step k attempt nw Wtot maxW zoff0 wlen0 src0 max_rs max_out etiles ltiles dsum bytes eslot lslot"
//      "off rs lim utt j_rs j_lim j_rows eq loud", "chunks (j0 n dst)*", and one line of words per section that exists:
//      "ints", "rs", "lim", "utt", "jrs", "jlim", "jrows", "eq", "loud"      -- or "error k text" and the case ends --      then "end"
#include <cstdio>
#include <cstring>
#include <vector>

#include "stream_step.hpp"

using namespace sts;

template <class T> static void words(const char* name, const char* ht, size_t off, size_t n) {
    std::printf("%s", name);
    for (size_t i = 0; i < n; i++) {
        T v;
        std::memcpy(&v, ht + off + i * sizeof(T), sizeof(T));
        std::printf(" %lld", (long long)v);
    }
    std::printf("\n");
}

static void print_step(long long k, int attempt, const StepOut& o, const char* ht, int eslot, int lslot) {
    const StepTab& t = o.tab;
    const size_t nw = (size_t)t.nw, nu = t.joined ? 1 : nw;
    std::printf("step %lld %d %d %ld %d %d %d %d %lld %lld %lld %lld %lld %zu %d %d\n", k, attempt, o.nw, o.Wtot, o.maxW, o.zoff0, o.wlen0, o.src0,
                o.max_rs, o.max_out, o.etiles, o.ltiles, o.dsum, t.bytes, eslot, lslot);
    std::printf("off %zu %zu %zu %zu %zu %zu %zu %zu\n", t.rs, t.lim, t.utt, t.j_rs, t.j_lim, t.j_rows, t.eq_rows, t.loud_rows);
    std::printf("chunks");
    for (size_t i = 0; i < o.n.size(); i++) std::printf(" %lld %lld %lld", o.j0[i], o.n[i], o.dst[i]);
    std::printf("\n");
    words<int>("ints", ht, 0, (size_t)StepTab::ints(t.nw));
    words<long long>("rs", ht, t.rs, nw * 5);
    words<long long>("lim", ht, t.lim, nw * 7);
    if (t.gain) words<int>("utt", ht, t.utt, nw);
    if (t.joined) {
        words<long long>("jrs", ht, t.j_rs, 5);
        words<long long>("jlim", ht, t.j_lim, 7);
        words<long long>("jrows", ht, t.j_rows, nw * 5);
    }
    if (t.eq) words<long long>("eq", ht, t.eq_rows, nu * kEqsRow);
    if (t.loud) words<long long>("loud", ht, t.loud_rows, nu * kLdsRow);
}

int main() {
    long long form, hop, C, halo, P, Q, H, srs, slim, seq, sld, gain, mix, retry, B;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &form, &hop, &C, &halo, &P, &Q, &H, &srs, &slim,
                      &seq, &sld, &gain, &mix, &retry, &B) == 15) {
        std::vector<int> F((size_t)B), f0((size_t)B), zoff((size_t)B), sid((size_t)B);
        for (std::vector<int>* v : {&F, &f0, &zoff, &sid}) for (int& x : *v) if (std::scanf("%d", &x) != 1) return 2;
        const bool joined = form == 2, open = form == 1;
        JsPlan js;
        if (joined) {
            std::vector<long long> sil((size_t)B);
            long long total_sil = 0, Hd = 0, Ho = 0;
            for (auto& s : sil) if (std::scanf("%lld", &s) != 1) return 2;
            if (std::scanf("%lld %lld %lld", &total_sil, &Hd, &Ho) != 3) return 2;
            js.layout((int)B, F.data(), sil.data(), total_sil);
            js.hop = (int)hop; js.C = C; js.Hd = (int)Hd; js.Ho = (int)Ho; js.P = srs ? P : 1; js.Q = srs ? Q : 1; js.H = slim ? (int)H : 0;
        }
        // the chain as the engine plans it for these flags: the stage loudness reads is the plan's, not this program's
        const OutChain oc = plan_out_chain(OutFacts{true, (int)B, srs != 0, gain != 0, joined, seq != 0, sld ? 1 : 0, slim != 0, false, false, seq != 0, sld != 0});
        if (oc.eqst != (seq != 0) || oc.lst != (sld != 0) || oc.run[OS_RESAMPLE] != (srs != 0) || oc.run[OS_LIMIT] != (slim != 0)) return 3;
        StepCall c;
        c.C = (long)C; c.halo = (long)halo; c.hop = (int)hop; c.P = srs ? P : 1; c.Q = srs ? Q : 1; c.H = slim ? H : 0;
        c.srs = srs != 0; c.slim = slim != 0; c.seq = seq != 0; c.sld = sld != 0; c.gain = gain != 0; c.mix = mix != 0;
        c.lsrc = oc.src[OS_LOUD];
        std::printf("case %d\n", c.lsrc);
        const int nu = joined ? 1 : (int)B;
        EqsTrack eqt; eqt.begin(nu);
        LdsTrack ldt; ldt.begin(nu);
        std::vector<long long> Nu((size_t)nu);
        for (int b = 0; b < nu; b++) Nu[(size_t)b] = stream_out_count((joined ? js.FJ : (long long)F[(size_t)b]) * hop, c.P, c.Q);
        ldt.layout(Nu.data());
        std::vector<long> pos(f0.begin(), f0.end());        // an open stream: every slot's next frame
        std::vector<char> ht(StepTab((int)B, true, true, true, joined).bytes);
        std::vector<StepWin> win;
        StepOut o;
        bool repeated = false;
        for (long long k = 0;; k++) {
            win.clear();
            for (int b = 0; b < (int)B && !joined; b++) {
                const long f = open ? pos[(size_t)b] : (long)(k * C);
                if (f < F[(size_t)b]) win.push_back(StepWin{b, F[(size_t)b], f, zoff[(size_t)b], sid[(size_t)b]});
            }
            if (joined ? k >= js.steps() : win.empty()) break;
            std::memset(ht.data(), 0x5a, ht.size());
            const char* bad = joined ? step_build_joined(c, js, k, zoff.data(), sid.data(), eqt, ldt, ht.data(), o)
                                     : step_build(c, win.data(), (int)win.size(), eqt, ldt, ht.data(), o);
            if (bad) { std::printf("error %lld %s\n", k, bad); break; }
            if (o.tab.bytes > ht.size()) return 4;
            print_step(k, repeated && k == retry ? 1 : 0, o, ht.data(), eqt.slot, ldt.slot);
            if (k == retry && !repeated) { repeated = true; eqt.drop(); ldt.drop(); k--; continue; }
            eqt.commit(); ldt.commit();
            if (open) for (const StepWin& w : win) pos[(size_t)w.b] += (long)C;
        }
        std::printf("end\n");
    }
    return 0;
}
