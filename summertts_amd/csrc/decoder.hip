// decoder.hip -- stage 5 of a run (engine.hip): one decode pass over windows of z.  conv_pre, the upsampler / ResBlock stages, the
// tail, and what follows the float wave (resampler, loudness, limiter, taps).  Per ResBlock layer: ResStage::plan_layer says WHICH
// kernel runs it, the fill_* functions build its arguments, ResStage::launch sends it out and ResStage::book books it.
#include "run_ctx.hpp"
#include "knobs.hpp"

#include <math.h>
#include <string.h>
#include <utility>

namespace sts {

// hand copy of conv_common.hpp MAX_HALO, the staged window of conv_h2p.hip (that header is device code: host code cannot include it)
static constexpr int MAX_HALO_H2P = 64;

// Frames of z (per side) that influence one output sample through the decoder: conv_pre, every upsampler,
// the widest ResBlock chain of every stage, and the tail.  Conservative (rounded up at every level).
int decoder_halo_frames(const Model& M) {
    double R = M.dec_type == 0 ? (M.conv_post.k - 1) / 2 : (M.conv_post.k - 1) / 2 + 12;   // tail: reflect pad, iSTFT overlap, synthesis FIR
    const int nk = M.n_resk;
    for (int i = M.n_up - 1; i >= 0; i--) {
        double rb = 0;
        for (int j = 0; j < nk; j++) {
            const DResBlock& b = M.rb[(size_t)i * nk + j];
            double r = 0;
            for (size_t d = 0; d < b.c1.size(); d++) r += b.c1[d].dil * (b.c1[d].k - 1) / 2 + b.c2[d].dil * (b.c2[d].k - 1) / 2;
            if (r > rb) rb = r;
        }
        R += rb;
        const DConv& up = M.ups[i];
        R = ceil((R + up.k) / (double)up.stride) + 1;     // through the transposed conv (kernel k, stride s)
    }
    R += (M.conv_pre.k - 1) / 2;
    return (int)ceil(R) + 1;
}

// The windows of one decode pass.  Window w covers frames [zoff[w], zoff[w] + wlen[w]) of the packed z and owns the compact range
// starting at coff[w] in every decoder buffer.  inl: a single window by value (wlen0 its real length, zoff0 its offset inside z);
// otherwise the geometry is read from the device tables d_win = the int block of the step's table (stream_step.hpp StepTab: zoff, coff,
// wlen) -- a call that does not stream uploads the same three columns  (wlen0 < 0, or no_inline_seg).
struct WinGeom {
    bool inl; int nw, zoff0, wlen0; const int* d_win;
    // in the decoder's buffers at `scale` positions per frame (+ extra per window); in z
    SegView seg(int scale, int extra) const { return inl ? SegView{nullptr, nullptr, scale, extra, 0, wlen0} : SegView{d_win + StepTab::coff(nw), d_win + StepTab::wlen(nw), scale, extra, 0, 0}; }
    SegView zseg() const { return inl ? SegView{nullptr, nullptr, 1, 0, zoff0, wlen0} : SegView{d_win + StepTab::zoff(nw), d_win + StepTab::wlen(nw), 1, 0, 0, 0}; }
    const int* len() const { return inl ? nullptr : d_win + StepTab::wlen(nw); }     // (null: one window of ilen() frames)
    int ilen() const { return inl ? wlen0 : 0; }
};

// The buffers of one decoder stage inside its region (run_frame_workspace sizes regA / regB for (3 + 4 nk) tensors of ce floats): the
// upsampler output; per chain t1 (conv1's output) and the pair pa / pb a layer's input and output alternate between; pre-split path only:
// per chain pn (planes of the layer output), then the planes P0 and the x16 copy X0 of the stage input
struct StageBufs {
    float* reg; size_t ce; int nk;
    float* up() const { return reg; }
    float* t1(int j) const { return reg + (size_t)(1 + 3 * j) * ce; }
    float* pa(int j) const { return t1(j) + ce; }
    float* pb(int j) const { return pa(j) + ce; }
    float* pn(int j) const { return reg + (size_t)(1 + 3 * nk + j) * ce; }
    float* P0() const { return reg + (size_t)(1 + 4 * nk) * ce; }
    float* X0() const { return P0() + ce; }
    float* next(int j, const float* cur) const { return cur == pa(j) ? pb(j) : pa(j); }
};

// rank[j] = number of chains cheaper than chain j (smaller kernel; ties by index): picks the chain's prioritised auxiliary stream
static void chain_rank(const Model& M, int i, int rank[8]) {
    const int nk = M.n_resk;
    for (int j = 0; j < nk && j < 8; j++) {
        rank[j] = 0;
        for (int q = 0; q < nk && q < 8; q++) {
            const int kj = M.rb[(size_t)i * nk + j].c1[0].k, kq = M.rb[(size_t)i * nk + q].c1[0].k;
            rank[j] += kq < kj || (kq == kj && q < j);
        }
    }
}

// the two convs of a ResBlock layer, cur + conv2(lrelu(conv1(lrelu(cur))))   (/root/reference/src/modules/ResBlock1.cpp:55-69)
static std::pair<ConvOpt, ConvOpt> resblock_opts(const float* cur) {
    ConvOpt o1; o1.in_act = 1; o1.slope = 0.1f;
    ConvOpt o2 = o1; o2.res = cur; o2.epi = EPI_RESADD;
    return {o1, o2};
}

// the kernel that runs one layer of all chains of a grouped stage (ResStage::per_chain is orthogonal: the same kernel, once per chain)
enum class LayerKind {
    FusedBf3,       // the whole layer in one launch, split-bf16 / two-term fp16 (resblock_bf3)
    FusedWino,      // the whole layer in one launch, fp32 MFMA in the Winograd domain (resblock_wino)
    FusedDirect,    // the whole layer in one launch, fp32 MFMA direct form (resblock_layer)
    H2PPair,        // pre-split channel-minor pair (split_planes at the stage's entry + 2 x conv_h2p_group)
    StagedBf3,      // staged grouped pair, split-bf16 / two-term fp16 (2 x conv_bf3_group)
    StagedMfma      // staged grouped pair, fp32 MFMA (2 x conv_mfma_group; members a group cannot take: conv_mfma / conv_generic)
};
static bool is_fused(LayerKind k) { return k == LayerKind::FusedBf3 || k == LayerKind::FusedWino || k == LayerKind::FusedDirect; }

// arguments of one layer; each struct is a kernarg block of kMaxGroup members, built at most once per layer and only for the kind that uses it
struct LayerArgs {
    ConvGroup G1, G2;           // the two convs as conv_args books them (every kind books through it; the staged kinds launch them)
    ResLayerGroup R;            // fused kinds
    H2PGroup H1, H2;            // pre-split pair
    double fl, flw;             // the layer's FLOPs; the same with every conv scaled to its Winograd form
};

// The ResBlock chains of decoder stage i: they only meet in the final sum (Generator_hifigan.cpp:159-173).
struct Engine::ResStage {
    Engine& e; const int i, nk, nd0; const DConv& up; const Lvl& l2; const StageBufs b;
    bool grouped = false, per_chain = false, h2p_stage = false;    // the stage plan (plan())
    int rank[8] = {};
    const float* cur[kMaxGroup] = {};                              // grouped form: where each chain's tensor is now
    ResStage(Engine& e_, int i_, const Lvl& l2_, float* reg, size_t ce)
        : e(e_), i(i_), nk(e_.model.n_resk), nd0(nk > 0 ? (int)e_.model.rb[(size_t)i_ * nk].c1.size() : 0), up(e_.model.ups[i_]), l2(l2_), b{reg, ce, nk} {
        chain_rank(e.model, i, rank);
    }
    const DResBlock& rb(int j) const { return e.model.rb[(size_t)i * nk + j]; }
    hipStream_t aux(int j) const { return e.aux_[rank[j] % kAux]; }       // heaviest chain: highest priority
    long fused128_tiles() const { return (long)((l2.max_len + 117) / 118) * l2.nb * nk; }
    void fork() const { (void)hipEventRecord(e.ev_fork_, e.stream); for (int k = 0; k < kAux; k++) (void)hipStreamWaitEvent(e.aux_[k], e.ev_fork_, 0); }
    void join(int n) const { for (int k = 0; k < n; k++) { (void)hipEventRecord(e.ev_join_[k], e.aux_[k]); (void)hipStreamWaitEvent(e.stream, e.ev_join_[k], 0); } }

    bool probe_grouped();
    void plan();
    bool fuse_candidate(int d) const;
    void fill_convs(int d, LayerArgs& A);
    void fill_fused(int d, ResLayerGroup& R) const;
    void fill_h2p(int d, H2PGroup& H1, H2PGroup& H2) const;
    LayerKind plan_layer(int d, LayerArgs& A) const;
    void launch(LayerKind k, int d, const LayerArgs& A) const;
    void book(LayerKind k, const LayerArgs& A);
    void run_grouped(const float** outs);
    void run_forked(const float** outs);
};

// Can one layer of all chains go out as one grouped launch?  Probed with layer 0 (geometry is the same for every layer of a chain).
// The members' arguments come from conv_args, which books; the probe takes back flops_ and bytes_ -- and NOT bytes_w_: every stage leaves
// nk extra first-layer weight reads in sts_profile.bytes_decoder_min.  Known and kept (the field is compared across versions).
bool Engine::ResStage::probe_grouped() {
    ConvGroup G; G.n = nk;
    const double f0 = e.flops_[3], b0 = e.bytes_[3];
    for (int j = 0; j < nk; j++) G.g[j] = e.conv_args(rb(j).c1[0], b.up(), l2, b.up(), l2, ConvOpt(), nullptr);
    e.flops_[3] = f0; e.bytes_[3] = b0;              // (bytes_w_[3] stays booked, see above)
    return conv_group_eligible(G);
}

// the stage plan: grouped (layer d of ALL chains as one launch; else run_forked), per_chain (lab), h2p_stage (the pre-split path)
void Engine::ResStage::plan() {
    grouped = e.conv_mode == 0 && nk >= 2 && nk <= kMaxGroup;
    for (int j = 0; j < nk && grouped; j++) grouped = (int)rb(j).c1.size() == nd0;
    grouped = grouped && probe_grouped();
    if (!grouped) return;
    // experiment knob STS_CHAIN_STREAMS=<stage mask>: the chains of the masked stages go out as per-chain launches on
    // the prioritised auxiliary streams (heaviest chain first) instead of one grouped launch per layer
    static const int chain_streams_env = exp_int("STS_CHAIN_STREAMS", 0);
    const int chain_streams = e.chain_streams_dbg >= 0 ? e.chain_streams_dbg : chain_streams_env;     // (lab: sts_debug_set STS_DBG_CHAIN_STREAMS)
    per_chain = ((chain_streams >> i) & 1) && nk <= kAux;
    // the pre-split path (conv_h2p.hip) takes a stage only whole: between its layers the chains' tensors live in the x16 layout
    // Measured (profiles/r06_h2p_thresholds_and_two_products.log, r06_h2p_vs_fused128_ab.log).  128 channels: the pre-split pair beats BOTH the
    // staged grouped pair (one HiFi-GAN utterance, 1 002 tiles of 128 x 128: -1.4 % of the trunk) and the fused 128-channel layer kernel
    // (2 ... 64 utterances: -4.6 ... -11 % of the trunk although the fused kernel keeps the intermediate on chip -- its whole-window staging and
    // one-workgroup-per-CU residency cost more than the 8 bytes per value it saves); below ~3 tiles per CU (one MB-iSTFT utterance: 294) the
    // entry split and the second conv's two output tensors cost more than the faster K loop returns.  256+ channels: from ~2 tiles per CU on
    // (one HiFi-GAN utterance = 252 tiles needs the K split over two wave groups the staged kernel has).  h2p (lab): 2 = always, 3 / 4 = always for
    // the 128-channel / the wider stages only.  (The 64-channel stage was tried on this path too: it LOSES 1 % to the fused layer kernel at 32 utterances
    // and 4 % at one -- 4 chunks x k steps are too few to pay for an unfused pair's two epilogues; profiles/r06_h2p_c64_ab.log.)
    const long h2p_tiles = (long)((l2.max_len + 127) / 128) * (up.Cout / 128) * l2.nb * nk;
    const long h2p_min = up.Cout == 128 ? 768 : 512;
    h2p_stage = e.conv_math == 3 && e.h2p && !per_chain && up.Cout % 128 == 0 && (double)l2.ld * 32.0 < 2.0e9 &&
                (e.h2p == 2 || (e.h2p == 3 && up.Cout == 128) || (e.h2p == 4 && up.Cout != 128) || h2p_tiles >= h2p_min);
    for (int j = 0; j < nk && h2p_stage; j++)
        for (int d = 0; d < nd0 && h2p_stage; d++) {
            const DConv &c1 = rb(j).c1[d], &c2 = rb(j).c2[d];
            h2p_stage = c1.wh2p && c2.wh2p && c1.Cin == up.Cout && c1.Cout == up.Cout && c2.Cin == up.Cout && c2.Cout == up.Cout &&
                        (c1.k & 1) && (c2.k & 1) && c1.dil >= 1 && c2.dil >= 1 && c1.pad == c1.dil * (c1.k - 1) / 2 && c2.pad == c2.dil * (c2.k - 1) / 2 &&
                        c1.dil * (c1.k - 1) <= MAX_HALO_H2P && c2.dil * (c2.k - 1) <= MAX_HALO_H2P && !c1.depthwise && !c2.depthwise && !c1.transposed && !c2.transposed;
        }
}

// narrow stages: may the whole layer d (conv1 -> lrelu -> conv2 -> + x) of all chains go out as one launch?  (The kernels' own
// eligibility tests judge the filled arguments afterwards, plan_layer.)
bool Engine::ResStage::fuse_candidate(int d) const {
    static const bool no_fuse = exp_flag("STS_NO_FUSE");   // experiment knob
    static const int fuse_maxc = exp_int("STS_FUSE_MAXC", 128);   // experiment knob
    static const bool bf3_nofuse = exp_flag("STS_BF3_NOFUSE");   // experiment knob
    const int C = up.Cout;
    if (no_fuse || C > fuse_maxc) return false;
    // split-bf16 arithmetic: the 64/32-channel stages always run fused; the 128-channel stage (whole window = 147 KB of
    // LDS, one 8-wave workgroup per CU) from ~8 tiles per CU on -- the trunk is power-bound at batch (docs/HISTORY.md 5d), so
    // dropping the intermediate's HBM round trip pays (batch 8: -3 %), while a single utterance's 1 089 tiles on 256
    // workgroup slots only tie the unfused pair
    static const int bf3_fuse128_tiles = exp_int("STS_BF3_FUSE128_TILES", 2048);   // experiment knob
    if (e.conv_math != 1 && (bf3_nofuse || C > 128 || (C > 64 && fused128_tiles() < bf3_fuse128_tiles))) return false;
    for (int j = 0; j < nk; j++) {
        const DConv &c1 = rb(j).c1[d], &c2 = rb(j).c2[d];
        if (!(c1.Cin == C && c1.Cout == C && c2.Cin == C && c2.Cout == C && c1.Cin_pad == C &&
              c1.Cout_pad == C && c2.Cin_pad == C && c2.Cout_pad == C && !c1.depthwise && !c2.depthwise &&
              !c1.transposed && !c2.transposed && c2.dil == 1 && c1.pad == c1.dil * (c1.k - 1) / 2 &&
              c2.pad == (c2.k - 1) / 2)) return false;
    }
    // the 128-channel variant runs 8-wave workgroups, two per CU: only worth it when the grid fills the chip twice
    if (C > 64 && fused128_tiles() < 512) return false;
    return !(C > 64 && h2p_stage);       // (round 6: the pre-split pair instead of the fused 128-channel layer kernel)
}

// The two convs of layer d of every chain, cur -> t1 -> the other half of pa / pb.  conv_args books their FLOPs / algorithmic bytes:
// every kind is booked here, exactly as for the two separate convs, whichever kernel then runs the layer.
void Engine::ResStage::fill_convs(int d, LayerArgs& A) {
    auto wino_ratio = [](int k) { int n3, n2; wino_split(k, &n3, &n2); return (4.0 * n3 + 3.0 * n2) / (2.0 * k); };
    A.G1.n = A.G2.n = nk; A.fl = A.flw = 0;
    for (int j = 0; j < nk; j++) {
        const DConv &c1 = rb(j).c1[d], &c2 = rb(j).c2[d];
        const auto o = resblock_opts(cur[j]);
        double f = 0;
        A.G1.g[j] = e.conv_args(c1, cur[j], l2, b.t1(j), l2, o.first, &f); A.fl += f; A.flw += f * wino_ratio(c1.k);
        A.G2.g[j] = e.conv_args(c2, b.t1(j), l2, b.next(j, cur[j]), l2, o.second, &f); A.fl += f; A.flw += f * wino_ratio(c2.k);
    }
}

void Engine::ResStage::fill_fused(int d, ResLayerGroup& R) const {
    memset(&R, 0, sizeof(R));
    R.n = nk; R.C = up.Cout; R.ld = l2.ld; R.slope = 0.1f; R.seg = l2.seg; R.B = l2.nb; R.max_n = l2.max_len;
    for (int j = 0; j < nk; j++) {
        const DConv &c1 = rb(j).c1[d], &c2 = rb(j).c2[d];
        if (fill_res_member(c1, c2, cur[j], b.next(j, cur[j]), e.conv_math == 3, R.g[j])) { R.math = 1; R.ovf = e.ovf_; }
    }
}

// ---- round 6: the wide stages on pre-split, channel-minor activations (conv_h2p.hip).  The stage input is split once
// (planes P0 of lrelu(x) + the x16 copy X0 for the residual); conv1 reads planes and writes planes of lrelu(out); conv2 reads those
// and the x16 residual and writes the next layer's x16 + planes -- or, in the last layer, the fp32 [C][ld] tensor the next stage reads.
// Buffers: t1 (planes of conv1's output), pa / pb (x16 ping-pong, last layer: fp32), pn (planes of the layer output), per chain.
void Engine::ResStage::fill_h2p(int d, H2PGroup& H1, H2PGroup& H2) const {
    memset(&H1, 0, sizeof(H1)); memset(&H2, 0, sizeof(H2));
    H1.n = H2.n = nk; H1.seg = H2.seg = l2.seg; H1.B = H2.B = l2.nb; H1.max_n = H2.max_n = l2.max_len; H1.ovf = H2.ovf = e.ovf_;
    for (int j = 0; j < nk; j++) {
        const DConv &c1 = rb(j).c1[d], &c2 = rb(j).c2[d];
        float *t1 = b.t1(j), *pn = b.pn(j), *nxt = b.next(j, cur[j]);
        H2PArgs& a1 = H1.g[j];
        a1.xp = d == 0 ? (const void*)b.P0() : (const void*)pn; a1.xp_ld = l2.ld; a1.wb = c1.wh2p; a1.wscale = c1.h2_scale; a1.bias = c1.bias;
        a1.yp = t1; a1.yp_ld = l2.ld; a1.yp_slope = 0.1f;
        a1.Cin = c1.Cin; a1.Cout = c1.Cout; a1.ntap = c1.k; a1.tap_step = c1.dil; a1.tap_off = -c1.pad;
        H2PArgs& a2 = H2.g[j];
        a2.xp = t1; a2.xp_ld = l2.ld; a2.wb = c2.wh2p; a2.wscale = c2.h2_scale; a2.bias = c2.bias;
        a2.res16 = d == 0 ? b.X0() : cur[j]; a2.res_ld = l2.ld;
        if (d + 1 == nd0) { a2.y = nxt; a2.y_ld = l2.ld; }
        else { a2.y16 = nxt; a2.y16_ld = l2.ld; a2.yp = pn; a2.yp_slope = 0.1f; a2.yp_ld = l2.ld; }
        a2.Cin = c2.Cin; a2.Cout = c2.Cout; a2.ntap = c2.k; a2.tap_step = c2.dil; a2.tap_off = -c2.pad;
    }
}

// WHICH kernel runs layer d (A.G1 / A.G2 filled).  Fills the arguments its choice rests on: A.R when a fused kind is in reach, A.H1 / A.H2
// when the pre-split pair runs.
LayerKind Engine::ResStage::plan_layer(int d, LayerArgs& A) const {
    const bool bf3 = e.conv_math != 1;          // (fuse_candidate has no fused kind for split-bf16 under STS_BF3_NOFUSE)
    if (fuse_candidate(d)) {
        fill_fused(d, A.R);
        if (resblock_layer_eligible(A.R)) {
            if (bf3 && resblock_bf3_eligible(A.R)) return LayerKind::FusedBf3;
            // both convs in the Winograd domain when the model carries the transformed weights (-31 % MFMAs);
            // the direct-form fused kernel otherwise
            static const bool no_wino = exp_flag("STS_NO_WINO");   // experiment knob
            return !no_wino && resblock_wino_eligible(A.R) ? LayerKind::FusedWino : LayerKind::FusedDirect;
        }
    }
    if (h2p_stage) { fill_h2p(d, A.H1, A.H2); return LayerKind::H2PPair; }
    // per chain every conv finds its own kernel (launch): the arithmetic alone names the kind
    if (per_chain) return bf3 ? LayerKind::StagedBf3 : LayerKind::StagedMfma;
    return bf3 && conv_bf3_group_eligible(A.G1) && conv_bf3_group_eligible(A.G2) ? LayerKind::StagedBf3 : LayerKind::StagedMfma;
}

// sends layer d out: one grouped launch (a pair: two) on the engine's stream, or -- per_chain -- the same per chain on its auxiliary stream
void Engine::ResStage::launch(LayerKind k, int d, const LayerArgs& A) const {
    const hipStream_t stream = e.stream;
    static const char* gt = exp_env("STS_GROUP_TILE");   // experiment knob: per-stage tile digits, e.g. "4335"
    const int gtile = gt && (int)strlen(gt) > i ? gt[i] - '0' : -1;
    if (is_fused(k)) {
        auto run = [&](const ResLayerGroup& R, hipStream_t st) {
            static const int bv = exp_int("STS_BF3_LAYER_VARIANT", -1);   // experiment knob
            if (k == LayerKind::FusedBf3) resblock_bf3(R, st, bv);
            else if (k == LayerKind::FusedWino) resblock_wino(R, st);
            else resblock_layer(R, st);
        };
        if (!per_chain) return run(A.R, stream);
        for (int j = 0; j < nk; j++) { ResLayerGroup R1 = A.R; R1.n = 1; R1.g[0] = A.R.g[j]; run(R1, aux(j)); }
    } else if (k == LayerKind::H2PPair) {
        if (d == 0) split_planes(b.up(), l2.ld, up.Cout, l2.seg, l2.nb, l2.max_len, 0.1f, b.P0(), b.X0(), l2.ld, e.ovf_, stream);
        const int ht = e.h2p_tile < 0 ? -1 : (up.Cout == 128 ? (e.h2p_tile & 0xff) : ((e.h2p_tile >> 8) & 0xff));   // lab: low byte = the 128-channel stage, next = wider ones; 0xff = automatic
        conv_h2p_group(A.H1, stream, ht == 0xff ? -1 : ht);
        conv_h2p_group(A.H2, stream, ht == 0xff ? -1 : ht);
    } else if (per_chain) {
        for (int j = 0; j < nk; j++)
            for (const ConvArgs* ca : {&A.G1.g[j], &A.G2.g[j]}) {
                if (k == LayerKind::StagedBf3 && conv_bf3_eligible(*ca)) conv_bf3(*ca, aux(j), -1);
                else if (conv_mfma_eligible(*ca)) conv_mfma(*ca, aux(j), gtile);
                else conv_generic(*ca, aux(j));
            }
    } else if (k == LayerKind::StagedBf3) {
        static const char* bgt = exp_env("STS_BF3_GROUP_TILE");   // experiment knob: per-stage tile digits
        const int bt = bgt && (int)strlen(bgt) > i ? (bgt[i] >= '0' && bgt[i] <= '9' ? bgt[i] - '0' : (bgt[i] >= 'a' && bgt[i] <= 'z' ? bgt[i] - 'a' + 10 : -1)) : -1;
        conv_bf3_group(A.G1, stream, bt);
        conv_bf3_group(A.G2, stream, bt);
    } else {
        // every layer is checked on its own: later layers have larger dilations, and a halo beyond the staged
        // LDS window (e.g. k = 11 with dilation 7) must take the per-conv path, which falls back to conv_generic
        for (const ConvGroup* G : {&A.G1, &A.G2}) {
            if (conv_group_eligible(*G)) conv_mfma_group(*G, stream, gtile);
            else for (int j = 0; j < nk; j++) { if (conv_mfma_eligible(G->g[j])) conv_mfma(G->g[j], stream, -1); else conv_generic(G->g[j], stream); }
        }
    }
}

// The one place the decoder writes the matrix-core accounts (Engine::conv books the convs it routes itself).  mfma_launches_ counts a fused
// layer as 1 and a pair as 2 also when per_chain sends out nk times as many kernels: decoder_mfma_launches is compared across versions.
void Engine::ResStage::book(LayerKind k, const LayerArgs& A) {
    e.mfma_flops_ += A.fl;
    if (k == LayerKind::FusedWino) e.mfma_exec_ += A.flw;
    else if (k == LayerKind::FusedDirect || k == LayerKind::StagedMfma) e.mfma_exec_ += A.fl;
    else e.bf16_exec_ += e.products() * A.fl;
    e.mfma_launches_ += is_fused(k) ? 1 : 2;
}

// Layer d of ALL chains goes out as one grouped launch: 2 * nd launches per stage instead of
// 2 * nd * nResK, nResK times the workgroups per launch (a batch-1 stage otherwise yields only a
// few hundred), and chains of different kernel size backfill each other inside the grid.
void Engine::ResStage::run_grouped(const float** outs) {
    LayerArgs A;
    for (int j = 0; j < nk; j++) cur[j] = b.up();
    if (per_chain) fork();
    for (int d = 0; d < nd0; d++) {
        fill_convs(d, A);
        const LayerKind k = plan_layer(d, A);
        launch(k, d, A);
        book(k, A);
        for (int j = 0; j < nk; j++) cur[j] = b.next(j, cur[j]);
    }
    if (per_chain) join(kAux);
    for (int j = 0; j < nk; j++) outs[j] = cur[j];
}

// not grouped: every conv through Engine::conv, the chains concurrently on separate HIP streams
void Engine::ResStage::run_forked(const float** outs) {
    const bool forked = nk > 1 && nk <= 8;
    if (forked) fork();
    for (int j = 0; j < nk; j++) {
        if (forked) e.cur_ = aux(j);
        const float* x = b.up();
        for (size_t d = 0; d < rb(j).c1.size(); d++) {
            const auto o = resblock_opts(x);
            float* nxt = b.next(j, x);
            e.conv(rb(j).c1[d], x, l2, b.t1(j), l2, o.first);
            e.conv(rb(j).c2[d], b.t1(j), l2, nxt, l2, o.second);
            x = nxt;
        }
        outs[j] = x;
    }
    if (forked) { join(nk < kAux ? nk : kAux); e.cur_ = e.stream; }
}

// ---- stage 5: one decode pass over `nw` windows of z (WinGeom; normal call: the windows ARE the utterances and zoff == coff == offF)
// ---------------- decoder trunk (Generator_hifigan.cpp:139-175 and the identical loops of MS/Istft/MBB)
// (zoff0 = frame offset of window 0 inside z: the by-value form of a single window; wlen0: its real length, < 0: device tables)
int Engine::run_decode(RunCtx& c, int nw, long Wtot, int maxW, int zoff0, int wlen0) {
    RUN_ALIASES(c)
    stage_begin(3);
    const WinGeom win{nw == 1 && !no_inline_seg && wlen0 >= 0, nw, zoff0, wlen0, d_win};
    auto lvF = [&](int scale, int extra) {
        Lvl l; l.seg = win.seg(scale, extra);
        l.nb = nw; l.max_len = maxW * scale + extra;
        l.total = Wtot * scale + (long)nw * extra; l.ld = l.total;
        return l;
    };
    Lvl lz; lz.seg = win.zseg();
    lz.nb = nw; lz.max_len = maxW; lz.total = Fld; lz.ld = Fld;
    const Lvl lw1 = lvF(1, 0);
    {
        ConvOpt op;
        if (M.dec_type == 0 && ms && c.bstream) {
            // a stream of several utterances: the conditioning is indexed by window, not by utterance -- gather each window's speaker (the
            // sid table of the step) and run dec_cond over the nw windows
            Lvl lw; lw.seg = SegView{nullptr, nullptr, 1, 0, 0, nw}; lw.nb = 1; lw.max_len = nw; lw.total = nw; lw.ld = nw;
            // (a run with a speaker mix: the step's table holds each window's UTTERANCE there, and the windows take that column of the blended
            // bt.g [gin][B] -- the same gather with bt.g as the table; a window's index is not its utterance's once a short one has finished)
            // (a planned open stream's step: the table is the stream's gpool [gin][max_live] and the column the window's slot)
            if (c.mix) gather_speaker(bt.g, c.live && c.live->gpool ? c.live->max_live : B, M.gin, d_win + StepTab::sid(nw), nw, bf.gwin, stream);
            else gather_speaker(M.emb_g, M.spk_num, M.gin, d_win + StepTab::sid(nw), nw, bf.gwin, stream);
            conv(M.dec_cond, bf.gwin, lw, bf.cond_win, lw, ConvOpt()); op.ubias = bf.cond_win;
        } else if (M.dec_type == 0 && ms) { conv(M.dec_cond, bt.g, lvB, bt.cond_dec, lvB, ConvOpt()); op.ubias = bt.cond_dec; }
        conv(M.conv_pre, bf.z, lz, bf.x0, lw1, op);
    }
    const float* x = bf.x0;
    int S = 1;
    Lvl lx = lw1;
    // the mean over a stage's ResBlock chains is not formed by a launch of its own: the conv that consumes it (the next upsampler, the
    // output conv) adds the chains' outputs up while it stages its input window (ConvArgs::nsum), -4 launches / ~40 us per step
    struct { const float* p[3] = {nullptr, nullptr, nullptr}; int n = 0; float* dst = nullptr; long count = 0; } mean;
    auto with_mean = [&](ConvOpt& o) { if (mean.n >= 2) { o.sum1 = mean.p[1]; o.sum2 = mean.p[2]; o.nsum = mean.n; o.sum_dst = mean.dst; o.sum_n = mean.count; } };
    static const bool no_sum_fold = exp_flag("STS_NO_SUM_FOLD");   // experiment knob
    mark(5);
    in_mfma_region_ = true;
    for (int i = 0; i < M.n_up; i++) {
        const DConv& up = M.ups[i];
        const int S2 = S * M.up_rate[i];
        const Lvl l2 = lvF(S2, 0);
        const size_t ce = (size_t)up.Cout * l2.total;
        ResStage st(*this, i, l2, (i & 1) ? bf.regB : bf.regA, ce);
        float* bup = st.b.up();
        ConvOpt ou; ou.in_act = 1; ou.slope = 0.1f;
        {   // experiment knob: per-stage kernel variant of the upsamplers, e.g. STS_UP_TILE=6--- (digit = conv mode - 2, '-' = automatic)
            static const char* ut = exp_env("STS_UP_TILE");
            if (ut && (int)strlen(ut) > i && ut[i] >= '0' && ut[i] <= '7') ou.tile = ut[i] - '0';
        }
        with_mean(ou);
        conv(up, x, lx, bup, l2, ou);
        mean.n = 0;
        const int nk = st.nk;
        const float* outs[8];
        st.plan();
        if (st.grouped) st.run_grouped(outs); else st.run_forked(outs);
        // xs = ((rb_0 + rb_1) + ...) / nResK (Generator_hifigan.cpp:159-173): formed by the consumer while it stages its input (2 or 3
        // chains), or -- the fallback -- by a launch that writes it over the (now dead) upsampler output
        if (nk == 1) x = outs[0];                       // (x / 1 == x)
        else if (nk <= 3 && !no_sum_fold) { mean.p[0] = outs[0]; mean.p[1] = outs[1]; mean.p[2] = nk > 2 ? outs[2] : nullptr; mean.n = nk; mean.dst = bup; mean.count = (long)ce; x = outs[0]; }
        else { sum_scale(bup, outs, nk, (long)ce, stream); x = bup; }
        S = S2; lx = l2;
    }
    in_mfma_region_ = false;
    mark(6);

    // ---------------- decoder tail
    // (the output chain decides whether the tail writes its float wave, and whether its int16 samples are the PCM or scratch)
    float* wave = c.oc.wave[OS_TAIL] ? bf.wave : nullptr;
    int16_t* const pcm = bf.pcm_nat;
    const long Ntot = Wtot * hop;
    if (M.dec_type == 0) {          // Generator_hifigan.cpp:177-179 + SynthesizerTrn.cpp:389-396
        ConvOpt o; o.in_act = 1; o.slope = 1e-2f; o.epi = EPI_TANH_PCM; o.pcm = pcm; o.aux = wave;
        with_mean(o);
        conv(M.conv_post, x, lx, nullptr, lx, o);
    } else {                        // Generator_MBB.cpp:174-202, Generator_MS.cpp:198-228, Generator_Istft.cpp:180-197
        const Lvl lsb = lvF(S, 1);
        ConvOpt o; o.in_act = 1; o.slope = 1e-2f; o.reflect = 1;
        with_mean(o);
        conv(M.conv_post, x, lx, bf.tailA, lsb, o);
        const int bands = M.dec_type == 2 ? 1 : 4;
        const Lvl ltm = lvF(S * 4, 0), lo = lvF(S * 16, 0);
        if (tail_fused && M.dec_type != 2 && sbC == 72 && istft_tail_fused_ok(bands, M.fir_taps, M.fir_pad)) {
            // spectrum + inverse DFT / overlap-add + synthesis filter + int16 cast in one launch (misc_kernels.hip istft_tail_fused_kernel)
            istft_tail_fused(bf.tailA, lsb.ld, lsb.seg, M.synth_fir, M.fir_taps, M.fir_pad, (float)M.subbands, M.fir_bias, wave, pcm, lo.seg, nw, ltm.max_len, stream);
        } else {
            istft_spectrum(bf.tailA, lsb.ld, sbC, bf.tailB, lsb.total, stream);
            float* tm = bf.tailC;
            istft_ola(bf.tailB, lsb.ld, bands, 18, lsb.seg, tm, ltm.ld, ltm.seg, nw, ltm.max_len, stream);
            if (M.dec_type == 2) {
                quantize_pcm(tm, pcm, Ntot, stream);
                if (wave) HIPCK(hipMemcpyAsync(wave, tm, (size_t)Ntot * 4, hipMemcpyDeviceToDevice, stream));
            } else synth_fir(tm, ltm.ld, ltm.seg, M.synth_fir, M.fir_taps, M.fir_pad, (float)M.subbands, M.fir_bias /* 0 unless the blob's learned filter carries one (MS); the PQMF bank has none */, wave, pcm, lo.seg, nw, ltm.max_len, stream);
        }
        flops_[3] += 2.0 * (double)Ntot * (16.0 * 4 + 4 * 18 * 4 / 4.0);
    }
    return decode_end(c, wave, win, Wtot, maxW);
}

// the end of a decode: a walk down the output chain (out_chain.hpp) behind the tail with one current float signal -- each running stage
// reads it, writes its own buffer, which becomes the current one, and casts into the PCM when the plan names it the writer -- then the
// taps.  (A stream: run_stream_steps runs the chain from the resampler on, on each step's windows.)
int Engine::decode_end(RunCtx& c, const float* wave, const WinGeom& win, long Wtot, int maxW) {
    const OutChain& oc = c.oc;
    const int hop = c.hop, wlen0 = win.wlen0;
    const bool whole = !c.ss;
    int nw = win.nw;
    long long max_out = out_count((long long)maxW * hop);
    WinGeom dw = win;                       // the utterances everything behind the gain plan and the join sees
    const float* const raw = wave;          // (the "wave" tap stays the un-gained signal)
    const float* cur = wave;
    auto pcm_of = [&](int stage) { return oc.writer == stage ? c.bf.pcm : nullptr; };
    if (oc.run[OS_GAIN] && c.gain) {    // (the native-rate plan stage: the gain kernel, then the warp of a pitch plan, each if its plan is there)
        // the gain plan on every window's native samples at their absolute positions (a streaming window: halo included), one launch
        GainArgs g{};
        g.x = cur; g.y = c.bf.wave_gain; g.pcm = c.pitch ? nullptr : pcm_of(OS_GAIN);
        g.wseg = win.seg(hop, 0); g.hop = hop;
        if (c.ss) { const StepTab t(nw, true, false, false, false, c.pitch); g.utt = (const int*)(c.bf.stab + t.utt); g.wtab = (const long long*)(c.bf.stab + t.rs); }
        if (c.ss && c.pitch) {      // (a warped step: the RsRow describes the warped window, the decode window's u0 is the PsRow's)
            const StepTab t(nw, true, false, false, false, true);
            g.wtab = (const long long*)(c.bf.stab + t.ps_rows); g.wstride = (int)(sizeof(PsRow) / 8); g.wcol = 1;
        }
        g.tseg = c.lvT.seg; g.cum = c.bt.cum; g.q = c.bt.gain_q; g.h = c.bt.gain_h;
        gain_plan_run(g, nw, (long long)maxW * hop, stream);
        cur = g.y;
    }
    int sig_scale = hop;                    // native samples per unit of dw's lengths
    if (oc.run[OS_GAIN] && c.pitch && whole) {      // (a stream: run_stream_steps runs the range form on each step's windows)
        // the pitch plan's warp of every utterance (gained or not), one launch.  From here on utterance b is N'_b samples long: dw carries
        // the warped counts at scale 1 for the resampler's segments and for signal()
        PitchArgs p{};
        pitch_args_carve(p, c.bt.pitch_words, nw, c.pitch_rows);
        p.x = cur; p.y = c.bf.wave_pitch; p.pcm = pcm_of(OS_GAIN); p.table = d_pitch_table_;
        pitch_plan_run(p, nw, c.pitch_max, pitch_table_in_lds(), stream);
        cur = p.y;
        dw = WinGeom{win.inl, nw, 0, (int)c.pitch_nout[0], c.bt.pitch_win};
        sig_scale = 1; max_out = out_count(c.pitch_max);
    }
    if (oc.run[OS_JOIN] && whole) {     // (a joined stream: run_stream_steps joins each step's windows into a window of J)
        // the B sentences (gained or not) into the one joined signal, silence included, one launch.  From here on there is ONE utterance of
        // F_J frames: one resampled signal, one loudness, one set of limiter stats
        JoinArgs j{};
        j.x = cur; j.y = c.bf.wave_join; j.pcm = pcm_of(OS_JOIN);
        j.wseg = win.seg(hop, 0);
        if (win.inl) j.isil = join_sil[0]; else j.sil = c.bt.join_sil;
        j.B = nw; j.hop = hop; j.h = join_h; j.NJ = c.FJ * hop;
        join_run(j, stream);
        cur = j.y;
        dw = WinGeom{true, 1, 0, (int)c.FJ, nullptr};
        nw = 1; max_out = out_count(c.FJ * hop);
    }
    // EqArgs / LoudArgs / LimArgs: the float signal at the output rate and its utterances' lengths
    auto signal = [&](auto& a) {
        a.x = cur;
        a.len = dw.len(); a.ilen = dw.ilen(); a.scale = sig_scale;
        a.P = c.rsP; a.Q = c.rsQ;
    };
    if (oc.run[OS_RESAMPLE] && whole) {
        ResampleArgs a{};
        a.x = cur;
        a.seg = dw.seg(sig_scale, 0);
        a.table = d_rs_table; a.P = rs.P; a.Q = rs.Q; a.K = rs.K;
        a.pcm = c.bf.pcm_rs; a.wave_out = c.bf.wave_out;
        resample_pcm(a, nw, max_out, stream);
        cur = a.wave_out;
    }
    if (oc.run[OS_EQ] && whole) {       // (a stream: run_stream_steps runs its stream mode on each step's windows)
        // the equaliser on every utterance of the float signal at the output rate (two launches)
        EqArgs a{};
        signal(a);
        a.S = c.eqS; a.tab = d_eq_;
        a.y = c.bf.wave_eq; a.pcm = pcm_of(OS_EQ);
        eq_ws_carve(a, c.bf.eqws, nw, c.Ocap);
        eq_run(a, nw, max_out, stream);
        cur = a.y;
    }
    const float* gloud = nullptr;
    if (oc.run[OS_LOUD] && whole) {     // (a stream that measures: run_stream_steps runs the stream mode on what each step delivers)
        // loudness of every window (= utterance) of the current signal; normalising, the gain cast writes the PCM unless the limiter does
        if (loud_k_rate_ != out_rate) {
            if (!loud_coef(out_rate, &loud_k_)) return fail(STS_EINVAL, "loudness: output rate outside [8000, 48000]");
            loud_k_rate_ = out_rate;
        }
        LoudArgs a{};
        signal(a);
        a.target = loud_target; a.ceiling = loud_peak; a.k = loud_k_;
        loud_ws_carve(a, c.bf.lws, nw, c.Ocap);
        a.out = loud_dev_;
        a.no_clamp = oc.loud_no_clamp;
        loudness_run(a, nw, max_out, pcm_of(OS_LOUD), stream);
        if (oc.lim_gloud) gloud = a.gain;
    }
    if (oc.run[OS_LIMIT] && whole) {
        // the limiter on the same signal (times the loudness gain when normalising)
        LimArgs a{};
        signal(a);
        a.H = c.limd.H; a.c = c.limd.c; a.G = c.limd.G; a.gloud = gloud;
        a.y = c.bf.wave_lim; a.pcm = pcm_of(OS_LIMIT); a.stat = (unsigned*)c.bf.limws;
        limiter_run(a, nw, max_out, stream);
        HIPCK(hipMemcpyAsync(lim_host_, c.bf.limws, (size_t)nw * 16, hipMemcpyDeviceToHost, stream));
    }
    mark(4);
    if (raw && record_taps) {
        tap("wave", raw, 1, Wtot * hop, (wlen0 >= 0 ? (long)wlen0 : Wtot) * hop);
        if (c.gain && !c.ss) tap("wave_gain", c.bf.wave_gain, 1, Wtot * hop, (wlen0 >= 0 ? (long)wlen0 : Wtot) * hop);
        if (c.pitch) tap("wave_pitch", c.bf.wave_pitch, 1, (long)c.pitch_total, (long)c.pitch_total);
        if (c.join && !c.ss) tap("wave_join", c.bf.wave_join, 1, (long)(c.FJ * hop), (long)(c.FJ * hop));
        if ((c.bf.wave_out || c.bf.wave_lim || c.bf.wave_eq) && !c.ss) {    // (a stream has moved the pinned block p_lenF points into: not read then)
            long long n = 0;        // samples at the output rate: what both taps hold
            if (c.join) n = out_count(c.FJ * hop);
            else if (c.pitch) for (int b = 0; b < c.B; b++) n += out_count(c.pitch_nout[(size_t)b]);
            else if (wlen0 >= 0) n = out_count((long long)wlen0 * hop);
            else for (int b = 0; b < c.B; b++) n += out_count((long long)c.p_lenF[b] * hop);
            if (c.bf.wave_out) tap("wave_out", c.bf.wave_out, 1, (long)c.Ocap, (long)n);
            if (c.bf.wave_eq) tap("wave_eq", c.bf.wave_eq, 1, (long)c.Ocap, (long)n);
            if (c.bf.wave_lim) tap("wave_lim", c.bf.wave_lim, 1, (long)c.Ocap, (long)n);
        }
    }
    return STS_OK;
}

}  // namespace sts
