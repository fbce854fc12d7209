// kernels.hpp -- device-kernel interface of the MI355X (gfx950) SummerTTS acoustic engine.
//
// Activation layout (same memory order as the reference's column-major Eigen MatrixXf [time, chan],
// /root/reference/src/header/nn_conv1d.h:13-29): channel-major, time contiguous, fp32.  A batch of
// utterances is PACKED along the time axis of one buffer  a[c * ld + pos]; a SegView says where
// utterance b lives so that convolution halos never cross utterance boundaries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/summertts_hip.h"
#include "pitch_layout.hpp"
#include "utt_tables.hpp"

namespace sts {

// Utterance b occupies positions [off[b]*scale + b*extra, ... + len[b]*scale + extra) of a packed row.
// off/len are in "base units" (phonemes for the text-side buffers, frames for the acoustic side);
// scale is the upsampling factor accumulated so far; extra is 1 for the MB-iSTFT tail (frames+1 rows).
// A single-segment view may carry its geometry BY VALUE (off == nullptr: the one segment is {ioff, ilen}): for the
// reference's own call shape -- one utterance per infer() -- every kernel then starts without the dependent scalar load
// of its segment table (one memory round trip less on each of the ~140 latency-bound launches of a batch-1 step).
struct SegView {
    const int* off;
    const int* len;
    int scale;
    int extra;
    int ioff, ilen;
};

enum Epilogue : int {
    EPI_STORE = 0,       // y = v
    EPI_RESADD = 1,      // y = v + res
    EPI_SUB = 3,         // y = y - v                                       (coupling: x1 -= m)
    EPI_GATE = 4,        // y = tanh(v_t) * sigmoid(v_s)                     (WN gated unit)
    EPI_RESSKIP = 5,     // rows <  H: y[row] += v ; rows >= H: aux[row-H] (+)= v   (WN res/skip)
    EPI_TANH_PCM = 6,    // wave = tanh(v) ; pcm = trunc(wave * 32737)       (HiFi-GAN tail, Cout == 1)
};

struct ConvArgs {
    const float* x; long x_ld;      // input  [Cin][x_ld]
    float* y; long y_ld;            // output [Cout][y_ld]
    const float* w;                 // packed weights [ntap][Cin_pad][Cout_pad] (co contiguous); depthwise: [ntap][Cout_pad]
    const float* bias;              // [Cout_pad] (packed row order) or null
    const float* ubias; int ubias_ld;  // per-utterance bias [Cout][ubias_ld = B] or null
    const float* res; long res_ld;  // residual input (EPI_RESADD)
    float* aux; long aux_ld;        // skip output (EPI_RESSKIP) / float wave (EPI_TANH_PCM)
    int16_t* pcm;                   // EPI_TANH_PCM
    int Cin, Cout, Cin_pad, Cout_pad, ntap;
    int tap_step, tap_off;          // input position of output n, tap j: n + j*tap_step + tap_off
    int out_stride, out_off;        // output position of n: n*out_stride + out_off (polyphase transposed conv)
    int transposed, n_extra;        // n runs over [0, transposed ? in_len + n_extra : out_len)
    int depthwise;
    int in_act; float in_slope;     // input activation: 0 none, 1 leaky-relu(slope) (slope 0 == relu)
    int in_reflect;                 // logical input = reflect-pad-left-1 view of x (MB-iSTFT tail)
    int epi, epi_flag; float epi_scale; int H;
    int gate_perm;                  // EPI_GATE rows are packed as (tanh16, sigmoid16) inside every 32-row tile
    SegView in_seg, out_seg;
    int B, max_n;                   // batch size, max n_count over the batch (grid sizing)
    // cross-workgroup split of K (split-K kernel only, EPI_STORE only): slice s of `kslices` accumulates its share of the
    // (tap, channel) groups and writes a PARTIAL output to y + s * kslice_stride (bias rides on slice 0); the consumer
    // (layer_norm: LnArgs::nb) adds the partials up.  For convs with a long K and too few output tiles to fill the chip
    // (FFN second conv at batch 1: K = 2304 over 24 tiles).
    int kslices; long kslice_stride;
    // optional Winograd form of the same weights (conv_wino_*): [seg][4][Cin_pad][Cout_pad], see wino_pack()
    const float* wu; int wino_n3, wino_n2;
    // optional split-bf16 form of the same weights (conv_bf3.hip): every fp32 weight as three bf16 terms, fragment-packed by
    // bf3_pack(); null = this conv only has the fp32 matrix-core path
    const void* wb3;
    // optional restriction of the OUTPUT to the columns n in [keep_lo, keep_hi) (keep_hi == 0: all; plain / residual epilogue of
    // non-polyphase convs only).  No caller sets it since the persistent stage kernel of round 3 was deleted (round 5); the epilogues keep the test
    int keep_lo, keep_hi;
    // arithmetic of the wb3 copy (conv_bf3.hip): 0 = three bf16 terms / six products, 1 = two fp16 terms / three products with the
    // weights scaled by a power of two (wscale = its inverse, applied to the finished tile); ovf (math 1): raised when a staged
    // input value does not fit fp16
    int math; float wscale; unsigned* ovf;
    // optional extra input terms (same layout, ld and segments as x): the logical input is ((x + xs1) [+ xs2]) / nsum for nsum = 2 / 3
    // (0 / 1: plain x) -- the mean over a decoder stage's ResBlock chains (Generator_hifigan.cpp:159-173) formed in the staging code
    // of the conv that consumes it instead of by a launch of its own.  Taken by conv_bf3 (conv_bf3_takes_sum) and conv_cout1 only.
    const float* xs1; const float* xs2; int nsum;
    // polyphase transposed conv with ROW-INTERLEAVED phases (conv_bf3 only; 0 = off, else == out_stride in {2, 4, 8}): the packed rows are
    // rho = cout * stride + phase (Cout / Cout_pad count those merged rows, bias is per merged row), so a lane's four consecutive accumulator
    // rows are consecutive OUTPUT POSITIONS of one channel and the tile leaves through 16-byte (stride 2: 8-byte) stores that fill whole
    // sectors -- the phase-major form writes one dword per lane at a stride of `stride` dwords (round 6, profiles/r06_upsampler_rowph.log)
    int rowph;
};

// Segmented Winograd F(2,3): a k-tap filter is cut into n3 three-tap segments followed by n2 two-tap segments
// (k = 3 n3 + 2 n2, n2 in {0,1,2}); every segment contributes 4 (3-tap) or 3 (2-tap) products per pair of
// outputs instead of 6 / 4, and all segments accumulate into the same four Winograd-domain sums.
__host__ __device__ inline void wino_split(int k, int* n3, int* n2) { *n2 = (k % 3 == 0) ? 0 : (k % 3 == 2 ? 1 : 2); *n3 = (k - 2 * *n2) / 3; }
// w: [Cout][k][Cin] source order (or any accessor order given by the strides), dst: [seg][4][Cin_pad][Cout_pad]
void wino_pack(const float* w, long s_out, long s_tap, long s_in, int Cout, int k, int Cin, int Cin_pad, int Cout_pad, float* dst);
bool conv_wino_eligible(const ConvArgs& a);
void conv_wino(const ConvArgs& a, hipStream_t st);

struct LnArgs {
    const float* a; long a_ld;      // v = a (+ b_0 + b_1 + ... + b_{nb-1}, in this order)
    const float* b; long b_ld;      // b_p = b + p * b_stride (split-K partial outputs of the producing conv); nb <= 1: one operand
    int nb; long b_stride;
    const float* res; long res_ld;  // out = res + f(v) when non-null
    float* y; long y_ld;
    const float* gamma; const float* beta;
    int C;
    int pre_relu, post_gelu;
    // optional fused depthwise conv on the input: v = dw_b[c] + sum_j dw_w[j*dw_ld + c] * a[c][pos + j*dw_dil - dw_pad]
    // (DDSConv's separable conv feeds straight into its LayerNorm, /root/reference/src/modules/DDSConv.cpp:97-100)
    const float* dw_w; const float* dw_b; int dw_k, dw_dil, dw_pad, dw_ld;
    SegView seg; int B, max_len;
};

// Fused column-block layer (col_layer.hip): [depthwise conv + LayerNorm + GELU] -> 1x1 conv (C -> C) -> (+ add) ->
// LayerNorm -> [GELU] -> [+ res], one workgroup per 16 time steps, all C channels.
struct ColLayerArgs {
    const float* x; long x_ld;                  // input [C][ld]
    // optional rank-1 term of the input: h[c][t] = (xs_w[c] * xr[t] + xs_b[c]) + x[c][t] -- the 1 -> C "pre" conv of a ConvFlow
    // (/root/reference/src/modules/ConvFlow.cpp:252-254: pre(x0) + g) folded into the first DDSConv layer; xr == null: xr = 0.  Product and
    // both sums are rounded to float one by one, as the separate conv rounds them (col_layer.hip cl_fold: no FMA)
    const float* xs_w; const float* xs_b; const float* xr;
    const float* dw_w; const float* dw_b; int dw_k, dw_dil, dw_pad, dw_ld;   // optional depthwise conv (null: plain input)
    const float* g1; const float* b1;           // LayerNorm after the depthwise conv (followed by GELU)
    const float* wc; const float* bias;         // 1x1 conv weights in the kernel's own A-strip order (col_layer_pack)
    const float* add; long add_ld;              // v = add + conv(..)   (null: v = conv(..))
    const float* g2; const float* b2; int post_gelu;
    const float* res; long res_ld;              // out = res + f(v)
    float* y; long y_ld;
    int C;
    SegView seg; int B, max_len;
    // optional tail (the last DDSConv layer of a ConvFlow of the stochastic duration predictor): the layer's output stays in LDS, the
    // 1x1 projection to the 29 spline parameters (/root/reference/src/modules/ConvFlow.cpp:256-258) and the reverse spline step with
    // the channel flip (StochasticDurationPredictor.cpp:136-142: (r0, r1) -> (spline(r1 | h), r0)) run in the same launch; y is not written
    const float* tp_w; const float* tp_b;       // projection weights [C][32] (cin-major, rows >= 29 zero) and bias [29]; null: no tail
    float tp_fs;                                // sqrt(filter channels)
    const float* tp_r0; const float* tp_r1;     // latent halves in (null: zeros)
    float* tp_o0; float* tp_o1;                 // latent halves out
};
bool col_layer_eligible(const ColLayerArgs& a);
bool col_layer_width_ok(int C);
// w: [C out][C in] (blob order of a 1x1 conv) -> dst[C * C] in col_layer_kernel's A-strip order
void col_layer_pack(const float* w, int C, float* dst);
void col_layer(const ColLayerArgs& a, hipStream_t st);

// [embedding | LayerNorm(a + partials)] -> x_out, then y = conv1x1(x_out) with npass * C output rows (col_layer.hip)
struct ColProjArgs {
    const int* ids; const float* emb; int vocab; float emb_scale;        // embedding form (ids != null)
    const float* a; long a_ld; const float* bp; long b_ld; int nb; long b_stride;   // LayerNorm form: v = a + bp_0 + ... + bp_{nb-1}
    const float* gamma; const float* beta;
    float* x_out; long x_ld;                    // the staged input, also written out (residual of the layer's post-LayerNorm)
    const float* wc; const float* bias; int Cout, npass;    // weights in col_proj_pack order, bias in plain row order
    float* y; long y_ld;
    int C;
    SegView seg; int B, max_len;
    // split != 0: grid z = npass (+ 1 with a rider); workgroup z forms x for its 16 columns itself and runs pass z ONLY (one A strip, one
    // MFMA chain); z = 0 alone writes x_out.  The same sums in the same order as split == 0, where one workgroup runs every pass.
    int split;
    // optional rider of the split form (wc2 != null): one more single-pass 1x1 conv over the same staged x, with its own weights
    // (col_proj_pack order), bias and output, Cout2 <= C rows; it is workgroup z = npass
    const float* wc2; const float* bias2; float* y2; long y2_ld; int Cout2;
};
bool col_proj_eligible(const ColProjArgs& a);
void col_proj(const ColProjArgs& a, hipStream_t st);
void col_proj_pack(const float* w, int C, int Cout, float* dst);

struct AttnArgs {
    const float* q; const float* k; const float* v; float* o; long ld;
    const float* relk; const float* relv;   // [kc][px] (reference column-major [px, kc])
    int kc, px, win, nheads;
    SegView seg; int B, max_len;
    int block_min_wgs;              // the 16-queries-per-workgroup matrix-core kernel from this many workgroups on (0: default 96)
    int attn_reg;                   // 1: the one-query kernel with its operands in registers where the shape allows (attention_reg_kernel)
};


// ---- one launch per WaveNet layer of the reverse flow (wn_flow.hip, round 4).  All intermediate tensors are CHANNEL-MINOR [frame][channel]
// (packed frames as everywhere else); group g of G = H / Cg handles the gated channels [g Cg, (g + 1) Cg).
struct FlowLayerArgs {
    SegView seg; int B, max_len; long tot;      // frame-level segments of the packed batch; tot = frames of the whole batch (buffer extents)
    int H, half, G, Cg, k, halo;                // WaveNet width, C / 2, channel groups, gate conv taps and (k - 1) / 2
    int layer;                                  // 0: first layer of a coupling (stages x0, runs `pre` inside the launch)
    // layer 0: x0 rows (channel-major [half][x0_ld]) + pend_n pending -m slices (channel-minor [frame][half], pend_stride floats apart)
    // of the previous coupling; their sum is x0' -- written to x0_out (channel-major, another buffer than x0; null: nothing pending)
    const float* x0; long x0_ld; const float* pend; int pend_n; long pend_stride; float* x0_out; long x0_out_ld;
    const void* w_pre; const float* b_pre; float s_pre;         // `pre` (1x1, half -> H): two-term fp16 pack (natural k order), bias, 2^-s
    // layer > 0: h = h_in + part_in[0 .. part_n)   (channel-minor [frame][H], slices part_stride floats apart)
    const float* h_in; const float* part_in; int part_n; long part_stride;
    float* h_out;                               // this layer's h (each group writes its channel slice of its own columns)
    float* part_out;                            // this layer's partial res sums (group g -> slice g), same strides
    float* macc; long macc_stride; int macc_init;     // -m partial accumulators [frame][half] per group; macc_init: first layer of the coupling
    const void* w_gate; const float* b_gate; float s_gate;      // gate conv, rows (tanh16, sigmoid16) per 32-row tile; layer 0: perm_k order
    const float* ubias; int ubias_ld;           // speaker conditioning of the gate rows [2H][B] or null
    const void* w_c; float s_c; int rows_c, rows_res;           // 1x1 conv on the gated channels (perm_k order, all H channels, chunk-major): rows = [res | -m] padded to 32
    const float* b_res; const float* b_m;       // biases (added once: by group 0; b_m with macc_init)
    unsigned* ovf;                              // raised when a staged value leaves the fp16 range
};
struct FlowFinishArgs {
    SegView seg; int B, max_len; int half;
    const float* src; long src_ld; float* dst; long dst_ld;     // channel-major rows of one half
    const float* macc; int n; long macc_stride;
};
bool flow_layer_shape_ok(int H, int half, int k, int dil, int n_layers);
int flow_layer_groups(int H);
void flow_layer(const FlowLayerArgs& a, hipStream_t st, int nt = 32);       // nt: output frames per workgroup, 32 or 16 (same bits)
void flow_finish(const FlowFinishArgs& a, hipStream_t st);

// ---- launchers (all asynchronous on `st`) ------------------------------------------------------
// Matrix-core (v_mfma_f32_32x32x2_f32) implicit-GEMM conv.  Returns false when the shape is not
// eligible (caller then uses conv_generic).  `tile` < 0 picks a tile configuration heuristically.
bool conv_mfma_eligible(const ConvArgs& a);
void conv_mfma(const ConvArgs& a, hipStream_t st, int tile = -1);
// several independent convs of identical geometry in one grid (decoder ResBlock chains of one stage)
constexpr int kMaxGroup = 4;
struct ConvGroup { ConvArgs g[kMaxGroup]; int n; };
// One ResBlock1 layer, x + conv2(lrelu(conv1_dilated(lrelu(x)))), as ONE kernel for narrow stages
// (C = 32 / 64): the intermediate never leaves the CU (LDS).  Up to kMaxGroup chains per grid.
struct ResLayerArgs {
    const float* x; float* y;                 // [C][ld], distinct buffers
    const float *w1, *b1, *w2, *b2;           // packed [k][C][C] (cout contiguous), biases may be null
    int k1, dil1, k2;
    const float *wu1, *wu2;                   // Winograd-domain copies [seg][4][C][C] (wino_pack) or null
    const void *wb1, *wb2;                    // split-bf16 copies (bf3_pack; wb2 with the k order of the parked intermediate) or null
    float ws1, ws2;                           // ResLayerGroup::math 1: inverse weight scales of wb1 / wb2 (ConvArgs::wscale)
};
struct ResLayerGroup {
    ResLayerArgs g[kMaxGroup];                // must stay the first member (indexed through the kernarg pointer)
    int n, C; long ld; float slope;
    SegView seg; int B; int max_n;
    int math; unsigned* ovf;                  // arithmetic of wb1 / wb2 and its overflow flag (ConvArgs::math / ovf)
};
bool resblock_layer_eligible(const ResLayerGroup& G);
void resblock_layer(const ResLayerGroup& G, hipStream_t st);
// the same layer with both convs in the Winograd domain (segmented F(2,3), see conv_wino_body)
bool resblock_wino_eligible(const ResLayerGroup& G);
void resblock_wino(const ResLayerGroup& G, hipStream_t st);
bool conv_group_eligible(const ConvGroup& G);
// fp32 conv on the bf16 matrix cores: both operands split exactly into three bf16 terms (x = hi + mid + lo, 24 mantissa
// bits), the six products of order <= 2^-16 accumulated in fp32 (conv_bf3.hip)
bool conv_bf3_eligible(const ConvArgs& a);
// an eligible conv whose automatic tile is instantiated with the summed-input staging (ConvArgs::nsum >= 2)
bool conv_bf3_takes_sum(const ConvArgs& a);
bool conv_cout1_takes(const ConvArgs& a);      // conv_generic would route this conv to the single-output-channel FIR kernel
void conv_bf3(const ConvArgs& a, hipStream_t st, int tile = -1);
// workgroups the automatic tile choice would launch (the caller keeps latency-bound launches on the split-K fp32 kernel)
long conv_bf3_blocks(const ConvArgs& a);
bool conv_bf3_group_eligible(const ConvGroup& G);
void conv_bf3_group(const ConvGroup& G, hipStream_t st, int tile = -1);
// wp: packed fp32 weights [nslab][Cin_pad][Cout_pad] (nslab = taps, or phases x taps of a polyphase transposed conv)
// -> dst: [slab-major, see conv_bf3.hip] 3 x bf16; returns the number of bytes written (dst == null: size query)
// perm_k: the 16 input channels of a chunk in the order the fused layer kernel parks its intermediate in (k slot (h, e) of a
// chunk = channel 8 (e >> 2) + 4 h + (e & 3): the accumulator rows one lane holds)
// math 1: the two-term fp16 form of the same layout (three planes P0 / P1 / P2, conv_bf3.hip MATH 1); *wscale receives the inverse
// of the power of two the weights were scaled by
size_t bf3_pack(const float* wp, int nphase, int ntap, int Cin_pad, int Cout_pad, void* dst, bool perm_k = false, int math = 0, float* wscale = nullptr);
// slack behind a packed weight tensor, zero-filled: the kernels' unconditional prefetches run one step past the end.  Floats behind an fp32
// copy and behind the split copies the loader makes of it, bytes behind a pre-split (conv_h2p.hip / conv_h2w.hip) copy and behind a lone wb3
constexpr size_t kWeightSlackFloats = 1024, kPresplitSlackBytes = 8192, kBf3SlackBytes = 4096;
// one ResBlock1 layer on the bf16 matrix cores: x + conv2(lrelu(conv1_dilated(lrelu(x)))), whole input window staged once
bool resblock_bf3_eligible(const ResLayerGroup& G);
void resblock_bf3(const ResLayerGroup& G, hipStream_t st, int variant = -1);
void conv_mfma_group(const ConvGroup& G, hipStream_t st, int tile = -1);

// ---- two-term fp16 convs on PRE-SPLIT, channel-minor activations (conv_h2p.hip, round 6): the wide ResBlock stages of the decoder trunk.
// The producer (the split kernel at a stage's entry, then every conv's own epilogue) applies the consumer's leaky relu, splits each value into
// its two fp16 terms (conv_bf3_dev.hpp split8h) and stores them in the order the matrix core reads its operands in, so that a consumer's
// input staging is a plain copy global -> LDS (buffer_load ... lds: no registers, no VALU work) instead of 8 dword loads + ~60 VALU + 2 LDS
// stores per 32 positions x 16 channels.
//   planes  [2 planes][C / 16 chunks][ld positions][2 units][8 fp16]    byte (p, c, t, h) = p * 2 C ld + (c ld + t) 32 + 16 h
//   x16     [C / 16 chunks][ld positions][2 units][8 fp32]               the fp32 value itself (residual operand), same order
//   element e of unit h of chunk c = channel 16 c + 8 (e >> 2) + 4 h + (e & 3)   (the accumulator rows one lane holds: bf3_pack perm_k)
// A tensor in either layout takes 4 C ld bytes -- the size of the fp32 [C][ld] tensor it replaces.
struct H2PArgs {
    const void* xp; long xp_ld;           // input planes (C = Cin)
    const void* wb; float wscale;         // bf3_pack(perm_k = true, math = 1) copy of the weights and the inverse of their power-of-two scale
    const float* bias;                    // [Cout] or null
    const float* res16; long res_ld;      // residual in x16 layout or null
    float* y; long y_ld;                  // fp32 [Cout][y_ld] output or null (the last layer of a chain: what the next stage reads)
    float* y16; long y16_ld;              // x16 output or null (the next layer's residual)
    void* yp; long yp_ld; float yp_slope; // planes of lrelu(out, yp_slope) or null (the next conv's input)
    int Cin, Cout, ntap, tap_step, tap_off;
};
struct H2PGroup { H2PArgs g[kMaxGroup]; int n; SegView seg; int B, max_n; unsigned* ovf; };   // g must stay the first member
bool conv_h2p_group_eligible(const H2PGroup& G);
void conv_h2p_group(const H2PGroup& G, hipStream_t st, int tile = -1);
// ---- the same stages in the Winograd domain (conv_h2w.hip, round 6 lab): segmented F(2,3) / F(2,2), two-term fp16 MFMAs on transformed operands,
// activations as x16 only (raw fp32, channel-minor); the input transform + split happen in registers from an LDS copy of the raw window
struct H2WArgs {
    const float* x16; long x_ld;          // input (C channels); lrelu(in_slope) applied by the kernel (1 = none)
    const void* wu; float wscale;         // bf3_pack(perm_k, math 1) of the h2w_transform_weights pseudo-taps and the inverse of their scale
    const float* bias;
    const float* res16; long res_ld;      // residual (x16) or null
    float* y16; long y16_ld;              // x16 output of lrelu(out, out_slope) (1 = raw) or null
    float* y; long y_ld;                  // fp32 [C][y_ld] output or null
    float in_slope, out_slope;
    int C, k, dil;                        // Cin = Cout = C, "same" padding dil (k - 1) / 2
};
struct H2WGroup { H2WArgs g[kMaxGroup]; int n; SegView seg; int B, max_n; unsigned* ovf; };   // g first (kernarg indexing); members share the dilation
bool conv_h2w_group_eligible(const H2WGroup& G);
void conv_h2w_group(const H2WGroup& G, hipStream_t st);
int h2w_transform_weights(const float* wp, int k, int Cin, int Cout, float* dst);        // wp [k][Cin][Cout] -> dst [4 n3 + 3 n2][Cin][Cout]
void to_x16(const float* x, long x_ld, int C, long n, float* x16, long out_ld, hipStream_t st);
// fp32 [C][ld] -> planes of lrelu(x, slope) (+ the x16 copy when x16 != null) at the positions of the nb segments of `seg` only (max_n >=
// every segment's length); positions outside them are neither converted nor range-checked
void split_planes(const float* x, long x_ld, int C, const SegView& seg, int nb, long max_n, float slope, void* planes, float* x16, long out_ld,
                  unsigned* ovf, hipStream_t st);
void conv_generic(const ConvArgs& a, hipStream_t st);

void embed(const int* ids, const float* emb, int vocab, int H, float scale, float* x, long ld, int total, hipStream_t st);
void layer_norm(const LnArgs& a, hipStream_t st);
// attention = "which kernel for these AttnArgs" (pure host predicates, the LDS-size tests included) + the launch
enum AttnKernel : int { ATTN_NONE = 0, ATTN_GENERIC = 1, ATTN_REG = 2, ATTN_MFMA = 3 };
struct AttnPlan { int kernel; int jpl; int Tpad; size_t lds; };      // jpl: keys per lane of attention_reg_kernel (2 | 4), 0 otherwise
bool attention_admits(const AttnArgs& a, int kernel, AttnPlan* plan);      // do the kernel's shape limits (fixed-size arrays, LDS) hold?
AttnPlan attention_choose(const AttnArgs& a);                       // the engine's choice (ATTN_NONE: no kernel admits the shape)
void attention_launch(const AttnArgs& a, const AttnPlan& p, hipStream_t st);
int attention(const AttnArgs& a, hipStream_t st);                   // launch(choose); returns the AttnKernel launched
// y[c][seg b] += u[c*B + b]
void add_ubias(float* y, long ld, const float* u, int C, SegView seg, int B, int max_len, hipStream_t st);
void gather_speaker(const float* emb_g, int spk_num, int gin, const int* sid, int B, float* g, hipStream_t st);
// Speaker blending (the definition is in include/summertts_hip.h, sts_set_speaker_mix)
constexpr int kMixMaxTerms = 16;
constexpr float kMixMaxWeight = 16.f;
// one entry against a table of spk_num rows of gin floats (spk_num 0: a single-speaker model, which takes empty entries only)
bool speaker_mix_valid(int spk_num, int gin, const sts_speaker_mix& m, const char** why);
// The flattened term table of B entries, 32-bit words: [off B + 1 | vidx B | vw B | tsid K | tw K | vec V * gin]: entry b owns the terms
// off[b] .. off[b + 1) and, when vidx[b] >= 0, row vidx[b] of vec with the weight vw[b] (K terms and V vectors in all)
struct SpeakerMixTab { const int* off; const int* vidx; const float* vw; const int* tsid; const float* tw; const float* vec; };
void speaker_mix_flatten(const sts_speaker_mix* mixes, int B, int gin, std::vector<int32_t>& words, int* K);      // entries speaker_mix_valid accepted
inline SpeakerMixTab speaker_mix_tab(const int* words, int B, int K) {
    const int* tsid = words + 3 * (size_t)B + 1;
    return SpeakerMixTab{words, words + B + 1, (const float*)(words + 2 * (size_t)B + 1), tsid, (const float*)(tsid + K), (const float*)(tsid + 2 * (size_t)K)};
}
// g[c][b] = (float)(sum_k (double)tw[k] (double)emb_g(tsid[k], c) [+ (double)vw[b] (double)vec[vidx[b]][c]]), float64 accumulation in term
// order; an entry with no term and no vector takes row sid[b] as gather_speaker does.  One thread per (utterance, channel), g in
// gather_speaker's layout: one launch serves a batch that has both kinds
void speaker_blend(const float* emb_g, int spk_num, int gin, const int* sid, int B, const SpeakerMixTab& t, float* g, hipStream_t st);
// y =(((r0 + r1) + r2) + ...) / count  (ResBlock sum, /root/reference/src/models/Generator_hifigan.cpp:159-173)
void sum_scale(float* y, const float* const* r, int count, long n, hipStream_t st);
void flip_channels(float* x, long ld, int C, long n, float* tmp, hipStream_t st);

// SDP spline step: (r0, r1) -> (spline^-1(r1 | h), r0) ; h = [29][ld]
void spline_step(const float* h, long ld, float filter_sqrt, const float* r0, const float* r1,
                 float* o0, float* o1, long n, hipStream_t st);
// logw -> durations.  sdp: logw = (r0 - ea_m) * exp(-ea_logs) (ElementwiseAffine inverse) else logw = r0.
// dur[pos] = forced ? forced[pos] : (int)ceil(exp(logw) * ls[b]);  cum[pos] = inclusive prefix inside the
// utterance;  frames[b] = max(sum, 1).
// host_out (optional): host-MAPPED pinned memory (device pointer), laid out [flag][dur: total][frames: B] (the flag word is never used for data); every workgroup
// also writes its results there and the last one to finish publishes `seq` in the flag word -- the host learns the frame
// counts by polling that word instead of a device-to-host copy + stream synchronisation.  arrive: a zeroed device counter.
void durations(const float* r0, int sdp, float ea_m, float ea_logs, const float* ls, const int* forced,
               float* logw_out, int* dur, int* cum, int* frames, SegView seg, int B, hipStream_t st,
               int* host_out = nullptr, long total = 0, int seq = 0, unsigned* arrive = nullptr,
               int* len_out = nullptr, int* win_len_out = nullptr, int cap = 0);     // optional: frames[b] clamped to cap, into two device tables
// Duration plans (duration_plan.hip; the definition is there and in include/summertts_hip.h sts_set_duration_plan)
constexpr int kDurMax = 100000;             // == the durations kernel's clamp per phoneme
constexpr int kDurMaxTarget = 1 << 20;      // frames of a fitted utterance
// one utterance's plan: rate (or null) finite in [1/64, 64], fixed (or null) in [-1, kDurMax], target 0 or in [1, kDurMaxTarget] and feasible
bool dur_plan_valid(int n, const float* rate, const int32_t* fixed, int32_t target, const char** why);
// steps 3-4 of the definition on the host, for a plan dur_plan_valid accepted
void duration_fit(const float* w, const int32_t* fixed, int n, int32_t target, int32_t* out);
struct DurPlanArgs {
    const float* r0; int sdp; float ea_m, ea_logs; const float* ls;    // the duration predictor's output, as durations() takes it
    const float* w_in;                   // or the weights themselves (sts_duration_plan_apply): r0, ls and rate are then unused
    const float* rate; const int* fixed; // [total] each, or null
    const int* target;                   // [B]: 0 = no target
    int* forced;                         // out [total]: what durations() then takes as its forced durations
    float* dur_w;                        // out [total] or null: w (the "dur_w" tap)
    long long* rem;                      // scratch [total]
    SegView seg;
};
// one workgroup of 256 threads per utterance
void duration_plan(const DurPlanArgs& a, int B, hipStream_t st);
// z[c][offF[b] + f] = m[c][offT[b] + phoneme(f)]
// nz (optional; null or nz->logs null = the noise-free regulator): z_p = m_expand + eps * logs_expand * ns[b] (SynthesizerTrn.cpp:383),
// logs with m's geometry, per-utterance ns / seed tables on the device (noise.hpp)
struct PriorNoise { const float* logs; const float* ns; const uint64_t* seed; };
void expand_frames(const float* m, long m_ld, const int* cum, SegView segT, SegView segF, int C,
                   float* z, long z_ld, int B, int max_frames, hipStream_t st, const PriorNoise* nz = nullptr);
// the SDP latent of every utterance (flipped, scaled by nsw[b]) into the two rows the first reverse ConvFlow reads
void sdp_noise(SegView seg, int B, int max_len, const float* nsw, const uint64_t* seed, float* r0, float* r1, hipStream_t st);

// MB-iSTFT tail.  sb: subband conv output [nb*18 or 18][ld] with per-utterance frames = 16*len+1.
// spec: [bands*18][ld] (re, im per bin) ; tm: [bands][ld4] with per-utterance n = 4*(frames-1).
void istft_spectrum(const float* sb, long ld, int rows, float* spec, long total, hipStream_t st);
void istft_ola(const float* spec, long ld, int bands, int band_rows, SegView seg_frames, float* tm, long tm_ld,
               SegView seg_tm, int B, int max_n, hipStream_t st);
// polyphase synthesis FIR over the x4 zero-stuffed band signals: out[i] = sum_tau sum_b g*tm[b][(i+tau-pad)/4]*fir[tau*4+b]
void synth_fir(const float* tm, long tm_ld, SegView seg_tm, const float* fir, int ntap, int pad, float gain, float bias,
               float* wave, int16_t* pcm, SegView seg_out, int B, int max_n, hipStream_t st);
// istft_spectrum + istft_ola + synth_fir as one launch (4 bands + synthesis filter: the MBB / MS decoders); sb as for istft_spectrum
bool istft_tail_fused_ok(int bands, int ntap, int pad);
void istft_tail_fused(const float* sb, long ld, SegView seg_frames, const float* fir, int ntap, int pad, float gain, float bias, float* wave, int16_t* pcm,
                      SegView seg_out, int B, int max_n, hipStream_t st);
// pcm = (int16)(int32)(wave * 32737)   (SynthesizerTrn.cpp:389-396: truncation, wrap-around)
void quantize_pcm(const float* wave, int16_t* pcm, long n, hipStream_t st);

// Output sample-rate conversion (resample.hip; the filter is defined there and in include/summertts_hip.h sts_resample_table)
constexpr int kResampleMinRate = 8000, kResampleMaxRate = 48000, kResampleMaxP = 1024, kResampleMaxK = 72;
struct ResampleDesign { int P = 1, Q = 1, K = 0; };
// false: a rate outside [8000, 48000] or P > 1024
bool resample_design(int in_rate, int out_rate, ResampleDesign* d);
// the float32 table [P][2K] (host, float64 design)
void resample_table(const ResampleDesign& d, int in_rate, int out_rate, float* table);
struct ResampleArgs {
    const float* x; SegView seg;         // native float wave, windows in frames (scale = samples per frame)
    const float* table; int P, Q, K;
    int16_t* pcm; float* wave_out;       // outputs, packed utterance after utterance; wave_out optional (taps)
    // streaming (wtab != null): window w reads its row of the step's table (stream_step.hpp RsRow) -- the windows' chunks packed back to back
    const long long* wtab;
};
// grid: nwin windows x ceil(max_out / 1024) tiles; max_out = the most outputs one window emits
void resample_pcm(const ResampleArgs& a, int nwin, long long max_out, hipStream_t st);
// streaming at the native rate: window w's kept samples src[src_off[w] ..) -> dst[dst_off[w] .. dst_off[w + 1]) (one packed chunk
// buffer per step); max_n = the most samples one window keeps
void stream_pack(const int16_t* src, int16_t* dst, const int* src_off, const int* dst_off, int nwin, long long max_n, hipStream_t st);
// an open stream adopts the latents of an admission (live_stream.hip): B column segments of the channel-major src [C][ld_src] into
// dst [C][ld_dst], one launch.  tab (device): long long src_off[B] | long long dst_off[B] | int len[B]; segment b is columns
// [src_off[b], src_off[b] + len[b]) of every row of src, to [dst_off[b], ..) of dst.  max_len = the longest segment.  Nothing outside
// the destination ranges is written.
static inline size_t adopt_tab_bytes(int B) { return (size_t)B * 20; }
void adopt_z(const float* src, long long ld_src, float* dst, long long ld_dst, int C, const long long* tab, int B, int max_len, hipStream_t st);
// ... and the tables of an admission into a PLANNED open stream (live_stream.hip adopt_tables_kernel), one launch next to adopt_z: for
// newcomer b with the table row {slot, toff, n, poff, h} -- column b of g [gin][B] -> column slot of gpool [gin][max_live] (gpool null:
// the model has no conditioned decoder, nothing moves); n > 0: cum[toff .. + n) and q[toff .. + n) -> rows 0 and 1 of pool [2][ld_pool]
// at column poff, and the slot words [off | n | h][max_live] of `slot` = {poff, n, h}; n == 0 (it carries no gain plan): the words =
// {neutral, 1, 0}, the pool's shared neutral column.  slot < 0: nothing.  The table rides behind adopt_z's in the same upload, from the
// next 8-byte boundary (adopt_tables_tab_off).
struct AdoptTablesArgs {
    const float* g; float* gpool; int gin, B, max_live;
    const int* cum; const int* q;        // the admission's packed phoneme tables (q null when no newcomer carries a gain plan)
    int* pool; long long ld_pool;        // [2][ld_pool]: row 0 cum, row 1 q
    int* swords; int neutral;            // [3][max_live]; the column of the pool a plain slot's words name
    const int* tab;                      // device: int [B][5]
};
static inline size_t adopt_tables_tab_off(int B) { return (adopt_tab_bytes(B) + 7) & ~(size_t)7; }
static inline size_t adopt_tables_tab_bytes(int B) { return (size_t)B * 20; }
// max_n = the most phonemes one newcomer carries
void adopt_tables(const AdoptTablesArgs& a, int max_n, hipStream_t st);

// Loudness measurement and normalisation (loudness.hip; the definition is there and in include/summertts_hip.h sts_set_loudness)
constexpr int kLoudMinRate = 8000, kLoudMaxRate = 48000, kLoudPow = 9;
// K-weighting {b0, b1, b2, a1, a2} of the shelf, then of the high-pass, float64 (false: rate outside [8000, 48000])
bool kweight_coeffs(int rate, double c[10]);
// what the kernels need of a rate: the filter, S = samples per 100 ms sub-block, Mp[d] = M^(2^d) for the chunk map M = A^32 (row-major 4 x 4)
struct LoudCoef { double c[10]; double Mp[kLoudPow][16]; int S; };
bool loud_coef(int rate, LoudCoef* k);
struct LoudArgs {
    const float* x;                      // the float signal, utterances packed back to back
    const int* len; int ilen, scale, P, Q;   // utterance b has ceil(len[b] scale P / Q) samples (len == null: one utterance, ilen)
    float target, ceiling;               // T (LUFS) and C (dBFS)
    LoudCoef k;
    long long* utab; double* E; double* tsum; float* tpeak; float* gain;   // workspace (loud_ws_carve)
    float* out;                          // [B] sts_loudness {lufs, peak, gain, blocks} or null
    int no_clamp;                        // the limiter holds the ceiling: g = g_L (step 5 without its peak clamp)
};
// workspace of B utterances of total_samples samples in all (the frame-level arena's dry run sizes it)
size_t loud_ws_bytes(int B, long long total_samples);
void loud_ws_carve(LoudArgs& a, void* ws, int B, long long total_samples);
// 3 launches (4 with pcm: the gain cast pcm = pcm_cast(x g) into pcm, packed like x); max_len = the longest utterance's sample count or more
void loudness_run(const LoudArgs& a, int B, long long max_len, int16_t* pcm, hipStream_t st);
// streaming (loud_stream.hpp has the row, the state's layout and the result tables): window w reads its row from wtab[8 w ..] -- the
// utterance whose carried state it continues, its input window and the range it consumes.  state: [B][2] slots, read slot `slot`, written
// slot 1 - slot.  E: [nwin][tiles] end states of the step.  tsum / tpeak: the call's tables, every touched tile's entries are written.
struct LoudStreamArgs {
    const float* x;
    LoudCoef k;
    const long long* wtab; char* state; int slot;
    double* E; double* tsum; float* tpeak;
};
// one step: 2 launches over (max_tiles, nwin) workgroups; max_tiles = the most tiles one of its windows touches (lds_tiles)
void loud_stream_run(const LoudStreamArgs& a, int nwin, long long max_tiles, hipStream_t st);
// the gate alone (loud_gate_kernel, one launch) on result tables a stream filled: a.utab[3 b + 1] = the samples consumed,
// a.utab[3 b + 2] = the utterance's first tile, a.tsum / a.tpeak / a.gain / a.out / a.k / a.target / a.ceiling / a.no_clamp as in a whole call
void loud_gate_run(const LoudArgs& a, int B, hipStream_t st);

// Look-ahead peak limiter (limiter.hip; the definition is there and in include/summertts_hip.h sts_set_limiter)
constexpr int kLimMinRate = 8000, kLimMaxRate = 48000, kLimMaxH = 480;
// mode 0 or 1, gain in [-40, 40] dB, ceiling in [-30, 0] dBFS, look-ahead in [0.25, 10] ms (false for NaN)
bool limiter_args_valid(int mode, float gain_db, float ceiling_dbfs, float lookahead_ms);
// H = floor(ms rate / 1000 + 0.5), c = 10^(ceiling / 20), G = 10^(gain / 20), float64 (false: rate outside [8000, 48000] or a bad argument)
struct LimiterDesign { int H = 0; double c = 1.0, G = 1.0; };
bool limiter_design(int rate, float gain_db, float ceiling_dbfs, float lookahead_ms, LimiterDesign* d);
struct LimArgs {
    const float* x;                      // the float signal, utterances packed back to back (wtab: the windows of a streaming step)
    const int* len; int ilen, scale, P, Q;   // utterance b has ceil(len[b] scale P / Q) samples (len == null: one utterance, ilen)
    int H; double c, G;
    const float* gloud;                  // [B] loudness gain of each utterance (loud_gate_kernel's word), or null: 1
    float* y; int16_t* pcm;              // outputs packed like x, each optional (16-byte aligned)
    unsigned* stat;                      // [B][4] raw words {bits of g0, bits of 1.0f - bits of min s, bits of max |y|, limited} or null
    // streaming: segment w reads its row of the step's table (stream_step.hpp LimRow)
    const long long* wtab;
};
// one memset (stat) + one launch; max_out = the most outputs one utterance (segment) emits, or more
void limiter_run(const LimArgs& a, int B, long long max_out, hipStream_t st);

// Gain plans (gain_plan.hip; the definition is there and in include/summertts_hip.h sts_set_gain_plan)
constexpr int kGainOne = 1 << 20, kGainMaxH = 400;
// one utterance's plan: gain_db (or null) -INFINITY or finite in [-96, 24], ramp_ms finite in [0, 50] (false for NaN)
bool gain_plan_valid(int n, const float* gain_db, float ramp_ms, const char** why);
// step 1 of the definition on the host, for a plan gain_plan_valid accepted: q [n] and h, each optional
void gain_design(const float* gain_db, int n, float ramp_ms, int32_t* q, int32_t* h);
struct GainArgs {
    const float* x;                      // the native float wave: the members' samples as the decoder packs its windows
    float* y; int16_t* pcm;              // outputs packed like x, each optional (y 16-byte, pcm 8-byte aligned)
    SegView wseg;                        // member i's place in x, in frames (off == null: one member {ioff, ilen}); its scale is not read: hop is
    int hop;                             // samples per frame
    // streaming (null otherwise: member i is the whole utterance i): member i belongs to utterance utt[i] and its first sample is sample
    // u0 of row i of the resampler's table of the step (stream_step.hpp RsRow) -- word wcol of the wstride-word row i of wtab; wstride
    // 0 means the RsRow {5, 0}.  (A step through the pitch warp names its PsRow: there the RsRow describes the warped window.)
    const int* utt; const long long* wtab; int wstride, wcol;
    SegView tseg;                        // utterance b's phonemes in cum / q
    const int* cum;                      // inclusive cumulative frame counts inside each utterance (the durations kernel's)
    const int* q;                        // fixed-point gain per phoneme, packed like cum
    const int* h;                        // [utterances] half ramp width in samples, 0 .. kGainMaxH
};
// one launch: nmem members x ceil(max_len / 4096) tiles; max_len = the longest member's sample count or more
void gain_plan_run(const GainArgs& a, int nmem, long long max_len, hipStream_t st);

// Pitch plans (pitch_plan.hip; the definition is there and in include/summertts_hip.h sts_set_pitch_plan; the host arithmetic in
// pitch_layout.hpp)
double bessel_i0(double x);              // (resample.hip) modified Bessel function of the first kind, order 0, for x <= 10
// one utterance's plan: cents (or null) each in [-600, 600]
bool pitch_plan_valid(int n, const int32_t* cents, const char** why);
// the prototype h0: kPitchTableFloats floats (sts_pitch_table)
void pitch_table(float* table);
// The tables of one launch, built on the host from the final durations: words = [member B x {xoff, N, yoff, N', toff, rows} | o_i+1 |
// (a_i << 32) + e_i | step_i | c_i (double) | K_i], the five per-phoneme arrays TT long each and packed over the planned members only.
struct PitchTables { std::vector<long long> words; long long TT = 0, total_out = 0, max_out = 0; std::vector<long long> nout; };
// member b: n[b] phonemes with the durations dur[b] and the steps step[b] (null: no plan, the member is copied), its samples from xoff[b]
// on in x; the outputs are packed back to back in member order.  Null, or why the layout is refused
const char* pitch_tables(int B, const int32_t* n, const int32_t* const* dur, const int64_t* const* step, const long long* xoff, int hop,
                         PitchTables* t);
struct PitchArgs {
    const float* x;                      // the native float wave
    float* y; int16_t* pcm;              // the warped signals, packed back to back by the members' N', each optional
    const long long* mem;                // [members][6] (PitchTables::words on the device; pitch_args_carve sets these six)
    const long long *oend, *pos0, *step; const double* c; const long long* K;
    const float* table;                  // the prototype (device memory)
    // the range form only (pitch_range_run; null otherwise): one PsRow per window (pitch_stream.hpp), 10 words each.  x is then the
    // step's float wave and y / pcm the step's buffers; of mem only N, toff and rows are read
    const long long* rows;
};
void pitch_args_carve(PitchArgs& a, const long long* dev_words, int B, long long TT);
// one launch: nmem members x ceil(max_out / 256) tiles; max_out = the longest member's N' or more.  table_in_lds: every workgroup stages
// the prototype (64 KiB) in LDS instead of reading it from global memory
bool pitch_table_in_lds();              // the shipped choice (sts_debug_pitch_bench times both)
void pitch_plan_run(const PitchArgs& a, int nmem, long long max_out, bool table_in_lds, hipStream_t st);
// the range form, one launch: nwin windows x ceil(max_out / 256) tiles; max_out = the most outputs [yl0, yl1) one window emits or more.
// The prototype is read from global memory.  A sample is bit for bit the whole-utterance kernel's (one device function makes both)
void pitch_range_run(const PitchArgs& a, int nwin, long long max_out, hipStream_t st);

// Paragraph join (join.hip; the definition is there and in include/summertts_hip.h sts_infer_ids_joined)
constexpr int kJoinMaxFrames = 100000, kJoinMaxH = 800;
// every gap (null: all 0), lead and trail in [0, 100000] frames, fade_ms finite in [0, 50] (false for NaN), B >= 1
bool join_valid(int B, const sts_join* j, const char** why);
// step 1 of the definition: h = floor(fade_ms 16 + 0.5)
int join_design(float fade_ms);
// silence in front of sentence b, in frames: sil[b] = lead + gap_0 + .. + gap_{b-1}; returns lead + every gap + trail (64-bit: the
// caller bounds it).  j == null: all zeros
long long join_silence(int B, const sts_join* j, long long* sil);
struct JoinArgs {
    const float* x;                      // the native float waves of the B sentences, packed back to back in call order
    float* y; int16_t* pcm;              // the joined signal J [NJ] and its cast, each optional (y 16-byte, pcm 8-byte aligned)
    SegView wseg;                        // sentence b's place in x, in frames (off == null: one sentence {ioff, ilen}); off[b] = len[0] + .. + len[b - 1]
    const int* sil;                      // [B] silence frames in front of sentence b in J (join_silence); null: one sentence behind isil frames
    int isil;
    int B, hop, h;                       // sentences, samples per frame, fade length in samples (0 .. kJoinMaxH)
    long long NJ;                        // samples of J: (sum len + lead + every gap + trail) hop
};
// one launch: ceil(NJ / span) workgroups, each owning a contiguous span of J (silence included: no memset)
void join_run(const JoinArgs& a, hipStream_t st);
// The windowed join (a joined stream's step, sts_join_apply_range): the samples [g0, g1) of J from a step's decoded windows
struct JoinWinArgs {
    const float* x;                      // the step's decoded windows, packed compactly (16-byte aligned)
    float* y;                            // J[g0, g1) at y[i - g0], optional (16-byte aligned)
    int16_t* pcm;                        // the cast of the kept samples [k0, k1) at pcm[i - k0], optional (8-byte aligned)
    const long long* rows;               // [nw][5] = {st, en, S, N, xoff} (join_stream.hpp JsRow), ascending, device memory
    int nw, hop, h;                      // rows (0: only silence), samples per frame, fade length in samples
    long long g0, g1, k0, k1;            // samples of J; multiples of hop, g0 <= k0 <= k1 <= g1
};
// one launch: ceil((g1 - g0) / span) workgroups, each owning a contiguous span (silence included: no memset)
void join_window_run(const JoinWinArgs& a, hipStream_t st);

// Parametric equaliser (eq.hip; the definition is there and in include/summertts_hip.h sts_set_eq)
constexpr int kEqMinRate = 8000, kEqMaxRate = 48000, kEqMaxBands = STS_EQ_MAX_BANDS, kEqDim = 2 * kEqMaxBands, kEqPow = 9;
// the validity rules at an output rate (n_bands 0 is valid: the stage is off); why: the refusal's text, or null
bool eq_valid(int rate, int n_bands, const sts_eq_band* bands, const char** why);
// {b0, b1, b2, a1, a2} of every band, normalised by a0, float64 (bands eq_valid accepted)
void eq_design(int rate, int n_bands, const sts_eq_band* bands, double* coeffs);
// what the kernels read from device memory: the coefficients, and Mp[d] = M^(2^d) for the chunk map M = A^32 of the cascade's state
// (per section: last output, last output - the one before), row-major with stride kEqDim
struct EqTable { double c[kEqMaxBands][5]; double Mp[kEqPow][kEqDim * kEqDim]; };
void eq_table(int S, const double* coeffs, EqTable* t);
struct EqArgs {
    const float* x;                      // the float signal, utterances packed back to back
    const int* len; int ilen, scale, P, Q;   // utterance b has ceil(len[b] scale P / Q) samples (len == null: one utterance, ilen)
    int S; const EqTable* tab;           // sections (1 .. 4) and their tables (device memory)
    float* y; int16_t* pcm;              // outputs packed like x, each optional (not x)
    long long* utab; double* E;          // workspace (eq_ws_carve)
    // streaming (wtab != null; eq_stream.hpp has the row and the state's layout): window w reads its row from wtab[12 w ..] -- the
    // utterance whose carried state it continues, its input window, the range of y to produce into y[ybase ..), the kept range whose
    // int16 samples go to pcm[pdst ..).  state: [B][2] slots, read slot `slot`, written slot 1 - slot.  E: [nwin][tiles] end states
    const long long* wtab; char* state; int slot;
};
// workspace of B utterances of total_samples samples in all (the frame-level arena's dry run sizes it)
size_t eq_ws_bytes(int B, long long total_samples);
void eq_ws_carve(EqArgs& a, void* ws, int B, long long total_samples);
// 2 launches; max_len = the longest utterance's sample count or more
void eq_run(const EqArgs& a, int B, long long max_len, hipStream_t st);
// streaming: 2 launches over nwin windows x max_tiles tiles (eqs_tiles of the step's longest row, or more)
void eq_stream_run(const EqArgs& a, int nwin, long long max_tiles, hipStream_t st);

}  // namespace sts
