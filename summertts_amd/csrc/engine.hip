// engine.hip -- ids -> int16 PCM on one MI355X.  Restates the pipeline of
// /root/reference/src/models/SynthesizerTrn.cpp:357-400 for a BATCH of utterances packed along time:
//   TextEncoder -> duration predictor -> [one D2H of the frame counts] -> length regulator ->
//   reverse flow -> decoder -> int16.
// Everything runs on the engine's own HIP stream; the only host synchronisation inside a run is the
// data-dependent frame count F (SynthesizerTrn.cpp:376-381).  The decoder stage (run_decode) lives in decoder.hip.
#include "run_ctx.hpp"
#include "para_stream.hpp"
#include <time.h>
#include "knobs.hpp"
#include "../../include/tts_logger.h"

#include <algorithm>
#include <chrono>
#include <limits.h>
#include <math.h>
#include <new>
#include <stdlib.h>
#include <string.h>
#include <thread>

namespace sts {

// what an open stream fixed stays fixed, and the engine runs nothing else, until sts_stream_close (engine.hpp stream_open); an open
// paragraph likewise, until sts_para_close (engine.hpp para_open)
#define STS_NOT_WHILE_OPEN(what) \
    do { \
        if (live_) return fail(STS_ESTATE, "a stream is open on this engine (sts_stream_close first): it refuses " what); \
        if (para_) return fail(STS_ESTATE, "a paragraph is open on this engine (sts_para_close first): it refuses " what); \
    } while (0)
// ... the form of the four table setters (duration plan, speaker mix, gain plan, forced durations): a PLANNED open stream lets them
// through -- what they set applies to its next admission
#define STS_NOT_WHILE_OPEN_UNPLANNED(what) \
    do { \
        if (live_ && !live_->planned()) return fail(STS_ESTATE, "an unplanned stream is open on this engine (sts_stream_open_ex with capacity_phonemes > 0 admits tables): it refuses " what); \
        if (para_) return fail(STS_ESTATE, "a paragraph is open on this engine (sts_para_close first): it refuses " what); \
    } while (0)

Engine::~Engine() {
    if (live_) (void)stream_close();
    if (para_) (void)para_close();
    if (stream) (void)hipStreamSynchronize(stream);
    free_model(model);
    if (arenaT_.base) (void)hipFree(arenaT_.base);
    if (arenaF_.base) (void)hipFree(arenaF_.base);
    if (pinned_) (void)hipHostFree(pinned_);
    if (pinned_pcm_) (void)hipHostFree(pinned_pcm_);
    if (d_rs_table) (void)hipFree(d_rs_table);
    if (loud_host_) (void)hipHostFree(loud_host_);
    if (lim_host_) (void)hipHostFree(lim_host_);
    if (d_eq_) (void)hipFree(d_eq_);
    if (d_pitch_table_) (void)hipFree(d_pitch_table_);
    if (ovf_host_) (void)hipHostFree(ovf_host_);
    if (hmap_) (void)hipHostFree(hmap_);
    if (arrive_) (void)hipFree(arrive_);
    if (have_events_) {
        for (auto& e : ev_) (void)hipEventDestroy(e);
        (void)hipEventDestroy(ev_fork_);
        if (ev_setup_) (void)hipEventDestroy(ev_setup_);
        for (auto& e : ev_join_) (void)hipEventDestroy(e);
        for (auto& a : aux_) if (a) (void)hipStreamDestroy(a);
    }
    if (stream) (void)hipStreamDestroy(stream);
}

static int default_conv_math();
// one polite spin-wait step on whatever host this is built for (the x86 builtin alone broke aarch64 / ppc64 builds)
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__) || defined(__arm__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

int Engine::init(const float* blob, int64_t bytes, int dev) {
    conv_math = default_conv_math();
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(STS_EDEVICE, "no HIP device visible: the SummerTTS HIP engine needs an AMD GPU (gfx950) -- there is no CPU fallback");
    if (dev < 0 || dev >= count) return fail(STS_EINVAL, "device index out of range");
    device = dev;
    HIPCK(hipSetDevice(dev));
    HIPCK(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev_) HIPCK(hipEventCreate(&e));
    HIPCK(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&ev_setup_, hipEventDisableTiming));
    for (auto& e : ev_join_) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    {   // the chain with the largest kernel size (most FLOPs) is the critical path of a decoder stage:
        // give it the highest queue priority, the lightest chain the lowest
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo = least priority (numerically greatest)
        for (int k = 0; k < kAux; k++) {
            int pr = lo + (hi - lo) * k / (kAux > 1 ? kAux - 1 : 1);
            HIPCK(hipStreamCreateWithPriority(&aux_[k], hipStreamNonBlocking, pr));
        }
    }
    cur_ = stream;
    have_events_ = true;
    if (!blob || bytes < 32) return fail(STS_EMODEL, "model blob too small");
    if (!load_model(blob, bytes / (int64_t)sizeof(float), model)) return fail(STS_EMODEL, "model parse failed: " + model.error);
    return STS_OK;
}

bool Engine::ensure(Arena& a, size_t bytes) {
    if (bytes <= a.cap) return true;
    (void)hipStreamSynchronize(stream);
    if (a.base) (void)hipFree(a.base);
    a.base = nullptr; a.cap = 0;
    size_t want = bytes + bytes / 4 + (1u << 20);
    if (hipMalloc((void**)&a.base, want) != hipSuccess) { if (hipMalloc((void**)&a.base, bytes) != hipSuccess) return false; want = bytes; }
    a.cap = want;
    return true;
}

bool Engine::ensure_pinned(size_t bytes) {
    if (bytes <= pinned_cap_) return true;
    (void)hipStreamSynchronize(stream);
    if (pinned_) (void)hipHostFree(pinned_);
    pinned_ = nullptr; pinned_cap_ = 0;
    size_t want = bytes * 2 + 4096;
    if (hipHostMalloc((void**)&pinned_, want, hipHostMallocDefault) != hipSuccess) return false;
    pinned_cap_ = want;
    return true;
}

// STS_DBG_POISON (tests): no result may depend on what a buffer held before the call.  The arenas are filled right after each layout, before
// the call's first upload or kernel writes into them -- never between its stages or stream steps, which legitimately read what earlier
// ones wrote.  (The arena's capacity exceeds `used` by at least 4 KB: rounding up to whole words stays inside it.)
void Engine::poison_arena(const Arena& a) {
    if (!poison || !a.base || a.used == 0) return;
    const size_t words = (a.used + 3) / 4;
    if (hipMemsetD32Async((hipDeviceptr_t)a.base, (int)poison, words, stream) == hipSuccess) poison_bytes_ += (int64_t)words * 4;
}
void Engine::poison_host16(void* p, size_t samples) {
    if (!poison || !p) return;
    const uint16_t v = (uint16_t)(poison & 0xffffu);
    uint16_t* q = (uint16_t*)p;
    for (size_t i = 0; i < samples; i++) q[i] = v;
    poison_bytes_ += (int64_t)samples * 2;
}
void Engine::poison_host32(void* p, size_t words) {
    if (!poison || !p) return;
    uint32_t* q = (uint32_t*)p;
    for (size_t i = 0; i < words; i++) q[i] = poison;
    poison_bytes_ += (int64_t)words * 4;
}

void Engine::stage_begin(int s) { cur_stage_ = s; }
static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// profiling 1: all eight stage events; 2: only the two that bracket the decoder's matrix-core region (events 5 / 6) -- every event is a barrier
// packet between two kernels (5-10 us of bubble each, docs/HISTORY.md 12-4), so the headline step pays for two of them, not eight
void Engine::mark(int i) { if (profiling == 1 || (profiling == 2 && (i == 5 || i == 6))) (void)hipEventRecord(ev_[i], stream); }

// builds the kernel arguments of one conv and books its FLOPs / minimum HBM bytes
// default arithmetic of the trunk convs: STS_CONV_MATH = f16x2 (two fp16 terms, three products: the default) | bf16x3 (three bf16
// terms, six products) | f32 (the exact-fp32 MFMA instruction)          (conv_bf3.hip)
static int default_conv_math() {
    const char* v = getenv("STS_CONV_MATH");
    if (!v || !*v) return 3;
    if (!strcmp(v, "f16x2") || !strcmp(v, "3")) return 3;
    if (!strcmp(v, "bf16x3") || !strcmp(v, "0")) return 0;
    if (!strcmp(v, "f32") || !strcmp(v, "fp32") || !strcmp(v, "1")) return 1;
    // (a typo such as "bf16" used to select a default silently)
    tts_log(TTS_LOG_WARNING, (std::string("summertts_hip: STS_CONV_MATH=") + v + " is not one of f16x2 | bf16x3 | f32 -- ignored, the default (f16x2) applies\n").c_str());
    return 3;
}

ConvArgs Engine::conv_args(const DConv& c, const float* x, const Lvl& lin, float* y, const Lvl& lout, const ConvOpt& o, double* flops) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.x_ld = lin.ld; a.y = y; a.y_ld = lout.ld;
    a.w = c.w; a.wb3 = c.wb3; a.bias = c.bias; a.ubias = o.ubias; a.ubias_ld = lout.nb;
    if (conv_math == 3 && c.wh2) { a.wb3 = c.wh2; a.math = 1; a.wscale = c.h2_scale; a.ovf = ovf_; }     // "f16x2": the two-term fp16 copy
    a.res = o.res; a.res_ld = o.res_ld ? o.res_ld : lout.ld;
    a.aux = o.aux; a.aux_ld = o.aux_ld ? o.aux_ld : lout.ld;
    a.pcm = o.pcm;
    a.Cin = c.Cin; a.Cout = c.Cout; a.Cin_pad = c.Cin_pad; a.Cout_pad = c.Cout_pad;
    if (c.transposed) {
        a.ntap = c.J; a.tap_step = -1; a.tap_off = 0; a.out_stride = c.stride; a.out_off = -c.pad;
        a.transposed = 1; a.n_extra = c.J - 1; a.max_n = lin.max_len + c.J - 1;
    } else {
        a.ntap = c.k; a.tap_step = c.dil; a.tap_off = -(o.pad_l >= 0 ? o.pad_l : c.pad); a.out_stride = 1; a.out_off = 0;
        a.max_n = lout.max_len;
    }
    a.depthwise = c.depthwise;
    a.in_act = o.in_act; a.in_slope = o.slope; a.in_reflect = o.reflect;
    a.epi = o.epi; a.epi_flag = o.epi_flag; a.epi_scale = o.epi_scale; a.H = c.H; a.gate_perm = c.gate_perm;
    a.in_seg = lin.seg; a.out_seg = lout.seg; a.B = lout.nb;
    a.kslices = o.kslices; a.kslice_stride = o.kslice_stride;
    if (o.nsum >= 2) { a.xs1 = o.sum1; a.xs2 = o.sum2; a.nsum = o.nsum; }
    const double positions = c.transposed ? (double)lin.total : (double)lout.total;
    const double fl = 2.0 * c.macs_per_out * positions;
    flops_[cur_stage_] += fl;
    {   // algorithmic HBM bytes: input once, output once, weights once (+ residual / read-modify-write operands)
        const size_t wfl = c.depthwise ? (size_t)c.k * c.Cout : (size_t)c.k * c.Cin * c.Cout;
        double by = 4.0 * ((double)c.Cin * lin.total + (double)c.Cout * lout.total);
        if (o.res || o.epi == EPI_SUB || o.epi == EPI_RESSKIP) by += 4.0 * (double)c.Cout * lout.total;
        bytes_[cur_stage_] += by;                         // (scales with the positions)
        bytes_w_[cur_stage_] += 4.0 * (double)wfl;        // (does not)
    }
    if (flops) *flops = fl;
    return a;
}

void Engine::conv(const DConv& c, const float* x, const Lvl& lin, float* y, const Lvl& lout, const ConvOpt& o) {
    double fl = 0;
    ConvArgs a = conv_args(c, x, lin, y, lout, o, &fl);
    const bool can_mfma = conv_mode != 1 && conv_mfma_eligible(a);
    // split-bf16 arithmetic: the decoder trunk always; other matrix-core convs (flow, text encoder, conv_pre) from the grid size on
    // at which they stop being launch-latency-bound (a batch of a few dozen utterances); conv_math 2 = wherever eligible (tests)
    const bool use_bf3 = conv_mode == 0 && conv_math != 1 && o.tile < 0 && conv_bf3_eligible(a) &&
                         (in_mfma_region_ || conv_math == 2 || conv_bf3_blocks(a) >= 384);
    if (use_bf3 && c.transposed && ups_rowph && a.epi == EPI_STORE && !a.ubias && (a.math == 1 ? c.wh2r : c.wb3r)) {
        // upsamplers: the copy whose rows interleave the phases (rho = cout * stride + phase) -- same sums in the same order, whole-sector stores
        a.wb3 = a.math == 1 ? c.wh2r : c.wb3r;
        a.bias = c.bias ? c.bias_r : nullptr;
        a.Cout = a.Cout_pad = c.Cout_pad * c.stride;
        a.rowph = c.stride;
    }
    if (a.nsum >= 2 && !(use_bf3 ? conv_bf3_takes_sum(a) : (!can_mfma && conv_cout1_takes(a)))) {
        // this conv's kernel cannot form the mean of its input terms while staging: one launch materialises it (the round-3 form)
        const float* r[3] = {x, o.sum1, o.sum2};
        sum_scale(o.sum_dst, r, a.nsum, o.sum_n, cur_);
        a.x = o.sum_dst; a.xs1 = a.xs2 = nullptr; a.nsum = 0;
    }
    if (use_bf3) {
        if (in_mfma_region_) { mfma_flops_ += fl; bf16_exec_ += products() * fl; mfma_launches_++; }
        static const int bt = exp_int("STS_BF3_TILE", -1);   // experiment knob
        conv_bf3(a, cur_, bt);
    } else if (can_mfma) {
        if (in_mfma_region_) { mfma_flops_ += fl; mfma_exec_ += fl; mfma_launches_++; }
        conv_mfma(a, cur_, o.tile >= 0 ? o.tile : (conv_mode >= 2 ? conv_mode - 2 : -1));
    } else {
        // the generic kernel knows nothing of cross-workgroup K slices: it writes the complete sum into slice 0, so the
        // consumer's other partial operands must read as zero
        if (a.kslices > 1 && a.kslice_stride > 0)
            (void)hipMemsetAsync(a.y + a.kslice_stride, 0, (size_t)(a.kslices - 1) * (size_t)a.kslice_stride * sizeof(float), cur_);
        conv_generic(a, cur_);
    }
}

// Cross-workgroup K split for a conv whose output has too few tiles to fill the chip while its K loop is long (text-encoder
// FFN second conv at batch 1: 24 tiles x K = 2304): slices are sized so that about one workgroup per CU results and
// every slice keeps >= 24 groups of 8 input channels.  1 = no split.
int Engine::pick_kslices(const DConv& c, const Lvl& lout) const {
    if (conv_mode != 0 || c.depthwise || c.transposed || c.Cin < 32) return 1;
    const long tiles = (long)((lout.max_len + 31) / 32) * (c.Cout_pad / 32) * lout.nb;
    const long groups = (long)c.k * (c.Cin_pad / 8);
    int s = 1;
    while (s < 8 && tiles * (s * 2) <= 256 && groups / (s * 2) >= 24) s *= 2;
    return s;
}

void Engine::ln(const DLn& l, const float* a, const float* b, const float* res, float* y, const Lvl& lv, int pre_relu, int post_gelu, int nb, long b_stride) {
    LnArgs g;
    memset(&g, 0, sizeof(g));
    g.a = a; g.a_ld = lv.ld; g.b = b; g.b_ld = lv.ld; g.res = res; g.res_ld = lv.ld; g.y = y; g.y_ld = lv.ld;
    g.nb = nb; g.b_stride = b_stride;
    g.gamma = l.g; g.beta = l.b; g.C = l.C; g.pre_relu = pre_relu; g.post_gelu = post_gelu;
    g.seg = lv.seg; g.B = lv.nb; g.max_len = lv.max_len;
    bytes_[cur_stage_] += 4.0 * (double)l.C * (double)lv.total * (2.0 + (b ? 1.0 : 0.0) + (res ? 1.0 : 0.0));
    layer_norm(g, cur_);
}

// /root/reference/src/modules/DDSConv.cpp:84-111: x += gelu(LN2(conv1x1(gelu(LN1(dwconv(x))))))
// Returns the buffer that holds the result (h or t1: the fused layers ping-pong between them).
// `pre` (optional): the ConvFlow's 1 -> C input conv, h = (pre(pre_in) + pre_res) (/root/reference/src/modules/ConvFlow.cpp:252-254;
// pre_in == null: the all-zero latent).  Where the first layer runs fused, h is never materialised: the kernel evaluates it at its
// depthwise taps; otherwise the conv runs first, into `h`.
float* Engine::dds(const DDds& d, float* h, float* t1, float* t2, const Lvl& lv, const DConv* pre, const float* pre_in, const float* pre_res,
                   const SplineTail* tail, bool* tail_done) {
    if (tail_done) *tail_done = false;
    static const bool no_col = exp_flag("STS_NO_COL_LAYER");   // experiment knob
    float* cur = h;
    bool pre_pending = pre != nullptr;
    auto run_pre = [&]() {      // the unfused form of the input conv (zero input: a memset feeds it)
        if (!pre_pending) return;
        pre_pending = false;
        const float* in = pre_in;
        if (!in) { (void)hipMemsetAsync(t2, 0, (size_t)lv.total * sizeof(float), cur_); in = t2; }
        ConvOpt oa; oa.epi = EPI_RESADD; oa.res = pre_res;
        conv(*pre, in, lv, h, lv, oa);
    };
    for (int i = 0; i < d.n; i++) {
        const DConv& c = d.sep[i];
        const DConv& pw = d.pw[i];
        if (!no_col && conv_mode != 1 && !pw.depthwise && pw.k == 1 && pw.Cin == pw.Cout && pw.Cin == d.n1[i].C && pw.Cin == d.n2[i].C &&
            pw.Cin_pad == pw.Cin) {
            // the whole layer as ONE launch (col_layer.hip); output goes to the other buffer: neighbouring workgroups still
            // read `cur` through the dilated depthwise taps
            ColLayerArgs g;
            float* nxt = cur == h ? t1 : h;
            fill_col_dds(c, d.n1[i], pw, d.n2[i], cur, nxt, lv, g);
            if (pre_pending && i == 0 && pre->Cin == 1 && pre->k == 1 && pre->Cout == pw.Cin && !pre->depthwise && pre_res) {
                // fold h = (w r + b) + g into the layer: x = res = g, rank-1 term from the conv's single input row
                fill_col_pre(*pre, pre_in, pre_res, g);
                if (col_layer_eligible(g)) {
                    pre_pending = false;
                    flops_[cur_stage_] += 2.0 * pre->macs_per_out * (double)lv.total;
                } else { g.x = cur; g.res = cur; g.xs_w = g.xs_b = g.xr = nullptr; }
            }
            run_pre();
            if (tail && tail_done && dds_tail && i == d.n - 1 && tail->proj && tail->proj->k == 1 && !tail->proj->depthwise && tail->proj->Cout == 29 &&
                tail->proj->Cout_pad == 32 && tail->proj->Cin == pw.Cin && tail->proj->Cin_pad == pw.Cin && tail->proj->w && tail->proj->bias) {
                // the layer's output feeds only the projection: both and the spline step in this launch
                ColLayerArgs gt = g;
                fill_col_tail(*tail->proj, tail->filter_sqrt, tail->r0, tail->r1, tail->o0, tail->o1, gt);
                if (col_layer_eligible(gt)) {
                    flops_[cur_stage_] += 2.0 * (c.macs_per_out + pw.macs_per_out + tail->proj->macs_per_out) * (double)lv.total;
                    bytes_[cur_stage_] += 4.0 * ((double)pw.Cin * lv.total + (double)pw.Cin * pw.Cout + (double)pw.Cin * 32 + 4.0 * lv.total);
                    col_layer(gt, cur_);
                    *tail_done = true;
                    return nxt;                 // (not written: the caller ignores it when the tail ran)
                }
            }
            if (col_layer_eligible(g)) {
                flops_[cur_stage_] += 2.0 * (c.macs_per_out + pw.macs_per_out) * (double)lv.total;
                bytes_[cur_stage_] += 4.0 * ((double)pw.Cin * lv.total * 2.0 + (double)pw.Cin * pw.Cout);
                col_layer(g, cur_);
                cur = nxt;
                continue;
            }
        }
        run_pre();
        {   // depthwise conv fused into the LayerNorm that consumes it (one launch instead of two)
            LnArgs g;
            memset(&g, 0, sizeof(g));
            g.a = cur; g.a_ld = lv.ld; g.y = t2; g.y_ld = lv.ld;
            g.gamma = d.n1[i].g; g.beta = d.n1[i].b; g.C = d.n1[i].C; g.post_gelu = 1;
            g.dw_w = c.w; g.dw_b = c.bias; g.dw_k = c.k; g.dw_dil = c.dil; g.dw_pad = c.pad; g.dw_ld = c.Cout_pad;
            g.seg = lv.seg; g.B = lv.nb; g.max_len = lv.max_len;
            flops_[cur_stage_] += 2.0 * c.macs_per_out * (double)lv.total;
            bytes_[cur_stage_] += 4.0 * (double)g.C * (double)lv.total * 2.0;
            layer_norm(g, cur_);
        }
        float* other = cur == h ? t1 : h;       // conv output; `cur` stays the residual and is updated in place
        conv(pw, t2, lv, other, lv, ConvOpt());
        ln(d.n2[i], other, nullptr, cur, cur, lv, 0, 1);
    }
    return cur;
}

void Engine::tap(const char* name, const float* d, int channels, long ld, long length) {
    if (!record_taps) return;
    Tap& t = taps[name];
    t.channels = channels; t.length = length;
    t.data.resize((size_t)channels * length);
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy2D(t.data.data(), (size_t)length * sizeof(float), d, (size_t)ld * sizeof(float),
                      (size_t)length * sizeof(float), (size_t)channels, hipMemcpyDeviceToHost);
}

// sts_set_output_rate: the filter's table is built on the host and uploaded once here, not per call.  An invalid rate changes nothing.
int Engine::set_output_rate(int rate) {
    STS_NOT_WHILE_OPEN("the output rate");
    if (rate == 0) rate = kNativeRate;
    ResampleDesign d;
    if (rate != kNativeRate && !resample_design(kNativeRate, rate, &d)) return fail(STS_EINVAL, "output rate must be 0 or an integer in [8000, 48000] with P = rate / gcd(16000, rate) <= 1024");
    if (rate == out_rate) return STS_OK;
    if (rate == kNativeRate) { out_rate = rate; rs = ResampleDesign(); return STS_OK; }   // (the table stays allocated for a later rate)
    std::vector<float> h((size_t)d.P * 2 * d.K);
    resample_table(d, kNativeRate, rate, h.data());
    HIPCK(hipSetDevice(device));
    if (stream) HIPCK(hipStreamSynchronize(stream));
    float* t = nullptr;        // (the old table stays in place until the new one is on the device)
    HIPCK(hipMalloc((void**)&t, h.size() * sizeof(float)));
    if (hipMemcpy(t, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(t); return fail(STS_EDEVICE, "resampler table upload failed"); }
    if (d_rs_table) (void)hipFree(d_rs_table);
    d_rs_table = t; out_rate = rate; rs = d;
    return STS_OK;
}
// sts_set_loudness: persists; an invalid argument changes nothing
int Engine::set_loudness(int mode, float target, float peak) {
    STS_NOT_WHILE_OPEN("the loudness setting");
    if (!loudness_args_valid(mode, target, peak))
        return fail(STS_EINVAL, "loudness: mode 0 (off), 1 (measure) or 2 (normalize), target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS");
    loud_mode = mode; loud_target = target; loud_peak = peak;
    return STS_OK;
}
// sts_set_limiter: persists; an invalid argument changes nothing
int Engine::set_limiter(int mode, float gain_db, float ceiling_dbfs, float lookahead_ms) {
    STS_NOT_WHILE_OPEN("the limiter setting");
    if (!limiter_args_valid(mode, gain_db, ceiling_dbfs, lookahead_ms))
        return fail(STS_EINVAL, "limiter: mode 0 (off) or 1 (on), gain in [-40, 40] dB, ceiling in [-30, 0] dBFS, look-ahead in [0.25, 10] ms");
    lim_mode = mode; lim_gain_db = gain_db; lim_ceiling = ceiling_dbfs; lim_ms = lookahead_ms;
    return STS_OK;
}
// sts_set_eq: persists; checked against the current output rate; an invalid argument changes nothing
int Engine::set_eq(int n_bands, const sts_eq_band* bands) {
    STS_NOT_WHILE_OPEN("the equaliser");
    const char* why = nullptr;
    if (!eq_valid(out_rate, n_bands, bands, &why)) return fail(STS_EINVAL, why);
    eq_n = n_bands;
    for (int i = 0; i < n_bands; i++) eq_bands[i] = bands[i];
    eq_dirty_ = true;
    return STS_OK;
}
// a run with an EQ, before anything is enqueued: the bands must fit the rate of THIS run; new bands or a new rate: tables to the device
int Engine::eq_prepare() {
    const char* why = nullptr;
    if (!eq_valid(out_rate, eq_n, eq_bands, &why)) return fail(STS_EINVAL, std::string(why) + " -- the equaliser no longer fits the output rate (sts_set_eq again)");
    if (!eq_dirty_ && eq_tab_rate_ == out_rate && d_eq_) return STS_OK;
    double coef[5 * STS_EQ_MAX_BANDS];
    eq_design(out_rate, eq_n, eq_bands, coef);
    EqTable t;
    eq_table(eq_n, coef, &t);
    if (stream) HIPCK(hipStreamSynchronize(stream));      // (no earlier run still reads the old tables)
    if (!d_eq_) HIPCK(hipMalloc((void**)&d_eq_, sizeof(EqTable)));
    HIPCK(hipMemcpy(d_eq_, &t, sizeof(EqTable), hipMemcpyHostToDevice));
    eq_dirty_ = false; eq_tab_rate_ = out_rate;
    return STS_OK;
}
// sts_set_forced_durations: null or count <= 0 drops pending ones
void Engine::set_forced_durations(const int32_t* dur, int64_t count) {
    pend.have_forced = dur && count > 0;
    if (pend.have_forced) pend.forced_dur.assign(dur, dur + count);
}
// What the four table setters share: B == 0 or no table drops the pending one (`have`), B < 0 (or no n where the kind has phoneme
// counts, with_n) and B > max_B (message `over`, or the B >= 0 one) are refused, valid(b, &why) is asked per utterance, and a kind with
// phoneme counts may have 2^24 in all (*total).  False: *rc is the setter's answer and nothing else has changed
template <typename Valid>
bool Engine::table_begin(const char* what, bool given, bool& have, int B, const int32_t* n, bool with_n, int max_B, const char* over, long* total, int* rc,
                         Valid&& valid) {
    *rc = STS_OK;
    if (B == 0 || !given) { have = false; return false; }
    const std::string required = std::string(what) + (with_n ? ": B >= 0 and n are required" : ": B >= 0 is required");
    if (B < 0 || (with_n && !n)) { *rc = fail(STS_EINVAL, required); return false; }
    if (B > max_B) { *rc = fail(STS_EINVAL, over ? over : required); return false; }
    *total = 0;
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (!valid(b, &why)) { *rc = fail(STS_EINVAL, why); return false; }
        if (with_n && (*total += n[b]) > (1 << 24)) { *rc = fail(STS_EINVAL, "batch too large"); return false; }
    }
    return true;
}
// sts_set_duration_plan: copied as the flattened rate / fixed / target of the whole batch
int Engine::set_duration_plan(int B, const int32_t* n, const sts_dur_plan* plans) {
    STS_NOT_WHILE_OPEN_UNPLANNED("a duration plan");
    PendingTables& t = pend; long total = 0; int rc;
    if (!table_begin("duration plan", plans, t.have_plan, B, n, true, INT_MAX, nullptr, &total, &rc, [&](int b, const char** why) {
            return dur_plan_valid(n[b], plans[b].rate, plans[b].fixed, plans[b].target_frames, why); })) return rc;
    t.plan_n.assign(n, n + B);
    t.plan_rate.assign((size_t)total, 1.0f); t.plan_fixed.assign((size_t)total, -1); t.plan_target.assign((size_t)B, 0);
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        if (plans[b].rate) std::copy(plans[b].rate, plans[b].rate + n[b], t.plan_rate.begin() + (long)off);
        if (plans[b].fixed) std::copy(plans[b].fixed, plans[b].fixed + n[b], t.plan_fixed.begin() + (long)off);
        t.plan_target[b] = plans[b].target_frames;
        off += (size_t)n[b];
    }
    t.have_plan = true;
    return STS_OK;
}
// sts_set_speaker_mix: flattened into the term table the run uploads
int Engine::set_speaker_mix(int B, const sts_speaker_mix* mixes) {
    STS_NOT_WHILE_OPEN_UNPLANNED("a speaker mix");
    PendingTables& t = pend; long total = 0; int rc;
    if (!table_begin("speaker mix", mixes, t.have_mix, B, nullptr, false, 1 << 20, nullptr, &total, &rc, [&](int b, const char** why) {
            return speaker_mix_valid(model.is_ms == 1 ? model.spk_num : 0, model.gin, mixes[b], why); })) return rc;
    speaker_mix_flatten(mixes, B, model.gin, t.mix_words, &t.mix_K);
    t.mix_B = B;
    t.have_mix = true;
    return STS_OK;
}
// sts_set_gain_plan: designed here (q per phoneme, h per utterance)
int Engine::set_gain_plan(int B, const int32_t* n, const sts_gain_plan* plans) {
    STS_NOT_WHILE_OPEN_UNPLANNED("a gain plan");
    PendingTables& t = pend; long total = 0; int rc;
    if (!table_begin("gain plan", plans, t.have_gain, B, n, true, INT_MAX, nullptr, &total, &rc, [&](int b, const char** why) {
            return gain_plan_valid(n[b], plans[b].gain_db, plans[b].ramp_ms, why); })) return rc;
    t.gain_n.assign(n, n + B);
    t.gain_words.assign((size_t)total + (size_t)B, 0);
    t.gain_has.assign((size_t)B, 0);
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        t.gain_has[(size_t)b] = plans[b].gain_db != nullptr;
        gain_design(plans[b].gain_db, n[b], plans[b].ramp_ms, t.gain_words.data() + off, t.gain_words.data() + total + b);
        off += (size_t)n[b];
    }
    t.have_gain = true;
    return STS_OK;
}
// sts_set_pitch_plan: the cents of the whole batch, copied (one grid row per utterance: at most 65535)
int Engine::set_pitch_plan(int B, const int32_t* n, const sts_pitch_plan* plans) {
    STS_NOT_WHILE_OPEN_UNPLANNED("a pitch plan");      // (a planned open stream lets the setter through; its admission then refuses the plan)
    PendingTables& t = pend; long total = 0; int rc;
    if (!table_begin("pitch plan", plans, t.have_pitch, B, n, true, 65535, "pitch plan: at most 65535 utterances", &total, &rc, [&](int b, const char** why) {
            return pitch_plan_valid(n[b], plans[b].cents, why); })) return rc;
    t.pitch_n.assign(n, n + B);
    t.pitch_cents.assign((size_t)total, 0);
    t.pitch_has.assign((size_t)B, 0);
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        t.pitch_has[(size_t)b] = plans[b].cents != nullptr;
        if (plans[b].cents) std::copy(plans[b].cents, plans[b].cents + n[b], t.pitch_cents.begin() + (long)off);
        off += (size_t)n[b];
    }
    t.have_pitch = true;
    return STS_OK;
}
// The tables of nb utterances on `eng` (engine.hpp): per kind, the members' views in one array, through the kind's setter
int apply_utt_tables(Engine& eng, int nb, const int32_t* n, const UttTables* const* members, int kinds) {
    if (kinds < 0) {
        kinds = 0;
        for (int i = 0; i < nb; i++)
            kinds |= (members[i]->has_duration() ? kTabDuration : 0) | (members[i]->has_mix() ? kTabMix : 0) | (members[i]->has_gain() ? kTabGain : 0) |
                     (members[i]->has_pitch() ? kTabPitch : 0);
    }
    int rc = STS_OK;
    if (kinds & kTabDuration) {
        std::vector<sts_dur_plan> v((size_t)nb);
        for (int i = 0; i < nb; i++) v[(size_t)i] = members[i]->view_duration();
        rc = eng.set_duration_plan(nb, n, v.data());
    }
    if (rc == STS_OK && (kinds & kTabMix)) {
        std::vector<sts_speaker_mix> v((size_t)nb);
        for (int i = 0; i < nb; i++) v[(size_t)i] = members[i]->view_mix();
        rc = eng.set_speaker_mix(nb, v.data());
    }
    if (rc == STS_OK && (kinds & kTabGain)) {
        std::vector<sts_gain_plan> v((size_t)nb);
        for (int i = 0; i < nb; i++) v[(size_t)i] = members[i]->view_gain();
        rc = eng.set_gain_plan(nb, n, v.data());
    }
    if (rc == STS_OK && (kinds & kTabPitch)) {
        std::vector<sts_pitch_plan> v((size_t)nb);
        for (int i = 0; i < nb; i++) v[(size_t)i] = members[i]->view_pitch();
        rc = eng.set_pitch_plan(nb, n, v.data());
    }
    if (rc != STS_OK) eng.drop_tables();
    return rc;
}
// sts_get_speaker_embedding: row sid of the device-resident table (one strided copy of gin floats)
int Engine::speaker_embedding(int sid, float* out, int64_t capacity) const {
    if (!out) return STS_EINVAL;
    if (model.is_ms != 1 || !model.emb_g || sid < 0 || sid >= model.spk_num || capacity < model.gin) return STS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return STS_EDEVICE;
    if (hipMemcpy2D(out, sizeof(float), model.emb_g + sid, (size_t)model.spk_num * sizeof(float), sizeof(float), (size_t)model.gin,
                    hipMemcpyDeviceToHost) != hipSuccess) return STS_EDEVICE;
    return STS_OK;
}
// sts_get_phoneme_offsets: host arithmetic on the durations the last run downloaded -- phoneme i with f frames before it in its utterance
// starts at output sample ceil(f hop P / Q) (f hop at the native rate), the convention of a streaming chunk's sample_offset
int Engine::phoneme_offsets(int64_t* start, int64_t capacity) {
    if (!start) return fail(STS_EINVAL, "null argument");
    if ((int64_t)durations_h.size() > capacity) return fail(STS_ESTATE, "destination too small");
    if (last_pitch_start.size() == durations_h.size() && !durations_h.empty()) {      // (a run with a pitch plan: positions in the warped signal)
        for (size_t k = 0; k < durations_h.size(); k++) start[k] = out_count(last_pitch_start[k]);
        return STS_OK;
    }
    size_t i = 0;
    const bool joined = last_join_start.size() == last_n.size() && !last_n.empty();      // (a joined run: positions in the joined output)
    for (size_t b = 0; b < last_n.size(); b++) {
        long long f = 0;
        const long long base = joined ? last_join_start[b] : 0;
        for (int t = 0; t < last_n[b] && i < durations_h.size(); t++, i++) { start[i] = out_count(base + f * model.hop_total); f += durations_h[i]; }
    }
    return STS_OK;
}
// sts_get_join_offsets: the sentence starts of the last (joined) run in output samples, ceil(start_b P / Q)
int Engine::join_offsets(int64_t* start, int64_t capacity) {
    if (!start) return fail(STS_EINVAL, "null argument");
    if (last_join_start.empty()) return fail(STS_ESTATE, "the last call was not a joined one");
    if ((int64_t)last_join_start.size() > capacity) return fail(STS_EINVAL, "capacity below the last call's sentence count");
    for (size_t b = 0; b < last_join_start.size(); b++) start[b] = out_count(last_join_start[b]);
    return STS_OK;
}
// sts_infer_ids_joined: the join is validated and laid out here (silence frames in front of each sentence, h); an invalid join changes
// nothing.  The run itself is run()'s, with join_on set: run_setup uploads the table, decode_end launches the join kernel (a stream:
// run_stream_steps launches the windowed one per step)
int Engine::run_joined(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const sts_join* join, const StreamSpec* ss) {
    STS_NOT_WHILE_OPEN("a joined run");
    if (refuse_pitch("a joined run")) { drop_tables(); return STS_EINVAL; }
    const char* why = nullptr;
    if (!join_valid(B, join, &why)) return fail(STS_EINVAL, why);
    if (!ids || !n) return fail(STS_EINVAL, "empty batch");
    std::vector<long long> sil((size_t)B);
    join_total_sil = join_silence(B, join, sil.data());
    if (join_total_sil * model.hop_total > 2000000000LL) return fail(STS_EINVAL, "the joined signal is too long for one call (N_J <= 2 10^9 native samples)");
    join_sil.resize((size_t)B);
    for (int b = 0; b < B; b++) join_sil[b] = (int32_t)sil[b];
    join_h = join ? join_design(join->fade_ms) : 0;
    join_on = true;
    const int rc = run(B, ids, n, sid, ls, ss);
    join_on = false;
    return rc;
}
int Engine::stream_halo(bool warped) const {
    const int h = decoder_halo_frames(model);
    // the limiter reads the float signal 2H output samples beyond a chunk's edges: 2H Q / P native samples (+ 1 for the rounding of the
    // chunk's first output position), on top of the resampler's K
    long long extra = resampling() ? rs.K : 0;
    if (lim_mode != 0) {
        LimiterDesign d;
        if (limiter_design(out_rate, lim_gain_db, lim_ceiling, lim_ms, &d)) {
            const long long P = resampling() ? rs.P : 1, Q = resampling() ? rs.Q : 1;
            extra += (2LL * d.H * Q + P - 1) / P + 1;
        }
    }
    // (a stream through the pitch warp: extra is in warped samples, the warp's taps reach kPitchMaxK further -- pitch_stream.hpp)
    if (warped) return (int)pitch_stream_halo(h, extra, model.hop_total);
    return h + (int)((extra + model.hop_total - 1) / model.hop_total);
}

// ---- stage 0: batch geometry at the phoneme level, phoneme-level workspace, the one host-to-device copy of a run
int Engine::run_setup(RunCtx& c) {
    Model& M = model;
    const int B = c.B; const int32_t* const* ids = c.ids; const int32_t* n = c.n; const int32_t* sid = c.sid; const float* ls = c.ls;
    // ---------------- host-side batch geometry (phoneme level)
    std::vector<int>& offT = c.offT; std::vector<int>& lenT = c.lenT;
    offT.assign(B, 0); lenT.assign(B, 0);
    long& Ttot = c.Ttot; int& maxT = c.maxT;
    Ttot = 0; maxT = 0;
    for (int b = 0; b < B; b++) {
        if (n[b] <= 0 || !ids[b]) return fail(STS_EINVAL, "utterance with no phonemes");
        for (int i = 0; i < n[b]; i++)
            if (ids[b][i] < 0 || ids[b][i] >= M.vocab) return fail(STS_EINVAL, "phoneme id outside the model vocabulary");
        offT[b] = (int)Ttot; lenT[b] = n[b]; Ttot += n[b]; if (n[b] > maxT) maxT = n[b];
    }
    if (Ttot > (1 << 24)) return fail(STS_EINVAL, "batch too large");
    if ((size_t)(M.hidden / 2 + 8 + 5 * (size_t)maxT) * 4 > 150 * 1024) return fail(STS_EINVAL, "utterance too long for the attention kernel");
    if (pend.have_plan && pend.have_forced) { pend.have_forced = false; pend.have_plan = false; return fail(STS_EINVAL, "a duration plan and forced durations are both pending: both are dropped"); }
    if (pend.have_forced && (long)pend.forced_dur.size() != Ttot) { pend.have_forced = false; return fail(STS_EINVAL, "forced durations do not match the batch"); }
    // (a table these checks refuse: run() drops it)
    if (pend.have_plan && !table_matches(pend.plan_n, B, n)) return fail(STS_EINVAL, other_batch_message("duration plan"));
    if (pend.have_mix && pend.mix_B != B) return fail(STS_EINVAL, other_batch_message("speaker mix", false));
    if (pend.have_gain && !table_matches(pend.gain_n, B, n)) return fail(STS_EINVAL, other_batch_message("gain plan"));
    std::vector<float> eff_rate; std::vector<int32_t> eff_fixed, eff_target;
    const float* src_rate = pend.plan_rate.data(); const int32_t* src_fixed = pend.plan_fixed.data(); const int32_t* src_target = pend.plan_target.data();
    // a pitch plan: whole-utterance calls only; the run's duration plan is the pending one (or the neutral one) with every rate multiplied
    // by the phoneme's ratio -- one fp32 multiply here; the plan kernel is the one of any planned run.  Forced durations are used as given
    if (pend.have_pitch) {
        if (!table_matches(pend.pitch_n, B, n)) return fail(STS_EINVAL, other_batch_message("pitch plan"));
        // (a closed stream takes the plan through the range warp when sts_set_pitch_streaming is on: DESIGN.md 9l "Streamed")
        const bool warp_stream = pitch_streaming && c.ss && !join_on && !c.live && c.para_k < 0;
        if ((c.ss || join_on) && !warp_stream) return fail(STS_EINVAL, "a pitch plan applies to whole-utterance calls only: streaming and joined runs refuse it");
        if (warp_stream && ((eq_n > 0 && eq_streaming) || (loud_mode == 1 && loud_streaming) || record_taps))
            return fail(STS_EINVAL, "a pitch plan in a stream does not run with the streamed equaliser, streamed loudness or record taps: their state is carried across the chunk grid");
        if (!pend.have_forced) {     // (copies: the split-bf16 repeat of this call sets up again from the same pending plan)
            if (pend.have_plan) { eff_rate = pend.plan_rate; eff_fixed = pend.plan_fixed; eff_target = pend.plan_target; }
            else { eff_rate.assign((size_t)Ttot, 1.0f); eff_fixed.assign((size_t)Ttot, -1); eff_target.assign((size_t)B, 0); }
            for (int b = 0; b < B; b++)
                for (int i = 0; i < n[b]; i++) {
                    const size_t k = (size_t)offT[b] + i;
                    if (pend.pitch_cents[k] == 0) continue;
                    if (eff_fixed[k] >= 0) return fail(STS_EINVAL, "pitch plan: a phoneme with a fixed length must have 0 cents (a break is silent)");
                    if (eff_target[b] > 0) return fail(STS_EINVAL, "pitch plan: an utterance that is fitted to target_frames admits no non-zero cents");
                    eff_rate[k] *= pitch_ratio(pend.pitch_cents[k]);
                    if (!(eff_rate[k] >= 1.0f / 64.0f && eff_rate[k] <= 64.0f)) return fail(STS_EINVAL, "pitch plan: rate times ratio must stay in [1/64, 64]");
                }
            src_rate = eff_rate.data(); src_fixed = eff_fixed.data(); src_target = eff_target.data();
        }
    }
    const bool pitch = c.pitch = pend.have_pitch;
    c.pitch_rows = 0;
    if (pitch) for (int b = 0; b < B; b++) c.pitch_rows += pend.pitch_has[(size_t)b] ? n[b] : 0;
    const bool plan = c.plan = pend.have_plan || (pitch && !pend.have_forced);
    const bool gain = c.gain = pend.have_gain;
    const bool join = c.join = join_on;
    const bool mix = c.mix = pend.have_mix && M.is_ms == 1;       // (a single-speaker model accepts empty entries only: nothing to blend)
    // the staging block (utt_tables.hpp): where every section stands, on the device and in pinned memory alike
    const StageLayout L((size_t)B, (size_t)Ttot, mix ? pend.mix_words.size() : 0, gain ? pend.gain_words.size() : 0, join, plan, pend.have_forced);
    // sampling noise of every utterance: the caller's per-utterance table (sts_pool, sts_multi) or the engine's setting with seed + b
    c.nz.resize(B);
    for (int b = 0; b < B; b++) {
        c.nz[b] = (int)noise_utt.size() == B ? noise_utt[b] : Noise{noise.ns, noise.nsw, noise.seed + (uint64_t)b};
        if (M.dur_type != 0) c.nz[b].nsw = 0.f;        // the Fix duration predictor has no latent (FixDurationPredictor.cpp:75)
        c.any_ns |= c.nz[b].ns != 0.f; c.any_nsw |= c.nz[b].nsw != 0.f;
    }

    const int H = c.H = M.hidden, C = c.C = M.inter;
    const int FF = c.FF = M.n_layers ? M.ffn[0].c1.Cout : 0;
    const int fdp = c.fdp = M.dur_type == 0 ? M.sdp_pre.Cout : M.fix_c1.Cout;
    const int wnH = c.wnH = M.n_flows ? M.cp[0].wn.H : 0;
    const int wnL = c.wnL = M.n_flows ? M.cp[0].wn.n : 0;

    Lvl& lvT = c.lvT; lvT = Lvl(); lvT.nb = B; lvT.max_len = maxT; lvT.total = Ttot; lvT.ld = Ttot;
    const int ffn2_slices = c.ffn2_slices = M.n_layers ? pick_kslices(M.ffn[0].c2, lvT) : 1;
    BufT& bt = c.bt;
    auto layoutT = [&](Arena& A) {
        A.used = 0;
        // one device block mirroring the pinned staging block: a single host-to-device copy per run
        int* const d = bt.meta_i = A.get<int>(L.words);
        bt.ls = (float*)(d + L.ls); bt.ns = (float*)(d + L.ns); bt.nsw = (float*)(d + L.nsw);
        bt.seed = (uint64_t*)(d + L.seed);
        bt.ids = d + L.ids;
        bt.mix = mix ? d + L.mix : nullptr;
        bt.gain_q = gain ? d + L.gain_q : nullptr;
        bt.gain_h = gain ? d + L.gain_h : nullptr;
        bt.join_sil = join ? d + L.join_sil : nullptr;
        bt.plan_rate = plan ? (float*)(d + L.plan_rate) : nullptr;
        bt.plan_fixed = plan ? d + L.plan_fixed : nullptr;
        bt.plan_target = plan ? d + L.plan_target : nullptr;
        bt.forced = d + L.forced;
        bt.x = A.get<float>((size_t)H * Ttot); bt.qkv = A.get<float>((size_t)3 * H * Ttot);
        bt.att = A.get<float>((size_t)H * Ttot); bt.y = A.get<float>((size_t)H * Ttot * ffn2_slices);
        bt.x1 = A.get<float>((size_t)H * Ttot); bt.ffh = A.get<float>((size_t)FF * Ttot);
        bt.m = A.get<float>((size_t)C * Ttot);
        bt.logs = (c.any_ns || record_taps) ? A.get<float>((size_t)C * Ttot) : nullptr;
        bt.dh = A.get<float>((size_t)(fdp > H ? fdp : H) * Ttot); bt.dt1 = A.get<float>((size_t)fdp * Ttot);
        bt.dt2 = A.get<float>((size_t)fdp * Ttot); bt.dc = A.get<float>((size_t)fdp * Ttot);
        bt.dhh = A.get<float>((size_t)fdp * Ttot); bt.dp29 = A.get<float>((size_t)29 * Ttot);
        for (auto& r : bt.dr) r = A.get<float>(Ttot);
        bt.dlogw = A.get<float>(Ttot);
        bt.dur = A.get<int>(Ttot + B); bt.cum = A.get<int>(Ttot);
        bt.frames = bt.dur + Ttot;     // contiguous with dur: ONE D2H brings both
        bt.g = A.get<float>((size_t)(M.gin > 0 ? M.gin : 1) * B);
        bt.cond_dp = A.get<float>((size_t)(fdp > H ? fdp : H) * B);
        bt.cond_dec = A.get<float>((size_t)(M.up_init > 0 ? M.up_init : 1) * B);
        bt.cond_wn = A.get<float>((size_t)(2 * wnH * wnL + 4) * B * (M.n_flows > 0 ? M.n_flows : 1));   // one block per coupling
        bt.plan_rem = plan ? A.get<long long>(Ttot) : nullptr;
        bt.dur_w = plan && record_taps ? A.get<float>(Ttot) : nullptr;
        bt.pitch_words = pitch ? A.get<long long>((size_t)6 * B + 5 * (size_t)c.pitch_rows) : nullptr;
        bt.pitch_win = pitch ? A.get<int>((size_t)3 * B) : nullptr;
    };
    arenaT_.measuring = true; layoutT(arenaT_);
    if (!ensure(arenaT_, arenaT_.used + 4096)) return fail(STS_EDEVICE, "out of device memory (phoneme-level workspace)");
    arenaT_.measuring = false; layoutT(arenaT_);
    poison_arena(arenaT_);

    // ---------------- one H2D: geometry + ids (+ forced durations)
    const size_t up_bytes = c.up_bytes = L.words * 4 + 1024;
    const size_t pitch_stage = pitch ? ((size_t)6 * B + 5 * (size_t)c.pitch_rows) * 8 + (size_t)3 * B * 4 + 16 : 0;     // (pitch_geometry)
    if (!ensure_pinned(up_bytes + ((size_t)Ttot + B) * 4 + pitch_stage)) return fail(STS_EDEVICE, "pinned host allocation failed");
    int* pm = c.pm = (int*)pinned_;
    int* p_offT = c.p_offT = pm, *p_lenT = c.p_lenT = pm + B, *p_sid = c.p_sid = pm + 2 * B, *p_one = c.p_one = pm + 5 * B;
    c.p_offF = pm + 3 * B; c.p_lenF = pm + 4 * B;
    for (int b = 0; b < B; b++) { p_offT[b] = offT[b]; p_lenT[b] = lenT[b]; p_sid[b] = sid ? sid[b] : 0; }
    p_one[0] = 0; p_one[1] = B;
    if (B == 1) { int* pw0 = pm + 5 * B + 2; c.p_offF[0] = 0; c.p_lenF[0] = 0; pw0[0] = 0; pw0[1] = 0; pw0[2] = 0; }   // (a launch-ahead run: the durations kernel fills the two lengths on the device)
    int* d_offT = c.d_offT = bt.meta_i, *d_lenT = c.d_lenT = bt.meta_i + B, *d_one = c.d_one = bt.meta_i + 5 * B;
    c.d_sid = bt.meta_i + 2 * B; c.d_offF = bt.meta_i + 3 * B; c.d_lenF = bt.meta_i + 4 * B; c.d_win = bt.meta_i + 5 * B + 2;
    float* p_ls = (float*)(pm + L.ls); float* p_ns = (float*)(pm + L.ns); float* p_nsw = (float*)(pm + L.nsw); uint64_t* p_seed = (uint64_t*)(pm + L.seed);
    for (int b = 0; b < B; b++) { p_ls[b] = ls ? ls[b] : 1.0f; p_ns[b] = c.nz[b].ns; p_nsw[b] = c.nz[b].nsw; p_seed[b] = c.nz[b].seed; }
    for (int b = 0; b < B; b++) memcpy(pm + L.ids + offT[b], ids[b], sizeof(int) * n[b]);
    if (mix) memcpy(pm + L.mix, pend.mix_words.data(), sizeof(int) * pend.mix_words.size());
    if (gain) memcpy(pm + L.gain_q, pend.gain_words.data(), sizeof(int) * pend.gain_words.size());
    if (join) memcpy(pm + L.join_sil, join_sil.data(), sizeof(int) * B);
    if (pend.have_forced) memcpy(pm + L.forced, pend.forced_dur.data(), sizeof(int) * Ttot);
    if (plan) {
        memcpy(pm + L.plan_rate, src_rate, sizeof(float) * Ttot);
        memcpy(pm + L.plan_fixed, src_fixed, sizeof(int) * Ttot);
        memcpy(pm + L.plan_target, src_target, sizeof(int) * B);
    }
    HIPCK(hipMemcpyAsync(bt.meta_i, pm, L.copy_words * 4, hipMemcpyHostToDevice, stream));
    if (B > 1) HIPCK(hipEventRecord(ev_setup_, stream));     // (run_durations, batches launched from the memo: the host rewrites part of this block)

    // single-segment views travel by value (kernels.hpp SegView): no segment-table load in the kernels of a one-utterance call
    static const bool no_inline_seg_knob = exp_flag("STS_NO_INLINE_SEG");   // experiment knob
    const bool no_inline_seg = c.no_inline_seg = no_inline_seg_knob;
    const bool inl = c.inl = B == 1 && !no_inline_seg;
    c.ms = M.is_ms == 1;
    lvT.seg = inl ? SegView{nullptr, nullptr, 1, 0, 0, lenT[0]} : SegView{d_offT, d_lenT, 1, 0, 0, 0};
    Lvl& lvB = c.lvB; lvB = Lvl(); lvB.seg = no_inline_seg ? SegView{d_one, d_one + 1, 1, 0, 0, 0} : SegView{nullptr, nullptr, 1, 0, 0, B};
    lvB.nb = 1; lvB.max_len = B; lvB.total = B; lvB.ld = B;

    return STS_OK;
}

// ---- stage 1: TextEncoder (/root/reference/src/models/TextEncoder.cpp:50-74, attention_encoder.cpp:78-94)
int Engine::run_text_encoder(RunCtx& c) {
    RUN_ALIASES(c)
    // ---------------- TextEncoder (/root/reference/src/models/TextEncoder.cpp:50-74, attention_encoder.cpp:78-94)
    stage_begin(0);
    // The producer of a layer's input x -- the embedding for layer 0, the previous layer's second LayerNorm (which also adds
    // the FFN's split-K partials) afterwards -- runs inside the launch of the first conv that consumes x (col_proj_kernel)
    // where the width is instantiated and the grid is small; otherwise as its own launch.
    static const bool no_colp = exp_flag("STS_NO_COL_LAYER") || exp_flag("STS_NO_COL_PROJ");   // experiment knobs
    // Measured (profiles/r02 notes in docs/HISTORY.md 5b): with a handful of column blocks (one 128-phoneme utterance = 8) a
    // three-pass q/k/v projection makes each of the few workgroups pull 3 x 147 KB of weights through one CU and loses to
    // the separate LayerNorm + chip-wide conv (23 vs 18 us); from a few dozen blocks on it wins (batch 8: -12 us per layer).
    // A single-pass conv (the encoder's output projection) wins at every size -- so below 24 blocks every pass gets a workgroup of
    // its own (ColProjArgs::split): 10.3 us against 8.9 + 7.6 us for the LayerNorm and the conv (profiles/colp_split_ab_log.md).
    const long colp_blocks = (long)((Ttot + 15) / 16);
    const bool colp_grid = (long)((maxT + 15) / 16) * B <= 512;
    bool& dh_in_enc = c.dh_in_enc;
    dh_in_enc = false;
    auto produce_x_and_conv = [&](int l, const DConv& c, float* y) {
        // l = index of the layer whose input is produced (l == n_layers: the encoder's output projection)
        ColProjArgs pj;
        memset(&pj, 0, sizeof(pj));
        pj.x_out = bt.x; pj.x_ld = Ttot; pj.wc = c.wc; pj.bias = c.bias_rows; pj.Cout = c.Cout; pj.npass = (c.Cout + H - 1) / H;
        pj.y = y; pj.y_ld = Ttot; pj.C = H; pj.seg = lvT.seg; pj.B = B; pj.max_len = maxT;
        if (l == 0) { pj.ids = bt.ids; pj.emb = M.emb; pj.vocab = M.vocab; pj.emb_scale = sqrtf((float)M.hidden); }
        else { pj.a = bt.x1; pj.a_ld = Ttot; pj.bp = bt.y; pj.b_ld = Ttot; pj.nb = ffn2_slices; pj.b_stride = (long)H * Ttot;
               pj.gamma = M.ln2[l - 1].g; pj.beta = M.ln2[l - 1].b; }
        // several passes: all in one workgroup from 24 column blocks on (the measured win at batch); below, one workgroup per (column
        // block, pass) -- 24 workgroups of one pass each at 128 phonemes, the shape of the output projection's launch (STS_DBG_COL_PROJ)
        const bool one_launch = pj.npass == 1 || col_proj_mode != 0;
        pj.split = pj.npass > 1 && (col_proj_mode == 3 || (col_proj_mode == 1 && colp_blocks < 24));
        // the stochastic duration predictor's `pre` conv reads the encoder's output x: it rides in the output projection's launch as one
        // more workgroup per column block (single speaker: no per-utterance bias; hidden -> hidden: the staged block is its whole input)
        const DConv& sp = M.sdp_pre;
        const bool ride = l == M.n_layers && sdp_pre_ride && M.dur_type == 0 && !ms && sp.k == 1 && sp.Cin == H && sp.Cout == H && sp.wc;
        if (ride) { pj.split = 1; pj.wc2 = sp.wc; pj.bias2 = sp.bias_rows; pj.y2 = bt.dh; pj.y2_ld = Ttot; pj.Cout2 = sp.Cout; }
        const bool ok = !no_colp && conv_mode != 1 && colp_grid && one_launch && c.k == 1 && c.Cin == H && M.emb_size == H && c.wc &&
                        (l == 0 || M.ln2[l - 1].C == H) && col_proj_eligible(pj);
        if (ok) {
            const int zs = pj.split ? pj.npass + (ride ? 1 : 0) : 1;      // workgroups per column block: each reads the input stage's operands
            flops_[0] += 2.0 * c.macs_per_out * (double)Ttot;
            bytes_[0] += 4.0 * ((double)H * Ttot * (1.0 + zs * (l == 0 ? 0.0 : 1.0 + ffn2_slices)) + (double)c.Cout * Ttot + (double)H * c.Cout);
            if (ride) {       // (booked to the duration stage, as the separate conv is)
                flops_[1] += 2.0 * sp.macs_per_out * (double)Ttot;
                bytes_[1] += 4.0 * ((double)sp.Cin * Ttot + (double)sp.Cout * Ttot);
                bytes_w_[1] += 4.0 * (double)sp.Cin * sp.Cout;
                dh_in_enc = true;
            }
            col_proj(pj, stream);
            return;
        }
        if (l == 0) embed(bt.ids, M.emb, M.vocab, M.emb_size, sqrtf((float)M.hidden), bt.x, Ttot, (int)Ttot, stream);
        else ln(M.ln2[l - 1], bt.x1, bt.y, nullptr, bt.x, lvT, 0, 0, ffn2_slices, (long)H * Ttot);
        conv(c, bt.x, lvT, y, lvT, ConvOpt());
    };
    for (int l = 0; l < M.n_layers; l++) {
        const DMha& a = M.mha[l];
        produce_x_and_conv(l, a.qkv, bt.qkv);
        AttnArgs at;
        memset(&at, 0, sizeof(at));
        at.q = bt.qkv; at.k = bt.qkv + (size_t)H * Ttot; at.v = bt.qkv + (size_t)2 * H * Ttot; at.o = bt.att; at.ld = Ttot;
        at.relk = a.relk; at.relv = a.relv; at.kc = a.kc; at.px = a.px; at.win = a.win; at.nheads = 2;
        at.seg = lvT.seg; at.B = B; at.max_len = maxT; at.block_min_wgs = attn_block_min_wgs; at.attn_reg = attn_reg;
        attention(at, stream);
        flops_[0] += 2.0 * 2.0 * (double)a.ch * (double)maxT * (double)Ttot;   // ~ QK^T + PV
        bytes_[0] += 4.0 * 4.0 * (double)H * (double)Ttot;                       // q, k, v in; o out
        {   // output projection + residual + LayerNorm: one launch (col_layer.hip) where the width is instantiated
            static const bool no_col = exp_flag("STS_NO_COL_LAYER");   // experiment knob
            ColLayerArgs g;
            fill_col_oproj(a.o, M.ln1[l], bt.att, bt.x, bt.x1, lvT, g);
            if (!no_col && conv_mode != 1 && a.o.Cin == H && a.o.Cout == H && a.o.Cin_pad == H && M.ln1[l].C == H && col_layer_eligible(g)) {
                flops_[0] += 2.0 * a.o.macs_per_out * (double)Ttot;
                bytes_[0] += 4.0 * ((double)H * Ttot * 3.0 + (double)H * H);
                col_layer(g, stream);
            } else {
                conv(a.o, bt.att, lvT, bt.y, lvT, ConvOpt());
                ln(M.ln1[l], bt.x, bt.y, nullptr, bt.x1, lvT, 0, 0);
            }
        }
        const DFfn& f = M.ffn[l];
        ConvOpt o1; o1.pad_l = f.ksize == 1 ? 0 : (f.ksize - 1) / 2;
        conv(f.c1, bt.x1, lvT, bt.ffh, lvT, o1);
        ConvOpt o2 = o1; o2.in_act = 1; o2.slope = 0.f;   // nn_relu fused into the consumer's staging
        // few output tiles, long K: split K over workgroups into partial outputs that the LayerNorm below adds up
        o2.kslices = ffn2_slices; o2.kslice_stride = (long)H * Ttot;
        conv(f.c2, bt.ffh, lvT, bt.y, lvT, o2);
        // (the layer's second LayerNorm runs with the next consumer of x: the next layer's q/k/v conv or the output proj)
    }
    produce_x_and_conv(M.n_layers, M.proj, bt.m);
    if (bt.logs) conv(M.proj_logs, bt.x, lvT, bt.logs, lvT, ConvOpt());   // (the prior's scale: only calls that sample it or record taps)
    tap("x_enc", bt.x, H, Ttot, Ttot);
    tap("m", bt.m, C, Ttot, Ttot);
    if (bt.logs) tap("logs", bt.logs, C, Ttot, Ttot);
    mark(1);
    return STS_OK;
}

// ---- stage 2: speaker conditioning, duration predictor, durations -> frame counts on the host (the one data-dependent sync)
int Engine::run_durations(RunCtx& c) {
    Model& M = model;
    const int B = c.B; const StreamSpec* const ss = c.ss; const long Ttot = c.Ttot;
    [[maybe_unused]] const int H = c.H, fdp = c.fdp;
    Lvl &lvT = c.lvT, &lvB = c.lvB; BufT& bt = c.bt;
    const size_t up_bytes = c.up_bytes; int* const pm = c.pm; int* const p_offF = c.p_offF; int* const p_lenF = c.p_lenF;
    int* const d_sid = c.d_sid; int* const d_offF = c.d_offF;
    const bool inl = c.inl, ms = c.ms; const int maxT = c.maxT; (void)maxT;

    // ---------------- speaker conditioning vectors (all 1x1 convs on g; SynthesizerTrn.cpp:363-372)
    stage_begin(1);
    if (ms && c.mix) speaker_blend(M.emb_g, M.spk_num, M.gin, d_sid, B, speaker_mix_tab(bt.mix, B, pend.mix_K), bt.g, stream);     // (in place of the gather)
    else if (ms) gather_speaker(M.emb_g, M.spk_num, M.gin, d_sid, B, bt.g, stream);

    // ---------------- duration predictor
    const float* r_final = nullptr;
    if (M.dur_type == 0) {   // /root/reference/src/models/StochasticDurationPredictor.cpp:117-149
        ConvOpt op;
        if (ms) { conv(M.sdp_cond, bt.g, lvB, bt.cond_dp, lvB, ConvOpt()); op.ubias = bt.cond_dp; }
        if (!c.dh_in_enc) conv(M.sdp_pre, bt.x, lvT, bt.dh, lvT, op);      // (else: written by the launch of the encoder's output projection)
        const float* dh = dds(M.sdp_dds, bt.dh, bt.dt1, bt.dt2, lvT);
        conv(M.sdp_proj, dh, lvT, bt.dc, lvT, ConvOpt());
        // the latent z (StochasticDurationPredictor.cpp:129-131): rand_gen(2, T) * noise_scale_w, flipped.  Without noise it is all
        // zeros and null inputs stand for it; with noise (some utterance has nsw != 0) it is written into the rows flow n-1 reads
        const float *r0 = nullptr, *r1 = nullptr;
        float *n0 = bt.dr[2], *n1 = bt.dr[3], *s0 = bt.dr[0], *s1 = bt.dr[1];
        if (c.any_nsw) { sdp_noise(lvT.seg, B, maxT, bt.nsw, bt.seed, bt.dr[0], bt.dr[1], stream); r0 = bt.dr[0]; r1 = bt.dr[1]; }
        else if (M.sdp_flows <= 1) { HIPCK(hipMemsetAsync(bt.dr[0], 0, (size_t)Ttot * 4, stream)); r0 = bt.dr[0]; }
        for (int i = M.sdp_flows - 1; i > 0; i--) {   // flow 0 is skipped, as in the reference
            const DConvFlow& cf = M.cf[i];
            // DDSConv(pre(x0) + g): the 1 -> C input conv and the "+ g" ride inside the first DDSConv layer
            const SplineTail tl{&cf.proj, sqrtf((float)cf.filter), r0, r1, n0, n1};
            bool tail_done = false;
            const float* dhh = dds(cf.dds, bt.dhh, bt.dt1, bt.dt2, lvT, &cf.pre, r0, bt.dc, &tl, &tail_done);
            if (!tail_done) {
                conv(cf.proj, dhh, lvT, bt.dp29, lvT, ConvOpt());
                spline_step(bt.dp29, Ttot, sqrtf((float)cf.filter), r0, r1, n0, n1, Ttot, stream);
            }
            r0 = n0; r1 = n1;
            float* t;
            t = n0; n0 = s0; s0 = t;
            t = n1; n1 = s1; s1 = t;
        }
        r_final = r0;
    } else {                 // /root/reference/src/models/FixDurationPredictor.cpp:75-96
        const float* xin = bt.x;
        if (ms) {
            conv(M.fix_cond, bt.g, lvB, bt.cond_dp, lvB, ConvOpt());
            HIPCK(hipMemcpyAsync(bt.dh, bt.x, (size_t)H * Ttot * 4, hipMemcpyDeviceToDevice, stream));
            add_ubias(bt.dh, Ttot, bt.cond_dp, H, lvT.seg, B, maxT, stream);
            xin = bt.dh;
        }
        conv(M.fix_c1, xin, lvT, bt.dt1, lvT, ConvOpt());
        ln(M.fix_n1, bt.dt1, nullptr, nullptr, bt.dt1, lvT, 1, 0);
        conv(M.fix_c2, bt.dt1, lvT, bt.dt2, lvT, ConvOpt());
        ln(M.fix_n2, bt.dt2, nullptr, nullptr, bt.dt2, lvT, 1, 0);
        conv(M.fix_proj, bt.dt2, lvT, bt.dr[0], lvT, ConvOpt());
        r_final = bt.dr[0];
    }
    // ---------------- the one data-dependent sync: frame counts (+ durations for the API).  The durations kernel writes them
    // straight into host-mapped pinned memory and raises a sequence flag; the host polls that word -- no device-to-host copy
    // kernel and no stream-synchronise wake-up between the duration predictor and the flow (STS_NO_MAPPED_SYNC=1: the copy path)
    static const bool no_mapped = exp_flag("STS_NO_MAPPED_SYNC");
    const size_t hm_ints = (size_t)Ttot + B + 1;
    if (!no_mapped && hm_ints > hmap_cap_) {
        (void)hipStreamSynchronize(stream);
        if (hmap_) (void)hipHostFree(hmap_);
        hmap_ = nullptr; hmap_dev_ = nullptr; hmap_cap_ = 0;
        if (hipHostMalloc((void**)&hmap_, (hm_ints * 2 + 64) * 4, hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer((void**)&hmap_dev_, hmap_, 0) == hipSuccess) { hmap_cap_ = hm_ints * 2 + 64; memset(hmap_, 0, hmap_cap_ * 4); }
        else { if (hmap_) (void)hipHostFree(hmap_); hmap_ = nullptr; hmap_dev_ = nullptr; }
        if (!arrive_ && hipMalloc((void**)&arrive_, 64) == hipSuccess) (void)hipMemsetAsync(arrive_, 0, 64, stream);
    }
    const bool mapped = c.mapped = !no_mapped && hmap_ && arrive_;
    if (mapped) { seq_ = seq_ == 0x7fffffff ? 1 : seq_ + 1; }
    // Launch-ahead (one utterance, plain call): the flow and the decoder are enqueued for a PREDICTED frame capacity and read the real
    // count from device memory, where the durations kernel leaves it (clamped to the capacity).  The host never waits between the duration
    // predictor and the flow; it reads the count after the last kernel is enqueued and sizes the PCM download with it.
    // The prediction is a MEMO, not a guess (round 5): the reference's noise scale is hard-coded 0 (SynthesizerTrn.cpp:357), so the
    // frame count is a pure function of (phoneme ids, speaker, length scale); the engine remembers the count of its last 1 024 distinct (engine.hpp kMemoEntries)
    // requests under a 64-bit hash of exactly those inputs.  A request it has seen runs ahead with the exact count -- never more than the
    // 63 frames of bucket padding the waiting path also carries, never a miss; any other request takes the waiting path.  Should the
    // count land in another 64-frame bucket than predicted (a hash collision), the two stages are repeated the waiting way, so the samples a
    // request returns never depend on what the engine served before (dispatch decisions are taken per bucket).
    // Batches (round 5): the memo is per UTTERANCE.  When every member of a packed batch has been served before, the frame
    // geometry of the whole batch is known on the host before the duration predictor has run: the tables the batched kernels read are
    // uploaded from the memo, flow + decoder are enqueued right behind the durations kernel, and the counts that kernel wrote are compared
    // with the memo after the run's one stream synchronisation (a difference = a hash collision: the two stages are repeated the waiting
    // way).  Identical geometry => identical launches => bit-identical PCM; the host -- a pool or multi-device worker -- no longer
    // spins through the text encoder and the duration predictor.
    long pred = 0;
    c.req_keys.assign(B, 0ull);
    for (int b = 0; b < B; b++) {
        unsigned long long h = 1469598103934665603ull;
        auto mix = [&h](unsigned v) { for (int q = 0; q < 4; q++) { h ^= (v >> (8 * q)) & 0xffu; h *= 1099511628211ull; } };
        mix((unsigned)c.n[b]);
        if (launch_ahead != 2) {          // (2: test mode -- the key is the phoneme count alone, i.e. every request of a length collides)
            mix((unsigned)(c.sid ? c.sid[b] : 0)); { const float lsb = c.ls ? c.ls[b] : 1.0f; unsigned u; memcpy(&u, &lsb, 4); mix(u); }
            for (int t = 0; t < c.n[b]; t++) mix((unsigned)c.ids[b][t]);
        }
        if (c.nz[b].nsw != 0.f) {         // sampled durations depend on (nsw, seed) too; a noise-free key never carries these words
            unsigned u; memcpy(&u, &c.nz[b].nsw, 4); mix(u); mix((unsigned)c.nz[b].seed); mix((unsigned)(c.nz[b].seed >> 32));
            h ^= 0x5bd1e995ull; h *= 1099511628211ull;
        }
        c.req_keys[b] = h | 1ull;
    }
    c.predF.clear();
    if (launch_ahead && !ss && !pend.have_forced && !c.plan && !c.mix && !c.gain && !c.pitch && !c.join && !record_taps && mapped) {     // (a planned or mixed run's frame count is not a function of the memo's key; a run with a gain plan and a joined run stay off the memo by contract)
        c.predF.resize(B);
        for (int b = 0; b < B; b++) {
            const auto it = seen_tf_.find(c.req_keys[b]);
            if (it == seen_tf_.end()) { c.predF.clear(); break; }
            c.predF[b] = it->second;
        }
    }
    if (B == 1 && !c.predF.empty()) pred = c.predF[0];
    c.ahead = pred > 0;
    c.ahead_b = B > 1 && !c.predF.empty();
    c.hop = M.hop_total;
    const long cap = c.ahead ? (pred + 63) / 64 * 64 : 0;
    if (c.plan) {        // the plan kernel turns logw and the plan into the forced durations the durations kernel then takes
        DurPlanArgs pa{};
        pa.r0 = r_final; pa.sdp = M.dur_type == 0 ? 1 : 0; pa.ea_m = M.ea_m; pa.ea_logs = M.ea_logs; pa.ls = bt.ls;
        pa.rate = bt.plan_rate; pa.fixed = bt.plan_fixed; pa.target = bt.plan_target;
        pa.forced = bt.forced; pa.dur_w = bt.dur_w; pa.rem = bt.plan_rem; pa.seg = lvT.seg;
        duration_plan(pa, B, stream);
    }
    durations(r_final, M.dur_type == 0 ? 1 : 0, M.ea_m, M.ea_logs, bt.ls, (pend.have_forced || c.plan) ? bt.forced : nullptr, bt.dlogw,
              bt.dur, bt.cum, bt.frames, lvT.seg, B, stream, mapped ? hmap_dev_ : nullptr, Ttot, seq_, arrive_,
              c.ahead ? c.d_lenF : nullptr, c.ahead ? c.d_win + 2 : nullptr, (int)cap);
    c.forced = pend.have_forced || c.plan || c.mix || c.gain || c.pitch || c.join;      // (none of these runs feeds the memo: its key hashes sid, not the mix)
    pend.have_forced = false;
    mark(2);
    sync_wait_ms_ = 0;
    if (c.ahead) {
        c.Ftot = cap; c.maxF = (int)cap;                // (capacity; the real count replaces it in run_output)
        return frame_geometry(c);
    }
    if (c.ahead_b) {                                    // the batch's geometry from the memo; checked against the kernel's counts in run_output
        // p_offF / p_lenF live in the pinned block run_setup uploaded: that copy (issued ~0.3 ms of host work ago) must have read them before the
        // host rewrites them (nothing enforced it)
        HIPCK(hipEventSynchronize(ev_setup_));
        c.Ftot = 0; c.maxF = 0;
        for (int b = 0; b < B; b++) {
            const int f = (int)c.predF[b];
            c.p_offF[b] = (int)c.Ftot; c.p_lenF[b] = f; c.Ftot += f; if (f > c.maxF) c.maxF = f;
        }
        return frame_geometry(c);
    }
    int rc = wait_frame_counts(c);
    if (rc != STS_OK) return rc;
    return frame_geometry(c);
}

static inline int wait_class(long phonemes) { int c = 0; while ((1L << (c + 1)) <= phonemes && c < 23) c++; return c; }
void Engine::nap_before_wait(int which, long phonemes) {
    if (!polite_wait) return;
    const WaitEst& e = wait_est_[which][wait_class(phonemes)];
    if (e.us <= 0.0 || e.phonemes <= 0) return;
    const double scale = phonemes < e.phonemes ? (double)phonemes / (double)e.phonemes : 1.0;      // (a smaller request of the class: never oversleep it)
    const double nap = e.us * scale * 0.8 - 70.0;            // (less the timer slack of a normal thread)
    if (nap < 40.0) return;
    struct timespec ts; ts.tv_sec = (time_t)(nap * 1e-6); ts.tv_nsec = (long)((nap - (double)ts.tv_sec * 1e6) * 1e3);
    (void)nanosleep(&ts, nullptr);
}
void Engine::note_wait(int which, long phonemes, double waited_us, bool was_ready_at_wake) {
    if (!polite_wait) return;
    WaitEst& e = wait_est_[which][wait_class(phonemes)];
    // ready at the first look after the nap = the estimate is too long (by an unknown amount): shrink it; otherwise the wait was measured
    if (e.us <= 0.0) { e.us = waited_us * 0.5; e.phonemes = phonemes; }
    else if (was_ready_at_wake) e.us *= 0.85;
    else { e.us = e.us * 0.7 + waited_us * 0.3; e.phonemes = phonemes; }
}
// the run's one stream synchronisation
int Engine::final_sync(long phonemes) {
    if (!polite_wait) { HIPCK(hipStreamSynchronize(stream)); return STS_OK; }
    const double t0 = now_us();
    nap_before_wait(1, phonemes);
    const bool ready = hipStreamQuery(stream) == hipSuccess;
    HIPCK(hipStreamSynchronize(stream));
    note_wait(1, phonemes, now_us() - t0, ready);
    return STS_OK;
}

// blocks until the durations kernel's results are on the host: durations_h, per-utterance frame offsets / counts, Ftot, maxF
int Engine::wait_frame_counts(RunCtx& c) {
    const int B = c.B; const long Ttot = c.Ttot; BufT& bt = c.bt;
    int* const p_offF = c.p_offF; int* const p_lenF = c.p_lenF;
    int* p_down = (int*)(pinned_ + c.up_bytes);
    {
        const auto w0 = std::chrono::steady_clock::now();
        bool polled_unready = true;
        if (c.mapped) {
            volatile int* flag = hmap_;                 // word 0 = sequence flag, then dur[Ttot], frames[B]
            bool ok = false;
            polled_unready = false;
            // (sts_pool / sts_multi workers sleep through most of this wait: engine.hpp polite_wait)
            nap_before_wait(0, Ttot);
            for (long spin = 0; ; spin++) {
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq_) { ok = true; polled_unready = spin > 0; break; }
                cpu_relax();
                if (spin >= 20000) std::this_thread::yield();
                if ((spin & 0x3ff) == 0x3ff) {      // every ~1k polls: did the stream die?  (a kernel fault would spin forever)
                    const hipError_t q = hipStreamQuery(stream);
                    if (q == hipSuccess) { ok = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq_; break; }
                    if (q != hipErrorNotReady) return fail(STS_EDEVICE, std::string("stream failed before the frame counts arrived: ") + hipGetErrorString(q));
                    if (std::chrono::steady_clock::now() - w0 > std::chrono::milliseconds(50)) {
                        HIPCK(hipStreamSynchronize(stream));
                        ok = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq_;
                        break;
                    }
                }
            }
            if (!ok) return fail(STS_EDEVICE, "frame counts did not arrive");
            p_down = hmap_ + 1;
        } else {
            HIPCK(hipMemcpyAsync(p_down, bt.dur, ((size_t)Ttot + B) * 4, hipMemcpyDeviceToHost, stream));
            HIPCK(hipStreamSynchronize(stream));
        }
        const double waited_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        sync_wait_ms_ += waited_ms;
        if (c.mapped) note_wait(0, Ttot, waited_ms * 1e3, !polled_unready);
    }
    durations_h.assign(p_down, p_down + Ttot);
    last_n.assign(c.lenT.begin(), c.lenT.end());
    tap("logw", bt.dlogw, 1, Ttot, Ttot);
    if (bt.dur_w) tap("dur_w", bt.dur_w, 1, Ttot, Ttot);
    c.Ftot = 0; c.maxF = 0;
    for (int b = 0; b < B; b++) {
        int f = p_down[Ttot + b];
        p_offF[b] = (int)c.Ftot; p_lenF[b] = f; c.Ftot += f; if (f > c.maxF) c.maxF = f;
    }
    if (!c.forced && (int)c.req_keys.size() == B)      // the memo of run_durations: every utterance's frame count (replaces, never a running maximum)
        for (int b = 0; b < B; b++) {
            const auto it = seen_tf_.find(c.req_keys[b]);
            if (it != seen_tf_.end()) { it->second = p_lenF[b]; continue; }
            if (seen_order_.size() >= kMemoEntries) { seen_tf_.erase(seen_order_.front()); seen_order_.pop_front(); }
            seen_tf_.emplace(c.req_keys[b], (long)p_lenF[b]);
            seen_order_.push_back(c.req_keys[b]);
        }
    return STS_OK;
}

// the one place that decides the output chain of a run (out_chain.hpp), with the limiter's design and the resampler's ratio for it
int Engine::plan_output(RunCtx& c) {
    c.oc = plan_out_chain(OutFacts{c.ss != nullptr, c.B, resampling(), c.gain || c.pitch, c.join, eq_n > 0, loud_mode, lim_mode != 0, record_taps, stream_direct != 0, eq_streaming, loud_streaming, c.pitch && c.ss != nullptr});
    if (c.oc.run[OS_RESAMPLE]) { c.rsP = rs.P; c.rsQ = rs.Q; }
    c.eqS = eq_n;
    if (c.oc.run[OS_LIMIT] && !limiter_design(out_rate, lim_gain_db, lim_ceiling, lim_ms, &c.limd)) return fail(STS_EINVAL, "limiter: output rate outside [8000, 48000]");
    return STS_OK;
}

// A run with a pitch plan, when the durations are on the host (they come with the frame counts): the warp's layout in 64-bit integers
// (kernels.hpp pitch_tables), the window table of the warped signals for everything behind the warp, both uploaded from the pinned block
// behind the durations' place in it -- no host wait beyond the one for the frame counts -- and the phoneme starts for
// sts_get_phoneme_offsets.  The prototype goes to the device once per engine.
int Engine::pitch_geometry(RunCtx& c) {
    const int B = c.B, hop = c.hop;
    if (!d_pitch_table_) {
        std::vector<float> proto(kPitchTableFloats);
        pitch_table(proto.data());
        HIPCK(hipMalloc((void**)&d_pitch_table_, proto.size() * 4));
        HIPCK(hipMemcpy(d_pitch_table_, proto.data(), proto.size() * 4, hipMemcpyHostToDevice));
    }
    std::vector<int64_t> steps((size_t)c.Ttot);
    std::vector<const int32_t*> dur((size_t)B);
    std::vector<const int64_t*> step((size_t)B);
    std::vector<long long> xoff((size_t)B);
    for (int b = 0; b < B; b++) {
        const size_t t = (size_t)c.offT[b];
        dur[b] = durations_h.data() + t;
        step[b] = pend.pitch_has[(size_t)b] ? steps.data() + t : nullptr;
        if (step[b]) for (int i = 0; i < c.lenT[b]; i++) steps[t + i] = pitch_step(pend.pitch_cents[t + i]);
        xoff[b] = (long long)c.p_offF[b] * hop;
    }
    PitchTables tab;
    if (const char* bad = pitch_tables(B, c.lenT.data(), dur.data(), step.data(), xoff.data(), hop, &tab)) return fail(STS_EINVAL, bad);
    if (tab.TT != c.pitch_rows) return fail(STS_EDEVICE, "pitch plan: the tables do not have the size the setup reserved");
    if (tab.total_out > 2000000000LL || out_count(tab.total_out) + B > 2147483647LL) return fail(STS_EINVAL, "batch produces too many samples for one call");
    c.pitch_nout = tab.nout; c.pitch_total = tab.total_out; c.pitch_max = tab.max_out;
    if (c.ss) c.pitch_words_h = tab.words;         // (a stream: every step's geometry reads them, pitch_stream.hpp)
    // phoneme starts in the warped signal: o_i of a planned utterance (the words' o_i+1 column), frames * hop of a copied one
    last_pitch_start.assign((size_t)c.Ttot, 0);
    {
        const long long* mem = tab.words.data();
        const long long* oend = mem + 6 * (size_t)B;
        for (int b = 0; b < B; b++) {
            const size_t t = (size_t)c.offT[b];
            const long long toff = mem[6 * (size_t)b + 4], rows = mem[6 * (size_t)b + 5];
            long long f = 0;
            for (int i = 0; i < c.lenT[b]; i++) {
                if (!step[b]) last_pitch_start[t + i] = f * hop;
                else last_pitch_start[t + i] = (i == 0 || rows < c.lenT[b]) ? 0 : oend[toff + i - 1];     // (rows < n: all durations 0, every start 0)
                f += durations_h[t + i];
            }
        }
    }
    // staging behind the durations' download: [words | win: off B, off B, N' B]
    char* stage = pinned_ + c.up_bytes + (((size_t)c.Ttot + B) * 4 + 7) / 8 * 8;
    memcpy(stage, tab.words.data(), tab.words.size() * 8);
    int* win = (int*)(stage + tab.words.size() * 8);
    long long off = 0;
    for (int b = 0; b < B; b++) {
        win[StepTab::zoff(B) + b] = (int)off; win[StepTab::coff(B) + b] = (int)off; win[StepTab::wlen(B) + b] = (int)tab.nout[b];
        off += tab.nout[b];
    }
    HIPCK(hipMemcpyAsync(c.bt.pitch_words, stage, tab.words.size() * 8, hipMemcpyHostToDevice, stream));
    HIPCK(hipMemcpyAsync(c.bt.pitch_win, win, (size_t)3 * B * 4, hipMemcpyHostToDevice, stream));
    return STS_OK;
}

// the output chain, frame capacity (one utterance: buckets of 64 frames), geometry tables on the device, room for the PCM download
int Engine::frame_geometry(RunCtx& c) {
    Model& M = model;
    { const int rc = plan_output(c); if (rc != STS_OK) return rc; }
    const int B = c.B; const StreamSpec* const ss = c.ss;
    int* const pm = c.pm; int* const p_offF = c.p_offF; int* const p_lenF = c.p_lenF;
    const int hop = c.hop = M.hop_total;
    c.Fld = (B == 1 && !ss) ? (c.Ftot + 63) / 64 * 64 : c.Ftot;
    c.maxFld = (B == 1 && !ss) ? (int)c.Fld : c.maxF;
    if ((double)c.Fld * hop > 2.0e9 || (double)c.Fld * hop * 8 > 6.0e10) return fail(STS_EINVAL, "batch produces too many samples for one call");
    if (c.pitch) { const int rc = pitch_geometry(c); if (rc != STS_OK) return rc; }
    if (c.join) {     // the joined signal's layout (64-bit host arithmetic): F_J frames, sentence b at last_join_start[b]
        c.FJ = (long long)c.Ftot + join_total_sil;
        const long long NJ = c.FJ * hop;
        if (NJ > 2000000000LL || out_count(NJ) > 2147483647LL) return fail(STS_EINVAL, "the joined signal is too long for one call (N_J <= 2 10^9 native and L_out <= 2^31 - 1 output samples)");
        last_join_start.resize(B);
        for (int b = 0; b < B; b++) last_join_start[b] = ((long long)p_offF[b] + join_sil[b]) * hop;
    }
    if (!c.ahead) {   // frame geometry + (normal call) the decode windows = the utterances, in the same copy
        int* pw = pm + 5 * B + 2;
        for (int b = 0; b < B; b++) { pw[StepTab::zoff(B) + b] = p_offF[b]; pw[StepTab::coff(B) + b] = p_offF[b]; pw[StepTab::wlen(B) + b] = p_lenF[b]; }
        // (a single utterance carries its geometry in the kernel arguments: nothing on the device reads these tables)
        if (!c.inl || ss) HIPCK(hipMemcpyAsync(c.d_offF, p_offF, (size_t)(5 * B + 2) * 4, hipMemcpyHostToDevice, stream));
    }
    h_pcm = nullptr; pcm_in_host_ = false;
    if (host_pcm && !ss) {   // room for the PCM download that rides at the end of this run
        const long long native = c.join ? c.FJ * hop : c.pitch ? c.pitch_total : (long long)c.Fld * hop;       // (a joined run returns the joined signal, a run with a pitch plan the warped ones)
        const size_t need = (size_t)(out_count(native) + (c.oc.run[OS_RESAMPLE] ? B : 0)) * 2 + 256;
        if (need > pinned_pcm_cap_) {
            if (pinned_pcm_) (void)hipHostFree(pinned_pcm_);
            pinned_pcm_ = nullptr; pinned_pcm_cap_ = 0;
            pinned_pcm_dev_ = nullptr;
            if (hipHostMalloc((void**)&pinned_pcm_, need + need / 2, hipHostMallocMapped) != hipSuccess) return fail(STS_EDEVICE, "pinned host allocation failed");
            pinned_pcm_cap_ = need + need / 2;
            if (hipHostGetDevicePointer((void**)&pinned_pcm_dev_, pinned_pcm_, 0) != hipSuccess) { pinned_pcm_dev_ = nullptr; (void)hipGetLastError(); }
        }
    }
    return STS_OK;
}

// ---- stage 3: frame-level workspace (flow buffers over all frames, decoder buffers over the decode windows)
int Engine::run_frame_workspace(RunCtx& c) {
    Model& M = model;
    const int B = c.B; const StreamSpec* const ss = c.ss; const int hop = c.hop;
    const long Ftot = c.Fld; const int maxF = c.maxFld;        // (capacity: == the counts except for one utterance, see RunCtx::Fld)
    const int C = c.C, wnH = c.wnH; const bool inl = c.inl;
    int* const p_lenF = c.p_lenF; int* const d_offF = c.d_offF; int* const d_lenF = c.d_lenF;
    // ---------------- frame-level workspace.  The flow works on all Ftot frames; the decoder works on
    // "windows" of z: whole utterances normally (Wcap == Ftot), one chunk plus its two halos when streaming.
    const bool warp = c.pitch && ss;        // a stream through the pitch warp: the larger halo, a step's warped windows, the warped tables
    const int halo = c.halo = stream_halo(warp);
    long Wcap = Ftot;
    if (ss) {    // a step decodes at most one window per utterance, each at most a chunk plus two halos: sum_b min(F_b, C + 2 halo)
        Wcap = 0;
        for (int b = 0; b < B; b++) Wcap += std::min<long>(p_lenF[b], (long)ss->chunk_frames + 2 * halo);
    }
    if (ss && c.join && c.para_k >= 0) {
        // one step of an open paragraph: c.js is the paragraph's plan (para_step), the workspace is what this one step decodes
        JsStep t;
        c.js.step(c.para_k, t);
        Wcap = std::max<long>(1, (long)t.Wtot);
    } else if (ss && c.join) {
        // a joined stream: the steps walk J (join_stream.hpp).  The workspace is the most frames one step decodes -- the maximum over the
        // steps of the summed window lengths, never the sum of the sentences
        JsPlan& js = c.js;
        std::vector<long long> sil(join_sil.begin(), join_sil.end());
        js.layout(B, p_lenF, sil.data(), join_total_sil);
        js.hop = hop; js.C = ss->chunk_frames;
        js.Hd = decoder_halo_frames(M); js.Ho = halo - js.Hd;
        js.P = resampling() ? rs.P : 1; js.Q = resampling() ? rs.Q : 1;
        js.H = c.oc.run[OS_LIMIT] ? c.limd.H : 0;
        Wcap = std::max<long>(1, (long)js.workspace());
    }
    c.Wcap = Wcap;
    int upS = 1;
    for (int u : M.up_rate) upS *= u;
    c.upS = upS;
    std::vector<size_t> stage_elems(M.n_up);
    size_t regA = 0, regB = 0;
    { int S = 1; for (int i = 0; i < M.n_up; i++) { S *= M.up_rate[i]; stage_elems[i] = (size_t)(3 + 4 * M.n_resk) * M.ups[i].Cout * Wcap * S;   // upsampler output + 3 per chain (+ the pre-split path: planes / x16 of the stage input, one more per chain)
          if (i & 1) { if (stage_elems[i] > regB) regB = stage_elems[i]; } else { if (stage_elems[i] > regA) regA = stage_elems[i]; } } }
    const long Lsb = c.Lsb = Wcap * upS + B;           // MB-iSTFT: frames + 1 per window
    const int sbC = c.sbC = M.conv_post.Cout;
    // the reverse flow as one launch per WaveNet layer (wn_flow.hip): every coupling must carry the fused operands, with one geometry
    bool use_ff = flow_fused && conv_mode == 0 && conv_math == 3 && !M.cp.empty() && wnH > 0;
    for (size_t i = 0; i < M.cp.size() && use_ff; i++)
        use_ff = M.cp[i].ff.ok && M.cp[i].wn.H == wnH && M.cp[i].wn.n == c.wnL && M.cp[i].ff.G == M.cp[0].ff.G && M.cp[i].wn.in[0].k == M.cp[0].wn.in[0].k;
    if (use_ff) {
        // one round of workgroups at most: a workgroup re-pulls its group's ~290 KB of weights for 32 frames, which pays while the launch
        // is latency-bound (668 frames: 0.31 vs 0.45 ms) and loses by 2.6x once it is not (batch 32: 7.3 vs 2.8 ms; profiles/r04_ab_log.md)
        long tiles = 0;
        if (B == 1) tiles = (Ftot + 31) / 32;
        else for (int b = 0; b < B; b++) tiles += (p_lenF[b] + 31) / 32;
        if (flow_fused < 2) use_ff = tiles * M.cp[0].ff.G <= 256;       // (2 / 3, tests and A/B: at any size)
        // 16 frames per workgroup where the 32-frame grid would leave at least half the CUs without one (one utterance of 668 frames: 126
        // workgroups on 256 CUs).  The two widths return the same bits, so this one choice may look at the frame count itself (a call
        // launched ahead: the count it expects) and not at the capacity, without the two kinds of call ever differing in a sample
        const long live = B == 1 ? ((c.ahead && !c.predF.empty() ? c.predF[0] : c.Ftot) + 31) / 32 : tiles;
        c.ffNT = flow_fused == 3 || (flow_fused == 1 && live * M.cp[0].ff.G <= n_cus / 2) ? 16 : 32;
    }
    c.use_ff = use_ff; c.ffG = use_ff ? M.cp[0].ff.G : 0;
    BufF& bf = c.bf;
    const OutChain& oc = c.oc;
    c.Ocap = oc.run[OS_RESAMPLE] ? out_count((long long)Wcap * hop) + B : (long long)Wcap * hop;
    if (c.join) c.Ocap = oc.run[OS_RESAMPLE] ? out_count(c.FJ * hop) + 1 : c.FJ * hop;
    if (c.pitch) c.Ocap = oc.run[OS_RESAMPLE] ? out_count(c.pitch_total) + B : c.pitch_total;      // (everything behind the warp sees the warped signals)
    const long long jwin = ss && c.join ? c.js.window_frames() * hop : c.FJ * hop;      // floats of the join's output: a step's window of J, or J
    if (ss && c.join) c.Ocap = oc.run[OS_RESAMPLE] ? out_count(jwin) + 4 : jwin;         // (the widened range of a step lies inside its window's outputs)
    if (ss && oc.run[OS_LIMIT] && oc.run[OS_RESAMPLE]) c.Ocap += B;       // (a window's widened output range is rounded per window)
    // one short utterance with the PCM wanted on the host: the chain's writer stores its int16 samples into the mapped pinned buffer itself
    // (posted writes over the host link, under the kernel's own run time) instead of a download queued behind it
    pcm_in_host_ = pcm_direct && host_pcm && !ss && B == 1 && !record_taps && pinned_pcm_dev_ && (size_t)c.Ocap * 2 + 256 <= pinned_pcm_cap_ &&
                   (size_t)c.Ocap * 2 <= ((size_t)4 << 20);
    auto layoutF = [&](Arena& A) {
        A.used = 0;
        for (int q = 0; q < 2; q++) {
            bf.ff_h[q] = A.get<float>(use_ff ? (size_t)wnH * Ftot : 1);
            bf.ff_part[q] = A.get<float>(use_ff ? (size_t)c.ffG * wnH * Ftot : 1);
            bf.ff_macc[q] = A.get<float>(use_ff ? (size_t)c.ffG * (C / 2) * Ftot : 1);
        }
        bf.ff_alt = A.get<float>(use_ff ? (size_t)C * Ftot : 1);
        bf.z = A.get<float>((size_t)C * Ftot); bf.h = A.get<float>((size_t)wnH * Ftot);
        bf.acts = A.get<float>((size_t)wnH * Ftot); bf.out = A.get<float>((size_t)wnH * Ftot);
        bf.fliptmp = A.get<float>((M.n_flows & 1) ? (size_t)C * Ftot : 1);
        bf.x0 = A.get<float>((size_t)M.up_init * Wcap);
        bf.regA = A.get<float>(regA + 1); bf.regB = A.get<float>(regB + 1);
        if (M.dec_type != 0) {
            bf.tailA = A.get<float>((size_t)sbC * Lsb); bf.tailB = A.get<float>((size_t)sbC * Lsb);
            bf.tailC = A.get<float>((size_t)4 * Wcap * upS * 4);
        } else { bf.tailA = bf.tailB = bf.tailC = nullptr; }
        // the output chain: a buffer exists iff a stage of this run reads or writes it (everything behind a join is sized for the one
        // joined utterance: c.Ocap)
        bf.wave = A.get<float>(oc.wave[OS_TAIL] ? (size_t)Wcap * hop : 1);
        bf.wave_gain = oc.wave[OS_GAIN] ? A.get<float>((size_t)Wcap * hop) : nullptr;
        bf.wave_join = oc.wave[OS_JOIN] ? A.get<float>((size_t)jwin) : nullptr;
        bf.pcm = A.get<int16_t>((size_t)c.Ocap);
        if (pcm_in_host_) bf.pcm = pinned_pcm_dev_;
        bf.pcm_nat = oc.pcm_nat ? A.get<int16_t>((size_t)Wcap * hop) : bf.pcm;
        bf.wave_out = oc.wave[OS_RESAMPLE] ? A.get<float>((size_t)c.Ocap) : nullptr;
        bf.pcm_rs = oc.pcm_rs ? A.get<int16_t>((size_t)c.Ocap) : bf.pcm;
        bf.lws = oc.lws ? A.get<char>(loud_ws_bytes(B, c.Ocap)) : nullptr;
        bf.limws = oc.limws ? A.get<char>((size_t)B * 16) : nullptr;
        bf.wave_lim = oc.wave[OS_LIMIT] ? A.get<float>((size_t)c.Ocap) : nullptr;
        bf.wave_eq = oc.wave[OS_EQ] ? A.get<float>((size_t)c.Ocap) : nullptr;
        bf.eqws = oc.eqws ? A.get<char>(eq_ws_bytes(B, c.Ocap)) : nullptr;
        bf.stab = nullptr; bf.spack = nullptr; bf.gwin = bf.cond_win = nullptr;
        if (ss) {
            bf.stab = A.get<char>(StepTab(B, c.gain, oc.eqst, oc.lst, c.join, warp).bytes);
            if (oc.spack) bf.spack = A.get<int16_t>((size_t)c.Ocap);
            if (M.dec_type == 0 && c.ms && c.bstream) { bf.gwin = A.get<float>((size_t)M.gin * B); bf.cond_win = A.get<float>((size_t)M.up_init * B); }
        }
        // (a stream that runs the EQ: behind everything else, so that every other buffer lies where it lies without it)
        bf.eqst = nullptr; bf.eqsE = nullptr;
        // (an open stream keeps the carried states and the result tables in pools of its own, by slot: stream_step names them.  Only the
        // step's tile end states and the gate's table and gains are of the step)
        const bool slot_state = c.live && !c.join;
        if (oc.eqst && !c.admission) {
            const int nu = c.join ? 1 : B;
            if (!slot_state) bf.eqst = A.get<char>(eqs_state_bytes(nu));
            bf.eqsE = (double*)A.get<char>(eqs_ws_bytes(nu, eqs_max_tiles(c.Ocap)));
        }
        // (and a stream that measures loudness behind that: the result tables hold every tile of every utterance's whole length)
        bf.ldst = nullptr; bf.ldsE = nullptr; bf.ldres = nullptr;
        if (oc.lst && !c.admission) {
            const int nu = c.join ? 1 : B;
            long long tiles = 0;
            if (c.join) tiles = lds_utt_tiles(out_count(c.FJ * hop));
            else if (!slot_state) for (int b = 0; b < B; b++) tiles += lds_utt_tiles(out_count((long long)p_lenF[b] * hop));
            if (!slot_state) bf.ldst = A.get<char>(lds_state_bytes(nu));
            bf.ldsE = (double*)A.get<char>(lds_ws_bytes(nu, lds_max_tiles(c.Ocap)));
            bf.ldres = A.get<char>(lds_res_bytes(nu, tiles));
        }
    };
    auto layoutF_all = [&](Arena& A) {
        layoutF(A);
        // (a run with a pitch plan: behind everything else, so that every other buffer lies where it lies without it)
        // (a stream: the warped windows of one step, each at most pitch_stream_cap samples and never more than its utterance's N')
        long long warped = c.pitch_total;
        if (warp) { warped = 0; for (int b = 0; b < B; b++) warped += std::min(c.pitch_nout[(size_t)b], pitch_stream_cap((long long)ss->chunk_frames + 2 * halo, hop)); }
        bf.wave_pitch = c.pitch ? A.get<float>((size_t)warped) : nullptr;
    };
    arenaF_.measuring = true; layoutF_all(arenaF_);
    if (!ensure(arenaF_, arenaF_.used + 4096)) return fail(STS_EDEVICE, "out of device memory (frame-level workspace)");
    arenaF_.measuring = false; layoutF_all(arenaF_);
    poison_arena(arenaF_);
    if ((oc.lws || oc.lst) && loud_cap_ < B) {      // host-mapped room for the results: the gating kernel writes them there, the run's last synchronisation covers them
        if (loud_host_) (void)hipHostFree(loud_host_);
        loud_host_ = nullptr; loud_dev_ = nullptr; loud_cap_ = 0;
        if (hipHostMalloc((void**)&loud_host_, (size_t)B * sizeof(sts_loudness), hipHostMallocMapped) != hipSuccess) { loud_host_ = nullptr; return fail(STS_EDEVICE, "pinned host allocation failed"); }
        if (hipHostGetDevicePointer((void**)&loud_dev_, loud_host_, 0) != hipSuccess) { (void)hipHostFree(loud_host_); loud_host_ = nullptr; return fail(STS_EDEVICE, "mapped pinned buffer has no device address"); }
        loud_cap_ = B;
    }
    if (oc.limws && lim_cap_ < B) {        // pinned room for the limiter's result words: downloaded behind its launch, the run's last synchronisation covers them
        if (lim_host_) { (void)hipStreamSynchronize(stream); (void)hipHostFree(lim_host_); }
        lim_host_ = nullptr; lim_cap_ = 0;
        if (hipHostMalloc((void**)&lim_host_, (size_t)B * 16, hipHostMallocDefault) != hipSuccess) { lim_host_ = nullptr; return fail(STS_EDEVICE, "pinned host allocation failed"); }
        lim_cap_ = B;
    }
    if (poison) {           // the host-visible outputs of this call, before the first kernel that writes them is enqueued
        if (host_pcm && !ss && pinned_pcm_) poison_host16(pinned_pcm_, std::min<size_t>((size_t)c.Ocap, pinned_pcm_cap_ / 2));
        if ((oc.lws || oc.lst) && loud_host_) poison_host32(loud_host_, (size_t)B * sizeof(sts_loudness) / 4);
        if (oc.limws && lim_host_) poison_host32(lim_host_, (size_t)B * 4);
    }

    Lvl& lv1 = c.lv1; lv1 = Lvl(); lv1.seg = (inl && !c.ahead) ? SegView{nullptr, nullptr, 1, 0, 0, p_lenF[0]} : SegView{d_offF, d_lenF, 1, 0, 0, 0};
    lv1.nb = B; lv1.max_len = maxF; lv1.total = Ftot; lv1.ld = Ftot;
    mark(7);
    return STS_OK;
}

// ---- stage 4: length regulator + reverse flow
int Engine::run_flow(RunCtx& c) {
    RUN_ALIASES(c)
    const long Fcount = c.Ftot;         // frames of the batch (taps); below, Ftot / maxF are the CAPACITY the buffers and launches are sized for
#define Ftot Fld
#define maxF maxFld
    // ---------------- length regulator (SynthesizerTrn.cpp:304-321, 380-383): z_p == m_expand, + eps * logs_expand * ns when sampling
    stage_begin(2);
    const PriorNoise pnz{c.any_ns ? bt.logs : nullptr, bt.ns, bt.seed};
    const int half = C / 2;
    if (use_ff) {
        expand_frames(bt.m, Ttot, bt.cum, lvT.seg, lv1.seg, C, bf.z, Ftot, B, maxF, stream, &pnz);
        tap("z_p", bf.z, C, Ftot, Fcount);
        const int G = ffG;
        const size_t hF = (size_t)half * Ftot;
        // where the newest version of each half of z lives: z itself, or the alternate buffer (a first layer that applies the previous
        // coupling's pending -m to its x0 half must not write over what its neighbours still read)
        const float* cur[2] = {bf.z, bf.z + hF};
        float* const home[2] = {bf.z, bf.z + hF};
        float* const alt[2] = {bf.ff_alt, bf.ff_alt + hF};
        int pend_set = -1, pend_half = -1;
        auto finish_half = [&](int hh, int set) {       // home[hh] = cur[hh] (+ the pending slices of `set`)
            FlowFinishArgs Fa;
            memset(&Fa, 0, sizeof(Fa));
            Fa.seg = lv1.seg; Fa.B = B; Fa.max_len = maxF; Fa.half = half;
            Fa.src = cur[hh]; Fa.src_ld = Ftot; Fa.dst = home[hh]; Fa.dst_ld = Ftot;
            Fa.macc = set >= 0 ? bf.ff_macc[set] : nullptr; Fa.n = set >= 0 ? G : 0; Fa.macc_stride = (long)hF;
            flow_finish(Fa, stream);
            cur[hh] = home[hh];
        };
        int cs = 0;
        for (int i = M.n_flows - 1; i >= 0; i--, cs ^= 1) {
            const DCoupling& cp = M.cp[i];
            const DWn& w = cp.wn;
            const DFlowFused& ff = cp.ff;
            const int x0h = cp.flipped ? 1 : 0, x1h = 1 - x0h;
            if (pend_set >= 0 && pend_half != x0h) { finish_half(pend_half, pend_set); pend_set = -1; }     // (couplings that do not alternate halves)
            if (w.has_cond) conv(w.cond, bt.g, lvB, bt.cond_wn, lvB, ConvOpt());
            (void)conv_args(cp.pre, nullptr, lv1, nullptr, lv1, ConvOpt(), nullptr);          // the stage's FLOP / byte account, as for the per-conv launches
            for (int l = 0; l < w.n; l++) {
                ConvOpt og; og.epi = EPI_GATE;
                (void)conv_args(w.in[l], nullptr, lv1, nullptr, lv1, og, nullptr);
                ConvOpt orr; orr.epi = EPI_RESSKIP;
                (void)conv_args(w.rs[l], nullptr, lv1, nullptr, lv1, orr, nullptr);
                FlowLayerArgs A;
                memset(&A, 0, sizeof(A));
                A.seg = lv1.seg; A.B = B; A.max_len = maxF; A.tot = Ftot;
                A.H = w.H; A.half = half; A.G = G; A.Cg = ff.Cg; A.k = w.in[l].k; A.halo = (w.in[l].k - 1) / 2;
                A.layer = l;
                if (l == 0) {
                    A.x0 = cur[x0h]; A.x0_ld = Ftot;
                    if (pend_set >= 0) {
                        A.pend = bf.ff_macc[pend_set]; A.pend_n = G; A.pend_stride = (long)hF;
                        A.x0_out = cur[x0h] == home[x0h] ? alt[x0h] : home[x0h]; A.x0_out_ld = Ftot;
                    }
                    A.w_pre = cp.pre.wh2; A.b_pre = cp.pre.bias; A.s_pre = cp.pre.h2_scale;
                    A.w_gate = ff.gate0; A.s_gate = ff.gate0_scale;
                } else {
                    A.h_in = bf.ff_h[(l - 1) & 1]; A.part_in = bf.ff_part[(l - 1) & 1]; A.part_n = G;
                    A.w_gate = w.in[l].wh2; A.s_gate = w.in[l].h2_scale;
                }
                A.part_stride = (long)((size_t)w.H * Ftot);
                A.h_out = bf.ff_h[l & 1]; A.part_out = bf.ff_part[l & 1];
                A.macc = bf.ff_macc[cs]; A.macc_stride = (long)hF; A.macc_init = l == 0;
                A.b_gate = w.in[l].bias;
                if (w.has_cond) { A.ubias = bt.cond_wn + (size_t)l * 2 * w.H * B; A.ubias_ld = B; }
                A.w_c = ff.wc[l]; A.s_c = ff.sc[l]; A.rows_c = ff.rows_c[l]; A.rows_res = ff.rows_res[l];
                A.b_res = ff.b_res[l]; A.b_m = ff.b_m;
                A.ovf = ovf_;
                flow_layer(A, stream, c.ffNT);
                if (l == 0 && pend_set >= 0) { cur[x0h] = A.x0_out; pend_set = -1; }
            }
            ConvOpt os; os.epi = EPI_SUB;
            (void)conv_args(cp.post, nullptr, lv1, nullptr, lv1, os, nullptr);
            pend_set = cs; pend_half = x1h;
        }
        if (pend_set >= 0) finish_half(pend_half, pend_set);
        for (int hh = 0; hh < 2; hh++) if (cur[hh] != home[hh]) finish_half(hh, -1);
    } else
    {
    expand_frames(bt.m, Ttot, bt.cum, lvT.seg, lv1.seg, C, bf.z, Ftot, B, maxF, stream, &pnz);
    tap("z_p", bf.z, C, Ftot, Fcount);

    // ---------------- reverse flow (ResidualCouplingBlock.cpp:59-70, ResidualCouplingLayer.cpp:47-66, WN.cpp:100-149)
    for (int i = M.n_flows - 1; i >= 0; i--) {
        const DCoupling& cp = M.cp[i];
        const float* x0 = bf.z + (size_t)(cp.flipped ? half : 0) * Ftot;
        float* dst = bf.z + (size_t)(cp.flipped ? 0 : half) * Ftot;
        const DWn& w = cp.wn;
        if (w.has_cond) conv(w.cond, bt.g, lvB, bt.cond_wn, lvB, ConvOpt());
        static const int flow_1x1_tile = exp_int("STS_FLOW_1X1_TILE", -1);   // experiment knob
        { ConvOpt op; op.tile = flow_1x1_tile; conv(cp.pre, x0, lv1, bf.h, lv1, op); }
        for (int l = 0; l < w.n; l++) {
            ConvOpt og; og.epi = EPI_GATE;
            if (w.has_cond) og.ubias = bt.cond_wn + (size_t)l * 2 * w.H * B;
            conv(w.in[l], bf.h, lv1, bf.acts, lv1, og);
            ConvOpt orr; orr.epi = EPI_RESSKIP; orr.epi_flag = l == 0 ? 1 : 0; orr.aux = bf.out; orr.tile = flow_1x1_tile;
            conv(w.rs[l], bf.acts, lv1, bf.h, lv1, orr);
        }
        ConvOpt os; os.epi = EPI_SUB; os.tile = flow_1x1_tile;
        conv(cp.post, bf.out, lv1, dst, lv1, os);
    }
    }
    if (M.n_flows & 1) flip_channels(bf.z, Ftot, C, Ftot, bf.fliptmp, stream);
    tap("z", bf.z, C, Ftot, Fcount);
    mark(3);
    return STS_OK;
#undef Ftot
#undef maxF
}

// The two-term fp16 arithmetic (conv_math 3) cannot hold an activation beyond fp16's range; its kernels raise a word in
// host-mapped memory when they stage one, and the whole utterance batch is then repeated in the split-bf16 form -- results never
// depend on the flag being rare.  A streaming call checks the word before each chunk leaves: raised during the first chunk (or
// before it: text encoder, flow) the call starts over, later only that chunk is decoded again -- split-bf16 from there on.
static constexpr int kRetrySplitBf16 = 1;     // run_once: nothing was handed out, repeat in the split-bf16 form
// An engine that had to repeat two calls in a row stays in the split-bf16 form (a model whose activations do not fit fp16 would
// otherwise pay for both forms on every call) until sts_set_conv_math is called again.
int Engine::run(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const StreamSpec* ss) {
    STS_NOT_WHILE_OPEN("a run");
    const int rc = run_any_math(B, ids, n, sid, ls, ss);
    pend.drop_call_tables();         // a table is for one call, whatever its outcome; the repeat inside the call above applied it again
    return rc;
}
// the overflow word of conv math 3 (host-mapped) and its device address, allocated by the first call that needs it
int Engine::ensure_overflow_word() {
    HIPCK(hipSetDevice(device));
    if (!ovf_host_) {
        if (hipHostMalloc((void**)&ovf_host_, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void**)&ovf_, ovf_host_, 0) != hipSuccess) {
            if (ovf_host_) (void)hipHostFree(ovf_host_);
            ovf_host_ = nullptr; ovf_ = nullptr;
            return fail(STS_EDEVICE, "host-mapped allocation failed");
        }
    }
    return STS_OK;
}
int Engine::run_any_math(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const StreamSpec* ss) {
    poison_bytes_ = 0;         // (a split-bf16 repeat lays the arenas out again and fills them again: both fills count)
    if (conv_math != 3) return run_once(B, ids, n, sid, ls, ss);
    if (h2_disabled) {
        conv_math = 0;
        const int rc0 = run_once(B, ids, n, sid, ls, ss);
        conv_math = 3;
        return rc0;
    }
    { const int rco = ensure_overflow_word(); if (rco != STS_OK) return rco; }
    *(volatile unsigned*)ovf_host_ = 0u;
    KeepForced keep_forced(pend);
    const long before = h2_fallbacks;
    int rc = run_once(B, ids, n, sid, ls, ss);
    if ((rc == STS_OK && !ss && *(volatile unsigned*)ovf_host_ != 0u) || rc == kRetrySplitBf16) {
        if (h2_fallbacks == 0)
            tts_log(TTS_LOG_WARNING, "summertts_hip: an activation left the fp16 range (|x| > 60000): this call is repeated in the split-bf16 form "
                                   "(same result, about twice the latency; sts_profile.conv_math_fallbacks counts these; STS_CONV_MATH=bf16x3 avoids them)\n");
        h2_fallbacks++;
        conv_math = 0;
        keep_forced.again();
        rc = run_once(B, ids, n, sid, ls, ss);
    }
    conv_math = 3;
    if (h2_fallbacks != before) {
        if (++h2_consecutive >= 2 && !h2_disabled) {
            h2_disabled = true;
            tts_log(TTS_LOG_WARNING, "summertts_hip: two calls in a row had to be repeated: this engine now stays in the split-bf16 form "
                                   "until sts_set_conv_math is called again (sts_profile.conv_math_pinned)\n");
        }
    } else h2_consecutive = 0;
    return rc;
}

int Engine::run_once(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const StreamSpec* ss) {
    Model& M = model;
    if (B <= 0 || !ids || !n) return fail(STS_EINVAL, "empty batch");
    if (ss && (ss->chunk_frames <= 0 || !ss->cb)) return fail(STS_EINVAL, "streaming takes a positive chunk size and a callback");
    HIPCK(hipSetDevice(device));
    taps.clear();
    memset(&prof, 0, sizeof(prof));
    for (double& f : flops_) f = 0;
    for (double& f : bytes_) f = 0;
    for (double& f : bytes_w_) f = 0;
    mfma_flops_ = 0; mfma_exec_ = 0; bf16_exec_ = 0; mfma_launches_ = 0; in_mfma_region_ = false;

    loud_res.clear(); loud_slots.clear(); lim_res.clear(); last_join_start.clear(); last_pitch_start.clear();
    if (ss && loud_mode != 0 && !loud_streaming)
        return fail(STS_EINVAL, "streaming is not available while loudness measurement or normalization is on (sts_set_loudness mode 0 first): "
                                "normalizing needs the whole utterance before its first sample leaves");
    if (ss && loud_mode == 2)
        return fail(STS_EINVAL, "streaming is not available while loudness is normalized (sts_set_loudness mode 2), also with "
                                "sts_set_loudness_streaming on: the gain needs the integrated loudness of the whole utterance before its first "
                                "sample leaves -- measure in a stream (mode 1), then set the limiter's gain (sts_set_limiter) for the next calls");
    if (ss && eq_n > 0 && !eq_streaming)
        return fail(STS_EINVAL, "streaming is not available while an equaliser is set (sts_set_eq with 0 bands first): an IIR has no finite "
                                "halo, and a state carried from chunk to chunk would make the PCM depend on the chunking -- unless the "
                                "carried-state stream mode is switched on (sts_set_eq_streaming)");
    if (eq_n > 0) { const int rce = eq_prepare(); if (rce != STS_OK) return rce; }
    host_t0_ = now_us(); host_t_sync_ = 0;
    RunCtx c;
    c.B = B; c.ids = ids; c.n = n; c.sid = sid; c.ls = ls; c.ss = ss; c.bstream = ss && B > 1;
    int rc;
    if ((rc = run_setup(c)) != STS_OK) return rc;
    mark(0);
    host_us_setup_ = (float)(now_us() - host_t0_); host_us_enq_ = 0;
    if ((rc = run_text_encoder(c)) != STS_OK) return rc;
    if ((rc = run_durations(c)) != STS_OK) return rc;
    if ((rc = run_frame_workspace(c)) != STS_OK) return rc;
    if ((rc = run_flow(c)) != STS_OK) return rc;
    return run_output(c);
}

// ---- stage 6: decode (one pass, or chunk by chunk when streaming), PCM to the host, profile
int Engine::run_output(RunCtx& c) {
    RUN_ALIASES(c)
    n_samples.resize(B);
    if (!ss) {
        // windows = utterances.  One utterance: by value when its frame count is known, from the device tables in a launch-ahead run
        int rc = run_decode(c, B, Fld, maxFld, 0, (B == 1 && !ahead) ? (int)Ftot : -1);
        if (rc != STS_OK) return rc;
        if (ahead) {
            // everything is enqueued.  The PCM download is queued for the CAPACITY (<= 63 frames more than needed) and the run's one
            // stream synchronisation happens before the count is looked at: the host never waits for the count by itself
            if (host_pcm && !pcm_in_host_) HIPCK(hipMemcpyAsync(pinned_pcm_, bf.pcm, (size_t)out_count((long long)Fld * hop) * 2, hipMemcpyDeviceToHost, stream));
            host_us_enq_ = (float)(now_us() - host_t0_);
            if ((rc = final_sync(c.Ttot)) != STS_OK) return rc;
            host_t_sync_ = now_us();
            if ((rc = wait_frame_counts(c)) != STS_OK) return rc;
            if ((c.Ftot + 63) / 64 * 64 != Fld) {
                // the count is not in the bucket this call was launched for (possible only when two requests share a hash): the output is
                // discarded, and flow + decoder run again the waiting way -- what a request returns does not depend on the engine's history
                ahead_misses++;
                HIPCK(hipStreamSynchronize(stream));
                c.ahead = false;
                flops_[2] = flops_[3] = bytes_[2] = bytes_[3] = bytes_w_[2] = bytes_w_[3] = 0;
                mfma_flops_ = 0; mfma_exec_ = 0; bf16_exec_ = 0; mfma_launches_ = 0; in_mfma_region_ = false;
                if ((rc = frame_geometry(c)) != STS_OK) return rc;
                if ((rc = run_frame_workspace(c)) != STS_OK) return rc;
                if ((rc = run_flow(c)) != STS_OK) return rc;
                return run_output(c);
            }
        }
    }
    const long Fcount = c.Ftot;                // (from here on: the real count)
    for (int b = 0; b < B; b++) n_samples[b] = (int32_t)out_count(c.pitch ? c.pitch_nout[(size_t)b] : (long long)p_lenF[b] * hop);     // (at the output rate)
    const int nres = c.join ? 1 : B;           // utterances the output side saw: a joined run's one signal
    if (c.join) n_samples.assign(1, (int32_t)out_count(c.FJ * hop));
    if (!ss) {
        d_pcm = bf.pcm;
        total_samples = 0;
        for (int b = 0; b < nres; b++) total_samples += n_samples[b];
        if (host_pcm) {
            if (!ahead && !pcm_in_host_) HIPCK(hipMemcpyAsync(pinned_pcm_, bf.pcm, (size_t)total_samples * 2, hipMemcpyDeviceToHost, stream));
            h_pcm = (const int16_t*)pinned_pcm_;
        }
        if (!ahead) {
            host_us_enq_ = (float)(now_us() - host_t0_);
            { const int rcs = final_sync(c.Ttot); if (rcs != STS_OK) return rcs; }
            host_t_sync_ = now_us();
        }
        if (c.ahead_b) {
            // a batch launched from the memo: the counts the durations kernel wrote (already on the host) must be the remembered ones
            const std::vector<long> pred = c.predF;
            int rc = wait_frame_counts(c);
            if (rc != STS_OK) return rc;
            bool same = true;
            for (int b = 0; b < B; b++) same = same && p_lenF[b] == (int)pred[b];
            c.ahead_b = false;
            if (!same) {
                ahead_misses++;
                flops_[2] = flops_[3] = bytes_[2] = bytes_[3] = bytes_w_[2] = bytes_w_[3] = 0;
                mfma_flops_ = 0; mfma_exec_ = 0; bf16_exec_ = 0; mfma_launches_ = 0; in_mfma_region_ = false;
                if ((rc = frame_geometry(c)) != STS_OK) return rc;
                if ((rc = run_frame_workspace(c)) != STS_OK) return rc;
                if ((rc = run_flow(c)) != STS_OK) return rc;
                return run_output(c);
            }
            prof.launch_ahead = 1;
        }
        HIPCK(hipGetLastError());
        if (loud_mode != 0) loud_res.assign((const sts_loudness*)loud_host_, (const sts_loudness*)loud_host_ + nres);   // (behind the run's last synchronisation)
        if (lim_mode != 0) { lim_res.resize(nres); limiter_stats_decode(lim_host_, nres, lim_res.data()); }
    } else {
        const int rc = run_stream_steps(c);
        if (rc != STS_OK) return rc;
        HIPCK(hipGetLastError());
    }
    const long Ntot = Fcount * hop;
    // one utterance: the launches were sized (and their FLOPs / bytes booked) for the frame capacity; the accounts report the real count
    if (Fld > 0 && Fld != Fcount) {
        const double r = (double)Fcount / (double)Fld;
        flops_[2] *= r; flops_[3] *= r; bytes_[2] *= r; bytes_[3] *= r; mfma_flops_ *= r; mfma_exec_ *= r; bf16_exec_ *= r;
    }
    for (int st = 0; st < 4; st++) bytes_[st] += bytes_w_[st];

    prof.frames = Fcount; prof.samples = Ntot; prof.phonemes = Ttot;
    prof.flops_text_encoder = flops_[0]; prof.flops_duration = flops_[1]; prof.flops_flow = flops_[2]; prof.flops_decoder = flops_[3];
    prof.flops_decoder_mfma = mfma_flops_; prof.decoder_mfma_launches = mfma_launches_; prof.bytes_decoder_min = bytes_[3] + 2.0 * (double)Ntot;
    prof.flops_decoder_mfma_executed = mfma_exec_; prof.flops_decoder_bf16_issued = bf16_exec_;
    prof.conv_math_fallbacks = h2_fallbacks; prof.conv_math_pinned = h2_disabled ? 1 : 0;
    prof.bytes_text_encoder = bytes_[0]; prof.bytes_duration = bytes_[1]; prof.bytes_flow = bytes_[2];
    prof.ms_sync_wait_host = (float)sync_wait_ms_; prof.launch_ahead = (ahead || prof.launch_ahead == 1) ? 1 : 0; prof.launch_ahead_misses = ahead_misses;
    if (profiling == 2) {
        float t = 0;
        (void)hipEventElapsedTime(&t, ev_[5], ev_[6]); prof.ms_decoder_mfma = t;
    } else if (profiling) {
        float t = 0;
        (void)hipEventElapsedTime(&t, ev_[0], ev_[1]); prof.ms_text_encoder = t;
        (void)hipEventElapsedTime(&t, ev_[1], ev_[2]); prof.ms_duration = t;
        (void)hipEventElapsedTime(&t, ev_[7], ev_[3]); prof.ms_flow = t;
        (void)hipEventElapsedTime(&t, ev_[3], ev_[4]); prof.ms_decoder = t;
        (void)hipEventElapsedTime(&t, ev_[5], ev_[6]); prof.ms_decoder_mfma = t;
        prof.ms_total_device = prof.ms_text_encoder + prof.ms_duration + prof.ms_flow + prof.ms_decoder;
    }
    prof.us_host_setup = host_us_setup_; prof.us_host_enqueue = host_us_enq_;
    prof.us_host_tail = host_t_sync_ > 0 ? (float)(now_us() - host_t_sync_) : 0.f;
    prof.poison_bytes = poison_bytes_;
    return STS_OK;
}

// ---- streaming (sts_infer_ids_stream, sts_infer_ids_batch_stream): step k decodes chunk k = frames [k C, min((k + 1) C, F_b))
// of every live utterance b as one window of a single decode pass -- the window [max(0, f0 - halo), min(F_b, f1 + halo)) at offF[b] + w0 of
// the packed z, the windows packed in utterance order.  The halo covers the decoder's receptive field, so the kept samples are computed from
// exactly the inputs the one-pass decode sees (bit-identical for a pinned kernel variant).  One kernel then gathers the windows' kept samples
// into one packed chunk buffer (stream_pack at the native rate, resample_pcm otherwise, the limiter behind either), one download (or posted
// writes into mapped pinned memory: stream_direct), one host synchronisation, and the step's chunks go to the caller in ascending utterance
// order before the next step is enqueued.  One utterance is the B == 1 case: its one window goes to run_decode by value, and at the native
// rate without a limiter nothing is packed -- the chunk is downloaded from where the decoder wrote it.
// (The tables of a step, their layout and the window geometry: stream_step.hpp, the one definition.)

// what the steps of one streaming call share
struct StreamRun {
    char* ht = nullptr;             // the step tables' pinned room
    int16_t* hp = nullptr;          // the step's packed chunks on the host
    // and on the device: written by the chain's writer when that is the resampler, the EQ or the limiter, else by stream_pack -- which
    // one utterance does without unless the chunks are to be stored into host memory
    int16_t* dst = nullptr;
    // the streamed EQ and streamed loudness: how far each utterance (a joined stream: J) is consumed and which state slot a step reads; the
    // slots flip only behind a step that does not run again.  Loudness: the call's result tables, which the gate reads behind the last step
    // (an open stream: its own tracks, by slot, which persist from step to step -- eqt / ldt name them; its result tables are its tile
    // pool's, and hu is pinned room behind the step tables for the gate's table of the step's retiring slots)
    EqsTrack eqt_call; LdsTrack ldt_call;
    EqsTrack* eqt = &eqt_call; LdsTrack* ldt = &ldt_call;
    double* ld_tsum = nullptr; float* ld_tpeak = nullptr; float* ld_gain = nullptr;
    long long* hu = nullptr;
};
// the windows the output side of a step sees: a plain step's nw decode windows, a joined step's one window of J
struct StreamTail {
    int n;
    const float* x; SegView seg;                    // what the resampler reads: the signal and the windows' places in it
    const int *pack_src, *pack_dst;                 // stream_pack's columns of the int block (a joined step: it never runs)
    size_t rs, lim, eq, loud;                       // their rows in the step's table (StepTab)
    long long max_rs, max_out, etiles, ltiles;      // launch dimensions (StepOut)
};

int Engine::run_stream_steps(RunCtx& c) {
    RUN_ALIASES(c)
    const long Cf = ss->chunk_frames;
    // one step of an open stream (stream_step): utterance b is the live slot c.live_slots[b] -- its z at its offset in the pool, its chunk
    // at its own next frame -- and the loop below runs once.  Everything else of a step is the closed call's
    LiveStream* const open = c.live;
    // one step of an open paragraph (para_step): joined AND open -- the plan's step c.para_k alone, every sentence's z at its place in the
    // pool; the step counter, the form-0 flag and the repeat of a step are the open stream's, the tables and launches the joined stream's
    const bool para = c.para_k >= 0;
    // (stream_host_buffers may move the pinned block the geometry tables live in)
    std::vector<int> offF, lenF, sidv;
    if (para) { offF.assign(c.para_zoff, c.para_zoff + c.js.s.size()); sidv.assign(c.para_sid, c.para_sid + c.js.s.size()); }
    else if (open) for (const int s : c.live_slots) { const LiveSlot& sl = open->slots[(size_t)s]; offF.push_back((int)sl.off); lenF.push_back((int)sl.F); sidv.push_back(sl.sid); }
    else { offF.assign(p_offF, p_offF + B); lenF.assign(p_lenF, p_lenF + B); sidv.assign(c.p_sid, c.p_sid + B); }
    const bool joined = c.join;       // a joined stream: the steps walk J, one chunk of the ONE signal per step (join_stream.hpp)
    const OutChain& oc = c.oc;
    StreamRun s;
    if (const int rc = stream_host_buffers(c, s)) return rc;
    c.d_win = (int*)bf.stab;
    StepCall call;
    call.C = Cf; call.halo = halo; call.hop = hop;
    call.srs = oc.run[OS_RESAMPLE]; call.slim = oc.run[OS_LIMIT]; call.seq = oc.eqst; call.sld = oc.lst; call.gain = c.gain; call.mix = c.mix;
    if (call.srs) { call.P = rs.P; call.Q = rs.Q; }
    if (call.slim) call.H = c.limd.H;
    call.lsrc = oc.src[OS_LOUD];
    const bool warp = c.pitch;      // a stream through the pitch warp (run_setup admits closed streams alone)
    if (warp) { call.pitch_words = c.pitch_words_h.data(); call.pitch_B = B; call.pitch_TT = c.pitch_rows; call.dec_halo = decoder_halo_frames(M); call.K = call.srs ? rs.K : 0; }
    std::vector<char> live(B, 1);
    if (ss->delivered) for (int b = 0; b < (joined ? 1 : B); b++) ss->delivered[b] = 0;
    d_pcm = nullptr; total_samples = 0;
    // an open stream with per-slot filter state (live_stream.hpp): positions and parity are the stream's, the rows name slots.  The one
    // parity is enough because every live slot has a window in this and every step
    const bool slot_eq = open && !para && open->eq_on && call.seq, slot_ld = open && !para && open->loud_on && call.sld;
    if (slot_eq) { s.eqt = &open->eqt; s.eqt->drop(); } else s.eqt->begin(joined ? 1 : B);
    if (call.sld && loud_k_rate_ != out_rate) {
        if (!loud_coef(out_rate, &loud_k_)) return fail(STS_EINVAL, "loudness: output rate outside [8000, 48000]");
        loud_k_rate_ = out_rate;
    }
    if (slot_ld) {      // the stream's result tables; of the step: the gate's table and gains
        s.ldt = &open->ldt; s.ldt->drop();
        s.ld_tsum = open->tsum; s.ld_tpeak = open->tpeak; s.ld_gain = (float*)(bf.ldres + (size_t)B * 3 * 8);
    } else if (call.sld) {     // the call's result tables, every utterance's tiles at its place
        const int nu = joined ? 1 : B;
        std::vector<long long> Nu(nu);
        if (joined) Nu[0] = out_count(c.FJ * hop);
        else for (int b = 0; b < B; b++) Nu[b] = out_count((long long)lenF[b] * hop);
        s.ldt->begin(nu);
        const long long tiles = s.ldt->layout(Nu.data());
        char* p = bf.ldres + (size_t)nu * 3 * 8;            // (in front: the gate's table {0, samples consumed, first tile} per utterance)
        s.ld_tsum = (double*)p; p += (size_t)tiles * kLdsSlots * 8;
        s.ld_tpeak = (float*)p; p += (size_t)tiles * 4;
        s.ld_gain = (float*)p;
    }
    std::vector<int> wb; std::vector<StepWin> win; StepOut st;
    std::vector<int> gated, stopped;                   // a measuring open stream: the slots this step's gate covers, those their callback stopped
    std::vector<std::pair<int, sts_loudness>> lres;
    const long jsteps = joined ? (long)c.js.steps() : 0;
    const long k_first = para ? (long)c.para_k : 0;
    for (long k = k_first;; k++) {
        // the utterances that get a chunk in this step (a joined stream: the one signal J; an open paragraph: its one step)
        wb.clear();
        if (joined) { if (para ? k == k_first : (k < jsteps && live[0])) wb.push_back(0); }
        else if (open) { if (k == 0) for (int b = 0; b < B; b++) wb.push_back(b); }      // (the one step: every live slot)
        else for (int b = 0; b < B; b++) if (live[b] && k * Cf < lenF[b]) wb.push_back(b);
        const int nu = (int)wb.size();
        if (nu == 0) break;
        // the step's tables (a joined step: of its own decode windows, none in a silence-only step, and of the one window of J)
        const char* bad;
        if (joined) bad = step_build_joined(call, c.js, k, offF.data(), sidv.data(), *s.eqt, *s.ldt, s.ht, st);
        else {
            win.clear();        // (an open stream: the slot's own next frame)
            for (const int b : wb) win.push_back(StepWin{b, lenF[b], open ? open->slots[(size_t)c.live_slots[b]].f : k * Cf, offF[b], sidv[b],
                                                         open && open->planned() ? c.live_slots[b] : -1, open ? c.live_slots[b] : -1});
            bad = step_build(call, win.data(), nu, *s.eqt, *s.ldt, s.ht, st);
        }
        if (bad) return fail(STS_EDEVICE, bad);
        const StepTab& t = st.tab;
        const int nw = st.nw;
        HIPCK(hipMemcpyAsync(c.d_win, s.ht, t.bytes, hipMemcpyHostToDevice, stream));
        // one decode over the windows (none: no decoder kernel).  One utterance: its window by value (no table load in the decoder's
        // kernels); several: the tables, also while one window is live (an open stream too: one form whatever the live count).
        // run_decode runs the chain up to the gain plan on the windows at their absolute positions
        if (nw > 0) {
            const int rc = B == 1 && !open && !warp ? run_decode(c, 1, st.Wtot, st.maxW, st.zoff0, st.wlen0) : run_decode(c, nw, st.Wtot, st.maxW, 0, -1);
            if (rc != STS_OK) return rc;
        }
        StreamTail tl{nw, c.stage_out(oc.src[OS_RESAMPLE]), SegView{c.d_win + StepTab::coff(nw), c.d_win + StepTab::wlen(nw), hop, 0, 0, 0},
                      c.d_win + StepTab::pack_src(nw), c.d_win + StepTab::pack_dst(nw), t.rs, t.lim, t.eq_rows, t.loud_rows,
                      st.max_rs, st.max_out, st.etiles, st.ltiles};
        if (warp) {         // the range warp over the step's windows; everything behind it sees window i as [yl0, yl1) of N' at its place in wave_pitch
            PitchArgs p{};
            pitch_args_carve(p, bt.pitch_words, B, c.pitch_rows);
            p.x = c.gain ? bf.wave_gain : bf.wave; p.y = bf.wave_pitch; p.pcm = oc.writer == OS_GAIN ? s.dst : nullptr; p.table = d_pitch_table_;
            p.rows = (const long long*)(bf.stab + t.ps_rows);
            pitch_range_run(p, nw, st.max_yl, stream);
            const int* seg = (const int*)(bf.stab + t.ps_seg);
            tl.x = bf.wave_pitch; tl.seg = SegView{seg, seg + nw, 1, 0, 0, 0};
            tl.pack_src = tl.pack_dst = nullptr;
        }
        if (joined) {       // the windowed join, then the output side on the one utterance J
            const JsStep& jt = st.jt;
            JoinWinArgs j{};
            j.x = c.stage_out(oc.src[OS_JOIN]); j.y = bf.wave_join; j.pcm = oc.writer == OS_JOIN ? s.dst : nullptr;
            j.rows = (const long long*)(bf.stab + t.j_rows);
            j.nw = nw; j.hop = hop; j.h = join_h;
            j.g0 = jt.g0 * hop; j.g1 = jt.g1 * hop; j.k0 = jt.f0 * hop; j.k1 = jt.f1 * hop;
            join_window_run(j, stream);
            tl.n = 1; tl.x = bf.wave_join; tl.seg = SegView{nullptr, nullptr, hop, 0, 0, (int)(jt.g1 - jt.g0)};
            tl.pack_src = tl.pack_dst = nullptr; tl.rs = t.j_rs; tl.lim = t.j_lim;
        }
        stream_tail(c, s, tl);
        if (slot_ld) {      // the gate over the slots this step retires behind their last chunk (known now), behind the loudness launches
            gated.clear();
            for (const int b : wb) { const LiveSlot& sl = open->slots[(size_t)c.live_slots[b]]; if (sl.f + Cf >= sl.F) gated.push_back(c.live_slots[b]); }
            for (size_t i = 0; i < gated.size(); i++) { s.hu[3 * i] = 0; s.hu[3 * i + 1] = s.ldt->pend[(size_t)gated[i]]; s.hu[3 * i + 2] = s.ldt->tbase[(size_t)gated[i]]; }
            if (const int rc = live_loud_gate(c, s, (int)gated.size())) return rc;
        }
        // where the step's chunks are on the device (nothing packed: the one window's kept samples, at its pack source in the decoder's own PCM)
        const int16_t* src = oc.chunk_in_place ? bf.pcm + st.src0 : s.dst;
        if (!stream_direct) HIPCK(hipMemcpyAsync(s.hp, src, (size_t)st.dsum * 2, hipMemcpyDeviceToHost, stream));
        HIPCK(hipStreamSynchronize(stream));
        // (an open stream: the hook counts its steps since open; an overflow repeats this step alone -- the earlier steps' chunks have left,
        // the stream stays in form 0 until it is closed, and stream_step restores the setting)
        if (conv_math == 3 && ((ovf_host_ && *(volatile unsigned*)ovf_host_ != 0u) || (stream_retry_step >= 0 && (open ? open->steps : (long long)k) == stream_retry_step))) {
            if (k == 0 && !open) return kRetrySplitBf16;  // nothing has left yet (run() repeats the call)
            if (open) open->form0 = true;
            h2_fallbacks++;
            conv_math = 0;                                 // (run() restores the setting)
            k--;                                           // this step again, every window of it
            s.eqt->drop();                                 // (from the state the first attempt started from)
            if (call.sld) s.ldt->drop();
            continue;
        }
        s.eqt->commit();
        if (call.sld) s.ldt->commit();
        if (slot_ld) { lres.clear(); stopped.clear(); for (size_t i = 0; i < gated.size(); i++) lres.emplace_back(gated[i], ((const sts_loudness*)loud_host_)[i]); }
        for (int i = 0; i < nu; i++) {                     // ascending utterance order
            const int b = wb[i];
            const int16_t* pcm = s.hp + st.dst[i];
            const int32_t n = (int32_t)st.n[i], j0 = (int32_t)st.j0[i];
            if (warp && n == 0) continue;                  // (a chunk of one sample may own no warped output: not delivered)
            total_samples += st.n[i];
            if (ss->delivered) ss->delivered[b] += n;
            if (open && !para) {       // (utt = the slot; it moves on by a chunk, and retires behind its last one or at its stop)
                const int sl = c.live_slots[b];
                const bool stop = ss->cb(ss->user, sl, pcm, n, j0) != 0;
                if (slot_ld && stop && std::find(gated.begin(), gated.end(), sl) == gated.end()) stopped.push_back(sl);
                open->delivered(sl, stop);
            } else if (para) {       // (the one signal; para_step moves the paragraph on)
                c.para_stop = ss->cb(ss->user, 0, pcm, n, j0) != 0;
            } else if (ss->cb(ss->user, b, pcm, n, j0) != 0) live[b] = 0;
        }
    }
    if (slot_ld) {
        // a slot its callback stopped is gated over what it delivered, as a closed stream's utterance is -- known only behind the step's
        // synchronisation, so these (rare) slots cost a launch and a synchronisation of their own
        if (!stopped.empty()) {
            for (size_t i = 0; i < stopped.size(); i++) { s.hu[3 * i] = 0; s.hu[3 * i + 1] = s.ldt->e[(size_t)stopped[i]]; s.hu[3 * i + 2] = s.ldt->tbase[(size_t)stopped[i]]; }
            if (const int rc = live_loud_gate(c, s, (int)stopped.size())) return rc;
            HIPCK(hipStreamSynchronize(stream));
            for (size_t i = 0; i < stopped.size(); i++) lres.emplace_back(stopped[i], ((const sts_loudness*)loud_host_)[i]);
            std::sort(lres.begin(), lres.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        }
        for (const auto& r : lres) { loud_slots.push_back(r.first); loud_res.push_back(r.second); }
        return STS_OK;
    }
    return call.sld ? stream_loud_gate(c, s) : STS_OK;
}

// the host side of a stream's steps: room for the step tables behind the geometry tables in the pinned block, and the chunks' buffer
// behind that -- or, with posted writes, in mapped pinned memory of its own, which the last kernel of a step stores the chunks into itself
int Engine::stream_host_buffers(RunCtx& c, StreamRun& s) {
    RUN_ALIASES(c)
    const size_t hp_off = (up_bytes + ((size_t)Ttot + B) * 4 + 255) & ~(size_t)255;
    const size_t tab_only = (StepTab(B, c.gain, c.oc.eqst, c.oc.lst, c.join, c.pitch).bytes + 255) & ~(size_t)255;
    const size_t tab_room = tab_only + (c.live && c.oc.lst ? ((size_t)B * 3 * 8 + 255) & ~(size_t)255 : 0);     // (an open stream: the gate's table)
    const size_t pcm_bytes = (size_t)c.Ocap * 2 + 256;
    if (!ensure_pinned(hp_off + tab_room + pcm_bytes)) return fail(STS_EDEVICE, "pinned host allocation failed");
    c.pm = (int*)pinned_;
    s.ht = pinned_ + hp_off;
    s.hu = (long long*)(s.ht + tab_only);
    s.hp = (int16_t*)(pinned_ + hp_off + tab_room);
    s.dst = c.oc.run[OS_PACK] ? bf.spack : bf.pcm;
    if (stream_direct) {
        if (pcm_bytes > pinned_pcm_cap_ || !pinned_pcm_dev_) {
            (void)hipStreamSynchronize(stream);
            if (pinned_pcm_) (void)hipHostFree(pinned_pcm_);
            pinned_pcm_ = nullptr; pinned_pcm_cap_ = 0; pinned_pcm_dev_ = nullptr;
            if (hipHostMalloc((void**)&pinned_pcm_, pcm_bytes, hipHostMallocMapped) != hipSuccess) return fail(STS_EDEVICE, "pinned host allocation failed");
            pinned_pcm_cap_ = pcm_bytes;
            if (hipHostGetDevicePointer((void**)&pinned_pcm_dev_, pinned_pcm_, 0) != hipSuccess) { pinned_pcm_dev_ = nullptr; return fail(STS_EDEVICE, "mapped pinned buffer has no device address"); }
        }
        s.dst = pinned_pcm_dev_; s.hp = (int16_t*)pinned_pcm_;
    }
    poison_host16(s.hp, (size_t)c.Ocap);
    return STS_OK;
}

// a step's launches behind the decoder (a joined step: behind the windowed join): resample or pack, the EQ and loudness from their carried
// states, the limiter -- every window in one launch each, the chain's writer storing the packed chunks
void Engine::stream_tail(RunCtx& c, const StreamRun& s, const StreamTail& t) {
    const OutChain& oc = c.oc;
    const BufF& bf = c.bf;
    if (oc.run[OS_RESAMPLE]) {
        ResampleArgs a{};
        a.x = t.x; a.seg = t.seg;
        a.table = d_rs_table; a.P = rs.P; a.Q = rs.Q; a.K = rs.K;
        a.pcm = oc.writer == OS_RESAMPLE ? s.dst : bf.pcm_rs; a.wave_out = bf.wave_out;
        a.wtab = (const long long*)(bf.stab + t.rs);
        resample_pcm(a, t.n, t.max_rs, stream);
    } else if (oc.run[OS_PACK]) {
        stream_pack(bf.pcm, s.dst, t.pack_src, t.pack_dst, t.n, t.max_out, stream);
    }
    if (oc.eqst) {          // its two launches follow the resampler
        EqArgs a{};
        a.x = c.stage_out(oc.src[OS_EQ]); a.S = c.eqS; a.tab = d_eq_;
        a.y = bf.wave_eq; a.pcm = oc.writer == OS_EQ ? s.dst : nullptr;
        a.E = bf.eqsE; a.state = bf.eqst; a.slot = s.eqt->slot; a.wtab = (const long long*)(bf.stab + t.eq);
        eq_stream_run(a, t.n, t.etiles, stream);
    }
    if (oc.lst) {           // its two launches follow the stage it reads: the nearest running float stage in front of it
        LoudStreamArgs a{};
        a.x = c.stage_out(oc.src[OS_LOUD]); a.k = loud_k_;
        a.wtab = (const long long*)(bf.stab + t.loud); a.state = bf.ldst; a.slot = s.ldt->slot;
        a.E = bf.ldsE; a.tsum = s.ld_tsum; a.tpeak = s.ld_tpeak;
        loud_stream_run(a, t.n, t.ltiles, stream);
    }
    if (oc.run[OS_LIMIT]) { // it writes the packed chunks in place of the resampler / the pack
        LimArgs a{};
        a.x = c.pitch && oc.src[OS_LIMIT] == OS_GAIN ? bf.wave_pitch : c.stage_out(oc.src[OS_LIMIT]);     // (a warped step: the plan stage's output is the warp's)
        a.H = c.limd.H; a.c = c.limd.c; a.G = c.limd.G;
        a.pcm = s.dst;
        a.wtab = (const long long*)(bf.stab + t.lim);
        limiter_run(a, t.n, t.max_out, stream);
    }
}

// the gate, once, on what every utterance delivered: its results go to the host-mapped block, this synchronisation covers them
int Engine::stream_loud_gate(RunCtx& c, StreamRun& s) {
    const int nu = c.join ? 1 : c.B;
    long long* hu = (long long*)s.ht;                       // (the step tables' pinned room: every upload from it has completed)
    for (int b = 0; b < nu; b++) { hu[3 * b] = 0; hu[3 * b + 1] = s.ldt->e[b]; hu[3 * b + 2] = s.ldt->tbase[b]; }
    HIPCK(hipMemcpyAsync(c.bf.ldres, hu, (size_t)nu * 3 * 8, hipMemcpyHostToDevice, stream));
    LoudArgs g{};
    g.k = loud_k_; g.target = loud_target; g.ceiling = loud_peak; g.no_clamp = c.oc.loud_no_clamp;
    g.utab = (long long*)c.bf.ldres; g.tsum = s.ld_tsum; g.tpeak = s.ld_tpeak; g.gain = s.ld_gain; g.out = loud_dev_;
    loud_gate_run(g, nu, stream);
    HIPCK(hipStreamSynchronize(stream));
    loud_res.assign((const sts_loudness*)loud_host_, (const sts_loudness*)loud_host_ + nu);
    return STS_OK;
}

// a measuring open stream's gate over n slots of a step (their rows {0, samples consumed, first tile} at s.hu): results to the host-mapped
// block in that order, covered by the next synchronisation
int Engine::live_loud_gate(RunCtx& c, StreamRun& s, int n) {
    if (n <= 0) return STS_OK;
    HIPCK(hipMemcpyAsync(c.bf.ldres, s.hu, (size_t)n * 3 * 8, hipMemcpyHostToDevice, stream));
    LoudArgs g{};
    g.k = loud_k_; g.target = loud_target; g.ceiling = loud_peak; g.no_clamp = c.oc.loud_no_clamp;
    g.utab = (long long*)c.bf.ldres; g.tsum = s.ld_tsum; g.tpeak = s.ld_tpeak; g.gain = s.ld_gain; g.out = loud_dev_;
    loud_gate_run(g, n, stream);
    return STS_OK;
}

int Engine::run_batch_stream(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, int chunk_frames,
                             int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* n_total) {
    if (B < 1 || !ids || !n || chunk_frames <= 0 || !cb) return fail(STS_EINVAL, "batched streaming takes B >= 1 utterances, a positive chunk size and a callback");
    std::vector<int32_t> got(B, 0);
    StreamSpec ss{chunk_frames, cb, user, got.data()};
    const int rc = run(B, ids, n, sid, ls, &ss);
    if (rc == STS_OK && n_total) for (int b = 0; b < B; b++) n_total[b] = got[b];
    return rc;
}

int Engine::run_joined_stream(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const sts_join* join,
                              int chunk_frames, int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* n_total) {
    if (B < 1 || !ids || !n || chunk_frames <= 0 || !cb) return fail(STS_EINVAL, "a joined stream takes B >= 1 sentences, a positive chunk size and a callback");
    int32_t got = 0;
    StreamSpec ss{chunk_frames, cb, user, &got};
    const int rc = run_joined(B, ids, n, sid, ls, join, &ss);
    if (rc == STS_OK && n_total) *n_total = got;
    return rc;
}

// ---- open streams (engine.hpp stream_open; live_stream.hpp; DESIGN.md 9c "Open streams").  Between two steps the engine keeps: z of every
// live utterance in the pool, the slot table {pool offset, F, sid, next frame}, the free column ranges, the step count and the form-0
// flag -- and, in a planned stream, each slot's conditioning vector, a gain-planned slot's phoneme columns and slot words, and the free
// phoneme ranges.  Nothing in the arenas survives a step: every step and every admission lays its workspace out again.
int Engine::stream_open(int chunk_frames, int max_live, long long capacity_frames, long long capacity_phonemes) {
    if (live_) return fail(STS_ESTATE, "a stream is already open on this engine (sts_stream_close first)");
    if (para_) return fail(STS_ESTATE, "a paragraph is open on this engine (sts_para_close first)");
    const Model& M = model;
    if (chunk_frames <= 0 || max_live < 1 || max_live > 1024 || capacity_frames < 1)
        return fail(STS_EINVAL, "an open stream takes a positive chunk size, 1 <= max_live <= 1024 and a positive capacity");
    if (capacity_phonemes < 0 || capacity_phonemes > (1 << 24)) return fail(STS_EINVAL, "an open stream's capacity_phonemes is 0 (no tables) or in [1, 2^24]");
    if ((double)capacity_frames * M.inter > 2.0e9 || (double)capacity_frames * M.hop_total > 2.0e9)
        return fail(STS_EINVAL, "an open stream's capacity_frames * inter_channels and capacity_frames * samples_per_frame may not exceed 2 10^9");
    // (with their stream modes on, the EQ and loudness mode 1 run from per-slot state: the pools below.  Mode 2 needs the whole utterance)
    if (eq_n > 0 && !eq_streaming) return fail(STS_EINVAL, "an open stream is not available while an equaliser is set: its state is carried per utterance in the frame arena");
    if (loud_mode == 2 || (loud_mode != 0 && !loud_streaming)) return fail(STS_EINVAL, "an open stream is not available while loudness measurement or normalization is on: its state is carried per utterance in the frame arena");
    if (record_taps) return fail(STS_EINVAL, "an open stream is not available while taps are recorded");
    if (refuse_pitch("an open stream")) return STS_EINVAL;
    if (pend.have_plan || pend.have_mix || pend.have_gain || pend.have_forced)
        return fail(STS_EINVAL, "an open stream is not available while a duration plan, a speaker mix, a gain plan or forced durations are pending: their tables are per call");
    HIPCK(hipSetDevice(device));
    LimiterDesign d{};
    if (lim_mode != 0 && !limiter_design(out_rate, lim_gain_db, lim_ceiling, lim_ms, &d)) return fail(STS_EINVAL, "limiter: output rate outside [8000, 48000]");
    if (conv_math == 3) { const int rc = ensure_overflow_word(); if (rc != STS_OK) return rc; }
    if (eq_n > 0) { const int rc = eq_prepare(); if (rc != STS_OK) return rc; }     // (the rate and the bands are fixed from here to close)
    LiveStream* L = new (std::nothrow) LiveStream();
    if (!L) return fail(STS_EDEVICE, "out of host memory");
    L->open(chunk_frames, max_live, capacity_frames, capacity_phonemes);
    L->halo = stream_halo(); L->hop = M.hop_total;
    L->P = resampling() ? rs.P : 1; L->Q = resampling() ? rs.Q : 1; L->H = lim_mode != 0 ? d.H : 0;
    L->form0 = conv_math == 3 && h2_disabled;
    // (a KB of slack behind the last row: a kernel that stages z in whole vectors may read past a row's last column, as in the arena)
    const size_t pool_bytes = ((size_t)M.inter * (size_t)capacity_frames + 256) * sizeof(float);
    // (a planned stream: the adoption table of its pools rides behind adopt_z's in the same block)
    const bool planned = capacity_phonemes > 0;
    const size_t tab_bytes = planned ? adopt_tables_tab_off(max_live) + adopt_tables_tab_bytes(max_live) : adopt_tab_bytes(max_live);
    if (hipMalloc((void**)&L->zpool, pool_bytes) != hipSuccess || hipMalloc(&L->tab_dev, tab_bytes) != hipSuccess ||
        hipHostMalloc(&L->tab_host, tab_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (L->zpool) (void)hipFree(L->zpool);
        if (L->tab_dev) (void)hipFree(L->tab_dev);
        delete L;
        return fail(STS_EDEVICE, "out of device memory (the open stream's latent pool)");
    }
    if (poison && hipMemsetD32Async((hipDeviceptr_t)L->zpool, (int)poison, pool_bytes / 4, stream) != hipSuccess) (void)hipGetLastError();
    live_ = L;
    loud_res.clear(); loud_slots.clear();       // (sts_stream_get_loudness: nothing has retired in this stream)
    // per-slot filter state (live_stream.hpp), for the stages that are on only: the EQ's and loudness' carried states, two state slots per
    // stream slot, and loudness' result tables over the tile pool -- [eqst | ldst | tsum | tpeak] in one allocation (an open costs the
    // pool's group its first chunk).  Nothing is cleared, here or at an admission: a slot's first step reads no state (e == 0)
    const bool feq = eq_n > 0, fld = loud_mode == 1;
    if (feq || fld) {
        L->open_filters(feq, fld);
        const size_t eb = feq ? eqs_state_bytes(max_live) : 0, lb = fld ? lds_state_bytes(max_live) : 0;
        const size_t sb = (size_t)L->capacity_tiles * kLdsSlots * 8, pb = ((size_t)L->capacity_tiles * 4 + 255) & ~(size_t)255;
        bool ok = hipMalloc(&L->filters_dev, eb + lb + sb + pb) == hipSuccess;
        if (ok) {
            char* p = (char*)L->filters_dev;
            if (feq) L->eqst = p;
            if (fld) { L->ldst = p + eb; L->tsum = (double*)(p + eb + lb); L->tpeak = (float*)(p + eb + lb + sb); }
        }
        if (ok && poison) ok = hipMemsetD32Async((hipDeviceptr_t)L->filters_dev, (int)poison, (eb + lb + sb + pb) / 4, stream) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)stream_close();        // (frees whatever was allocated)
            return fail(STS_EDEVICE, "out of device memory (the open stream's filter state)");
        }
    }
    if (!planned) return STS_OK;
    // the planned stream's pools: each slot's conditioning vector [gin][max_live] (a multi-speaker model with a conditioned decoder only),
    // the phoneme pool [cum | q][capacity_phonemes + 1] (the last column: the shared neutral row), the slot words [off | n | h][max_live]
    const bool has_g = M.is_ms == 1 && M.dec_type == 0 && M.gin > 0;
    const size_t g_words = has_g ? (size_t)M.gin * (size_t)max_live : 0;
    const size_t p_words = 2 * ((size_t)capacity_phonemes + 1), s_words = 3 * (size_t)max_live;
    bool ok = hipMalloc(&L->tables_dev, (g_words + p_words + s_words) * 4) == hipSuccess;       // (one allocation: an open costs the pool's group)
    if (ok) {
        if (has_g) L->gpool = (float*)L->tables_dev;
        L->ppool = (int*)L->tables_dev + g_words; L->swords = L->ppool + p_words;
    }
    if (ok && poison) ok = hipMemsetD32Async((hipDeviceptr_t)L->tables_dev, (int)poison, g_words + p_words + s_words, stream) == hipSuccess;
    if (ok) {    // the neutral row, behind the fill: cum 0 (no phoneme owns a frame: Q == 2^20 everywhere), q 2^20
        static const int neutral[2] = {0, kGainOne};
        ok = hipMemcpy2DAsync(L->ppool + capacity_phonemes, ((size_t)capacity_phonemes + 1) * 4, neutral, 4, 4, 2, hipMemcpyHostToDevice, stream) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        (void)stream_close();        // (frees whatever was allocated)
        return fail(STS_EDEVICE, "out of device memory (the planned stream's pools)");
    }
    return STS_OK;
}

int Engine::stream_close() {
    if (!live_) return fail(STS_ESTATE, "no stream is open on this engine");
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (live_->zpool) (void)hipFree(live_->zpool);
    if (live_->tables_dev) (void)hipFree(live_->tables_dev);
    if (live_->filters_dev) (void)hipFree(live_->filters_dev);
    if (live_->tab_dev) (void)hipFree(live_->tab_dev);
    if (live_->tab_host) (void)hipHostFree(live_->tab_host);
    delete live_;
    live_ = nullptr;
    loud_res.clear(); loud_slots.clear();       // (a stream's results end with it)
    return STS_OK;
}

// front and flow of the B newcomers in the arithmetic conv_math names, their slots and columns, their z into the pool.  kRetrySplitBf16:
// the overflow word was raised (conv math 3) -- nothing of the admission is kept, the caller repeats it in form 0
int Engine::stream_admit_once(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, int32_t* slot_out,
                              int32_t* n_samples_out, int32_t* admitted) {
    LiveStream& L = *live_;
    Model& M = model;
    const bool guarded = conv_math == 3;
    if (guarded) *(volatile unsigned*)ovf_host_ = 0u;
    poison_bytes_ = 0;
    host_t0_ = now_us(); host_t_sync_ = 0;
    StreamSpec ss{L.chunk, [](void*, int32_t, const int16_t*, int32_t, int32_t) { return 0; }, nullptr};
    RunCtx c;
    c.B = B; c.ids = ids; c.n = n; c.sid = sid; c.ls = ls; c.ss = &ss; c.bstream = B > 1;
    c.admission = true;                                        // (no output stage runs: the frame workspace holds nothing of the filters)
    int rc;
    if ((rc = run_setup(c)) != STS_OK) return rc;
    mark(0);
    if ((rc = run_text_encoder(c)) != STS_OK) return rc;
    if ((rc = run_durations(c)) != STS_OK) return rc;          // (a stream never launches ahead: the frame counts are on the host)
    std::vector<long> F((size_t)B); std::vector<int> sidv((size_t)B), slots((size_t)B, -1), nph((size_t)B, 0);
    for (int b = 0; b < B; b++) { F[(size_t)b] = c.p_lenF[b]; sidv[(size_t)b] = c.p_sid[b]; }
    // (a planned stream: an utterance whose gain plan came with gain_db takes n[b] columns of the phoneme pool; room is decided over all three)
    if (c.gain) for (int b = 0; b < B; b++) nph[(size_t)b] = pend.gain_has[(size_t)b] ? n[b] : 0;
    if (!L.admit(B, F.data(), sidv.data(), nph.data(), slots.data())) {    // no room now: the front work is lost, nothing has changed
        HIPCK(hipStreamSynchronize(stream));
        *admitted = 0;
        return STS_OK;
    }
    auto undo = [&](int code) { for (const int s : slots) if (s >= 0) { L.retire(s); L.admitted--; L.retired--; } return code; };
    if ((rc = run_frame_workspace(c)) != STS_OK) return undo(rc);
    if ((rc = run_flow(c)) != STS_OK) return undo(rc);
    // z of the newcomers leaves the arena: one table upload, one launch
    long long* const tab = (long long*)L.tab_host;
    int* const tlen = (int*)(tab + 2 * (size_t)B);
    for (int b = 0; b < B; b++) {
        tab[b] = c.p_offF[b]; tab[B + b] = slots[(size_t)b] >= 0 ? L.slots[(size_t)slots[(size_t)b]].off : 0;
        tlen[b] = slots[(size_t)b] >= 0 ? (int)F[(size_t)b] : 0;
    }
    size_t tab_bytes = adopt_tab_bytes(B);
    int max_n = 0;
    if (L.planned()) {      // the pools' table behind it, in the same upload: {slot, toff, n, poff, h} per newcomer
        int* const t5 = (int*)((char*)L.tab_host + adopt_tables_tab_off(B));
        for (int b = 0; b < B; b++) {
            const int s = slots[(size_t)b];
            const LiveSlot* sl = s >= 0 ? &L.slots[(size_t)s] : nullptr;
            const bool g = sl && sl->has_gain;
            t5[5 * b] = s; t5[5 * b + 1] = c.offT[(size_t)b]; t5[5 * b + 2] = g ? sl->pn : 0; t5[5 * b + 3] = g ? (int)sl->poff : 0;
            t5[5 * b + 4] = g ? pend.gain_words[(size_t)c.Ttot + (size_t)b] : 0;
            if (g) max_n = std::max(max_n, sl->pn);
        }
        tab_bytes = adopt_tables_tab_off(B) + adopt_tables_tab_bytes(B);
    }
    if (hipMemcpyAsync(L.tab_dev, tab, tab_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return undo(fail(STS_EDEVICE, "the adoption table's upload failed"));
    adopt_z(c.bf.z, c.Fld, L.zpool, L.capacity, c.C, (const long long*)L.tab_dev, B, c.maxF, stream);
    if (L.planned()) {      // every newcomer's column of gpool (mixed or plain: bt.g is the blend or the gather), a gain-planned one's cum / q / words
        AdoptTablesArgs a{};
        a.g = c.bt.g; a.gpool = L.gpool; a.gin = M.gin; a.B = B; a.max_live = L.max_live;
        a.cum = c.bt.cum; a.q = c.bt.gain_q;
        a.pool = L.ppool; a.ld_pool = L.capacity_phonemes + 1; a.swords = L.swords; a.neutral = (int)L.capacity_phonemes;
        a.tab = (const int*)((const char*)L.tab_dev + adopt_tables_tab_off(B));
        adopt_tables(a, max_n, stream);
    }
    if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return undo(fail(STS_EDEVICE, "the admission failed on the device"));
    if (guarded && (*(volatile unsigned*)ovf_host_ != 0u || stream_retry_step == -2)) return undo(kRetrySplitBf16);      // (-2, tests: every admission counts as raised)
    last_join_start.clear();    // (sts_get_durations / sts_get_phoneme_offsets report this admission's utterances, packed, as after a batch stream)
    n_samples.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        n_samples[(size_t)b] = (int32_t)out_count((long long)F[(size_t)b] * c.hop);
        if (slot_out) slot_out[b] = slots[(size_t)b];
        if (n_samples_out) n_samples_out[b] = n_samples[(size_t)b];
    }
    *admitted = B;
    return STS_OK;
}

int Engine::stream_admit(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const sts_stream_noise* nz,
                         int32_t* slot_out, int32_t* n_samples_out, int32_t* admitted) {
    if (!live_) return fail(STS_ESTATE, "no stream is open on this engine (sts_stream_open first)");
    if (refuse_pitch("an admission into an open stream")) { drop_tables(); if (admitted) *admitted = 0; return STS_EINVAL; }
    // (a planned stream: the pending tables are for this admission only, whatever its outcome -- no room and a failure included; dropped
    // here, behind the last attempt, so that the form-0 repeat below applies them again)
    struct Drop { Engine& e; ~Drop() { e.drop_tables(); } } drop{*this};
    if (!admitted) return fail(STS_EINVAL, "an admission needs the `admitted` output");
    *admitted = 0;
    LiveStream& L = *live_;
    if (B < 1 || !ids || !n) return fail(STS_EINVAL, "an admission takes B >= 1 utterances with ids and n");
    if (B > L.max_live) return fail(STS_EINVAL, "an admission of more utterances than the stream's max_live can never fit");
    for (int b = 0; nz && b < B; b++)
        if (!noise_scale_valid(nz[b].noise_scale) || !noise_scale_valid(nz[b].noise_scale_w)) return fail(STS_EINVAL, "noise scales must be finite and >= 0");
    if (L.free_slots() < B) return STS_OK;                     // (no room now, known before any front work)
    HIPCK(hipSetDevice(device));
    std::vector<Noise> keep; keep.swap(noise_utt);             // (NULL: run_setup takes the engine's setting with seed + b)
    if (nz) for (int b = 0; b < B; b++) noise_utt.push_back(Noise{nz[b].noise_scale, nz[b].noise_scale_w, nz[b].seed});
    const int math = conv_math;
    if (math == 3 && L.form0) conv_math = 0;
    KeepForced keep_forced(pend);
    int rc = stream_admit_once(B, ids, n, sid, ls, slot_out, n_samples_out, admitted);
    if (rc == kRetrySplitBf16) {                               // this admission alone: nothing of the newcomers has been delivered
        h2_fallbacks++;
        conv_math = 0;
        keep_forced.again();
        rc = stream_admit_once(B, ids, n, sid, ls, slot_out, n_samples_out, admitted);
    }
    conv_math = math;
    noise_utt.swap(keep);
    prof.conv_math_fallbacks = h2_fallbacks;
    return rc;
}

int Engine::stream_step(int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* live_after) {
    if (!live_) return fail(STS_ESTATE, "no stream is open on this engine (sts_stream_open first)");
    if (!cb) return fail(STS_EINVAL, "a step takes a callback");
    LiveStream& L = *live_;
    Model& M = model;
    if (live_after) *live_after = L.live_count();
    if (L.live_count() == 0) return STS_OK;
    HIPCK(hipSetDevice(device));
    StreamSpec ss{L.chunk, cb, user};
    RunCtx c;
    L.step_slots(c.live_slots);
    c.live = &L;
    const int B = c.B = (int)c.live_slots.size();
    c.ss = &ss; c.bstream = true;                              // (a window's index is never its utterance's: the conditioning is gathered per window)
    c.bt = BufT{}; c.bf = BufF{};
    c.ms = M.is_ms == 1; c.H = M.hidden; c.C = M.inter; c.hop = M.hop_total;
    c.wnH = M.n_flows ? M.cp[0].wn.H : 0; c.wnL = M.n_flows ? M.cp[0].wn.n : 0;
    // the decode workspace of this step's windows (transient: laid out per step; ensure() synchronises before it moves the arena).  The
    // flow's buffers are those of one frame -- no flow runs here -- and z is the pool
    std::vector<int> lenF((size_t)B), offF((size_t)B, 0);
    for (int b = 0; b < B; b++) lenF[(size_t)b] = (int)L.slots[(size_t)c.live_slots[(size_t)b]].F;
    c.p_lenF = lenF.data(); c.p_offF = offF.data();
    c.Ftot = c.Fld = 1; c.maxF = c.maxFld = 1;
    if (L.planned()) {
        // the gain stage runs in a step in which a live slot carries a gain plan, and only then (the chain is planned per step); the kernel
        // reads the stream's pools by slot -- utt[m] = the window's slot, the slot words as its segment table.  The windows of slots
        // without a plan read the shared neutral row (their words name it: n = 1, cum 0, q 2^20, h 0 -- env == 1.0f at every sample)
        c.gain = L.any_gain();
        c.lvT.seg = SegView{L.swords, L.swords + L.max_live, 1, 0, 0, 0};
        c.bt.cum = L.ppool; c.bt.gain_q = L.ppool + (L.capacity_phonemes + 1); c.bt.gain_h = L.swords + 2 * (size_t)L.max_live;
        // each window's conditioning: column `slot` of gpool (run_decode's gather with gpool as the table, as a closed stream's with bt.g)
        c.mix = L.gpool != nullptr;
        c.bt.g = L.gpool;
    }
    poison_bytes_ = 0;
    int rc;
    if ((rc = plan_output(c)) != STS_OK) return rc;
    if ((rc = run_frame_workspace(c)) != STS_OK) return rc;
    c.bf.z = L.zpool; c.Fld = L.capacity;
    // (and the carried filter states are the pools: run_frame_workspace carves none for an open stream)
    if (c.oc.eqst) c.bf.eqst = L.eqst;
    if (c.oc.lst) { c.bf.ldst = L.ldst; loud_res.clear(); loud_slots.clear(); }      // (the results of this step's retiring slots alone)
    const int math = conv_math;
    if (math == 3 && L.form0) conv_math = 0;
    if (conv_math == 3) *(volatile unsigned*)ovf_host_ = 0u;
    rc = run_stream_steps(c);
    conv_math = math;
    L.steps++;
    prof.conv_math_fallbacks = h2_fallbacks;
    if (rc == STS_OK && hipGetLastError() != hipSuccess) rc = fail(STS_EDEVICE, "the step failed on the device");
    if (live_after) *live_after = L.live_count();
    return rc;
}

// ---- open paragraphs (engine.hpp para_open; para_stream.hpp; DESIGN.md 9i "Open paragraphs").  Between two calls the engine keeps: z of
// every resident sentence in the pool, the plan's s / F of every sentence so far, the next chunk, the free column ranges, the step count
// and the form-0 flag.  Nothing in the arenas survives a call: every step and every append lays its workspace out again.
int Engine::para_open(int chunk_frames, int max_resident, long long capacity_frames, int lead_frames, float fade_ms) {
    if (live_) return fail(STS_ESTATE, "a stream is open on this engine (sts_stream_close first)");
    if (para_) return fail(STS_ESTATE, "a paragraph is already open on this engine (sts_para_close first)");
    const Model& M = model;
    // (stream_open's bounds and refusals, for the reasons given there)
    if (chunk_frames <= 0 || max_resident < 1 || max_resident > 1024 || capacity_frames < 1)
        return fail(STS_EINVAL, "an open paragraph takes a positive chunk size, 1 <= max_resident <= 1024 and a positive capacity");
    if ((double)capacity_frames * M.inter > 2.0e9 || (double)capacity_frames * M.hop_total > 2.0e9)
        return fail(STS_EINVAL, "an open paragraph's capacity_frames * inter_channels and capacity_frames * samples_per_frame may not exceed 2 10^9");
    if (eq_n > 0) return fail(STS_EINVAL, "an open paragraph is not available while an equaliser is set: its state is carried in the frame arena");
    if (loud_mode != 0) return fail(STS_EINVAL, "an open paragraph is not available while loudness measurement or normalization is on: its state is carried in the frame arena");
    if (record_taps) return fail(STS_EINVAL, "an open paragraph is not available while taps are recorded");
    if (refuse_pitch("an open paragraph")) return STS_EINVAL;
    if (pend.have_plan || pend.have_mix || pend.have_gain || pend.have_forced)
        return fail(STS_EINVAL, "an open paragraph is not available while a duration plan, a speaker mix, a gain plan or forced durations are pending: their tables are per call");
    const sts_join j{nullptr, lead_frames, 0, fade_ms};
    const char* why = nullptr;
    if (!join_valid(1, &j, &why)) return fail(STS_EINVAL, why);
    HIPCK(hipSetDevice(device));
    LimiterDesign d{};
    if (lim_mode != 0 && !limiter_design(out_rate, lim_gain_db, lim_ceiling, lim_ms, &d)) return fail(STS_EINVAL, "limiter: output rate outside [8000, 48000]");
    if (conv_math == 3) { const int rc = ensure_overflow_word(); if (rc != STS_OK) return rc; }
    ParaStream* P = new (std::nothrow) ParaStream();
    if (!P) return fail(STS_EDEVICE, "out of host memory");
    const int Hd = decoder_halo_frames(M);
    P->open(chunk_frames, max_resident, capacity_frames, lead_frames, M.hop_total, Hd, stream_halo() - Hd, resampling() ? rs.P : 1, resampling() ? rs.Q : 1,
            lim_mode != 0 ? d.H : 0);
    P->fade_h = join_design(fade_ms);
    if (!P->fits(lead_frames)) { delete P; return fail(STS_EINVAL, "the joined signal is too long for one call (N_J <= 2 10^9 native samples)"); }
    LiveStream& L = P->pool;
    L.form0 = conv_math == 3 && h2_disabled;
    // the pool, as an open stream's: its own allocation (never in arenaF_), a KB of slack behind the last row
    const size_t pool_bytes = ((size_t)M.inter * (size_t)capacity_frames + 256) * sizeof(float);
    if (hipMalloc((void**)&L.zpool, pool_bytes) != hipSuccess || hipMalloc(&L.tab_dev, adopt_tab_bytes(max_resident)) != hipSuccess ||
        hipHostMalloc(&L.tab_host, adopt_tab_bytes(max_resident), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (L.zpool) (void)hipFree(L.zpool);
        if (L.tab_dev) (void)hipFree(L.tab_dev);
        delete P;
        return fail(STS_EDEVICE, "out of device memory (the open paragraph's latent pool)");
    }
    if (poison && hipMemsetD32Async((hipDeviceptr_t)L.zpool, (int)poison, pool_bytes / 4, stream) != hipSuccess) (void)hipGetLastError();
    mfma_launches_ = 0;                                        // (sts_profile.decoder_mfma_launches: summed over the paragraph's steps)
    para_ = P;
    return STS_OK;
}

int Engine::para_close() {
    if (!para_) return fail(STS_ESTATE, "no paragraph is open on this engine");
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (para_->pool.zpool) (void)hipFree(para_->pool.zpool);
    if (para_->pool.tab_dev) (void)hipFree(para_->pool.tab_dev);
    if (para_->pool.tab_host) (void)hipHostFree(para_->pool.tab_host);
    delete para_;
    para_ = nullptr;
    return STS_OK;
}

int Engine::para_finish(int trail_frames) {
    if (!para_) return fail(STS_ESTATE, "no paragraph is open on this engine (sts_para_open first)");
    ParaStream& P = *para_;
    if (P.finished) return fail(STS_EINVAL, "the paragraph is finished already");
    if (P.sentences() == 0) return fail(STS_EINVAL, "a paragraph cannot finish without a sentence");
    if (trail_frames < 0 || trail_frames > kJoinMaxFrames) return fail(STS_EINVAL, "join: lead_frames and trail_frames must be in [0, 100000]");
    if (!P.finish(trail_frames)) return fail(STS_EINVAL, "the joined signal is too long for one call (N_J <= 2 10^9 native and L_out <= 2^31 - 1 output samples)");
    return STS_OK;
}

// stream_admit_once's shape: front and flow of the B new sentences in the arithmetic conv_math names, their place in J, their slots and
// columns, their z into the pool.  kRetrySplitBf16: the overflow word was raised (conv math 3) -- nothing of the append is kept, the
// caller repeats it in form 0
int Engine::para_append_once(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const long long* gap,
                             int32_t* frames_out, int64_t* start_out, int32_t* appended) {
    ParaStream& P = *para_;
    LiveStream& L = P.pool;
    const bool guarded = conv_math == 3;
    if (guarded) *(volatile unsigned*)ovf_host_ = 0u;
    poison_bytes_ = 0;
    host_t0_ = now_us(); host_t_sync_ = 0;
    StreamSpec ss{L.chunk, [](void*, int32_t, const int16_t*, int32_t, int32_t) { return 0; }, nullptr};
    RunCtx c;
    c.B = B; c.ids = ids; c.n = n; c.sid = sid; c.ls = ls; c.ss = &ss; c.bstream = B > 1;
    int rc;
    if ((rc = run_setup(c)) != STS_OK) return rc;
    mark(0);
    if ((rc = run_text_encoder(c)) != STS_OK) return rc;
    if ((rc = run_durations(c)) != STS_OK) return rc;          // (a stream never launches ahead: the frame counts are on the host)
    std::vector<long> F((size_t)B); std::vector<int> sidv((size_t)B); std::vector<long long> start((size_t)B);
    for (int b = 0; b < B; b++) { F[(size_t)b] = c.p_lenF[b]; sidv[(size_t)b] = c.p_sid[b]; }
    const int first = P.sentences();
    const int fit = P.append(B, F.data(), sidv.data(), gap, start.data());
    if (fit <= 0) {                                            // the front work is lost, nothing has changed
        HIPCK(hipStreamSynchronize(stream));
        if (fit < 0) return fail(STS_EINVAL, "the joined signal would be too long for one paragraph (N_J <= 2 10^9 native and L_out <= 2^31 - 1 output samples)");
        *appended = 0;
        return STS_OK;
    }
    auto undo = [&](int code) { P.undo(B); return code; };
    if ((rc = run_frame_workspace(c)) != STS_OK) return undo(rc);
    if ((rc = run_flow(c)) != STS_OK) return undo(rc);
    // z of the new sentences leaves the arena: one table upload, one launch
    long long* const tab = (long long*)L.tab_host;
    int* const tlen = (int*)(tab + 2 * (size_t)B);
    for (int b = 0; b < B; b++) { tab[b] = c.p_offF[b]; tab[B + b] = P.zoff[(size_t)(first + b)]; tlen[b] = (int)F[(size_t)b]; }
    if (hipMemcpyAsync(L.tab_dev, tab, adopt_tab_bytes(B), hipMemcpyHostToDevice, stream) != hipSuccess) return undo(fail(STS_EDEVICE, "the adoption table's upload failed"));
    adopt_z(c.bf.z, c.Fld, L.zpool, L.capacity, c.C, (const long long*)L.tab_dev, B, c.maxF, stream);
    if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return undo(fail(STS_EDEVICE, "the append failed on the device"));
    if (guarded && *(volatile unsigned*)ovf_host_ != 0u) return undo(kRetrySplitBf16);
    for (int b = 0; b < B; b++) {
        if (frames_out) frames_out[b] = (int32_t)F[(size_t)b];
        if (start_out) start_out[b] = out_count(start[(size_t)b] * c.hop);
    }
    *appended = B;
    return STS_OK;
}

int Engine::para_append(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const int32_t* gap_frames,
                        int32_t* frames_out, int64_t* start_out, int32_t* appended) {
    if (!para_) return fail(STS_ESTATE, "no paragraph is open on this engine (sts_para_open first)");
    if (!appended) return fail(STS_EINVAL, "an append needs the `appended` output");
    *appended = 0;
    if (refuse_pitch("an open paragraph")) return STS_EINVAL;
    ParaStream& P = *para_;
    if (P.finished) return fail(STS_EINVAL, "the paragraph is finished: it takes no more sentences");
    if (B < 1 || !ids || !n) return fail(STS_EINVAL, "an append takes B >= 1 sentences with ids and n");
    if (B > P.pool.max_live) return fail(STS_EINVAL, "an append of more sentences than the paragraph's max_resident can never fit");
    std::vector<long long> gap((size_t)B, 0);
    for (int b = 0; gap_frames && b < B; b++) {
        if (gap_frames[b] < 0 || gap_frames[b] > kJoinMaxFrames) return fail(STS_EINVAL, "join: every gap must be in [0, 100000] frames");
        gap[(size_t)b] = gap_frames[b];
    }
    if (P.sentences() == 0 && gap[0] != 0) return fail(STS_EINVAL, "the gap in front of a paragraph's first sentence must be 0: its lead was given to sts_para_open");
    if (P.stopped || P.pool.free_slots() < B) return STS_OK;  // (no room now, known before any front work; a stopped paragraph takes nothing)
    HIPCK(hipSetDevice(device));
    // global sentence i samples with seed + i, the scales as they are set now
    std::vector<Noise> keep; keep.swap(noise_utt);
    for (int b = 0; b < B; b++) noise_utt.push_back(Noise{noise.ns, noise.nsw, noise.seed + (uint64_t)(P.sentences() + b)});
    const int math = conv_math;
    if (math == 3 && P.pool.form0) conv_math = 0;
    int rc = para_append_once(B, ids, n, sid, ls, gap.data(), frames_out, start_out, appended);
    if (rc == kRetrySplitBf16) {                               // this append alone: nothing of the new sentences has been delivered
        h2_fallbacks++;
        conv_math = 0;
        rc = para_append_once(B, ids, n, sid, ls, gap.data(), frames_out, start_out, appended);
    }
    conv_math = math;
    noise_utt.swap(keep);
    prof.conv_math_fallbacks = h2_fallbacks;
    return rc;
}

// stream_step's shape with the join and the pool both set: ONE step of run_stream_steps, chunk P.k of J, if the frontier lets it leave
int Engine::para_step(int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* ready_after) {
    if (!para_) return fail(STS_ESTATE, "no paragraph is open on this engine (sts_para_open first)");
    if (!cb) return fail(STS_EINVAL, "a step takes a callback");
    ParaStream& P = *para_;
    LiveStream& L = P.pool;
    Model& M = model;
    auto ready = [&] { return (int32_t)std::min<long long>(P.ready(), 2147483647LL); };
    if (ready_after) *ready_after = ready();
    if (P.ready() == 0) return STS_OK;
    HIPCK(hipSetDevice(device));
    StreamSpec ss{L.chunk, cb, user};
    RunCtx c;
    c.live = &L; c.join = true;
    // (the sentences that have not retired alone: a step's host work does not grow with the paragraph's age.  Until finish F_J = the end
    // of the last sentence, which no clip of this step reaches)
    c.js = P.resident_plan(); c.FJ = P.js.FJ;
    c.para_k = P.k; c.para_zoff = P.zoff.data() + P.first_live; c.para_sid = P.sid.data() + P.first_live;
    JsStep t;
    c.js.step(P.k, t);
    // "utterances" of this context: the step's decode windows (at least one: the tables and the conditioning are sized by it)
    const int B = c.B = std::max<int>(1, (int)t.win.size());
    c.ss = &ss; c.bstream = true;                              // (a window's index is never its sentence's: the conditioning is gathered per window)
    c.bt = BufT{}; c.bf = BufF{};
    c.ms = M.is_ms == 1; c.H = M.hidden; c.C = M.inter; c.hop = M.hop_total;
    c.wnH = M.n_flows ? M.cp[0].wn.H : 0; c.wnL = M.n_flows ? M.cp[0].wn.n : 0;
    // the decode workspace of this step's windows (transient: laid out per step).  The flow's buffers are those of one frame -- no flow
    // runs here -- and z is the pool
    std::vector<int> lenF((size_t)B, 1), offF((size_t)B, 0);
    for (size_t i = 0; i < t.win.size(); i++) lenF[i] = (int)(t.win[i].w1 - t.win[i].w0);
    c.p_lenF = lenF.data(); c.p_offF = offF.data();
    c.Ftot = c.Fld = 1; c.maxF = c.maxFld = 1;
    poison_bytes_ = 0;
    const int keep_h = join_h;
    join_h = P.fade_h;
    auto leave = [&](int code) { join_h = keep_h; return code; };
    int rc;
    if ((rc = plan_output(c)) != STS_OK) return leave(rc);
    if ((rc = run_frame_workspace(c)) != STS_OK) return leave(rc);
    c.bf.z = L.zpool; c.Fld = L.capacity;
    const int math = conv_math;
    if (math == 3 && L.form0) conv_math = 0;
    if (conv_math == 3) *(volatile unsigned*)ovf_host_ = 0u;
    rc = run_stream_steps(c);
    conv_math = math;
    prof.decoder_mfma_launches = mfma_launches_;
    prof.conv_math_fallbacks = h2_fallbacks;
    if (rc == STS_OK && hipGetLastError() != hipSuccess) rc = fail(STS_EDEVICE, "the step failed on the device");
    // (a step that failed delivered nothing and counts nothing: L.steps stays the next chunk's index, so STS_DBG_STREAM_RETRY_STEP = k
    // names chunk k, as in a closed joined stream)
    if (rc == STS_OK) { L.steps++; P.delivered(c.para_stop); }
    if (ready_after) *ready_after = ready();
    return leave(rc);
}

}  // namespace sts
