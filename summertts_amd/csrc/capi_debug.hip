// capi_debug.hip -- the sts_debug_* entries of include/summertts_hip.h that launch kernels: one kernel (or one layer) on host arrays, for
// the float64 parity tests and the lab tools.  Weights go through the loader's layout code (model.hpp), buffers through a DevScratch.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "capi_common.hpp"
#include "dev_scratch.hpp"
#include "engine.hpp"

using namespace sts;

namespace {
// lengths[B] -> device table [offsets | lengths]; returns L = sum(lengths) or -1
long debug_segments(const int32_t* lengths, int32_t B, std::vector<int>& tab, int* max_len, int max_B = 65535, long max_L = 1 << 24) {
    if (!lengths || B < 1 || B > max_B) return -1;
    tab.assign(2 * (size_t)B, 0);
    long L = 0; *max_len = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 1 || L + lengths[b] > max_L) return -1;
        tab[b] = (int)L; tab[B + b] = lengths[b]; L += lengths[b];
        if (lengths[b] > *max_len) *max_len = lengths[b];
    }
    return L;
}
// the packed table of a conv entry: the same table under the entry's own texts and limits (any B >= 1, L = the sum)
int conv_segments(const int32_t* lengths, int32_t B, int32_t L, std::vector<int>& tab, int* max_len) {
    for (int b = 0; b < B; b++) if (lengths[b] <= 0) return set_err(STS_EINVAL, "packed conv: every segment length must be positive");
    if (debug_segments(lengths, B, tab, max_len, INT32_MAX, INT32_MAX) != L) return set_err(STS_EINVAL, "packed conv: L must equal the sum of the segment lengths");
    return STS_OK;
}
// steady-state time of `iters` launches on the stream, in ms per launch; negative: a HIP call failed
float time_launches(hipStream_t st, int iters, const std::function<void()>& launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    bool ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
              hipEventRecord(e0, st) == hipSuccess;
    for (int it = 0; it < iters && ok; it++) launch();
    ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (e0 && hipEventDestroy(e0) != hipSuccess) ok = false;
    if (e1 && hipEventDestroy(e1) != hipSuccess) ok = false;
    return ok ? ms / (float)iters : -1.f;
}
// the x16 / plane order (kernels.hpp H2PArgs): f(u, i) for every value, u its place in the device tensor, i its place in fp32 [C][L]
void x16_order(int C, long L, const std::function<void(size_t, size_t)>& f) {
    for (int c = 0; c < C / 16; c++) for (long t = 0; t < L; t++) for (int h = 0; h < 2; h++) for (int e = 0; e < 8; e++)
        f(((size_t)c * L + t) * 16 + h * 8 + e, (size_t)(16 * c + 8 * (e >> 2) + 4 * h + (e & 3)) * L + t);
}
// a conv's weights [Cout][k][Cin] (and bias) as an HConv
HConv host_conv(const float* w, const float* bias, int Cout, int Cin, int k) {
    HConv h;
    h.out_ch = Cout; h.in_ch = Cin; h.k = k; h.w = w; h.b = bias; h.has_bias = bias ? 1 : 0;
    return h;
}
}  // namespace

extern "C" {

int sts_debug_spline_step(int device, const float* h, int64_t n, float filter_sqrt, const float* r0, const float* r1, float* o0, float* o1) {
    if (!h || !o0 || !o1 || n < 1 || n > (1 << 24) || !(filter_sqrt > 0.f)) return set_err(STS_EINVAL, "h [29][n], 1 <= n <= 2^24, filter_sqrt > 0 and both outputs are required");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    // each output row is followed by a guard that reaches past the last 128-thread block of the launch; it must come back untouched
    const size_t guard = (size_t)((n + 127) / 128 * 128 - n) + 128;
    DevScratch d;
    const float *dh = d.up(h, (size_t)29 * n), *dr0 = d.up(r0, (size_t)n), *dr1 = d.up(r1, (size_t)n);
    float *d0 = d.out((size_t)n + guard), *d1 = d.out((size_t)n + guard);
    std::vector<uint32_t> back0((size_t)n + guard), back1((size_t)n + guard);
    if (d.ok) spline_step(dh, (long)n, filter_sqrt, dr0, dr1, d0, d1, (long)n, d.st);
    d.down(back0.data(), d0, back0.size() * 4);
    d.down(back1.data(), d1, back1.size() * 4);
    if (!d.finish()) return set_err(STS_EDEVICE, "the spline step failed on the device");
    for (size_t i = (size_t)n; i < back0.size(); i++)
        if (back0[i] != 0xFFFFFFFFu || back1[i] != 0xFFFFFFFFu) return set_err(STS_EDEVICE, "the spline step wrote past n");
    memcpy(o0, back0.data(), (size_t)n * 4);
    memcpy(o1, back1.data(), (size_t)n * 4);
    return STS_OK;
}

int sts_debug_attention(int device, const float* q, const float* k, const float* v, const float* relk, const float* relv, int32_t nheads,
                        int32_t kc, int32_t win, const int32_t* lengths, int32_t B, int variant, float* o, int32_t o_rows,
                        int32_t* variant_out, int32_t* jpl_out) {
    if (variant_out) *variant_out = 0;
    if (jpl_out) *jpl_out = 0;
    if (!q || !k || !v || !o) return set_err(STS_EINVAL, "q, k, v and o are required");
    if (nheads < 1 || nheads > 65535 || kc < 1 || kc > 4096 || win < 0 || win > 4096) return set_err(STS_EINVAL, "1 <= nheads <= 65535, 1 <= kc <= 4096, 0 <= win <= 4096");
    if ((win > 0) != (relk != nullptr) || (win > 0) != (relv != nullptr)) return set_err(STS_EINVAL, "relk and relv [kc][2 win + 1] go with win > 0, null with win = 0");
    if (variant < 0 || variant > 3) return set_err(STS_EINVAL, "variant: 0 = the engine's choice, 1 = generic, 2 = register, 3 = matrix-core");
    const long rows = (long)nheads * kc;
    if (o_rows < rows) return set_err(STS_EINVAL, "o holds at least nheads * kc rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || (double)o_rows * (double)L > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= 2^24, o_rows * sum <= 2^30");
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.kc = kc; a.win = win; a.px = win > 0 ? 2 * win + 1 : 0; a.nheads = nheads; a.B = B; a.max_len = max_len; a.ld = L;
    a.block_min_wgs = 0; a.attn_reg = 1;            // the engine's defaults (engine.hpp)
    AttnPlan plan;
    if (variant == 0) plan = attention_choose(a);
    else attention_admits(a, variant, &plan);
    if (plan.kernel == ATTN_NONE) return set_err(STS_EINVAL, variant == 0 ? "no attention kernel admits this shape (utterance too long for the attention kernel)" : "the shape is outside the forced kernel's limits");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    a.q = d.up(q, (size_t)rows * L); a.k = d.up(k, (size_t)rows * L); a.v = d.up(v, (size_t)rows * L);
    a.relk = d.up(relk, (size_t)kc * a.px); a.relv = d.up(relv, (size_t)kc * a.px);
    const int* dt = d.up(tab.data(), tab.size());
    a.o = d.out((size_t)o_rows * L);
    a.seg = SegView{dt, dt + B, 1, 0, 0, 0};
    if (d.ok) attention_launch(a, plan, d.st);
    d.down(o, a.o, (size_t)o_rows * L * 4);
    if (!d.finish()) return set_err(STS_EDEVICE, "the attention launch failed on the device");
    if (variant_out) *variant_out = plan.kernel;
    if (jpl_out) *jpl_out = plan.jpl;
    return STS_OK;
}

int sts_debug_layer_norm(int device, const float* a, const float* b, int32_t nb, int64_t b_stride, const float* res, const float* gamma,
                         const float* beta, int32_t C, int32_t pre_relu, int32_t post_gelu, const float* dw_w, const float* dw_b, int32_t dw_k,
                         int32_t dw_dil, int32_t dw_pad, const int32_t* lengths, int32_t B, float* y, int32_t y_rows) {
    if (!a || !gamma || !beta || !y) return set_err(STS_EINVAL, "a, gamma, beta and y are required");
    if (C < 1 || C > 65536 || y_rows < C) return set_err(STS_EINVAL, "1 <= C <= 65536 and y holds at least C rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || (double)y_rows * (double)L > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= 2^24, y_rows * sum <= 2^30");
    if (nb < 0 || nb > 8 || (nb > 0) != (b != nullptr)) return set_err(STS_EINVAL, "0 <= nb <= 8 partials in b (null with nb = 0)");
    if (nb > 1 && b_stride < (int64_t)C * L) return set_err(STS_EINVAL, "b_stride >= C * L floats between partials");
    if (dw_w && (dw_k < 1 || dw_k > 64 || dw_dil < 1 || dw_dil > 4096 || dw_pad < 0 || dw_pad > (1 << 20))) return set_err(STS_EINVAL, "depthwise conv: 1 <= k <= 64, 1 <= dil <= 4096, 0 <= pad <= 2^20");
    if (!dw_w && dw_b) return set_err(STS_EINVAL, "dw_b goes with dw_w");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    LnArgs g;
    memset(&g, 0, sizeof(g));
    const size_t n = (size_t)C * L;
    g.a = d.up(a, n); g.a_ld = L;
    g.nb = nb; g.b_stride = nb > 1 ? (long)b_stride : 0; g.b_ld = L;
    g.b = d.up(b, nb > 1 ? (size_t)(nb - 1) * (size_t)b_stride + n : n);
    g.res = d.up(res, n); g.res_ld = L;
    g.gamma = d.up(gamma, (size_t)C); g.beta = d.up(beta, (size_t)C);
    g.C = C; g.pre_relu = pre_relu != 0; g.post_gelu = post_gelu != 0;
    if (dw_w) { g.dw_w = d.up(dw_w, (size_t)dw_k * C); g.dw_b = d.up(dw_b, (size_t)C); g.dw_k = dw_k; g.dw_dil = dw_dil; g.dw_pad = dw_pad; g.dw_ld = C; }
    const int* dt = d.up(tab.data(), tab.size());
    g.y = d.out((size_t)y_rows * L); g.y_ld = L;
    g.seg = SegView{dt, dt + B, 1, 0, 0, 0}; g.B = B; g.max_len = max_len;
    if (d.ok) layer_norm(g, d.st);
    d.down(y, g.y, (size_t)y_rows * L * 4);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the LayerNorm launch failed on the device");
}

int sts_debug_resblock_layer(int device, const float* x, int32_t C, const int32_t* lengths, int32_t B, int64_t ld, int32_t n,
                             const float* const* w1, const float* const* b1, const int32_t* k1, const int32_t* dil1,
                             const float* const* w2, const float* const* b2, const int32_t* k2, float slope, int kind, int variant,
                             float* y, int32_t y_rows, uint32_t* ovf) {
    if (ovf) *ovf = 0;
    if (!x || !w1 || !k1 || !dil1 || !w2 || !k2 || !y) return set_err(STS_EINVAL, "x, y and the members' w1, k1, dil1, w2, k2 tables are required");
    if (kind < 1 || kind > 4) return set_err(STS_EINVAL, "kind: 1 = resblock_layer, 2 = resblock_wino, 3 = resblock_bf3 (bf16x3), 4 = resblock_bf3 (f16x2)");
    if (variant < -1 || variant > 1) return set_err(STS_EINVAL, "variant: -1 = automatic, 0 or 1");
    if (n < 1 || n > kMaxGroup) return set_err(STS_EINVAL, "1 <= n <= 4 members");
    if (C < 1 || C > 1024 || y_rows < C) return set_err(STS_EINVAL, "1 <= C <= 1024 and every y holds at least C rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || ld < L || (double)y_rows * (double)ld * n > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= ld, n * y_rows * ld <= 2^30");
    for (int j = 0; j < n; j++)
        if (!w1[j] || !w2[j] || k1[j] < 1 || k1[j] > 255 || k2[j] < 1 || k2[j] > 255 || dil1[j] < 1 || dil1[j] > 4096)
            return set_err(STS_EINVAL, "every member: w1, w2, 1 <= k1, k2 <= 255, 1 <= dil1 <= 4096");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    // the weights as the blob carries a ResBlock layer's convs, through the loader's packers
    HConv c1[kMaxGroup], c2[kMaxGroup];
    for (int j = 0; j < n; j++) {
        c1[j] = host_conv(w1[j], b1 ? b1[j] : nullptr, C, C, k1[j]); c1[j].dil = dil1[j]; c1[j].pad = dil1[j] * (k1[j] - 1) / 2;
        c2[j] = host_conv(w2[j], b2 ? b2[j] : nullptr, C, C, k2[j]); c2[j].pad = (k2[j] - 1) / 2;
    }
    Model m;
    struct Freed { Model& m; ~Freed() { (void)hipDeviceSynchronize(); free_model(m); } } freed{m};     // (runs after the buffers' and the stream's release)
    if (!load_resblock_layer(c1, c2, n, m)) return set_err(STS_EDEVICE, "packing the layer's weights failed: " + m.error);
    DevScratch d;
    const size_t yn = (size_t)y_rows * (size_t)ld;
    const float* dx = d.up(x, (size_t)C * (size_t)ld);
    const int* dt = d.up(tab.data(), tab.size());
    unsigned* dovf = (unsigned*)d.zeros(4);
    float* dy[kMaxGroup] = {};
    for (int j = 0; j < n; j++) dy[j] = d.out(yn);
    if (!d.ok) return set_err(STS_EDEVICE, "device buffers of the layer");
    // the group as Engine::ResStage::fill_fused fills it: every member reads the same x and writes its own y
    ResLayerGroup R;
    memset(&R, 0, sizeof(R));
    R.n = n; R.C = C; R.ld = (long)ld; R.slope = slope; R.seg = SegView{dt, dt + B, 1, 0, 0, 0}; R.B = B; R.max_n = max_len;
    for (int j = 0; j < n; j++) {
        if (fill_res_member(m.rb[j].c1[0], m.rb[j].c2[0], dx, dy[j], kind == 4, R.g[j])) { R.math = 1; R.ovf = dovf; }
        else if (kind == 4) return set_err(STS_EINVAL, "shape has no two-term fp16 copy of its weights");
    }
    const bool eligible = kind == 1 ? resblock_layer_eligible(R) : kind == 2 ? resblock_wino_eligible(R) : resblock_bf3_eligible(R);
    if (!eligible) return set_err(STS_EINVAL, kind == 1 ? "shape not eligible for resblock_layer" : kind == 2 ? "shape not eligible for resblock_wino" : "shape not eligible for resblock_bf3");
    if (kind == 1) resblock_layer(R, d.st);
    else if (kind == 2) resblock_wino(R, d.st);
    else resblock_bf3(R, d.st, variant);
    for (int j = 0; j < n; j++) d.down(y + (size_t)j * yn, dy[j], yn * 4);
    uint32_t word = 0;
    d.down(&word, dovf, 4);
    if (!d.finish()) return set_err(STS_EDEVICE, "the ResBlock layer launch failed on the device");
    if (ovf) *ovf = word;
    return STS_OK;
}

int sts_debug_col_layer(int device, const float* x, int32_t C, const int32_t* lengths, int32_t B, int64_t ld, const float* xs_w,
                        const float* xs_b, const float* xr, const float* dw_w, const float* dw_b, int32_t dw_k, int32_t dw_dil, int32_t dw_pad,
                        const float* g1, const float* b1, const float* w, const float* bias, const float* add, const float* g2,
                        const float* b2, int32_t post_gelu, int32_t use_res, const float* tp_w, const float* tp_b, float tp_fs,
                        const float* tp_r0, const float* tp_r1, int32_t alias, float* y, int32_t y_rows, float* o0, float* o1) {
    if (!x || !w || !g2 || !b2 || !y) return set_err(STS_EINVAL, "x, w, g2, b2 and y are required");
    if (C < 1 || C > 4096 || y_rows < C) return set_err(STS_EINVAL, "1 <= C <= 4096 and y holds at least C rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || ld < L || (double)y_rows * (double)ld > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= ld, y_rows * ld <= 2^30");
    if (dw_w && (dw_k < 1 || dw_k > 64 || dw_dil < 1 || dw_dil > 4096 || dw_pad < 0 || dw_pad > (1 << 20))) return set_err(STS_EINVAL, "depthwise conv: 1 <= k <= 64, 1 <= dil <= 4096, 0 <= pad <= 2^20");
    if (!dw_w && dw_b) return set_err(STS_EINVAL, "dw_b goes with dw_w");
    if (!xs_w && (xs_b || xr)) return set_err(STS_EINVAL, "xs_b and xr go with xs_w");
    if (tp_w ? (!o0 || !o1 || !(tp_fs > 0.f)) : (tp_b != nullptr)) return set_err(STS_EINVAL, "a tail needs o0, o1 and tp_fs > 0; tp_b goes with tp_w");
    if (alias < 0 || alias > 5 || (alias >= 2 && !tp_w) || ((alias == 2 || alias == 5) && !tp_r0) || ((alias == 3 || alias == 4) && !tp_r1))
        return set_err(STS_EINVAL, "alias: 0 none, 1 y = x, 2 o0 = r0, 3 o0 = r1, 4 o1 = r1, 5 o1 = r0 (2 - 5: a tail with that latent half)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    // the weights as the blob carries a ConvFlow's convs ([out][k][in]), through the loader's packers
    std::vector<float> dwt;
    HConv sep; HLn n1, n2;
    const HConv pre = host_conv(xs_w, xs_b, C, 1, 1), pw = host_conv(w, bias, C, C, 1), proj = host_conv(tp_w, tp_b, 29, C, 1);
    if (dw_w) {
        dwt.resize((size_t)C * dw_k);
        for (int c = 0; c < C; c++) for (int j = 0; j < dw_k; j++) dwt[(size_t)c * dw_k + j] = dw_w[(size_t)j * C + c];
        sep = host_conv(dwt.data(), dw_b, C, 1, dw_k); sep.dil = dw_dil; sep.pad = dw_pad;
    }
    n1.size = C; n1.g = g1; n1.b = b1;
    n2.size = C; n2.g = g2; n2.b = b2;
    Model m;
    struct Freed { Model& m; ~Freed() { (void)hipDeviceSynchronize(); free_model(m); } } freed{m};     // (runs after the buffers' and the stream's release)
    if (!load_col_layer(xs_w ? &pre : nullptr, dw_w ? &sep : nullptr, (g1 && b1) ? &n1 : nullptr, pw, n2, tp_w ? &proj : nullptr, m))
        return set_err(STS_EDEVICE, "packing the layer's weights failed: " + m.error);
    const DConvFlow& cf = m.cf[0];
    DevScratch d;
    const size_t xn = (size_t)C * (size_t)ld, yn = (size_t)y_rows * (size_t)ld;
    const float* dx = d.up(x, xn);
    const float* dadd = d.up(add, xn);
    const float* dxr = d.up(xr, (size_t)ld);
    const float* dr0 = d.up(tp_r0, (size_t)ld);
    const float* dr1 = d.up(tp_r1, (size_t)ld);
    const int* dt = d.up(tab.data(), tab.size());
    float* dy = d.out(yn);
    float* do0 = tp_w ? d.out((size_t)ld) : nullptr;
    float* do1 = tp_w ? d.out((size_t)ld) : nullptr;
    if (!d.ok) return set_err(STS_EDEVICE, "device buffers of the layer");
    Lvl lv;
    lv.seg = SegView{dt, dt + B, 1, 0, 0, 0}; lv.nb = B; lv.max_len = max_len; lv.total = L; lv.ld = (long)ld;
    // the kernarg block as the engine fills it; what the engine fixes per form and the entry leaves to the caller follows
    ColLayerArgs g;
    float* ydst = alias == 1 ? const_cast<float*>(dx) : dy;
    if (dw_w) fill_col_dds(cf.dds.sep[0], cf.dds.n1[0], cf.dds.pw[0], cf.dds.n2[0], dx, ydst, lv, g);
    else fill_col_oproj(cf.dds.pw[0], cf.dds.n2[0], dx, dadd, ydst, lv, g);
    g.C = C; g.add = dadd; g.add_ld = (long)ld; g.post_gelu = post_gelu != 0;
    g.res = use_res ? dx : nullptr; g.res_ld = (long)ld;
    if (xs_w) { fill_col_pre(cf.pre, dxr, dx, g); if (!use_res) g.res = nullptr; }
    if (tp_w)
        fill_col_tail(cf.proj, tp_fs, dr0, dr1, alias == 2 ? const_cast<float*>(dr0) : alias == 3 ? const_cast<float*>(dr1) : do0,
                      alias == 4 ? const_cast<float*>(dr1) : alias == 5 ? const_cast<float*>(dr0) : do1, g);
    if (!col_layer_eligible(g)) return set_err(STS_EINVAL, "shape not eligible for col_layer");
    col_layer(g, d.st);
    d.down(y, dy, yn * 4);
    if (tp_w) { d.down(o0, g.tp_o0, (size_t)ld * 4); d.down(o1, g.tp_o1, (size_t)ld * 4); }
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the column-block layer launch failed on the device");
}

int sts_debug_adopt_z(int device, const float* src, int32_t C, int64_t ld_src, float* dst, int64_t ld_dst, const int64_t* src_off,
                      const int64_t* dst_off, const int32_t* len, int32_t B) {
    if (!src || !dst || !src_off || !dst_off || !len || B < 1 || B > 65535 || C < 1 || ld_src < 1 || ld_dst < 1 ||
        (double)C * (double)ld_src > (double)(1 << 28) || (double)C * (double)ld_dst > (double)(1 << 28))
        return set_err(STS_EINVAL, "src [C][ld_src], dst [C][ld_dst] (at most 2^28 floats each), the three tables and 1 <= B <= 65535 are required");
    std::vector<std::pair<int64_t, int64_t>> ranges;
    int max_len = 0;
    for (int b = 0; b < B; b++) {
        if (len[b] < 0 || src_off[b] < 0 || dst_off[b] < 0 || src_off[b] + len[b] > ld_src || dst_off[b] + len[b] > ld_dst)
            return set_err(STS_EINVAL, "a segment leaves its matrix");
        if (len[b] > 0) ranges.emplace_back(dst_off[b], dst_off[b] + len[b]);
        max_len = std::max(max_len, (int)len[b]);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++) if (ranges[i].first < ranges[i - 1].second) return set_err(STS_EINVAL, "destination ranges overlap");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    std::vector<long long> tab(((size_t)B * 20 + 7) / 8);       // long long src_off[B] | long long dst_off[B] | int len[B] (kernels.hpp adopt_z)
    for (int b = 0; b < B; b++) { tab[(size_t)b] = src_off[b]; tab[(size_t)B + b] = dst_off[b]; ((int*)(tab.data() + 2 * (size_t)B))[b] = len[b]; }
    DevScratch d;
    const float* ds = d.up(src, (size_t)C * ld_src);
    float* dd = (float*)d.up(dst, (size_t)C * ld_dst);
    const long long* dt = d.up(tab.data(), tab.size());
    if (d.ok) adopt_z(ds, ld_src, dd, ld_dst, C, dt, B, max_len, d.st);
    d.down(dst, dd, (size_t)C * ld_dst * 4);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the adoption launch failed on the device");
}

int sts_debug_adopt_tables(int device, const float* g, int32_t gin, int32_t B, float* gpool, int32_t max_live, const int32_t* cum,
                           const int32_t* q, int64_t n_src, int32_t* pool, int64_t capacity_phonemes, int32_t* slot_words, const int32_t* slot,
                           const int32_t* src_off, const int32_t* n, const int32_t* dst_off, const int32_t* h) {
    if (!slot_words || !pool || !slot || !src_off || !n || !dst_off || !h || B < 1 || B > 65535 || max_live < 1 || max_live > (1 << 20) ||
        gin < 0 || gin > (1 << 16) || (gin > 0) != (g != nullptr) || (gin > 0) != (gpool != nullptr) || n_src < 0 || n_src > (1 << 24) ||
        capacity_phonemes < 1 || capacity_phonemes > (1 << 24))
        return set_err(STS_EINVAL, "g [gin][B] and gpool [gin][max_live] (both null with gin 0), pool [2][capacity_phonemes + 1], slot_words [3][max_live], the five tables and 1 <= B <= 65535 are required");
    std::vector<std::pair<int64_t, int64_t>> ranges;
    std::vector<char> taken((size_t)max_live, 0);
    int max_n = 0;
    for (int b = 0; b < B; b++) {
        if (slot[b] < -1 || slot[b] >= max_live) return set_err(STS_EINVAL, "a slot outside [-1, max_live)");
        if (slot[b] < 0) continue;
        if (taken[(size_t)slot[b]]) return set_err(STS_EINVAL, "two newcomers name one slot");
        taken[(size_t)slot[b]] = 1;
        if (n[b] < 0 || (n[b] > 0 && (!cum || !q || src_off[b] < 0 || dst_off[b] < 0 || (int64_t)src_off[b] + n[b] > n_src || (int64_t)dst_off[b] + n[b] > capacity_phonemes)))
            return set_err(STS_EINVAL, "a phoneme range leaves its array");
        if (n[b] > 0) ranges.emplace_back(dst_off[b], (int64_t)dst_off[b] + n[b]);
        max_n = std::max(max_n, (int)n[b]);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++) if (ranges[i].first < ranges[i - 1].second) return set_err(STS_EINVAL, "destination ranges overlap");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    std::vector<int> tab(5 * (size_t)B);
    for (int b = 0; b < B; b++) { int* t = tab.data() + 5 * (size_t)b; t[0] = slot[b]; t[1] = src_off[b]; t[2] = slot[b] >= 0 ? n[b] : 0; t[3] = dst_off[b]; t[4] = h[b]; }
    const size_t pw = 2 * ((size_t)capacity_phonemes + 1);
    DevScratch d;
    AdoptTablesArgs a{};
    a.g = d.up(g, (size_t)gin * B); a.gpool = (float*)d.up(gpool, (size_t)gin * max_live); a.gin = gin; a.B = B; a.max_live = max_live;
    a.cum = d.up(cum, (size_t)n_src); a.q = d.up(q, (size_t)n_src);
    a.pool = (int*)d.up(pool, pw); a.ld_pool = capacity_phonemes + 1; a.swords = (int*)d.up(slot_words, 3 * (size_t)max_live);
    a.neutral = (int)capacity_phonemes;
    a.tab = d.up(tab.data(), tab.size());
    if (d.ok) adopt_tables(a, max_n, d.st);
    d.down(gpool, a.gpool, (size_t)gin * max_live * 4);
    d.down(pool, a.pool, pw * 4);
    d.down(slot_words, a.swords, 3 * (size_t)max_live * 4);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the table adoption launch failed on the device");
}

// ------------------------------------------------------------------------------------------------
// op-level entries for the parity tests: one conv on host arrays through the same kernels
static int debug_conv1d_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                             int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                             int32_t in_act, int mode, float** y_out, int32_t* Lout_out, int32_t iters, float* ms_out,
                             const int32_t* lengths, int32_t B, uint32_t* ovf_out, const sts_conv_epi_opts* eo = nullptr, int32_t gap = 0);

int sts_debug_conv1d(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                     int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope, int32_t in_act,
                     int mode, float** y_out, int32_t* Lout_out) {
    return sts_debug_conv1d_bench(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode,
                                  y_out, Lout_out, 0, nullptr);
}

int sts_debug_conv1d_bench(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                           int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                           int32_t in_act, int mode, float** y_out, int32_t* Lout_out, int32_t iters, float* ms_out) {
    return debug_conv1d_impl(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode, y_out, Lout_out,
                             iters, ms_out, nullptr, 1, nullptr);
}

int sts_debug_conv1d_packed(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                            int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                            int32_t in_act, int mode, float** y_out, int32_t* Lout_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!lengths) return set_err(STS_EINVAL, "packed conv: null segment lengths");
    return debug_conv1d_impl(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode, y_out, Lout_out,
                             0, nullptr, lengths, B, ovf_out);
}

int sts_debug_conv1d_epi(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                         int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                         int32_t in_act, int mode, float** y_out, int32_t* Lout_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out,
                         const sts_conv_epi_opts* opts, int32_t gap) {
    if (!lengths) return set_err(STS_EINVAL, "packed conv: null segment lengths");
    if (!opts && gap != 0) return set_err(STS_EINVAL, "conv epilogues: a gap between the segments needs the options struct");
    return debug_conv1d_impl(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode, y_out, Lout_out,
                             0, nullptr, lengths, B, ovf_out, opts, gap);
}

// The argument checks of sts_debug_conv1d_epi's options (include/summertts_hip.h), none of which needs a device
static int check_epi_opts(const sts_conv_epi_opts& o, int Cout, bool tr, bool depthwise, int gap) {
    if (o.size_bytes < (int32_t)sizeof(sts_conv_epi_opts)) return set_err(STS_EINVAL, "conv epilogues: size_bytes is smaller than sts_conv_epi_opts");
    if (gap < 0 || gap > 4096) return set_err(STS_EINVAL, "conv epilogues: 0 <= gap <= 4096");
    if (depthwise) return set_err(STS_EINVAL, "conv epilogues: dense convs only");
    const int e = o.epi;
    if (e != EPI_STORE && e != EPI_RESADD && e != EPI_SUB && e != EPI_GATE && e != EPI_RESSKIP && e != EPI_TANH_PCM) return set_err(STS_EINVAL, "conv epilogues: unknown epi");
    if (e == EPI_GATE && (o.H <= 0 || Cout != 2 * o.H)) return set_err(STS_EINVAL, "conv epilogues: GATE needs H > 0 and Cout == 2 H");
    if (o.gate_perm && (e != EPI_GATE || o.H % 16 != 0)) return set_err(STS_EINVAL, "conv epilogues: gate_perm is the packing of a GATE conv with H % 16 == 0");
    if (e == EPI_RESSKIP && (o.H <= 0 || (Cout != o.H && Cout != 2 * o.H))) return set_err(STS_EINVAL, "conv epilogues: RESSKIP needs H > 0 and Cout == H or 2 H");
    if (e == EPI_RESSKIP && (!o.aux_out || (!(o.epi_flag & 1) && !o.aux_init) || (Cout != o.H && !o.y_init)))
        return set_err(STS_EINVAL, "conv epilogues: RESSKIP needs aux_out, aux_init (unless epi_flag & 1) and, with Cout == 2 H, y_init");
    if (e == EPI_TANH_PCM && (Cout != 1 || !o.pcm_out)) return set_err(STS_EINVAL, "conv epilogues: TANH_PCM needs Cout == 1 and pcm_out");
    if (e == EPI_RESADD && !o.res) return set_err(STS_EINVAL, "conv epilogues: RESADD needs res");
    if (e == EPI_SUB && !o.y_init) return set_err(STS_EINVAL, "conv epilogues: SUB needs y_init");
    if (o.nsum != 0 && o.nsum != 2 && o.nsum != 3) return set_err(STS_EINVAL, "conv epilogues: nsum is 0, 2 or 3");
    if ((o.nsum >= 2 && !o.xs1) || (o.nsum == 3 && !o.xs2)) return set_err(STS_EINVAL, "conv epilogues: nsum needs xs1 (and xs2 for 3)");
    if (o.kslices != 1 && o.kslices != 2 && o.kslices != 4 && o.kslices != 8) return set_err(STS_EINVAL, "conv epilogues: kslices is 1, 2, 4 or 8");
    if (o.kslices > 1 && e != EPI_STORE) return set_err(STS_EINVAL, "conv epilogues: K slices are partial sums of the STORE epilogue");
    if (o.in_reflect && tr) return set_err(STS_EINVAL, "conv epilogues: no reflect view on a transposed conv");
    return STS_OK;
}

// lengths == null: one segment of L positions (the stand-alone entries); else B segments packed back to back, as the engine packs a batch.
// eo != null (sts_debug_conv1d_epi): the epilogue and operand forms of ConvArgs, and `gap` unused columns behind every segment
static int debug_conv1d_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                             int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                             int32_t in_act, int mode, float** y_out, int32_t* Lout_out, int32_t iters, float* ms_out,
                             const int32_t* lengths, int32_t B, uint32_t* ovf_out, const sts_conv_epi_opts* eo, int32_t gap) {
    if (!x || !w || !y_out || !Lout_out || Cin <= 0 || Cout <= 0 || L <= 0 || k <= 0) return set_err(STS_EINVAL, "bad conv arguments");
    const bool tr = stride_t > 0;
    const bool packed = lengths != nullptr;
    if (eo) { if (const int rc = check_epi_opts(*eo, Cout, tr, depthwise != 0, gap)) return rc; }
    const int epi = eo ? eo->epi : EPI_STORE, nsl = eo ? eo->kslices : 1, reflect = eo && eo->in_reflect ? 1 : 0;
    int maxlen = L;
    std::vector<int> seg(8, 0);       // {off = 0, len = 1} | .. | overflow word [4] | .. | the packed table [8 ..)
    seg[1] = 1;
    if (packed) {
        if (B <= 0 || dil < 1) return set_err(STS_EINVAL, "packed conv: B >= 1 segments and dil >= 1");
        std::vector<int> tab;
        if (eo && (int64_t)B * gap >= L) return set_err(STS_EINVAL, "packed conv: L must equal the sum of the segment lengths and their gaps");
        if (const int rc = conv_segments(lengths, B, L - (eo ? B * gap : 0), tab, &maxlen)) return rc;
        if (eo) for (int b = 0; b < B; b++) tab[b] += b * gap;          // off[b] = sum_{i < b} (len_i + gap)
        seg.insert(seg.end(), tab.begin(), tab.end());
        if ((int64_t)L * (tr ? stride_t : 1) > (int64_t)1 << 26) return set_err(STS_EINVAL, "packed conv: at most 2^26 output positions");
        // the geometries the engine launches on packed buffers: output segment = input segment (x stride)
        if (tr ? (k < stride_t || ((k - stride_t) & 1) || pad != (k - stride_t) / 2 || dil != 1) : (!(k & 1) || pad != dil * (k - 1) / 2))
            return set_err(STS_EINVAL, "packed conv: 'same' padding (odd k, pad = dil (k - 1) / 2) or a transposed conv with pad = (k - stride) / 2");
    }
    const int Lout = (tr ? (L - 1) * stride_t - 2 * pad + (k - 1) + 1 : L + 2 * pad - dil * (k - 1)) + (reflect ? B : 0);     // (reflect view: one more position per segment)
    if (Lout <= 0) return set_err(STS_EINVAL, "empty output");
    auto r_up = [](int v, int m) { return (v + m - 1) / m * m; };
    const int cin_eff = depthwise ? 1 : Cin;
    const int Cin_pad = r_up(cin_eff, 16), Cout_pad = r_up(Cout, 32);
    const int J = tr ? (k + stride_t - 1) / stride_t : 1;
    const size_t wn = depthwise ? (size_t)k * Cout_pad : (tr ? (size_t)stride_t * J : (size_t)k) * Cin_pad * Cout_pad;
    // the fp32 copy the loader makes: plain / depthwise (pack_conv) or polyphase (pack_convT)
    const HConv hc = host_conv(w, bias, Cout, cin_eff, k);
    PackOpts po; po.depthwise = depthwise != 0;
    if (eo && eo->gate_perm) { po.gate = true; po.gate_H = eo->H; }        // the WN in_layer's packing (model.hip parse_pack_wn)
    std::vector<float> wp(wn, 0.f), bp(Cout_pad, 0.f);
    if (tr && !depthwise) { convT_layout(hc, stride_t, Cin_pad, Cout_pad, wp.data()); if (bias) memcpy(bp.data(), bias, sizeof(float) * Cout); }
    else conv_layout(hc, po, Cin_pad, Cout_pad, wp.data(), bias ? bp.data() : nullptr);
    // mode 12: the Winograd-domain kernel (pack_wino's transform, on shapes pack_wino declines as well)
    std::vector<float> wu;
    int wn3 = 0, wn2 = 0;
    if (mode == 12 && !depthwise && !tr) {
        wino_split(k, &wn3, &wn2);
        wu.resize((size_t)(wn3 + wn2) * 4 * Cin_pad * Cout_pad);
        wino_pack(w, (long)k * Cin, Cin, 1, Cout, k, Cin, Cin_pad, Cout_pad, wu.data());
    }
    // mode + 100 (transposed convs of stride 2 / 4 / 8 through the split-operand kernels): the row-interleaved-phase packing (ConvArgs::rowph)
    const bool rowph = mode >= 100;
    if (rowph) {
        mode -= 100;
        if (!tr || depthwise || Cout != Cout_pad || (stride_t != 2 && stride_t != 4 && stride_t != 8)) return set_err(STS_EINVAL, "row-interleaved phases: transposed conv, stride 2 / 4 / 8, Cout % 32 == 0");
    }
    // modes 13 / 20..25 / 28..33: the split-bf16 kernel (conv_bf3.hip), automatic tile / tile code (mode - 20)
    const bool h2 = (mode == 50 || (mode >= 60 && mode < 85)) && !depthwise;       // the two-term fp16 form of the same kernel
    if (h2) mode = mode == 50 ? 13 : mode - 40;
    const bool bf3 = (mode == 13 || (mode >= 20 && mode < 45)) && !depthwise;
    std::vector<unsigned char> wb3;
    float h2_scale = 1.0f;
    if (rowph && !bf3) return set_err(STS_EINVAL, "row-interleaved phases: split-operand modes only");
    if (bf3 && rowph) {      // merged rows, one "phase" of J taps (pack_bf3_rowph)
        const int rows = Cout_pad * stride_t;
        std::vector<float> wr((size_t)J * Cin_pad * rows, 0.f), br((size_t)rows, 0.f);
        rowph_layout(wp.data(), bp.data(), stride_t, J, Cin_pad, Cout_pad, wr.data(), br.data());
        wb3.resize(bf3_pack(wr.data(), 1, J, Cin_pad, rows, nullptr, false, h2 ? 1 : 0));
        bf3_pack(wr.data(), 1, J, Cin_pad, rows, wb3.data(), false, h2 ? 1 : 0, &h2_scale);
        bp.swap(br);
    } else if (bf3) {
        wb3.resize(bf3_pack(wp.data(), tr ? stride_t : 1, tr ? J : k, Cin_pad, Cout_pad, nullptr, false, h2 ? 1 : 0));
        bf3_pack(wp.data(), tr ? stride_t : 1, tr ? J : k, Cin_pad, Cout_pad, wb3.data(), false, h2 ? 1 : 0, &h2_scale);
    }
    // everything of the launch that is no device pointer
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x_ld = L; a.y_ld = Lout;
    a.Cin = cin_eff; a.Cout = Cout; a.Cin_pad = Cin_pad; a.Cout_pad = Cout_pad;
    a.depthwise = depthwise ? 1 : 0;
    if (tr) { a.ntap = J; a.tap_step = -1; a.tap_off = 0; a.out_stride = stride_t; a.out_off = -pad; a.transposed = 1; a.n_extra = J - 1; a.max_n = L + J - 1; }
    else { a.ntap = k; a.tap_step = dil; a.tap_off = -pad; a.out_stride = 1; a.out_off = 0; a.max_n = Lout; }
    a.in_act = in_act; a.in_slope = in_slope; a.epi = epi;
    a.B = 1;
    if (packed) { a.B = B; a.max_n = tr ? maxlen + J - 1 : maxlen + reflect; }
    if (h2) { a.math = 1; a.wscale = h2_scale; }
    if (rowph) { a.rowph = stride_t; a.Cout = a.Cout_pad = Cout_pad * stride_t; }
    if (!wu.empty()) { a.wino_n3 = wn3; a.wino_n2 = wn2; }
    // rows of y and aux, and the K-slice planes of y
    const int y_rows = eo && (epi == EPI_GATE || epi == EPI_RESSKIP) ? eo->H : Cout;
    const int aux_rows = epi == EPI_RESSKIP ? eo->H : (epi == EPI_TANH_PCM && eo->aux_out ? 1 : 0);
    const size_t yn = (size_t)y_rows * Lout * nsl;
    if (eo) {
        a.epi_flag = eo->epi_flag; a.H = eo->H; a.gate_perm = eo->gate_perm ? 1 : 0; a.in_reflect = reflect; a.nsum = eo->nsum >= 2 ? eo->nsum : 0;
        a.ubias_ld = B; a.res_ld = Lout; a.aux_ld = Lout;
        if (nsl > 1) { a.kslices = nsl; a.kslice_stride = (long)y_rows * Lout; }
        // what the named kernel family takes, by the engine's own eligibility functions (which look at no operand but whether the weight
        // copies exist): nothing falls back to another kernel
        static const float here = 0.f;
        ConvArgs p = a;
        if (bf3) p.wb3 = &here;
        if (!wu.empty()) p.wu = &here;
        if (eo->nsum >= 2) { p.xs1 = &here; p.xs2 = eo->nsum == 3 ? &here : nullptr; }
        if (rowph && (epi != EPI_STORE || eo->ubias)) return set_err(STS_EINVAL, "row-interleaved phases: the plain epilogue only");
        if (a.gate_perm && tr) return set_err(STS_EINVAL, "conv epilogues: no gate packing of a transposed conv");
        const bool mfma = !bf3 && mode != 12 && mode != 1 && conv_mfma_eligible(p);
        if (bf3 && !conv_bf3_eligible(p)) return set_err(STS_EINVAL, "shape or epilogue not eligible for the split-bf16 kernel");
        if (mode == 12 && !conv_wino_eligible(p)) return set_err(STS_EINVAL, "shape or epilogue not eligible for the Winograd kernel");
        if (!bf3 && mode >= 2 && mode != 12 && !mfma) return set_err(STS_EINVAL, "shape or epilogue not eligible for the matrix-core kernel");
        if (nsl > 1 && !(mfma && (mode == 8 || mode == 9))) return set_err(STS_EINVAL, "K slices: the split-K modes 8 / 9 only");
        if (a.nsum) {
            // (modes 42 / 43 = tiles 22 / 23: the tiles conv_bf3.hip's switch instantiates with SUM -- keep in step with it and with
            // conv_bf3_takes_sum, which cannot judge here because it asks for the AUTOMATIC tile of the shape)
            const bool folds = bf3 ? (tr && !reflect && (mode == 42 || mode == 43)) : (!mfma && mode != 12 && conv_cout1_takes(p));
            if (!folds) return set_err(STS_EINVAL, "nsum: the phase-merged split-operand tiles of a transposed conv (modes 42 / 43 / 82 / 83) and the single-output-channel kernel only");
        }
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "hipSetDevice failed");
    DevScratch d;
    a.x = d.up(x, (size_t)Cin * L);
    a.w = (const float*)d.zeros((wn + kWeightSlackFloats) * 4, wp.data(), wn * 4);
    const float* db = d.up(bp.data(), bp.size());
    a.bias = bias ? db : nullptr;
    // packed: a NaN pattern instead of zeros, so that a position no workgroup writes cannot pass
    if (!eo) a.y = packed ? d.out(yn) : (float*)d.zeros(yn * 4);
    const int* dseg = d.up(seg.data(), seg.size());
    if (!wu.empty()) a.wu = (const float*)d.zeros((wu.size() + kWeightSlackFloats) * 4, wu.data(), wu.size() * 4);
    if (bf3) a.wb3 = d.zeros(wb3.size() + kBf3SlackBytes, wb3.data(), wb3.size());
    const int oscale = tr ? stride_t : 1;
    if (eo) {
        // y / aux: the sentinel everywhere, then the caller's initial values inside the output segments alone.  A tensor with initial
        // values is the target of a read-modify-write epilogue: its sentinel is finite and tiny (0x2F5A5A5A = 1.99e-10), so that an update
        // that runs into an unused column changes its bits (NaN + v would keep the NaN's)
        auto initial = [&](const float* init, int rows, int planes) {
            std::vector<float> h((size_t)rows * Lout * planes);
            memset(h.data(), 0xFF, h.size() * 4);
            if (init) { const uint32_t s = 0x2F5A5A5Au; for (float& f : h) memcpy(&f, &s, 4); }
            if (init) for (int r = 0; r < rows; r++) for (int b = 0; b < B; b++) {
                const size_t o = (size_t)r * Lout + (size_t)seg[8 + b] * oscale + (size_t)b * reflect;
                memcpy(h.data() + o, init + o, ((size_t)lengths[b] * oscale + reflect) * 4);
            }
            return (float*)d.up(h.data(), h.size());
        };
        a.y = initial(eo->y_init, y_rows, nsl);
        if (aux_rows) a.aux = initial(eo->aux_init, aux_rows, 1);
        if (epi == EPI_TANH_PCM) a.pcm = d.out16((size_t)Lout);
        a.res = d.up(eo->res, (size_t)Cout * Lout);
        if (a.nsum) { a.xs1 = d.up(eo->xs1, (size_t)Cin * L); a.xs2 = d.up(eo->xs2, (size_t)Cin * L); }
        if (eo->ubias) {      // rows in the packed order of the weights: the same layout code, on ubias as a [Cout][1][B] filter
            std::vector<float> up((size_t)B * Cout_pad, 0.f), ub((size_t)Cout_pad * B, 0.f);
            conv_layout(host_conv(eo->ubias, nullptr, Cout, B, 1), po, B, Cout_pad, up.data(), nullptr);
            for (int r = 0; r < Cout_pad; r++) for (int b = 0; b < B; b++) ub[(size_t)r * B + b] = up[(size_t)b * Cout_pad + r];
            a.ubias = d.up(ub.data(), ub.size());
        }
    }
    if (!d.ok) return set_err(STS_EDEVICE, DevScratch::kNoBuffers);
    // segment lengths in base units: in = L, out = Lout -> two views over the same {off=0,len=1} table
    a.in_seg = SegView{dseg, dseg + 1, L, 0}; a.out_seg = SegView{dseg, dseg + 1, Lout, 0};
    // packed: real offset / length tables of B entries (behind the overflow word), output scale = stride
    if (packed) { a.in_seg = SegView{dseg + 8, dseg + 8 + B, 1, 0}; a.out_seg = SegView{dseg + 8, dseg + 8 + B, oscale, reflect}; }
    if (h2) a.ovf = (unsigned*)dseg + 4;     // (overflow word: behind the segment table)
    auto launch = [&]() {
        if (bf3) conv_bf3(a, d.st, mode == 13 ? -1 : mode - 20);
        else if (mode == 12) conv_wino(a, d.st);
        else if (mode != 1 && conv_mfma_eligible(a)) conv_mfma(a, d.st, mode >= 2 ? mode - 2 : -1);
        else conv_generic(a, d.st);
    };
    if (bf3 && !conv_bf3_eligible(a)) return set_err(STS_EINVAL, "shape not eligible for the split-bf16 kernel");
    if (mode == 12 && !conv_wino_eligible(a)) return set_err(STS_EINVAL, "shape not eligible for the Winograd kernel");
    if (!bf3 && mode >= 2 && mode != 12 && !conv_mfma_eligible(a)) return set_err(STS_EINVAL, "shape not eligible for the matrix-core kernel");
    launch();
    if (iters > 0 && ms_out) {   // steady-state timing of the same launch
        const float ms = time_launches(d.st, iters, launch);
        if (ms < 0.f) d.ok = false; else *ms_out = ms;
    }
    float* y = (float*)malloc(yn * 4);
    if (!y) return set_err(STS_EDEVICE, "out of host memory");
    d.down(y, a.y, yn * 4);
    if (eo) { d.down(eo->aux_out, a.aux, (size_t)aux_rows * Lout * 4); d.down(eo->pcm_out, a.pcm, (size_t)Lout * 2); }
    uint32_t word = 0;
    if (h2) d.down(&word, dseg + 4, 4);
    if (!d.finish()) { free(y); return set_err(STS_EDEVICE, "conv kernel failed"); }
    *y_out = y; *Lout_out = Lout;
    if (ovf_out) *ovf_out = word;
    return STS_OK;
}

// One "same"-padded conv through the pre-split path (conv_h2p.hip): x fp32 [Cin][L] -> split_planes -> conv_h2p_group (`members` identical
// members in one grid; member 0 is returned) -> all three output forms decoded to fp32 [Cout][L] on the host.
static int debug_conv_h2p_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                              const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                              int32_t iters, float* ms_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out);

int sts_debug_conv_h2p(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                       const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                       int32_t iters, float* ms_out) {
    return debug_conv_h2p_impl(device, x, Cin, L, w, bias, Cout, k, dil, res, in_slope, out_slope, tile, members, y_out, y16_out, yp_out, iters, ms_out,
                               nullptr, 1, nullptr);
}

// The same conv on B segments packed back to back (L = their sum): split_planes and conv_h2p_group both get the B-entry segment table and
// max_n = the longest segment; the plane and output buffers start out as a NaN pattern.
int sts_debug_conv_h2p_packed(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                              const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                              const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!lengths) return set_err(STS_EINVAL, "packed conv: null segment lengths");
    return debug_conv_h2p_impl(device, x, Cin, L, w, bias, Cout, k, dil, res, in_slope, out_slope, tile, members, y_out, y16_out, yp_out, 0, nullptr,
                               lengths, B, ovf_out);
}

static int debug_conv_h2p_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                              const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                              int32_t iters, float* ms_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!x || !w || Cin <= 0 || Cout <= 0 || L <= 0 || k <= 0 || !(k & 1) || dil < 1 || members < 1 || members > kMaxGroup) return set_err(STS_EINVAL, "bad conv arguments");
    if (Cin % 16 || Cout % 32) return set_err(STS_EINVAL, "pre-split conv: Cin % 16 == 0 and Cout % 32 == 0");
    const bool packed = lengths != nullptr;
    int maxlen = L;
    std::vector<int> tab;
    if (packed) {
        if (B <= 0) return set_err(STS_EINVAL, "packed conv: B >= 1 segments");
        if (const int rc = conv_segments(lengths, B, L, tab, &maxlen)) return rc;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "hipSetDevice failed");
    const int pad = dil * (k - 1) / 2;
    std::vector<float> wp((size_t)k * Cin * Cout, 0.f);
    conv_layout(host_conv(w, nullptr, Cout, Cin, k), PackOpts(), Cin, Cout, wp.data(), nullptr);
    std::vector<unsigned char> wb(bf3_pack(wp.data(), 1, k, Cin, Cout, nullptr, true, 1));
    float wscale = 1.0f;
    bf3_pack(wp.data(), 1, k, Cin, Cout, wb.data(), true, 1, &wscale);
    const size_t in_n = (size_t)Cin * L, out_n = (size_t)Cout * L, out_b = out_n * 4;
    DevScratch d;
    // (every buffer the kernels write starts out as NaNs, fp32 and fp16 alike)
    const float* dx = d.up(x, in_n);
    void* dxp = d.out(in_n);
    const void* dwb = d.zeros(wb.size() + kPresplitSlackBytes, wb.data(), wb.size());
    const float* db = (const float*)d.zeros((size_t)Cout * 4, bias, (size_t)Cout * 4);
    unsigned* dovf = (unsigned*)d.zeros(64);
    const int* dtab = d.up(tab.data(), tab.size());
    const float* dres = d.up(res, out_n);
    float* dres16 = res ? d.out(out_n) : nullptr;
    void* dtmp = res ? d.out(out_n) : nullptr;
    float* dy[kMaxGroup] = {}; float* dy16[kMaxGroup] = {}; void* dyp[kMaxGroup] = {};
    for (int m = 0; m < members; m++) { dy[m] = d.out(out_n); dy16[m] = d.out(out_n); dyp[m] = d.out(out_n); }
    if (!d.ok) return set_err(STS_EDEVICE, DevScratch::kNoBuffers);
    SegView whole{nullptr, nullptr, 1, 0, 0, L};
    int nb = 1;
    if (packed) { whole = SegView{dtab, dtab + B, 1, 0, 0, 0}; nb = B; }       // a real table of B entries
    split_planes(dx, L, Cin, whole, nb, maxlen, in_slope, dxp, nullptr, L, dovf, d.st);
    if (res) split_planes(dres, L, Cout, whole, nb, maxlen, 1.0f, dtmp, dres16, L, nullptr, d.st);
    H2PGroup G;
    memset(&G, 0, sizeof(G));
    G.n = members; G.seg = whole; G.B = nb; G.max_n = maxlen; G.ovf = dovf;
    for (int m = 0; m < members; m++) {
        H2PArgs& a = G.g[m];
        a.xp = dxp; a.xp_ld = L; a.wb = dwb; a.wscale = wscale; a.bias = bias ? db : nullptr; a.res16 = dres16; a.res_ld = L;
        a.y = iters < 0 ? nullptr : dy[m]; a.y_ld = L; a.y16 = dy16[m]; a.y16_ld = L; a.yp = dyp[m]; a.yp_ld = L; a.yp_slope = out_slope;    // (iters < 0: timing with a layer's second conv's outputs only)
        a.Cin = Cin; a.Cout = Cout; a.ntap = k; a.tap_step = dil; a.tap_off = -pad;
    }
    if (!conv_h2p_group_eligible(G)) return set_err(STS_EINVAL, "shape not eligible for the pre-split kernel");
    conv_h2p_group(G, d.st, tile);
    if (iters != 0 && ms_out) {
        const float ms = time_launches(d.st, iters < 0 ? -iters : iters, [&]() { conv_h2p_group(G, d.st, tile); });
        if (ms < 0.f) d.ok = false; else *ms_out = ms;
    }
    std::vector<float> t16(out_n);
    std::vector<uint16_t> tp(out_n * 2);
    d.down(y_out, dy[0], out_b);
    d.down(ovf_out, dovf, 4);
    d.down(t16.data(), dy16[0], out_b);
    d.down(tp.data(), dyp[0], out_b);
    if (!d.finish()) return set_err(STS_EDEVICE, "conv kernel failed");
    x16_order(Cout, L, [&](size_t u, size_t i) {
        if (y16_out) y16_out[i] = t16[u];
        if (yp_out) {
            _Float16 hi, lo;
            memcpy(&hi, &tp[u], 2); memcpy(&lo, &tp[out_n + u], 2);       // (out_n fp16 values per plane)
            yp_out[i] = (float)hi + (float)lo * (1.0f / 2048.0f);
        }
    });
    return STS_OK;
}

// One "same"-padded conv through the Winograd-domain lab path (conv_h2w.hip): x fp32 [C][L] -> to_x16 -> conv_h2w_group (`members` identical
// members) -> member 0's fp32 [C][L] output and its x16 output (lrelu(out, out_slope)) decoded to fp32 [C][L].
int sts_debug_conv_h2w(int device, const float* x, int32_t C, int32_t L, const float* w, const float* bias, int32_t k, int32_t dil, const float* res,
                       float in_slope, float out_slope, int members, float* y_out, float* y16_out, int32_t iters, float* ms_out) {
    if (!x || !w || C <= 0 || L <= 0 || k <= 0 || !(k & 1) || dil < 1 || members < 1 || members > kMaxGroup || C % 128) return set_err(STS_EINVAL, "bad conv arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "hipSetDevice failed");
    std::vector<float> wp((size_t)k * C * C, 0.f);
    conv_layout(host_conv(w, nullptr, C, C, k), PackOpts(), C, C, wp.data(), nullptr);
    int n3, n2; wino_split(k, &n3, &n2);
    const int ntapw = 4 * n3 + 3 * n2;
    std::vector<float> wu((size_t)ntapw * C * C);
    h2w_transform_weights(wp.data(), k, C, C, wu.data());
    std::vector<unsigned char> wb(bf3_pack(wu.data(), 1, ntapw, C, C, nullptr, true, 1));
    float wscale = 1.0f;
    bf3_pack(wu.data(), 1, ntapw, C, C, wb.data(), true, 1, &wscale);
    const size_t tn = (size_t)C * L;
    DevScratch d;
    const float* dx = d.up(x, tn);
    float* dx16 = d.out(tn);
    const void* dwb = d.zeros(wb.size() + kPresplitSlackBytes, wb.data(), wb.size());
    const float* db = (const float*)d.zeros((size_t)C * 4, bias, (size_t)C * 4);
    unsigned* dovf = (unsigned*)d.zeros(64);
    const float* dres = d.up(res, tn);
    float* dres16 = res ? d.out(tn) : nullptr;
    float* dy[kMaxGroup] = {}; float* dy16[kMaxGroup] = {};
    for (int m = 0; m < members; m++) { dy[m] = d.out(tn); dy16[m] = d.out(tn); }
    if (!d.ok) return set_err(STS_EDEVICE, DevScratch::kNoBuffers);
    to_x16(dx, L, C, L, dx16, L, d.st);
    if (res) to_x16(dres, L, C, L, dres16, L, d.st);
    H2WGroup G;
    memset(&G, 0, sizeof(G));
    G.n = members; G.seg = SegView{nullptr, nullptr, 1, 0, 0, L}; G.B = 1; G.max_n = L; G.ovf = dovf;
    for (int m = 0; m < members; m++) {
        H2WArgs& a = G.g[m];
        a.x16 = dx16; a.x_ld = L; a.wu = dwb; a.wscale = wscale; a.bias = bias ? db : nullptr; a.res16 = dres16; a.res_ld = L;
        a.y16 = dy16[m]; a.y16_ld = L; a.y = iters < 0 ? nullptr : dy[m]; a.y_ld = L; a.in_slope = in_slope; a.out_slope = out_slope; a.C = C; a.k = k; a.dil = dil;
    }
    if (!conv_h2w_group_eligible(G)) return set_err(STS_EINVAL, "shape not eligible for the Winograd-domain kernel");
    conv_h2w_group(G, d.st);
    if (iters != 0 && ms_out) {
        const float ms = time_launches(d.st, iters < 0 ? -iters : iters, [&]() { conv_h2w_group(G, d.st); });
        if (ms < 0.f) d.ok = false; else *ms_out = ms;
    }
    std::vector<float> t16(y16_out ? tn : 0);
    d.down(y_out, dy[0], tn * 4);
    if (y16_out) d.down(t16.data(), dy16[0], tn * 4);
    if (!d.finish()) return set_err(STS_EDEVICE, "conv kernel failed");
    if (y16_out) x16_order(C, L, [&](size_t u, size_t i) { y16_out[i] = t16[u]; });
    return STS_OK;
}

}  // extern "C"
