// duration_plan.hip -- duration plans (sts_set_duration_plan; include/summertts_hip.h has the full definition, DESIGN.md 9f the kernel
// structure).  For one utterance with weights w_i = exp(logw_i) * length_scale * rate_i, fixed lengths fixed_i and a target of F frames:
//   no target:  d_i = fixed_i >= 0 ? fixed_i : the durations kernel's clamp of ceil(w_i);
//   target F:   fixed phonemes keep fixed_i; the R' = F - sum fixed - #free frames beyond one per free phoneme are apportioned over the free
//               phonemes by largest remainder on the integer weights k_i = floor(min(w_i, 4096) 2^20): d_i = 1 + (R' k_i) div K + e_i,
//               e_i = 1 for the L = R' - sum (R' k_i) div K phonemes with the largest (R' k_i) mod K (ties: the lower index).
// Everything that decides a frame is 64-bit integer arithmetic: the order in which a sum or a count is reduced cannot change a result.
//
// duration_plan_kernel: one workgroup of 256 threads per utterance (the geometry of durations_kernel).  Thread tid owns phonemes tid, tid + 256,
// ...: it alone reads and writes their words of `forced` and of the remainder scratch, so the passes need no ordering through memory.
// Pass 1 forms w and k and reduces (K, sum fixed, #free); pass 2 divides; the L-th largest remainder theta is found by bisection over its VALUE
// (<= log2 K < 46 rounds of one block-wide count each -- linear in T per round, never a sort); every remainder above theta takes a frame and
// the rest go to the lowest indices with remainder == theta, found by a block-wide prefix count in index order.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/summertts_hip.h"
#include "kernels.hpp"

namespace sts {

__device__ __forceinline__ int seg_start(const SegView& s, int b) { return (s.off ? s.off[b] : s.ioff) * s.scale + b * s.extra; }
__device__ __forceinline__ int seg_len(const SegView& s, int b) { return (s.off ? s.len[b] : s.ilen) * s.scale + s.extra; }

// step 3: exactly the expression of durations_kernel (misc_kernels.hip)
__host__ __device__ static inline int dp_ceil_clamp(float w) {
    const float c = ceilf(w);
    return (c >= (float)kDurMax) ? kDurMax : (c > 0.f ? (int)c : 0);
}
// step 4: the integer weight (NaN, zero and anything below zero: 0; +inf: 4096 * 2^20)
__host__ __device__ static inline long long dp_weight(float w) {
    if (!(w > 0.f)) return 0;
    return (long long)floorf(fminf(w, 4096.f) * 1048576.f);
}

bool dur_plan_valid(int n, const float* rate, const int32_t* fixed, int32_t target, const char** why) {
    const char* dummy; if (!why) why = &dummy;
    if (n < 1) { *why = "duration plan: an utterance needs at least one phoneme"; return false; }
    if (target != 0 && (target < 1 || target > kDurMaxTarget)) { *why = "duration plan: target_frames must be 0 or in [1, 2^20]"; return false; }
    long long sfix = 0, nfree = 0;
    for (int i = 0; i < n; i++) {
        if (rate && !(rate[i] >= 1.0f / 64.0f && rate[i] <= 64.0f)) { *why = "duration plan: rate must be finite and in [1/64, 64]"; return false; }
        if (fixed && (fixed[i] < -1 || fixed[i] > kDurMax)) { *why = "duration plan: fixed must be in [-1, 100000]"; return false; }
        if (fixed && fixed[i] >= 0) sfix += fixed[i]; else nfree++;
    }
    if (target > 0) {
        if (nfree > 0 && (long long)target - sfix < nfree) { *why = "duration plan: the target leaves less than one frame per free phoneme"; return false; }
        if (nfree == 0 && sfix != (long long)target) { *why = "duration plan: every phoneme is fixed and their sum is not the target"; return false; }
    }
    return true;
}

// steps 3-4 on the host (sts_duration_fit).  The caller has validated (dur_plan_valid).
void duration_fit(const float* w, const int32_t* fixed, int n, int32_t target, int32_t* out) {
    if (target <= 0) {
        for (int i = 0; i < n; i++) out[i] = fixed && fixed[i] >= 0 ? fixed[i] : dp_ceil_clamp(w[i]);
        return;
    }
    std::vector<long long> k(n, -1);
    long long K = 0, sfix = 0, nfree = 0;
    for (int i = 0; i < n; i++) {
        if (fixed && fixed[i] >= 0) { out[i] = fixed[i]; sfix += fixed[i]; continue; }
        k[i] = dp_weight(w[i]); K += k[i]; nfree++;
    }
    if (nfree == 0) return;
    const long long R = (long long)target - sfix - nfree;
    const bool unit = K == 0;
    if (unit) K = nfree;
    std::vector<int> order; order.reserve((size_t)nfree);
    long long suma = 0;
    for (int i = 0; i < n; i++) {
        if (k[i] < 0) continue;
        const long long p = R * (unit ? 1 : k[i]);
        out[i] = 1 + (int32_t)(p / K); k[i] = p % K; suma += p / K;
        order.push_back(i);
    }
    const long long L = R - suma;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return k[a] > k[b]; });     // (stable: ties keep the index order)
    for (long long j = 0; j < L; j++) out[order[(size_t)j]] += 1;
}

__device__ __forceinline__ long long dp_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int dp_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void duration_plan_kernel(DurPlanArgs a) {
    __shared__ long long red[3][4];
    __shared__ int cnt[2][4];
    __shared__ int wsum[4];
    __shared__ int carry_s;
    const int b = blockIdx.x;
    const int T = seg_len(a.seg, b);
    const size_t base = (size_t)seg_start(a.seg, b);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.target ? a.target[b] : 0;
    const float scale = a.w_in ? 1.0f : a.ls[b];

    // ---- pass 1: w (and the tap), the unfitted durations, or the integer weights and their sums
    long long K = 0, sfix = 0, nfree = 0;
    for (int t = tid; t < T; t += 256) {
        float w;
        if (a.w_in) w = a.w_in[base + t];
        else {
            float lw = a.r0[base + t];
            if (a.sdp) lw = (lw - a.ea_m) * expf(a.ea_logs * (-1.0f));
            w = expf(lw) * scale;
            if (a.rate) w = w * a.rate[base + t];
        }
        if (a.dur_w) a.dur_w[base + t] = w;
        const int fx = a.fixed ? a.fixed[base + t] : -1;
        if (F <= 0) { a.forced[base + t] = fx >= 0 ? fx : dp_ceil_clamp(w); continue; }
        if (fx >= 0) { a.forced[base + t] = fx; a.rem[base + t] = -1; sfix += fx; }
        else { const long long k = dp_weight(w); a.rem[base + t] = k; K += k; nfree++; }
    }
    if (F <= 0) return;                       // (uniform: the whole workgroup leaves)
    K = dp_wave_sum(K); sfix = dp_wave_sum(sfix); nfree = dp_wave_sum(nfree);
    if (lane == 0) { red[0][wave] = K; red[1][wave] = sfix; red[2][wave] = nfree; }
    __syncthreads();
    K = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    sfix = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    nfree = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    __syncthreads();
    if (nfree == 0) return;
    long long R = (long long)F - sfix - nfree;
    if (R < 0) R = 0;                         // (the host refuses such a plan; never a negative product)
    const bool unit = K == 0;
    if (unit) K = nfree;

    // ---- pass 2: quotients into `forced`, remainders into the scratch; this thread's first remainder stays in a register
    long long suma = 0, r_first = -1;
    for (int t = tid; t < T; t += 256) {
        const long long k = a.rem[base + t];
        if (k < 0) continue;
        const long long p = R * (unit ? 1 : k);
        const long long q = p / K, r = p - q * K;
        a.forced[base + t] = 1 + (int)q;
        a.rem[base + t] = r;
        if (t == tid) r_first = r;
        suma += q;
    }
    suma = dp_wave_sum(suma);
    if (lane == 0) red[0][wave] = suma;
    __syncthreads();
    const long long L = R - (red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    if (L <= 0) return;                       // 0 <= L < #free

    // ---- the L-th largest remainder: the smallest theta with #{r > theta} < L, by bisection over [-1, K - 1]
    auto count_gt = [&](long long x, int par) -> int {
        int c = r_first > x ? 1 : 0;
        for (int t = tid + 256; t < T; t += 256) c += a.rem[base + t] > x ? 1 : 0;
        c = dp_wave_sum(c);
        if (lane == 0) cnt[par][wave] = c;
        __syncthreads();                      // (two buffers: a round's readers never meet the next round's writers)
        return cnt[par][0] + cnt[par][1] + cnt[par][2] + cnt[par][3];
    };
    long long lo = -1, hi = K - 1;
    int par = 0;
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)count_gt(mid, par) < L) hi = mid; else lo = mid;
        par ^= 1;
    }
    const long long theta = hi;
    const long long E = L - (long long)count_gt(theta, par);       // frames left for the phonemes with r == theta, lowest index first
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + tid;
        const long long r = t < T ? a.rem[base + t] : -1;
        const int eq = r == theta ? 1 : 0;
        int v = eq;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int pre = carry_s;
        for (int k = 0; k < wave; k++) pre += wsum[k];
        if (r > theta || (eq && (long long)(pre + v - 1) < E)) a.forced[base + t] += 1;
        __syncthreads();
        if (tid == 255) carry_s = pre + v;
        __syncthreads();
    }
}

void duration_plan(const DurPlanArgs& a, int B, hipStream_t st) {
    if (B <= 0) return;
    hipLaunchKernelGGL(duration_plan_kernel, dim3(B), dim3(256), 0, st, a);
}

}  // namespace sts
