// resample.hip -- output sample-rate conversion of the decoder's float wave (sts_set_output_rate): a windowed-sinc polyphase filter
// from the native 16 kHz to any integer rate in [8000, 48000], then the reference's int16 cast.  The filter (DESIGN.md 9b,
// include/summertts_hip.h sts_resample_table):
//   g = gcd(in, out), P = out / g, Q = in / g (P <= 1024); L_out = ceil(L_in P / Q)
//   output j sits at input position j Q / P: phase phi = (j Q) mod P, base n0 = (j Q) div P
//   c = 0.9 min(1, out / in) (cutoff, units of the input Nyquist), W = 32 / c, K = ceil(W), 2K taps per phase
//   tap m of phase phi reads input n0 - K + 1 + m at offset d = phi / P + K - 1 - m:
//   h = c sinc(c d) I0(beta sqrt(1 - (d / W)^2)) / I0(beta) for |d| < W, else 0; beta = 10
//   float64, every phase normalised to sum 1, rounded to float32: table [P][2K]
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "conv_common.hpp"
#include "devmath.hpp"
#include "kernels.hpp"

namespace sts {

static long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// modified Bessel function of the first kind, order 0 (power series; converges for the arguments used here, x <= 10)
double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; k++) {
        t *= q / ((double)k * (double)k);
        s += t;
        if (t < s * 1e-17) break;
    }
    return s;
}

bool resample_design(int in_rate, int out_rate, ResampleDesign* d) {
    if (in_rate < kResampleMinRate || in_rate > kResampleMaxRate || out_rate < kResampleMinRate || out_rate > kResampleMaxRate) return false;
    const long long g = gcd_ll(in_rate, out_rate);
    d->P = (int)(out_rate / g); d->Q = (int)(in_rate / g);
    if (d->P > kResampleMaxP) return false;
    const double c = 0.9 * std::min(1.0, (double)out_rate / (double)in_rate);
    d->K = (int)ceil(32.0 / c);
    return true;
}

void resample_table(const ResampleDesign& d, int in_rate, int out_rate, float* table) {
    const int P = d.P, K = d.K, T = 2 * K;
    const double c = 0.9 * std::min(1.0, (double)out_rate / (double)in_rate), W = 32.0 / c, beta = 10.0, i0b = bessel_i0(beta);
    const double pi = 3.14159265358979323846;
    std::vector<double> h(T);
    for (int ph = 0; ph < P; ph++) {
        double sum = 0.0;
        for (int m = 0; m < T; m++) {
            const double dd = (double)ph / (double)P + (double)(K - 1 - m);
            double v = 0.0;
            if (fabs(dd) < W) {
                const double x = c * dd;
                const double sinc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
                const double r = dd / W;
                v = c * sinc * bessel_i0(beta * sqrt(1.0 - r * r)) / i0b;
            }
            h[m] = v; sum += v;
        }
        for (int m = 0; m < T; m++) table[(size_t)ph * T + m] = (float)(h[m] / sum);
    }
}

__device__ __forceinline__ long long ceil_div_ll(long long a, long long b) { return (a + b - 1) / b; }

// One workgroup per (tile of RS_TILE outputs, window).  The input span of the tile -- [n0_first - K + 1, n0_last + K] -- is staged into LDS
// with zeros outside the utterance (and outside the decoded window, which the streaming halo makes sure is never read); so is the whole
// table when it is small (P <= 3 for 8, 12, 24, 32 and 48 kHz; the 441-phase tables of the 44.1 kHz family are read from global memory,
// L2-resident).  Each lane then runs the fp32 FMA chain over m = 0 .. 2K-1 of its output's phase row for RS_PER outputs, 256 apart
// (coalesced stores); the RS_PER chains are interleaved so that their loads are in flight together.
constexpr int RS_THREADS = 256, RS_PER = 4, RS_TILE = RS_THREADS * RS_PER;
constexpr int RS_LDS = 2 * RS_TILE + 2 * kResampleMaxK + 8;          // Q / P <= 2 (out >= in / 2) and K <= kResampleMaxK
constexpr int RS_TAB_LDS = 4096;                                     // tables up to this many floats are staged into LDS
template <typename Tab>
__device__ __forceinline__ void resample_chains(const Tab* tab, const float* xs, long long s0, long long t0, long long t1, long long P,
                                                long long Q, long long K, int T, long long ob, int tid, const ResampleArgs& a) {
    const Tab* h[RS_PER]; const float* xv[RS_PER]; float acc[RS_PER];
#pragma unroll
    for (int r = 0; r < RS_PER; r++) {
        long long j = t0 + r * RS_THREADS + tid;
        if (j >= t1) j = t0;                                          // (past the tile: computes output t0 again, stores nothing)
        const long long jq = j * Q, n0 = jq / P;
        h[r] = tab + (size_t)(jq - n0 * P) * T;
        xv[r] = xs + (n0 - K + 1 - s0);
        acc[r] = 0.f;
    }
#pragma unroll 4
    for (int m = 0; m < T; m++) {
#pragma unroll
        for (int r = 0; r < RS_PER; r++) acc[r] = fmaf(h[r][m], xv[r][m], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RS_PER; r++) {
        const long long j = t0 + r * RS_THREADS + tid;
        if (j < t1) {
            if (a.wave_out) a.wave_out[ob + j] = acc[r];
            a.pcm[ob + j] = pcm_cast(acc[r]);
        }
    }
}
__global__ __launch_bounds__(RS_THREADS) void resample_pcm_kernel(ResampleArgs a) {
    __shared__ float xs[RS_LDS];
    __shared__ float hs[RS_TAB_LDS];
    __shared__ unsigned long long s_obase;
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long P = a.P, Q = a.Q, K = a.K, T = 2 * a.K;
    const long long win = seg_len(a.seg, b), ib = seg_start(a.seg, b);     // window b: native samples [ib, ib + win) of x
    long long u0 = 0, L = win, j0 = 0, j1 = ceil_div_ll(win * P, Q);
    long long obw = 0;                                                  // (streaming: where window b's outputs start in pcm)
    if (a.wtab) { const long long* t = a.wtab + 5 * b; u0 = t[0]; L = t[1]; j0 = t[2]; j1 = t[3]; obw = t[4]; }   // (utterance samples [u0, u0 + win) of L)
    const long long t0 = j0 + (long long)blockIdx.x * RS_TILE;
    if (t0 >= j1) return;
    const long long t1 = t0 + RS_TILE < j1 ? t0 + RS_TILE : j1;
    // where window b's outputs start: the output counts of the windows before it, summed here (in a launch-ahead run the host does not know
    // the frame counts yet)
    if (tid == 0) s_obase = 0;
    __syncthreads();
    if (a.seg.off && !a.wtab) {
        unsigned long long part = 0;
        for (int q = tid; q < b; q += RS_THREADS) part += (unsigned long long)ceil_div_ll((long long)a.seg.len[q] * a.seg.scale * P, Q);
        if (part) atomicAdd(&s_obase, part);
    }
    const long long s0 = (t0 * Q) / P - K + 1;                                // first staged input position (utterance coordinates)
    const int span = (int)(((t1 - 1) * Q) / P + K - s0 + 1);
    for (int i = tid; i < span && i < RS_LDS; i += RS_THREADS) {
        const long long p = s0 + i;
        xs[i] = (p >= 0 && p < L && p >= u0 && p < u0 + win) ? a.x[ib + (p - u0)] : 0.f;
    }
    const bool tab_lds = P * T <= RS_TAB_LDS;
    if (tab_lds)
        for (int i = tid; i < (int)(P * T); i += RS_THREADS) hs[i] = a.table[i];
    __syncthreads();
    if (span > RS_LDS) return;                                                 // (never: the host admits only Q <= 2P, K <= kResampleMaxK)
    const long long ob = (long long)s_obase + obw - j0;
    if (tab_lds) resample_chains(hs, xs, s0, t0, t1, P, Q, K, (int)T, ob, tid, a);
    else resample_chains(a.table, xs, s0, t0, t1, P, Q, K, (int)T, ob, tid, a);
}

void resample_pcm(const ResampleArgs& a, int nwin, long long max_out, hipStream_t st) {
    if (nwin <= 0 || max_out <= 0) return;
    hipLaunchKernelGGL(resample_pcm_kernel, dim3((unsigned)((max_out + RS_TILE - 1) / RS_TILE), nwin), dim3(RS_THREADS), 0, st, a);
}

// One workgroup per (tile of SP_TILE samples, window): a plain int16 copy, SP_PER samples per lane 256 apart (coalesced)
constexpr int SP_THREADS = 256, SP_PER = 8, SP_TILE = SP_THREADS * SP_PER;
__global__ __launch_bounds__(SP_THREADS) void stream_pack_kernel(const int16_t* __restrict__ src, int16_t* __restrict__ dst,
                                                                 const int* __restrict__ src_off, const int* __restrict__ dst_off) {
    const int w = blockIdx.y;
    const long long d0 = dst_off[w], n = (long long)dst_off[w + 1] - d0, s0 = src_off[w];
    const long long t0 = (long long)blockIdx.x * SP_TILE;
    if (t0 >= n) return;
#pragma unroll
    for (int r = 0; r < SP_PER; r++) {
        const long long i = t0 + r * SP_THREADS + threadIdx.x;
        if (i < n) dst[d0 + i] = src[s0 + i];
    }
}

void stream_pack(const int16_t* src, int16_t* dst, const int* src_off, const int* dst_off, int nwin, long long max_n, hipStream_t st) {
    if (nwin <= 0 || max_n <= 0) return;
    hipLaunchKernelGGL(stream_pack_kernel, dim3((unsigned)((max_n + SP_TILE - 1) / SP_TILE), nwin), dim3(SP_THREADS), 0, st, src, dst, src_off, dst_off);
}

}  // namespace sts
