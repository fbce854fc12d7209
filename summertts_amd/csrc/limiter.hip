// limiter.hip -- look-ahead peak limiter on the float wave at the output rate (sts_set_limiter; include/summertts_hip.h has the full
// definition, DESIGN.md 9e the kernel structure).  For one utterance x[0 .. N), half window H, ceiling c, static gain g0:
//   v = float32(x g0);  q[n] = floor(min(1, c / |v[n]|) 2^30)  (2^30 outside the utterance, 0 for a non-finite sample);
//   m[k] = min q[k - H .. k + H];  S[n] = sum m[n - H .. n + H] (64-bit);  s[n] = float32(S[n] / ((2H + 1) 2^30));  y = float32(v s).
// q, m and S are integers: the order in which a window is reduced cannot change a bit, and y[n] is a function of x[n - 2H .. n + 2H] only.
//
// One workgroup per tile of LM_TILE outputs: q of tile +- 2H into LDS, the sliding minimum by doubling (m_2w[i] = min(m_w[i], m_w[i + w]),
// then the window of 2H + 1 as two overlapping power-of-two windows), the sliding sum per lane over a run of consecutive outputs (one full
// window sum, then one add and one subtract per output; m is stored with one pad word per 16 so that lanes 16 apart hit different banks),
// y staged in LDS and stored in 8-sample groups aligned in the packed signal (16-byte stores inside the tile, sample by sample at its edges).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/summertts_hip.h"
#include "devmath.hpp"
#include "kernels.hpp"

namespace sts {

constexpr int LM_THREADS = 256, LM_TILE = 4096, LM_GROUP = 8;
constexpr int LM_BUF = LM_TILE + 4 * kLimMaxH;            // q of a tile +- 2H; also holds m (tile +- H) with its pad words
constexpr int LM_ONE = 1 << 30;
static_assert((LM_TILE + 2 * kLimMaxH) / 16 * 17 + 17 <= LM_BUF, "the padded sliding minimum must fit the second buffer");

bool limiter_args_valid(int mode, float gain_db, float ceiling_dbfs, float lookahead_ms) {
    return (mode == 0 || mode == 1) && gain_db >= -40.f && gain_db <= 40.f && ceiling_dbfs >= -30.f && ceiling_dbfs <= 0.f &&
           lookahead_ms >= 0.25f && lookahead_ms <= 10.f;
}

bool limiter_design(int rate, float gain_db, float ceiling_dbfs, float lookahead_ms, LimiterDesign* d) {
    if (rate < kLimMinRate || rate > kLimMaxRate || !limiter_args_valid(1, gain_db, ceiling_dbfs, lookahead_ms)) return false;
    d->H = (int)floor((double)lookahead_ms * (double)rate / 1000.0 + 0.5);
    d->c = pow(10.0, (double)ceiling_dbfs / 20.0);
    d->G = pow(10.0, (double)gain_db / 20.0);
    return d->H >= 1 && d->H <= kLimMaxH;
}

// where a segment's input and output live: the window x[xbase .. xbase + xlen) holds utterance samples [u0, u0 + xlen) of N; outputs
// [j0, j1) go to y / pcm[dst ..)
struct LmSeg { long long xbase, u0, xlen, N, j0, j1, dst; };

__device__ __forceinline__ long long lm_len(const LimArgs& a, int b) {
    const long long u = a.len ? (long long)a.len[b] : (long long)a.ilen;
    return (u * a.scale * a.P + a.Q - 1) / a.Q;
}
__device__ __forceinline__ int lm_pad(int i) { return i + (i >> 4); }

__global__ __launch_bounds__(LM_THREADS) void limiter_kernel(LimArgs a) {
    __shared__ int bufA[LM_BUF];
    __shared__ int bufB[LM_BUF];
    __shared__ unsigned long long s_off;
    __shared__ unsigned s_st[3];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    LmSeg g;
    if (a.wtab) {
        const long long* w = a.wtab + 7 * (long long)b;
        g = LmSeg{w[0], w[1], w[2], w[3], w[4], w[5], w[6]};
        if (tid < 3) s_st[tid] = 0u;
        __syncthreads();
    } else {
        // utterance b's place in the packed signal: the sum of the lengths before it (integers: the order does not matter)
        if (tid == 0) s_off = 0ull;
        if (tid < 3) s_st[tid] = 0u;
        __syncthreads();
        unsigned long long po = 0;
        for (int q = tid; q < b; q += LM_THREADS) po += (unsigned long long)lm_len(a, q);
        if (po) atomicAdd(&s_off, po);
        __syncthreads();
        const long long off = (long long)s_off, N = lm_len(a, b);
        g = LmSeg{off, 0, N, N, 0, N, off};
    }
    const float g0 = a.gloud ? (float)(a.G * (double)a.gloud[b]) : (float)a.G;
    if (a.stat && blockIdx.x == 0 && tid == 0) a.stat[4 * b] = __float_as_uint(g0);
    const long long t0 = g.j0 + (long long)blockIdx.x * LM_TILE;
    if (t0 >= g.j1) return;
    const int nt = g.j1 - t0 < LM_TILE ? (int)(g.j1 - t0) : LM_TILE;
    const int H = a.H, W = 2 * H + 1, L = nt + 4 * H;
    const long long n0 = t0 - 2 * H, xend = g.u0 + g.xlen;
    const float* xw = a.x + g.xbase - g.u0;            // xw[n] = utterance sample n, for n inside the window

    for (int i = tid; i < L; i += LM_THREADS) {
        const long long n = n0 + i;
        int q = LM_ONE;
        if (n >= 0 && n < g.N && n >= g.u0 && n < xend) {
            const float v = xw[n] * g0;
            const double av = fabs((double)v);
            if (!isfinite(av)) q = 0;
            else if (av > a.c) q = (int)floor(a.c / av * 1073741824.0);
        }
        bufA[i] = q;
    }
    __syncthreads();
    // sliding minimum over 2H + 1: windows of 1, 2, 4 .. w <= 2H + 1 by doubling (entry i of a pass is exact for i <= L - 2w; the clamp only
    // keeps the others in bounds, nothing below reads them), then min(m_w[k], m_w[k + 2H + 1 - w])
    int* cur = bufA; int* nxt = bufB;
    int w = 1;
    while (2 * w <= W) {
        for (int i = tid; i < L; i += LM_THREADS) {
            const int k = i + w < L ? i + w : L - 1;
            nxt[i] = min(cur[i], cur[k]);
        }
        __syncthreads();
        int* t = cur; cur = nxt; nxt = t;
        w *= 2;
    }
    const int Lm = nt + 2 * H, d = W - w;
    for (int k = tid; k < Lm; k += LM_THREADS) nxt[lm_pad(k)] = min(cur[k], cur[k + d]);
    __syncthreads();
    const int* m = nxt;                 // m[lm_pad(k)], k = 0 .. nt + 2H: the minimum centred on utterance sample t0 - H + k
    float* ys = (float*)cur;            // (free from here on)

    // sliding sum: this lane's outputs [ja, jb) of the tile
    const int R = (nt + LM_THREADS - 1) / LM_THREADS;
    const int ja = tid * R, jb = ja + R < nt ? ja + R : nt;
    const unsigned long long full = (unsigned long long)W << 30;
    const double fullD = (double)full;
    unsigned long long Smin = full; unsigned cnt = 0; float pk = 0.f;
    if (ja < jb) {
        unsigned long long S = 0;
        for (int k = ja; k < ja + W; k++) S += (unsigned long long)m[lm_pad(k)];
        for (int j = ja;;) {
            const float s = (float)((double)S / fullD);
            const long long n = t0 + j;
            const float v = (n >= g.u0 && n < xend) ? xw[n] * g0 : 0.f;
            const float y = v * s;
            ys[j] = y;
            Smin = S < Smin ? S : Smin; cnt += S < full ? 1u : 0u; pk = fmaxf(pk, fabsf(y));      // (fmaxf: a NaN y leaves the peak alone)
            if (++j >= jb) break;
            S += (unsigned long long)m[lm_pad(j + 2 * H)];
            S -= (unsigned long long)m[lm_pad(j - 1)];
        }
    }
    if (a.stat) {
        // min s (as 1.0f's bits minus its own: a larger word is a smaller gain), max |y| (bits of a non-negative float), count
        unsigned df = 0x3f800000u - __float_as_uint((float)((double)Smin / fullD)), pb = __float_as_uint(pk);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned d2 = __shfl_xor(df, o, 64), p2 = __shfl_xor(pb, o, 64);
            df = d2 > df ? d2 : df; pb = p2 > pb ? p2 : pb; cnt += __shfl_xor(cnt, o, 64);
        }
        if (lane == 0) {
            if (df) atomicMax(&s_st[0], df);
            if (pb) atomicMax(&s_st[1], pb);
            if (cnt) atomicAdd(&s_st[2], cnt);
        }
    }
    __syncthreads();
    if (a.stat && tid == 0) {
        unsigned* st = a.stat + 4 * b;
        if (s_st[0]) atomicMax(st + 1, s_st[0]);
        if (s_st[1]) atomicMax(st + 2, s_st[1]);
        if (s_st[2]) atomicAdd(st + 3, s_st[2]);
    }
    // the tile's outputs at [D0, D0 + nt) of the packed destination, in groups of 8 aligned there
    const long long D0 = g.dst + (t0 - g.j0), D1 = D0 + nt;
    const long long gfirst = D0 / LM_GROUP, glast = (D1 + LM_GROUP - 1) / LM_GROUP;
    for (long long gi = gfirst + tid; gi < glast; gi += LM_THREADS) {
        const long long i0 = gi * LM_GROUP;
        if (i0 >= D0 && i0 + LM_GROUP <= D1) {
            const float* f = ys + (i0 - D0);
            if (a.y) {
                *(float4*)(a.y + i0) = make_float4(f[0], f[1], f[2], f[3]);
                *(float4*)(a.y + i0 + 4) = make_float4(f[4], f[5], f[6], f[7]);
            }
            if (a.pcm) {
                uint32_t wv[4];
#pragma unroll
                for (int i = 0; i < 4; i++) wv[i] = (uint32_t)(uint16_t)pcm_cast(f[2 * i]) | ((uint32_t)(uint16_t)pcm_cast(f[2 * i + 1]) << 16);
                *(uint4*)(a.pcm + i0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
            }
        } else {
            const long long lo = i0 > D0 ? i0 : D0, hi = i0 + LM_GROUP < D1 ? i0 + LM_GROUP : D1;
            for (long long i = lo; i < hi; i++) {
                const float f = ys[i - D0];
                if (a.y) a.y[i] = f;
                if (a.pcm) a.pcm[i] = pcm_cast(f);
            }
        }
    }
}

// sts_limiter_stats from the kernel's raw words
void limiter_stats_decode(const unsigned* raw, int B, sts_limiter_stats* out) {
    for (int b = 0; b < B; b++) {
        const unsigned* r = raw + 4 * b;
        const unsigned mb = 0x3f800000u - r[1];
        memcpy(&out[b].gain, &r[0], 4); memcpy(&out[b].min_gain, &mb, 4); memcpy(&out[b].peak_out, &r[2], 4);
        out[b].limited = (int32_t)r[3];
    }
}

void limiter_run(const LimArgs& a, int B, long long max_out, hipStream_t st) {
    if (B <= 0) return;
    if (a.stat) (void)hipMemsetAsync(a.stat, 0, (size_t)B * 16, st);
    const unsigned tiles = (unsigned)((max_out + LM_TILE - 1) / LM_TILE);
    hipLaunchKernelGGL(limiter_kernel, dim3(tiles > 0 ? tiles : 1, B), dim3(LM_THREADS), 0, st, a);
}

}  // namespace sts
