// gain_plan.hip -- per-phoneme volume envelopes on the decoder's float wave at the native rate (sts_set_gain_plan; include/summertts_hip.h
// has the full definition, DESIGN.md 9h the kernel structure).  For one utterance of F = max(1, sum d) frames of `hop` samples, phoneme i
// with the fixed-point gain q_i owning the samples of its d_i frames, half ramp width h:
//   Q[t] = q of the phoneme that owns t (2^20 where none does; Q[0] before the utterance, Q[N - 1] behind it);
//   S[t] = sum Q[t - h .. t + h] (64-bit);  env[t] = float32(S[t] / ((2h + 1) 2^20));  y[t] = x[t] env[t].
// Q and S are integers: the order in which a window is summed cannot change a bit, and env[t] is a function of the absolute sample index t
// only -- a streaming window gains its samples (halo included) at their positions in the utterance.
//
// Q is constant over a frame, so a workgroup stages one value PER FRAME that its tile +- h touches (an upper-bound search of the frame index
// in the utterance's inclusive cumulative frame counts: a phoneme of no frames can never be the answer, however many of them sit in a row)
// and the exclusive prefix E[k] = hop sum_{j < k} qf[j] over those frames.  With G(s) = sum_{u < s} Q[u], read off E and one product,
// S[t] = G(t + h + 1) - G(t - h): two closed-form evaluations per sample instead of a window walk, the same number for every h.
// The two staged arrays live in dynamic LDS sized by the launcher for the frames a tile +- kGainMaxH can touch at the launch's hop: 21
// entries (~0.3 KiB) at the 256 samples per frame of a model, 4898 (57 KiB) only at the one sample per frame sts_gain_plan_apply accepts.
// Samples leave in groups of 4 aligned in the packed buffer (one 16-byte load, one 16-byte and one 8-byte store per lane), sample by sample
// at a member's unaligned edges.
#include <math.h>
#include <stdint.h>

#include "../../include/summertts_hip.h"
#include "devmath.hpp"
#include "kernels.hpp"

namespace sts {

constexpr int GP_THREADS = 256, GP_TILE = 4096, GP_GROUP = 4;
// frames a tile +- h can touch: (nt + 2h) / hop + 2 at most
static inline int gp_max_frames(int hop) { return (GP_TILE + 2 * kGainMaxH) / hop + 2; }

bool gain_plan_valid(int n, const float* gain_db, float ramp_ms, const char** why) {
    if (n < 1) { *why = "gain plan: every utterance needs n >= 1 phonemes"; return false; }
    if (!(ramp_ms >= 0.f && ramp_ms <= 50.f)) { *why = "gain plan: ramp_ms must be finite and in [0, 50]"; return false; }
    if (gain_db)
        for (int i = 0; i < n; i++) {
            const float g = gain_db[i];
            if (!(g == -INFINITY || (g >= -96.f && g <= 24.f))) { *why = "gain plan: gain_db must be -INFINITY or finite in [-96, 24]"; return false; }
        }
    return true;
}

void gain_design(const float* gain_db, int n, float ramp_ms, int32_t* q, int32_t* h) {
    if (q)
        for (int i = 0; i < n; i++) {
            if (!gain_db) q[i] = kGainOne;
            else if (gain_db[i] == -INFINITY) q[i] = 0;
            else q[i] = (int32_t)floor(pow(10.0, (double)gain_db[i] / 20.0) * 1048576.0 + 0.5);
        }
    if (h) *h = (int32_t)floor((double)ramp_ms * 8.0 + 0.5);
}

__global__ __launch_bounds__(GP_THREADS) void gain_plan_kernel(GainArgs a) {
    extern __shared__ long long gp_lds[];           // [E: maxf + 1 long long | qf: maxf int], maxf = gp_max_frames(hop)
    __shared__ long long wsum[GP_THREADS / 64];
    const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hop = a.hop;
    long long* const E = gp_lds;
    int* const qf = (int*)(gp_lds + (GP_TILE + 2 * kGainMaxH) / hop + 3);
    // the member's samples in x / y / pcm, and where they sit in its utterance
    const long long xbase = (long long)(a.wseg.off ? a.wseg.off[m] : a.wseg.ioff) * hop;
    const long long xlen = (long long)(a.wseg.len ? a.wseg.len[m] : a.wseg.ilen) * hop;
    const long long s0 = (long long)blockIdx.x * GP_TILE;
    if (s0 >= xlen) return;
    const int nt = xlen - s0 < GP_TILE ? (int)(xlen - s0) : GP_TILE;
    const long long u0 = a.wtab ? a.wtab[(a.wstride ? a.wstride : 5) * (long long)m + a.wcol] : 0;
    const int b = a.utt ? a.utt[m] : m;
    const int toff = a.tseg.off ? a.tseg.off[b] : a.tseg.ioff, n = a.tseg.len ? a.tseg.len[b] : a.tseg.ilen;
    const int* cum = a.cum + toff;
    const int* q = a.q + toff;
    const int h = a.h[b];
    const int total = cum[n - 1];                   // frames the phonemes own (0: the utterance's one frame belongs to nobody)
    const long long F = total > 0 ? total : 1, N = F * hop;
    const long long t0 = u0 + s0;                   // the tile's first sample in the utterance; t0 + nt <= N
    // frames [fa, fb] hold every sample of [t0 - h, t0 + nt + h] that lies inside the utterance
    const long long lo = t0 - h > 0 ? t0 - h : 0;
    long long fa = lo / hop, fb = (t0 + nt + h) / hop;
    if (fa > F - 1) fa = F - 1;
    if (fb > F - 1) fb = F - 1;
    const int nf = (int)(fb - fa) + 1;              // <= (nt + 2h) / hop + 2 = the launcher's gp_max_frames(hop), as h <= kGainMaxH
    for (int j = tid; j < nf; j += GP_THREADS) {
        const int f = (int)(fa + j);
        int v = kGainOne;
        if (f < total) {                            // the first phoneme whose inclusive count exceeds f owns frame f
            int l = 0, r = n - 1;
            while (l < r) { const int mid = (l + r) >> 1; if (cum[mid] > f) r = mid; else l = mid + 1; }
            v = q[l];
        }
        qf[j] = v;
    }
    __syncthreads();
    // E[k] = hop * (qf[0] + .. + qf[k - 1]): a run of c frames per thread, the runs' sums scanned across the workgroup
    const int c = (nf + GP_THREADS - 1) / GP_THREADS;
    const int j0 = tid * c < nf ? tid * c : nf, j1 = j0 + c < nf ? j0 + c : nf;
    long long mine = 0;
    for (int j = j0; j < j1; j++) mine += qf[j];
    long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long long run = incl - mine;
    for (int w = 0; w < wave; w++) run += wsum[w];
    for (int j = j0; j < j1; j++) { E[j] = run * hop; run += qf[j]; }
    if (j1 == nf && j0 < nf) E[nf] = run * hop;
    __syncthreads();

    const long long base = fa * hop;                // absolute sample of local frame 0
    const long long q_first = qf[0], q_last = qf[nf - 1];
    // G(s) - G(base) for t0 - h <= s <= t0 + nt + h
    auto G = [&](long long s) -> long long {
        if (s < 0) return s * q_first;              // (then fa == 0: qf[0] is Q[0])
        if (s > N) return E[nf] + (s - N) * q_last; // (then fb == F - 1: qf[nf - 1] is Q[N - 1])
        const unsigned r = (unsigned)(s - base), k = r / (unsigned)hop, rem = r - k * (unsigned)hop;
        return rem ? E[k] + (long long)rem * qf[k] : E[k];
    };
    const double denom = (double)((long long)(2 * h + 1) << 20);
    auto gained = [&](long long t, float x) -> float {
        const long long S = G(t + h + 1) - G(t - h);
        return x * (float)((double)S / denom);
    };
    // the tile's samples at [D0, D0 + nt) of the packed buffers, in groups of 4 aligned there
    const long long D0 = xbase + s0, D1 = D0 + nt;
    const long long gfirst = D0 / GP_GROUP, glast = (D1 + GP_GROUP - 1) / GP_GROUP;
    for (long long gi = gfirst + tid; gi < glast; gi += GP_THREADS) {
        const long long i0 = gi * GP_GROUP;
        const long long t = t0 + (i0 - D0);
        if (i0 >= D0 && i0 + GP_GROUP <= D1) {
            const float4 x = *(const float4*)(a.x + i0);
            const float y0 = gained(t, x.x), y1 = gained(t + 1, x.y), y2 = gained(t + 2, x.z), y3 = gained(t + 3, x.w);
            if (a.y) *(float4*)(a.y + i0) = make_float4(y0, y1, y2, y3);
            if (a.pcm)
                *(uint2*)(a.pcm + i0) = make_uint2((uint32_t)(uint16_t)pcm_cast(y0) | ((uint32_t)(uint16_t)pcm_cast(y1) << 16),
                                                   (uint32_t)(uint16_t)pcm_cast(y2) | ((uint32_t)(uint16_t)pcm_cast(y3) << 16));
        } else {
            const long long il = i0 > D0 ? i0 : D0, ih = i0 + GP_GROUP < D1 ? i0 + GP_GROUP : D1;
            for (long long i = il; i < ih; i++) {
                const float y = gained(t0 + (i - D0), a.x[i]);
                if (a.y) a.y[i] = y;
                if (a.pcm) a.pcm[i] = pcm_cast(y);
            }
        }
    }
}

void gain_plan_run(const GainArgs& a, int nmem, long long max_len, hipStream_t st) {
    if (nmem <= 0) return;
    const unsigned tiles = (unsigned)((max_len + GP_TILE - 1) / GP_TILE);
    const int maxf = gp_max_frames(a.hop);
    const size_t lds = (size_t)(maxf + 1) * sizeof(long long) + (size_t)maxf * sizeof(int);
    hipLaunchKernelGGL(gain_plan_kernel, dim3(tiles > 0 ? tiles : 1, nmem), dim3(GP_THREADS), lds, st, a);
}

}  // namespace sts
