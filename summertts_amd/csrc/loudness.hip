// loudness.hip -- integrated loudness (ITU-R BS.1770-4, one channel, weight 1) and loudness normalisation of the float wave at the output
// rate (sts_set_loudness; include/summertts_hip.h has the full definition, DESIGN.md 9d the kernel structure).
//   K-weighting: two biquads in cascade (shelf, then high-pass), coefficients for any rate from the analog prototypes (kweight_coeffs);
//   blocks of 400 ms every 100 ms, absolute gate -70 LUFS, relative gate -10 LU; L = -0.691 + 10 log10(mean z of the gated blocks);
//   gain g = min(10^((T - L) / 20), 10^(C / 20) / peak) in float64, rounded to float32; PCM = pcm_cast(x * g).
//
// The IIR is sequential per utterance.  It runs as a two-level scan over chunks of LD_R samples (one per lane, LD_TILE per workgroup),
// everything in float64.  The state of the cascade (direct form I; the input history is read from x itself) is
//   s_n = (y1[n-1], y1[n-2], y2[n-1], y2[n-2]),   s_{n+1} = A s_n + (terms of x)
// so a chunk started from state s ends in M s + e, M = A^LD_R, e = its end state from zero state.  A workgroup scans the maps of its 256
// chunks (shuffles within a wave with M^(2^d), then the four waves in order); the tile's zero-start end state E_t goes to memory.  The next
// launch composes S_t = M^256 S_{t-1} + E_{t-1} for its tile, rebuilds the same scan, and re-runs every chunk from its true carry-in
// M^k S_t + Z_k, summing y^2 per 100 ms sub-block and max |x|.  Every sum has a fixed order and every chunk starts at a fixed offset from
// the utterance's first sample: an utterance's results are a function of its own samples only.
#include <math.h>
#include <stdint.h>

#include "devmath.hpp"
#include "kernels.hpp"
#include "loud_stream.hpp"

namespace sts {

constexpr int LD_THREADS = 256, LD_R = 32, LD_TILE = LD_THREADS * LD_R;     // 8192 samples per workgroup
constexpr int LD_SLOTS = 16;          // 100 ms sub-blocks one tile touches at most (S >= 800: 8192 / 800 + 2 <= 12)
constexpr int LD_LDS = LD_TILE + LD_TILE / LD_R;                              // one pad float per chunk: conflict-free strided reads
static_assert(LD_TILE == kLdsTile && LD_SLOTS == kLdsSlots, "loud_stream.hpp restates the tile and the slots per tile");

bool kweight_coeffs(int rate, double c[10]) {
    if (rate < kLoudMinRate || rate > kLoudMaxRate) return false;
    const double pi = 3.14159265358979323846, fs = (double)rate;
    {   // high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0; c[1] = 2.0 * (K * K - Vh) / a0; c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0; c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {   // high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0; c[9] = (1.0 - K / Q + K * K) / a0;
    }
    return true;
}

static void mat4_mul(const double* a, const double* b, double* o) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += a[i * 4 + k] * b[k * 4 + j];
            o[i * 4 + j] = s;
        }
}

bool loud_coef(int rate, LoudCoef* k) {
    double c[10];
    if (!kweight_coeffs(rate, c)) return false;
    for (int i = 0; i < 10; i++) k->c[i] = c[i];
    k->S = (int)floor(rate / 10.0 + 0.5);
    // homogeneous part of one step of the cascade on s = (y1[n-1], y1[n-2], y2[n-1], y2[n-2])
    const double A[16] = {-c[3], -c[4], 0.0, 0.0,
                          1.0, 0.0, 0.0, 0.0,
                          c[6] - c[5] * c[3], c[7] - c[5] * c[4], -c[8], -c[9],
                          0.0, 0.0, 1.0, 0.0};
    double M[16], t[16];
    for (int i = 0; i < 16; i++) M[i] = A[i];
    for (int r = 1; r < LD_R; r++) { mat4_mul(A, M, t); for (int i = 0; i < 16; i++) M[i] = t[i]; }   // A^LD_R
    for (int i = 0; i < 16; i++) k->Mp[0][i] = M[i];
    for (int d = 1; d < kLoudPow; d++) mat4_mul(k->Mp[d - 1], k->Mp[d - 1], k->Mp[d]);              // M^(2^d)
    return true;
}

size_t loud_ws_bytes(int B, long long total_samples) {
    const long long tiles = total_samples / LD_TILE + B + 1;
    return (size_t)B * 3 * 8 + (size_t)tiles * (4 * 8 + LD_SLOTS * 8 + 4) + (size_t)B * 4 + 1024;
}
void loud_ws_carve(LoudArgs& a, void* ws, int B, long long total_samples) {
    const long long tiles = total_samples / LD_TILE + B + 1;
    char* p = (char*)ws;
    a.utab = (long long*)p; p += (size_t)B * 3 * 8;
    a.E = (double*)p; p += (size_t)tiles * 4 * 8;
    a.tsum = (double*)p; p += (size_t)tiles * LD_SLOTS * 8;
    a.tpeak = (float*)p; p += (size_t)tiles * 4;
    a.gain = (float*)p;
}

__device__ __forceinline__ long long ld_len(const LoudArgs& a, int b) {
    const long long u = a.len ? (long long)a.len[b] : (long long)a.ilen;
    return (u * a.scale * a.P + a.Q - 1) / a.Q;
}

// o = Mx v
__device__ __forceinline__ void mv4(const double* Mx, const double v[4], double o[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = fma(Mx[i * 4 + 3], v[3], fma(Mx[i * 4 + 2], v[2], fma(Mx[i * 4 + 1], v[1], Mx[i * 4] * v[0])));
}
// v = M^n v for 0 <= n < 256 (n's bits, lowest first; the powers commute)
__device__ __forceinline__ void mpow_apply(const LoudCoef& k, int n, double v[4]) {
#pragma unroll
    for (int d = 0; d < 8; d++)
        if ((n >> d) & 1) { double o[4]; mv4(k.Mp[d], v, o); v[0] = o[0]; v[1] = o[1]; v[2] = o[2]; v[3] = o[3]; }
}

// x history of the chunk at utterance sample n0 (zero before the utterance's first sample)
__device__ __forceinline__ float ld_hist(const float* xu, long long n) { return n >= 0 ? xu[n] : 0.f; }

// Runs the cascade over xs[0 .. r) (LDS, stride 1) from state s with input history (xm1, xm2); s becomes the end state.  With ACC: the
// squares of the K-weighted output are summed into acc0 for the first `split` samples, acc1 for the rest.
template <bool ACC>
__device__ __forceinline__ void ld_chunk(const LoudCoef& k, const float* xs, int r, float xm1, float xm2, double s[4], int split,
                                         double& acc0, double& acc1) {
    const double b0 = k.c[0], b1 = k.c[1], b2 = k.c[2], a1 = k.c[3], a2 = k.c[4];
    const double h0 = k.c[5], h1 = k.c[6], h2 = k.c[7], c1 = k.c[8], c2 = k.c[9];
    double x1 = xm1, x2 = xm2, y1a = s[0], y1b = s[1], y2a = s[2], y2b = s[3];
    for (int i = 0; i < r; i++) {
        const double x0 = xs[i];
        const double y1 = fma(b0, x0, fma(b1, x1, fma(b2, x2, fma(-a1, y1a, -a2 * y1b))));
        const double y2 = fma(h0, y1, fma(h1, y1a, fma(h2, y1b, fma(-c1, y2a, -c2 * y2b))));
        if (ACC) { if (i < split) acc0 = fma(y2, y2, acc0); else acc1 = fma(y2, y2, acc1); }
        x2 = x1; x1 = x0; y1b = y1a; y1a = y1; y2b = y2a; y2a = y2;
    }
    s[0] = y1a; s[1] = y1b; s[2] = y2a; s[3] = y2b;
}

struct LdGeom { long long off, N, tbase; };

// utterance b's place in the packed signal and its first tile: sums over the utterances before it (a launch-ahead run's host does not know
// the lengths).  Integer sums: the order does not matter.
__device__ LdGeom ld_geom(const LoudArgs& a, int b, unsigned long long* s_red) {
    const int tid = threadIdx.x;
    if (tid < 2) s_red[tid] = 0;
    __syncthreads();
    unsigned long long po = 0, pt = 0;
    for (int q = tid; q < b; q += LD_THREADS) { const long long n = ld_len(a, q); po += (unsigned long long)n; pt += (unsigned long long)((n + LD_TILE - 1) / LD_TILE); }
    if (po) atomicAdd(&s_red[0], po);
    if (pt) atomicAdd(&s_red[1], pt);
    __syncthreads();
    LdGeom g{(long long)s_red[0], ld_len(a, b), (long long)s_red[1]};
    return g;
}

// Scans the chunk maps of a tile staged in LDS (sample p at p + p / LD_R, zeros behind the tile's last sample; this lane's chunk k = tid
// holds r <= LD_R samples and the input history (xm1, xm2)): returns this lane's carry-in relative to a zero tile start (Z) and, in et
// (every lane), the tile's zero-start end state.  A lane reads lower lanes and earlier waves only: Z of chunk k is a function of the
// chunks j < k, whatever lies behind them.
__device__ __forceinline__ void ld_scan_staged(const LoudCoef& k, const float* xs, double (*wt)[4], double Z[4], double et[4], int r,
                                               float xm1, float xm2) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double e[4] = {0.0, 0.0, 0.0, 0.0}, d0 = 0.0, d1 = 0.0;
    ld_chunk<false>(k, xs + tid * (LD_R + 1), r, xm1, xm2, e, 0, d0, d1);
    // inclusive scan within the wave: P_l = sum_{j <= l} M^(l - j) e_j
    double P[4] = {e[0], e[1], e[2], e[3]};
#pragma unroll
    for (int d = 0; d < 6; d++) {
        const int o = 1 << d;
        double q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = __shfl_up(P[i], o, 64);
        if (lane >= o) { double m[4]; mv4(k.Mp[d], q, m); for (int i = 0; i < 4; i++) P[i] += m[i]; }
    }
    double Pex[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { Pex[i] = __shfl_up(P[i], 1, 64); if (lane == 0) Pex[i] = 0.0; }
    if (lane == 63) for (int i = 0; i < 4; i++) wt[w][i] = P[i];
    __syncthreads();
    // the waves in order: W_w = M^64 W_{w-1} + T_{w-1}, W_0 = 0; the tile's end state is W_4
    double W[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < LD_THREADS / 64; q++) {
        if (q == w) for (int i = 0; i < 4; i++) Z[i] = W[i];
        double m[4]; mv4(k.Mp[6], W, m);
        for (int i = 0; i < 4; i++) W[i] = m[i] + wt[q][i];
    }
    for (int i = 0; i < 4; i++) et[i] = W[i];
    mpow_apply(k, lane, Z);
    for (int i = 0; i < 4; i++) Z[i] += Pex[i];
}

// Stages tile t of the utterance into LDS (sample p at p + p / LD_R) and scans its chunk maps (ld_scan_staged).
// Chunk k = samples [t LD_TILE + k LD_R, + r), r <= LD_R.
__device__ __forceinline__ void ld_tile_scan(const LoudArgs& a, const float* xu, long long N, long long t, float* xs, double (*wt)[4],
                                             double Z[4], double et[4], int& r, float& xm1, float& xm2) {
    const int tid = threadIdx.x;
    const long long t0 = t * LD_TILE;
    const long long nt = N - t0 < LD_TILE ? N - t0 : LD_TILE;
    for (int p = tid; p < LD_TILE; p += LD_THREADS) xs[p + p / LD_R] = p < nt ? xu[t0 + p] : 0.f;
    const long long n0 = t0 + (long long)tid * LD_R;
    r = N - n0 <= 0 ? 0 : (N - n0 < LD_R ? (int)(N - n0) : LD_R);
    xm1 = r > 0 ? ld_hist(xu, n0 - 1) : 0.f; xm2 = r > 0 ? ld_hist(xu, n0 - 2) : 0.f;
    __syncthreads();
    ld_scan_staged(a.k, xs, wt, Z, et, r, xm1, xm2);
}

// launch 1: every tile's zero-start end state E_t; block (0, b) also records utterance b's geometry
__global__ __launch_bounds__(LD_THREADS) void loud_scan_kernel(LoudArgs a) {
    __shared__ float xs[LD_LDS];
    __shared__ double wt[LD_THREADS / 64][4];
    __shared__ unsigned long long s_red[2];
    const int b = blockIdx.y;
    const LdGeom g = ld_geom(a, b, s_red);
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.utab[3 * b] = g.off; a.utab[3 * b + 1] = g.N; a.utab[3 * b + 2] = g.tbase; }
    const long long t = blockIdx.x;
    if (t * LD_TILE >= g.N) return;
    double Z[4], et[4]; int r; float xm1, xm2;
    ld_tile_scan(a, a.x + g.off, g.N, t, xs, wt, Z, et, r, xm1, xm2);
    if (threadIdx.x < 4) a.E[(g.tbase + t) * 4 + threadIdx.x] = et[threadIdx.x];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The true run of every chunk of a staged and scanned tile t whose last sample is utterance sample tend: S = the tile's carry S_t, Z this
// lane's carry-in relative to a zero tile start.  Sums y^2 per 100 ms sub-block (slot s = sub-block sb0 + s; a fixed reduction tree per
// slot) into ts[LD_SLOTS], max |x| of the tile into *tp.
__device__ __forceinline__ void ld_tile_sums(const LoudCoef& k, const float* xs, double (*red)[LD_SLOTS], float* pk, long long t, long long tend,
                                             int r, float xm1, float xm2, double S[4], const double Z[4], double* ts, float* tp) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    mpow_apply(k, tid, S);
    for (int i = 0; i < 4; i++) S[i] += Z[i];
    const int Ssb = k.S;
    const long long n0 = t * LD_TILE + (long long)tid * LD_R;
    const long long sb0 = (t * LD_TILE) / Ssb;
    const long long bin0 = n0 / Ssb;
    const int split = (int)((bin0 + 1) * Ssb - n0);
    double acc0 = 0.0, acc1 = 0.0;
    const float* xl = xs + tid * (LD_R + 1);
    ld_chunk<true>(k, xl, r, xm1, xm2, S, split, acc0, acc1);
    float p = 0.f;
    for (int i = 0; i < r; i++) p = fmaxf(p, fabsf(xl[i]));
    const int nslots = (int)(tend / Ssb - sb0 + 1);
    const int s0 = (int)(bin0 - sb0);
    for (int s = 0; s < nslots && s < LD_SLOTS; s++) {
        double v = r > 0 ? (s == s0 ? acc0 : (s == s0 + 1 ? acc1 : 0.0)) : 0.0;
        v = wave_sum(v);
        if (lane == 0) red[w][s] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p = fmaxf(p, __shfl_xor(p, o, 64));
    if (lane == 0) pk[w] = p;
    __syncthreads();
    if (tid < LD_SLOTS) ts[tid] = tid < nslots ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
    if (tid == 0) *tp = fmaxf(fmaxf(pk[0], pk[1]), fmaxf(pk[2], pk[3]));
}

// launch 2: the tile's carry S_t, the true run of every chunk, y^2 per 100 ms sub-block and max |x| of the tile
__global__ __launch_bounds__(LD_THREADS) void loud_measure_kernel(LoudArgs a) {
    __shared__ float xs[LD_LDS];
    __shared__ double wt[LD_THREADS / 64][4];
    __shared__ double red[LD_THREADS / 64][LD_SLOTS];
    __shared__ float pk[LD_THREADS / 64];
    const int b = blockIdx.y;
    const long long off = a.utab[3 * b], N = a.utab[3 * b + 1], tbase = a.utab[3 * b + 2];
    const long long t = blockIdx.x;
    if (t * LD_TILE >= N) return;
    const float* xu = a.x + off;
    double Z[4], et[4]; int r; float xm1, xm2;
    ld_tile_scan(a, xu, N, t, xs, wt, Z, et, r, xm1, xm2);
    // S_t = M^256 S_{t-1} + E_{t-1}, S_0 = 0 (every lane, same order)
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long q = 0; q < t; q++) {
        double m[4]; mv4(a.k.Mp[8], S, m);
        const double* Eq = a.E + (tbase + q) * 4;
        for (int i = 0; i < 4; i++) S[i] = m[i] + Eq[i];
    }
    const long long tend = (N - t * LD_TILE < LD_TILE ? N : (t + 1) * LD_TILE) - 1;
    ld_tile_sums(a.k, xs, red, pk, t, tend, r, xm1, xm2, S, Z, a.tsum + (tbase + t) * LD_SLOTS, a.tpeak + (tbase + t));
}

__device__ __forceinline__ double ld_subblock(const LoudArgs& a, long long tbase, long long j, int Ssb) {
    const long long ta = (j * Ssb) / LD_TILE, tb = ((j + 1) * Ssb - 1) / LD_TILE;
    double v = 0.0;
    for (long long t = ta; t <= tb; t++) v += a.tsum[(tbase + t) * LD_SLOTS + (j - (t * LD_TILE) / Ssb)];
    return v;
}
__device__ __forceinline__ double ld_block_z(const LoudArgs& a, long long tbase, long long j, int Ssb) {
    const double s = ((ld_subblock(a, tbase, j, Ssb) + ld_subblock(a, tbase, j + 1, Ssb)) + ld_subblock(a, tbase, j + 2, Ssb)) +
                     ld_subblock(a, tbase, j + 3, Ssb);
    return s / (4.0 * (double)Ssb);
}
__device__ __forceinline__ double ld_lufs(double z) { return -0.691 + 10.0 * log10(z); }

// sum and count over the workgroup (fixed tree)
__device__ void ld_block_reduce(double& v, int& n, double* sv, int* sn) {
    const int tid = threadIdx.x;
    sv[tid] = v; sn[tid] = n;
    __syncthreads();
    for (int o = LD_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { sv[tid] += sv[tid + o]; sn[tid] += sn[tid + o]; }
        __syncthreads();
    }
    v = sv[0]; n = sn[0];
    __syncthreads();
}

// launch 3: one workgroup per utterance -- blocks, both gates, L, the peak, the gain; results to a.out (mapped host memory in the engine)
__global__ __launch_bounds__(LD_THREADS) void loud_gate_kernel(LoudArgs a) {
    __shared__ double sv[LD_THREADS];
    __shared__ int sn[LD_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long N = a.utab[3 * b + 1], tbase = a.utab[3 * b + 2];
    const int Ssb = a.k.S;
    const long long nsb = N / Ssb, nblk = nsb >= 4 ? nsb - 3 : 0;
    double s1 = 0.0; int n1 = 0;
    for (long long j = tid; j < nblk; j += LD_THREADS) {
        const double z = ld_block_z(a, tbase, j, Ssb);
        if (ld_lufs(z) > -70.0) { s1 += z; n1++; }
    }
    ld_block_reduce(s1, n1, sv, sn);
    double L = -INFINITY; int n2 = 0;
    if (n1 > 0) {
        const double gr = ld_lufs(s1 / n1) - 10.0;
        double s2 = 0.0;
        for (long long j = tid; j < nblk; j += LD_THREADS) {
            const double z = ld_block_z(a, tbase, j, Ssb);
            const double l = ld_lufs(z);
            if (l > -70.0 && l > gr) { s2 += z; n2++; }
        }
        ld_block_reduce(s2, n2, sv, sn);
        if (n2 > 0) L = ld_lufs(s2 / n2);
    }
    if (tid != 0) return;
    float p = 0.f;
    const long long nt = (N + LD_TILE - 1) / LD_TILE;
    for (long long t = 0; t < nt; t++) p = fmaxf(p, a.tpeak[tbase + t]);
    double g = isfinite(L) ? pow(10.0, ((double)a.target - L) / 20.0) : 1.0;
    if (p > 0.f && !a.no_clamp) g = fmin(g, pow(10.0, (double)a.ceiling / 20.0) / (double)p);
    const float gf = (float)g;
    a.gain[b] = gf;
    if (a.out) {
        float* o = a.out + 4 * b;            // sts_loudness {lufs, peak, gain, blocks}
        o[0] = (float)L; o[1] = p; o[2] = gf;
        ((int32_t*)o)[3] = isfinite(L) ? n2 : 0;
    }
}

// launch 4 (normalising only): pcm = pcm_cast(x * g) -- per lane one 8-sample group of the packed signal (two 16-byte loads, one
// 16-byte store where the group lies inside the utterance; the utterance's edge groups sample by sample)
constexpr int LC_THREADS = 256, LC_GROUP = 8;
__global__ __launch_bounds__(LC_THREADS) void loud_gain_cast_kernel(LoudArgs a, int16_t* __restrict__ pcm) {
    const int b = blockIdx.y;
    const long long off = a.utab[3 * b], N = a.utab[3 * b + 1];
    const long long g0 = off / LC_GROUP, g1 = (off + N + LC_GROUP - 1) / LC_GROUP;
    const long long gi = g0 + (long long)blockIdx.x * LC_THREADS + threadIdx.x;
    if (gi >= g1 || N <= 0) return;
    const float gain = a.gain[b];
    const long long i0 = gi * LC_GROUP;
    if (i0 >= off && i0 + LC_GROUP <= off + N) {
        const float4 u = *(const float4*)(a.x + i0), v = *(const float4*)(a.x + i0 + 4);
        const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
        uint32_t wv[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            wv[i] = (uint32_t)(uint16_t)pcm_cast(f[2 * i] * gain) | ((uint32_t)(uint16_t)pcm_cast(f[2 * i + 1] * gain) << 16);
        *(uint4*)(pcm + i0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    } else {
        const long long lo = i0 > off ? i0 : off, hi = i0 + LC_GROUP < off + N ? i0 + LC_GROUP : off + N;
        for (long long i = lo; i < hi; i++) pcm[i] = pcm_cast(a.x[i] * gain);
    }
}

void loudness_run(const LoudArgs& a, int B, long long max_len, int16_t* pcm, hipStream_t st) {
    if (B <= 0) return;
    const unsigned tiles = (unsigned)((max_len + LD_TILE - 1) / LD_TILE);
    const dim3 grid(tiles > 0 ? tiles : 1, B);
    hipLaunchKernelGGL(loud_scan_kernel, grid, dim3(LD_THREADS), 0, st, a);
    if (tiles > 0) hipLaunchKernelGGL(loud_measure_kernel, grid, dim3(LD_THREADS), 0, st, a);
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(LD_THREADS), 0, st, a);
    if (pcm && max_len > 0)
        hipLaunchKernelGGL(loud_gain_cast_kernel, dim3((unsigned)((max_len / LC_GROUP + 2 + LC_THREADS - 1) / LC_THREADS), B), dim3(LC_THREADS), 0, st, a, pcm);
}

// ---- stream mode (LoudStreamArgs; loud_stream.hpp, DESIGN.md 9d "streamed") -----------------------------------------------------------
// A step continues utterance b from its carried state: input consumed up to e, the open tile te = e / LD_TILE with its carry S_te, its
// input so far and the two samples in front of it.  Workgroup (i, w) owns tile te + i of window w, up to the tile that holds j1.  It
// stages the tile's samples [t0, min(j1, t0 + LD_TILE)) -- those below e from the state, the others from the window, zeros beyond -- and
// runs ld_scan_staged / ld_tile_sums on them as the whole call does on a tile of an utterance that ends at j1: a chunk's carry-in reads
// the chunks in front of it only, so the sums of a tile the step completes are the whole call's, and those of the open tile are the
// whole call's of x[0 .. j1).  Launch 1 leaves the zero-start end state of every touched tile (used only of tiles the step completes) and
// the new open tile's input; launch 2 composes S_t = M^256 S_{t-1} + E_{t-1} upwards from S_te in the whole call's order and writes the
// sums, the peak and the new carry.  The state is read from one slot and written to the other: a step that runs twice starts twice from
// the same state, and writes the same sums.
struct LdsView {
    long long xbase, u0, j1, e, t0e, tbase;
    const double* sS; const float *sprev, *sx;
    double* dS; float *dprev, *dx;
};
__device__ __forceinline__ LdsView lds_view(const LoudStreamArgs& a, int w) {
    const long long* r = a.wtab + (size_t)kLdsRow * w;
    LdsView v;
    const long long b = r[0];
    v.xbase = r[1]; v.u0 = r[2]; v.j1 = r[4]; v.e = r[5]; v.tbase = r[6];
    v.t0e = v.e / LD_TILE * LD_TILE;
    char* rd = a.state + ((size_t)b * 2 + (size_t)a.slot) * kLdsSlotBytes;
    char* wr = a.state + ((size_t)b * 2 + (size_t)(1 - a.slot)) * kLdsSlotBytes;
    v.sS = (const double*)rd; v.sprev = (const float*)(rd + kLdsOffPrev); v.sx = (const float*)(rd + kLdsOffX);
    v.dS = (double*)wr; v.dprev = (float*)(wr + kLdsOffPrev); v.dx = (float*)(wr + kLdsOffX);
    return v;
}
// input sample n < j1 of the utterance: the window from e on, the state below it (the open tile, then the two samples in front of it)
__device__ __forceinline__ float lds_x(const LoudStreamArgs& a, const LdsView& v, long long n) {
    if (n < 0) return 0.f;
    if (n >= v.e) return a.x[v.xbase + (n - v.u0)];
    if (n >= v.t0e) return v.sx[n - v.t0e];
    return v.sprev[v.t0e - 1 - n];
}
// Stages the tile at t0's samples [0, nt) into LDS, zeros behind them, and sets this lane's chunk.  Ends with the barrier.
__device__ __forceinline__ void lds_stage(const LoudStreamArgs& a, const LdsView& v, long long t0, int nt, float* xs, int& r, float& xm1,
                                          float& xm2) {
    const int tid = threadIdx.x;
    const int pe = (int)(v.e - t0 < 0 ? 0 : (v.e - t0 < nt ? v.e - t0 : nt));      // [0, pe): consumed before this step (the open tile only)
    const float* xw = a.x + (v.xbase + (t0 - v.u0));                                // tile sample p >= pe is xw[p]
    for (int p = tid; p < LD_TILE; p += LD_THREADS) xs[p + p / LD_R] = p < pe ? v.sx[p] : (p < nt ? xw[p] : 0.f);
    const int c0 = tid * LD_R;
    r = nt - c0 <= 0 ? 0 : (nt - c0 < LD_R ? nt - c0 : LD_R);
    xm1 = r > 0 ? lds_x(a, v, t0 + c0 - 1) : 0.f; xm2 = r > 0 ? lds_x(a, v, t0 + c0 - 2) : 0.f;
    __syncthreads();
}

// stream launch 1: the zero-start end state of every tile the step touches; the tile that holds j1 leaves its input as the new open tile's
__global__ __launch_bounds__(LD_THREADS) void loud_stream_scan_kernel(LoudStreamArgs a) {
    __shared__ float xs[LD_LDS];
    __shared__ double wt[LD_THREADS / 64][4];
    const int w = blockIdx.y, tid = threadIdx.x;
    const LdsView v = lds_view(a, w);
    const long long t0 = v.t0e + (long long)blockIdx.x * LD_TILE;
    if (t0 > v.j1) return;
    const int nt = (int)(v.j1 - t0 < LD_TILE ? v.j1 - t0 : LD_TILE);
    int r; float xm1, xm2;
    lds_stage(a, v, t0, nt, xs, r, xm1, xm2);
    if (nt < LD_TILE) {         // (j1 lies in this tile: it is the open tile of the next step)
        for (int p = tid; p < nt; p += LD_THREADS) v.dx[p] = xs[p + p / LD_R];
        if (tid < 2) v.dprev[tid] = lds_x(a, v, t0 - 1 - tid);
    }
    double Z[4], et[4];
    ld_scan_staged(a.k, xs, wt, Z, et, r, xm1, xm2);
    if (tid < 4) a.E[((size_t)w * gridDim.x + blockIdx.x) * 4 + tid] = et[tid];
}

// stream launch 2: the tile's carry from the open tile's, the true run of every chunk, the tile's sums and peak, the new carry
__global__ __launch_bounds__(LD_THREADS) void loud_stream_measure_kernel(LoudStreamArgs a) {
    __shared__ float xs[LD_LDS];
    __shared__ double wt[LD_THREADS / 64][4];
    __shared__ double red[LD_THREADS / 64][LD_SLOTS];
    __shared__ float pk[LD_THREADS / 64];
    const int w = blockIdx.y, tid = threadIdx.x;
    const LdsView v = lds_view(a, w);
    const long long t0 = v.t0e + (long long)blockIdx.x * LD_TILE;
    if (t0 > v.j1) return;
    const int nt = (int)(v.j1 - t0 < LD_TILE ? v.j1 - t0 : LD_TILE);
    int r; float xm1, xm2;
    lds_stage(a, v, t0, nt, xs, r, xm1, xm2);
    double Z[4], et[4];
    ld_scan_staged(a.k, xs, wt, Z, et, r, xm1, xm2);
    // S_t upwards from the open tile's carry (zero at the utterance's start), the whole call's loop from there on
    double S[4];
    for (int i = 0; i < 4; i++) S[i] = v.e > 0 ? v.sS[i] : 0.0;
    const double* E = a.E + (size_t)w * gridDim.x * 4;
    for (int q = 0; q < (int)blockIdx.x; q++) {
        double m[4]; mv4(a.k.Mp[8], S, m);
        const double* Eq = E + (size_t)q * 4;
        for (int i = 0; i < 4; i++) S[i] = m[i] + Eq[i];
    }
    if (nt < LD_TILE && tid < 4) v.dS[tid] = S[tid];
    if (nt == 0) return;        // (j1 on a tile's edge: the new open tile is still empty -- its carry above is all there is to it)
    const long long t = t0 / LD_TILE;
    ld_tile_sums(a.k, xs, red, pk, t, t0 + nt - 1, r, xm1, xm2, S, Z, a.tsum + (v.tbase + t) * LD_SLOTS, a.tpeak + (v.tbase + t));
}

void loud_stream_run(const LoudStreamArgs& a, int nwin, long long max_tiles, hipStream_t st) {
    if (nwin <= 0 || max_tiles <= 0 || !a.wtab || !a.state || !a.E || !a.tsum || !a.tpeak) return;
    const dim3 grid((unsigned)max_tiles, nwin);
    hipLaunchKernelGGL(loud_stream_scan_kernel, grid, dim3(LD_THREADS), 0, st, a);
    hipLaunchKernelGGL(loud_stream_measure_kernel, grid, dim3(LD_THREADS), 0, st, a);
}

void loud_gate_run(const LoudArgs& a, int B, hipStream_t st) {
    if (B <= 0) return;
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(LD_THREADS), 0, st, a);
}

}  // namespace sts
