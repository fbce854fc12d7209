// eq.hip -- parametric equaliser on the float wave at the output rate (sts_set_eq; include/summertts_hip.h has the full definition,
// DESIGN.md 9j the kernel structure): a cascade of S <= 4 Audio-EQ-Cookbook biquads, direct form I in float64 from zero state per
// utterance, y = float32 of the last section, optionally pcm = pcm_cast(y).
//
// The IIR is sequential per utterance.  Like loudness.hip it runs as a two-level scan over chunks of EQ_R samples (one per lane, EQ_TILE
// per workgroup), everything in float64 -- here for a caller-chosen cascade, and with the filtered signal written out.  The state between
// two samples holds, per section s, (y_s[n-1], y_s[n-1] - y_s[n-2]): D = 2S values (section 1's input history is read from x itself).
// The (value, difference) basis keeps a pole pair next to z = 1 (20 Hz at q 8) well conditioned: the step matrix A then has entries of
// ordinary size where the basis (y[n-1], y[n-2]) has 2 and -1 cancelling to 1e-5.  A chunk started from state s ends in M s + e,
// M = A^EQ_R, e = its end state from zero state; the host builds M^(2^d) in long double and rounds once.  A is block lower triangular
// (section s reads sections <= s), so are its powers: the products skip the upper blocks.
//   launch 1: every tile's zero-start end state E_t (shuffles within a wave with M^(2^d), then the four waves in order).
//   launch 2: S_t = M^256 S_{t-1} + E_{t-1}, the same scan again, every chunk re-run from its true carry-in M^k S_t + Z_k by the
//             sequential recurrence of the definition; y (and the cast) leave through LDS in 16-byte groups.
// Every sum has a fixed order and every chunk starts at a fixed offset from the utterance's first sample: an utterance's output is a
// function of its own samples only.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "devmath.hpp"
#include "eq_stream.hpp"
#include "kernels.hpp"

namespace sts {

constexpr int EQ_THREADS = 256, EQ_R = 32, EQ_TILE = EQ_THREADS * EQ_R;       // 8192 samples per workgroup
constexpr int EQ_LDS = EQ_TILE + EQ_TILE / EQ_R;                                // one pad float per chunk: conflict-free strided access
constexpr int EQ_LD = kEqDim;                                                   // row stride of the tables
static_assert(EQ_TILE == kEqsTile && kEqDim == kEqsDim, "eq_stream.hpp restates the tile and the state's dimension");

bool eq_valid(int rate, int n_bands, const sts_eq_band* bands, const char** why) {
    const char* w = nullptr;
    if (rate < kEqMinRate || rate > kEqMaxRate) w = "eq: output rate outside [8000, 48000]";
    else if (n_bands < 0 || n_bands > kEqMaxBands) w = "eq: 0 to 4 bands";
    else if (n_bands > 0 && !bands) w = "eq: null bands";
    for (int i = 0; i < n_bands && !w; i++) {
        const sts_eq_band& b = bands[i];
        const double f = b.freq_hz, g = b.gain_db, q = b.q;
        if (b.type < STS_EQ_PEAK || b.type > STS_EQ_LOWPASS) w = "eq: band type 1 (peak), 2 (low shelf), 3 (high shelf), 4 (high-pass) or 5 (low-pass)";
        else if (!isfinite(f) || !isfinite(g) || !isfinite(q)) w = "eq: freq_hz, gain_db and q must be finite";
        else if (!(f >= 20.0 && f <= 0.45 * (double)rate)) w = "eq: freq_hz in [20, 0.45 x the output rate]";
        else if (!(q >= 0.1 && q <= 8.0)) w = "eq: q in [0.1, 8]";
        else if (!(g >= -24.0 && g <= 24.0)) w = "eq: gain_db in [-24, 24]";
        else if (q * (double)rate / f > 6400.0) w = "eq: q x rate / freq_hz must not exceed 6400 (poles too close to the unit circle)";
    }
    if (why) *why = w;
    return w == nullptr;
}

void eq_design(int rate, int n_bands, const sts_eq_band* bands, double* coeffs) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n_bands; i++) {
        const sts_eq_band& bd = bands[i];
        const double A = pow(10.0, (double)bd.gain_db / 40.0), w0 = 2.0 * pi * (double)bd.freq_hz / (double)rate;
        const double cw = cos(w0), sw = sin(w0), al = sw / (2.0 * (double)bd.q);
        double b[3], a[3];
        switch (bd.type) {
        case STS_EQ_PEAK:
            b[0] = 1.0 + al * A; b[1] = -2.0 * cw; b[2] = 1.0 - al * A;
            a[0] = 1.0 + al / A; a[1] = -2.0 * cw; a[2] = 1.0 - al / A;
            break;
        case STS_EQ_HIGHPASS:
            b[0] = (1.0 + cw) / 2.0; b[1] = -(1.0 + cw); b[2] = (1.0 + cw) / 2.0;
            a[0] = 1.0 + al; a[1] = -2.0 * cw; a[2] = 1.0 - al;
            break;
        case STS_EQ_LOWPASS:
            b[0] = (1.0 - cw) / 2.0; b[1] = 1.0 - cw; b[2] = (1.0 - cw) / 2.0;
            a[0] = 1.0 + al; a[1] = -2.0 * cw; a[2] = 1.0 - al;
            break;
        case STS_EQ_LOWSHELF: {
            const double s = 2.0 * sqrt(A) * al;
            b[0] = A * ((A + 1.0) - (A - 1.0) * cw + s); b[1] = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw); b[2] = A * ((A + 1.0) - (A - 1.0) * cw - s);
            a[0] = (A + 1.0) + (A - 1.0) * cw + s; a[1] = -2.0 * ((A - 1.0) + (A + 1.0) * cw); a[2] = (A + 1.0) + (A - 1.0) * cw - s;
            break;
        }
        default: {  // STS_EQ_HIGHSHELF
            const double s = 2.0 * sqrt(A) * al;
            b[0] = A * ((A + 1.0) + (A - 1.0) * cw + s); b[1] = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw); b[2] = A * ((A + 1.0) + (A - 1.0) * cw - s);
            a[0] = (A + 1.0) - (A - 1.0) * cw + s; a[1] = 2.0 * ((A - 1.0) - (A + 1.0) * cw); a[2] = (A + 1.0) - (A - 1.0) * cw - s;
            break;
        }
        }
        double* c = coeffs + 5 * i;
        c[0] = b[0] / a[0]; c[1] = b[1] / a[0]; c[2] = b[2] / a[0]; c[3] = a[1] / a[0]; c[4] = a[2] / a[0];
    }
}

// the tables of a cascade: the coefficients, and M^(2^d) for the chunk map M = A^EQ_R in the (value, difference) basis.  A's columns are
// one homogeneous step of the cascade from each basis state; everything in long double, rounded once.
void eq_table(int S, const double* coeffs, EqTable* t) {
    typedef long double ld;
    *t = EqTable{};
    const int D = 2 * S;
    for (int s = 0; s < S; s++) for (int i = 0; i < 5; i++) t->c[s][i] = coeffs[5 * s + i];
    ld A[kEqDim][kEqDim] = {}, M[kEqDim][kEqDim] = {}, T[kEqDim][kEqDim] = {};
    for (int j = 0; j < D; j++) {
        ld y1[kEqMaxBands] = {}, y2[kEqMaxBands] = {};
        if (j & 1) y2[j / 2] = -1.0L; else { y1[j / 2] = 1.0L; y2[j / 2] = 1.0L; }
        ld v0 = 0.0L, v1 = 0.0L, v2 = 0.0L;
        for (int s = 0; s < S; s++) {
            const double* c = coeffs + 5 * s;
            const ld w = (ld)c[0] * v0 + (ld)c[1] * v1 + (ld)c[2] * v2 - (ld)c[3] * y1[s] - (ld)c[4] * y2[s];
            v1 = y1[s]; v2 = y2[s];
            y2[s] = y1[s]; y1[s] = w; v0 = w;
        }
        for (int s = 0; s < S; s++) { A[2 * s][j] = y1[s]; A[2 * s + 1][j] = y1[s] - y2[s]; }
    }
    auto mul = [&](const ld (*a)[kEqDim], const ld (*b)[kEqDim], ld (*o)[kEqDim]) {
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) {
                ld s = 0.0L;
                for (int k = 0; k < D; k++) s += a[i][k] * b[k][j];
                o[i][j] = s;
            }
    };
    for (int i = 0; i < D; i++) M[i][i] = 1.0L;
    for (int r = 0; r < EQ_R; r++) { mul(A, M, T); memcpy(M, T, sizeof(M)); }          // A^EQ_R
    for (int d = 0; d < kEqPow; d++) {
        for (int i = 0; i < D; i++) for (int j = 0; j < D; j++) t->Mp[d][i * EQ_LD + j] = (double)M[i][j];
        mul(M, M, T); memcpy(M, T, sizeof(M));                                           // M^(2^d)
    }
}

static long long eq_tiles(int B, long long total_samples) { return total_samples / EQ_TILE + B + 1; }
size_t eq_ws_bytes(int B, long long total_samples) {
    return (size_t)B * 3 * 8 + (size_t)eq_tiles(B, total_samples) * kEqDim * 8 + 256;
}
void eq_ws_carve(EqArgs& a, void* ws, int B, long long total_samples) {
    (void)total_samples;
    char* p = (char*)ws;
    a.utab = (long long*)p; p += (size_t)B * 3 * 8;
    a.E = (double*)p;
}

__device__ __forceinline__ long long eq_len(const EqArgs& a, int b) {
    const long long u = a.len ? (long long)a.len[b] : (long long)a.ilen;
    return (u * a.scale * a.P + a.Q - 1) / a.Q;
}

// o = Mx v over the block-lower-triangular part (row i reads columns 0 .. 2 (i / 2) + 1), ascending
template <int S>
__device__ __forceinline__ void eq_mv(const double* __restrict__ Mx, const double (&v)[2 * S], double (&o)[2 * S]) {
#pragma unroll
    for (int i = 0; i < 2 * S; i++) {
        double acc = Mx[i * EQ_LD] * v[0];
#pragma unroll
        for (int j = 1; j < 2 * (i / 2) + 2; j++) acc = fma(Mx[i * EQ_LD + j], v[j], acc);
        o[i] = acc;
    }
}
// v = M^n v for 0 <= n < 2^BITS (n's bits, lowest first; the powers commute)
template <int S, int BITS>
__device__ __forceinline__ void eq_mpow(const EqTable* __restrict__ k, int n, double (&v)[2 * S]) {
#pragma unroll
    for (int d = 0; d < BITS; d++)
        if ((n >> d) & 1) {
            double o[2 * S];
            eq_mv<S>(k->Mp[d], v, o);
#pragma unroll
            for (int i = 0; i < 2 * S; i++) v[i] = o[i];
        }
}

// Runs the cascade over xs[0 .. r) (LDS, stride 1) from state st with input history (xm1, xm2): the recurrence of the definition, section
// by section; st becomes the end state.  With OUT: xs[i] = float32 of the last section's output, in place.
template <int S, bool OUT>
__device__ __forceinline__ void eq_chunk(const double (&c)[S][5], float* xs, int r, float xm1, float xm2, double (&st)[2 * S]) {
    double x1 = xm1, x2 = xm2, y1[S], y2[S];
#pragma unroll
    for (int s = 0; s < S; s++) { y1[s] = st[2 * s]; y2[s] = st[2 * s] - st[2 * s + 1]; }
    for (int i = 0; i < r; i++) {
        const double x0 = xs[i];
        double v0 = x0, v1 = x1, v2 = x2;
#pragma unroll
        for (int s = 0; s < S; s++) {
            const double w = fma(c[s][0], v0, fma(c[s][1], v1, fma(c[s][2], v2, fma(-c[s][3], y1[s], -c[s][4] * y2[s]))));
            v1 = y1[s]; v2 = y2[s];
            y2[s] = y1[s]; y1[s] = w; v0 = w;
        }
        if (OUT) xs[i] = (float)v0;
        x2 = x1; x1 = x0;
    }
#pragma unroll
    for (int s = 0; s < S; s++) { st[2 * s] = y1[s]; st[2 * s + 1] = y1[s] - y2[s]; }
}

struct EqGeom { long long off, N, tbase; };

// utterance b's place in the packed signal and its first tile: sums over the utterances before it (a launch-ahead run's host does not know
// the lengths).  Integer sums: the order does not matter.
__device__ __forceinline__ EqGeom eq_geom(const EqArgs& a, int b, unsigned long long* s_red) {
    const int tid = threadIdx.x;
    if (tid < 2) s_red[tid] = 0;
    __syncthreads();
    unsigned long long po = 0, pt = 0;
    for (int q = tid; q < b; q += EQ_THREADS) { const long long n = eq_len(a, q); po += (unsigned long long)n; pt += (unsigned long long)((n + EQ_TILE - 1) / EQ_TILE); }
    if (po) atomicAdd(&s_red[0], po);
    if (pt) atomicAdd(&s_red[1], pt);
    __syncthreads();
    EqGeom g{(long long)s_red[0], eq_len(a, b), (long long)s_red[1]};
    return g;
}

// The tile's samples move between memory and LDS in groups of four consecutive samples whose first sample sits at a 16-byte address of x:
// group g holds tile samples [4 g - h, 4 g - h + 4), h = the tile's first sample's index in its 16-byte line.  A group that lies inside
// [0, nt) moves as one vector where the other side's address is aligned too; the utterance's edge groups go sample by sample.
__device__ __forceinline__ int eq_phase(const float* p) { return (int)(((uintptr_t)p >> 2) & 3); }

// Scans the chunk maps of a tile staged in LDS (sample p at p + p / EQ_R; this lane's chunk k = tid holds r <= EQ_R samples and the input
// history (xm1, xm2)): returns this lane's carry-in relative to a zero tile start (Z) and, in et (every lane), the tile's zero-start end
// state.  A lane reads lower lanes and earlier waves only: Z of chunk k is a function of the chunks j < k, whatever lies behind them.
template <int S>
__device__ __forceinline__ void eq_scan_staged(const EqArgs& a, const double (&c)[S][5], float* xs, double (*wt)[kEqDim], double (&Z)[2 * S],
                                               double (&et)[2 * S], int r, float xm1, float xm2) {
    constexpr int D = 2 * S;
    const EqTable* __restrict__ k = a.tab;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double P[D];
#pragma unroll
    for (int i = 0; i < D; i++) P[i] = 0.0;
    eq_chunk<S, false>(c, xs + tid * (EQ_R + 1), r, xm1, xm2, P);
    // inclusive scan within the wave: P_l = sum_{j <= l} M^(l - j) e_j
#pragma unroll
    for (int d = 0; d < 6; d++) {
        const int o = 1 << d;
        double q[D], m[D];
#pragma unroll
        for (int i = 0; i < D; i++) q[i] = __shfl_up(P[i], o, 64);
        eq_mv<S>(k->Mp[d], q, m);
        if (lane >= o) {
#pragma unroll
            for (int i = 0; i < D; i++) P[i] += m[i];
        }
    }
    double Pex[D];
#pragma unroll
    for (int i = 0; i < D; i++) { Pex[i] = __shfl_up(P[i], 1, 64); if (lane == 0) Pex[i] = 0.0; }
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < D; i++) wt[w][i] = P[i];
    }
    __syncthreads();
    // the waves in order: W_w = M^64 W_{w-1} + T_{w-1}, W_0 = 0; the tile's end state is W_4
    double W[D];
#pragma unroll
    for (int i = 0; i < D; i++) { W[i] = 0.0; Z[i] = 0.0; }
#pragma unroll
    for (int q = 0; q < EQ_THREADS / 64; q++) {
        if (q == w) {
#pragma unroll
            for (int i = 0; i < D; i++) Z[i] = W[i];
        }
        double m[D];
        eq_mv<S>(k->Mp[6], W, m);
#pragma unroll
        for (int i = 0; i < D; i++) W[i] = m[i] + wt[q][i];
    }
#pragma unroll
    for (int i = 0; i < D; i++) et[i] = W[i];
    eq_mpow<S, 6>(k, lane, Z);
#pragma unroll
    for (int i = 0; i < D; i++) Z[i] += Pex[i];
}

// Stages tile t of the utterance into LDS (sample p at p + p / EQ_R) and scans its chunk maps (eq_scan_staged).
// Chunk k = samples [t EQ_TILE + k EQ_R, + r), r <= EQ_R.
template <int S>
__device__ __forceinline__ void eq_tile_scan(const EqArgs& a, const double (&c)[S][5], const float* xu, long long N, long long t, float* xs,
                             double (*wt)[kEqDim], double (&Z)[2 * S], double (&et)[2 * S], int& r, float& xm1, float& xm2) {
    const int tid = threadIdx.x;
    const long long t0 = t * EQ_TILE;
    const int nt = (int)(N - t0 < EQ_TILE ? N - t0 : EQ_TILE);
    const float* xt = xu + t0;
    const int h = eq_phase(xt);
    for (int g = tid; g < EQ_TILE / 4 + 1; g += EQ_THREADS) {
        const int p0 = 4 * g - h;
        if (p0 >= 0 && p0 + 4 <= nt) {
            const float4 v = *(const float4*)(xt + p0);
            xs[p0 + p0 / EQ_R] = v.x; xs[p0 + 1 + (p0 + 1) / EQ_R] = v.y; xs[p0 + 2 + (p0 + 2) / EQ_R] = v.z; xs[p0 + 3 + (p0 + 3) / EQ_R] = v.w;
        } else {
            const int lo = p0 > 0 ? p0 : 0, hi = p0 + 4 < nt ? p0 + 4 : nt;
            for (int p = lo; p < hi; p++) xs[p + p / EQ_R] = xt[p];
        }
    }
    const long long n0 = t0 + (long long)tid * EQ_R;
    r = N - n0 <= 0 ? 0 : (N - n0 < EQ_R ? (int)(N - n0) : EQ_R);
    xm1 = r > 0 && n0 >= 1 ? xu[n0 - 1] : 0.f; xm2 = r > 0 && n0 >= 2 ? xu[n0 - 2] : 0.f;
    __syncthreads();
    eq_scan_staged<S>(a, c, xs, wt, Z, et, r, xm1, xm2);
}

template <int S>
__device__ __forceinline__ void eq_load_coef(const EqArgs& a, double (&c)[S][5]) {
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int i = 0; i < 5; i++) c[s][i] = a.tab->c[s][i];
}

// launch 1: every tile's zero-start end state E_t; block (0, b) also records utterance b's geometry
template <int S>
__global__ __launch_bounds__(EQ_THREADS) void eq_scan_kernel(EqArgs a) {
    __shared__ float xs[EQ_LDS];
    __shared__ double wt[EQ_THREADS / 64][kEqDim];
    __shared__ unsigned long long s_red[2];
    const int b = blockIdx.y;
    const EqGeom g = eq_geom(a, b, s_red);
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.utab[3 * b] = g.off; a.utab[3 * b + 1] = g.N; a.utab[3 * b + 2] = g.tbase; }
    const long long t = blockIdx.x;
    if (t * EQ_TILE >= g.N) return;
    double c[S][5];
    eq_load_coef<S>(a, c);
    double Z[2 * S], et[2 * S]; int r; float xm1, xm2;
    eq_tile_scan<S>(a, c, a.x + g.off, g.N, t, xs, wt, Z, et, r, xm1, xm2);
#pragma unroll
    for (int i = 0; i < 2 * S; i++)
        if (threadIdx.x == i) a.E[(g.tbase + t) * kEqDim + i] = et[i];
}

// launch 2: the tile's carry S_t, the true run of every chunk in place in LDS, then y and the cast out of LDS
template <int S>
__global__ __launch_bounds__(EQ_THREADS) void eq_apply_kernel(EqArgs a) {
    constexpr int D = 2 * S;
    __shared__ float xs[EQ_LDS];
    __shared__ double wt[EQ_THREADS / 64][kEqDim];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long off = a.utab[3 * b], N = a.utab[3 * b + 1], tbase = a.utab[3 * b + 2];
    const long long t = blockIdx.x;
    if (t * EQ_TILE >= N) return;
    const EqTable* __restrict__ k = a.tab;
    double c[S][5];
    eq_load_coef<S>(a, c);
    const float* xu = a.x + off;
    double Z[D], et[D]; int r; float xm1, xm2;
    eq_tile_scan<S>(a, c, xu, N, t, xs, wt, Z, et, r, xm1, xm2);
    // S_t = M^256 S_{t-1} + E_{t-1}, S_0 = 0 (every lane, same order)
    double St[D];
#pragma unroll
    for (int i = 0; i < D; i++) St[i] = 0.0;
    for (long long q = 0; q < t; q++) {
        double m[D];
        eq_mv<S>(k->Mp[8], St, m);
        const double* Eq = a.E + (tbase + q) * kEqDim;
#pragma unroll
        for (int i = 0; i < D; i++) St[i] = m[i] + Eq[i];
    }
    eq_mpow<S, 8>(k, tid, St);
#pragma unroll
    for (int i = 0; i < D; i++) St[i] += Z[i];
    eq_chunk<S, true>(c, xs + tid * (EQ_R + 1), r, xm1, xm2, St);
    __syncthreads();
    // out of LDS: the groups of the load, a vector where the destination is aligned as well
    const long long t0 = t * EQ_TILE;
    const int nt = (int)(N - t0 < EQ_TILE ? N - t0 : EQ_TILE);
    const int h = eq_phase(xu + t0);
    float* yt = a.y ? a.y + off + t0 : nullptr;
    int16_t* pt = a.pcm ? a.pcm + off + t0 : nullptr;
    for (int g = tid; g < EQ_TILE / 4 + 1; g += EQ_THREADS) {
        const int p0 = 4 * g - h;
        const int lo = p0 > 0 ? p0 : 0, hi = p0 + 4 < nt ? p0 + 4 : nt;
        if (lo >= hi) continue;
        const bool whole = p0 >= 0 && p0 + 4 <= nt;
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { const int p = p0 + i; f[i] = p >= lo && p < hi ? xs[p + p / EQ_R] : 0.f; }
        if (yt) {
            if (whole && (((uintptr_t)(yt + p0)) & 15) == 0) *(float4*)(yt + p0) = make_float4(f[0], f[1], f[2], f[3]);
            else for (int p = lo; p < hi; p++) yt[p] = f[p - p0];
        }
        if (pt) {
            if (whole && (((uintptr_t)(pt + p0)) & 7) == 0)
                *(uint2*)(pt + p0) = make_uint2((uint32_t)(uint16_t)pcm_cast(f[0]) | ((uint32_t)(uint16_t)pcm_cast(f[1]) << 16),
                                                (uint32_t)(uint16_t)pcm_cast(f[2]) | ((uint32_t)(uint16_t)pcm_cast(f[3]) << 16));
            else for (int p = lo; p < hi; p++) pt[p] = pcm_cast(f[p - p0]);
        }
    }
}

template <int S>
static void eq_launch(const EqArgs& a, dim3 grid, bool apply, hipStream_t st) {
    hipLaunchKernelGGL(eq_scan_kernel<S>, grid, dim3(EQ_THREADS), 0, st, a);
    if (apply) hipLaunchKernelGGL(eq_apply_kernel<S>, grid, dim3(EQ_THREADS), 0, st, a);
}

void eq_run(const EqArgs& a, int B, long long max_len, hipStream_t st) {
    if (B <= 0 || a.S < 1 || a.S > kEqMaxBands) return;
    const unsigned tiles = (unsigned)((max_len + EQ_TILE - 1) / EQ_TILE);
    const dim3 grid(tiles > 0 ? tiles : 1, B);
    switch (a.S) {
    case 1: eq_launch<1>(a, grid, tiles > 0, st); break;
    case 2: eq_launch<2>(a, grid, tiles > 0, st); break;
    case 3: eq_launch<3>(a, grid, tiles > 0, st); break;
    default: eq_launch<4>(a, grid, tiles > 0, st); break;
    }
}

// ---- stream mode (EqArgs::wtab; eq_stream.hpp, DESIGN.md 9j "streamed") ---------------------------------------------------------------
// A step continues utterance b from its carried state: input consumed up to e, the open tile te = e / EQ_TILE with its carry S_te, its
// input so far and the two samples in front of it, and a ring of the last y.  Workgroup (i, w) owns tile te + i of window w, up to the tile
// that holds o1.  It stages the tile's samples [t0, min(o1, t0 + EQ_TILE)) -- those below e from the state, the others from the window --
// and runs eq_scan_staged / eq_chunk on them as the whole call does on the complete tile: a chunk's carry-in reads the chunks in front of
// it only, so every y it produces is the whole call's.  Launch 1 leaves the zero-start end state of every touched tile (used only of
// tiles the step completes) and the new open tile's input; launch 2 composes S_t = M^256 S_{t-1} + E_{t-1} upwards from S_te in the whole
// call's order, writes y, the cast and the new state.  The state is read from one slot and written to the other: a step that runs twice
// starts twice from the same state.
struct EqsView {
    long long xbase, u0, o0, o1, ybase, j0, j1, pdst, e, t0e;
    const double* sS; const float *sprev, *sx, *sy;
    double* dS; float *dprev, *dx, *dy;
};
__device__ __forceinline__ EqsView eqs_view(const EqArgs& a, int w) {
    const long long* r = a.wtab + (size_t)kEqsRow * w;
    EqsView v;
    const long long b = r[0];
    v.xbase = r[1]; v.u0 = r[2]; v.o0 = r[4]; v.o1 = r[5]; v.ybase = r[6]; v.j0 = r[7]; v.j1 = r[8]; v.pdst = r[9]; v.e = r[10];
    v.t0e = v.e / EQ_TILE * EQ_TILE;
    char* rd = a.state + ((size_t)b * 2 + (size_t)a.slot) * kEqsSlotBytes;
    char* wr = a.state + ((size_t)b * 2 + (size_t)(1 - a.slot)) * kEqsSlotBytes;
    v.sS = (const double*)rd; v.sprev = (const float*)(rd + kEqsOffPrev); v.sx = (const float*)(rd + kEqsOffX); v.sy = (const float*)(rd + kEqsOffY);
    v.dS = (double*)wr; v.dprev = (float*)(wr + kEqsOffPrev); v.dx = (float*)(wr + kEqsOffX); v.dy = (float*)(wr + kEqsOffY);
    return v;
}
// input sample n < o1 of the utterance: the window from e on, the state below it (the open tile, then the two samples in front of it)
__device__ __forceinline__ float eqs_x(const EqArgs& a, const EqsView& v, long long n) {
    if (n < 0) return 0.f;
    if (n >= v.e) return a.x[v.xbase + (n - v.u0)];
    if (n >= v.t0e) return v.sx[n - v.t0e];
    return v.sprev[v.t0e - 1 - n];
}
// Stages tile t0 / EQ_TILE's samples [0, nt) into LDS and sets this lane's chunk: 16-byte groups on either source where a group of four
// is whole there, sample by sample at the seam and the edges.  Ends with the barrier.
__device__ __forceinline__ void eqs_stage(const EqArgs& a, const EqsView& v, long long t0, int nt, float* xs, int& r, float& xm1, float& xm2) {
    const int tid = threadIdx.x;
    const int pe = (int)(v.e - t0 < 0 ? 0 : (v.e - t0 < nt ? v.e - t0 : nt));      // [0, pe): consumed before this step (the open tile only)
    for (int g = tid; 4 * g < pe; g += EQ_THREADS) {
        const int p0 = 4 * g;
        if (p0 + 4 <= pe) {
            const float4 q = *(const float4*)(v.sx + p0);
            xs[p0 + p0 / EQ_R] = q.x; xs[p0 + 1 + (p0 + 1) / EQ_R] = q.y; xs[p0 + 2 + (p0 + 2) / EQ_R] = q.z; xs[p0 + 3 + (p0 + 3) / EQ_R] = q.w;
        } else {
            for (int p = p0; p < pe; p++) xs[p + p / EQ_R] = v.sx[p];
        }
    }
    const long long off = v.xbase + (t0 - v.u0);                                    // tile sample p is a.x[off + p], for p >= pe
    const int h = (int)(((long long)((uintptr_t)a.x >> 2) + off) & 3);
    for (int g = tid; g < EQ_TILE / 4 + 1; g += EQ_THREADS) {
        const int p0 = 4 * g - h;
        const int lo = p0 > pe ? p0 : pe, hi = p0 + 4 < nt ? p0 + 4 : nt;
        if (lo >= hi) continue;
        if (lo == p0 && hi == p0 + 4) {
            const float4 q = *(const float4*)(a.x + (off + p0));
            xs[p0 + p0 / EQ_R] = q.x; xs[p0 + 1 + (p0 + 1) / EQ_R] = q.y; xs[p0 + 2 + (p0 + 2) / EQ_R] = q.z; xs[p0 + 3 + (p0 + 3) / EQ_R] = q.w;
        } else {
            for (int p = lo; p < hi; p++) xs[p + p / EQ_R] = a.x[off + p];
        }
    }
    const int c0 = tid * EQ_R;
    r = nt - c0 <= 0 ? 0 : (nt - c0 < EQ_R ? nt - c0 : EQ_R);
    xm1 = r > 0 ? eqs_x(a, v, t0 + c0 - 1) : 0.f; xm2 = r > 0 ? eqs_x(a, v, t0 + c0 - 2) : 0.f;
    __syncthreads();
}
// tile samples [lo, hi) out of LDS to dst[off + p]: 16-byte groups where four are whole and aligned at the destination
__device__ __forceinline__ void eqs_store_f(const float* xs, float* dst, long long off, int lo, int hi) {
    const int h = (int)(((long long)((uintptr_t)dst >> 2) + off) & 3);
    for (int g = threadIdx.x; g < EQ_TILE / 4 + 1; g += EQ_THREADS) {
        const int p0 = 4 * g - h;
        const int l = p0 > lo ? p0 : lo, u = p0 + 4 < hi ? p0 + 4 : hi;
        if (l >= u) continue;
        if (l == p0 && u == p0 + 4)
            *(float4*)(dst + (off + p0)) = make_float4(xs[p0 + p0 / EQ_R], xs[p0 + 1 + (p0 + 1) / EQ_R], xs[p0 + 2 + (p0 + 2) / EQ_R], xs[p0 + 3 + (p0 + 3) / EQ_R]);
        else for (int p = l; p < u; p++) dst[off + p] = xs[p + p / EQ_R];
    }
}
__device__ __forceinline__ void eqs_store_pcm(const float* xs, int16_t* dst, long long off, int lo, int hi) {
    const int h = (int)(((long long)((uintptr_t)dst >> 1) + off) & 3);
    for (int g = threadIdx.x; g < EQ_TILE / 4 + 1; g += EQ_THREADS) {
        const int p0 = 4 * g - h;
        const int l = p0 > lo ? p0 : lo, u = p0 + 4 < hi ? p0 + 4 : hi;
        if (l >= u) continue;
        if (l == p0 && u == p0 + 4) {
            const float f0 = xs[p0 + p0 / EQ_R], f1 = xs[p0 + 1 + (p0 + 1) / EQ_R], f2 = xs[p0 + 2 + (p0 + 2) / EQ_R], f3 = xs[p0 + 3 + (p0 + 3) / EQ_R];
            *(uint2*)(dst + (off + p0)) = make_uint2((uint32_t)(uint16_t)pcm_cast(f0) | ((uint32_t)(uint16_t)pcm_cast(f1) << 16),
                                                     (uint32_t)(uint16_t)pcm_cast(f2) | ((uint32_t)(uint16_t)pcm_cast(f3) << 16));
        } else for (int p = l; p < u; p++) dst[off + p] = pcm_cast(xs[p + p / EQ_R]);
    }
}

// stream launch 1: the zero-start end state of every tile the step touches; the tile that holds o1 leaves its input as the new open tile's
template <int S>
__global__ __launch_bounds__(EQ_THREADS) void eq_stream_scan_kernel(EqArgs a) {
    __shared__ float xs[EQ_LDS];
    __shared__ double wt[EQ_THREADS / 64][kEqDim];
    const int w = blockIdx.y, tid = threadIdx.x;
    const EqsView v = eqs_view(a, w);
    const long long t0 = v.t0e + (long long)blockIdx.x * EQ_TILE;
    if (t0 > v.o1) return;
    const int nt = (int)(v.o1 - t0 < EQ_TILE ? v.o1 - t0 : EQ_TILE);
    double c[S][5];
    eq_load_coef<S>(a, c);
    int r; float xm1, xm2;
    eqs_stage(a, v, t0, nt, xs, r, xm1, xm2);
    if (nt < EQ_TILE) {         // (o1 lies in this tile: it is the open tile of the next step)
        eqs_store_f(xs, v.dx, 0, 0, nt);
        if (tid < 2) v.dprev[tid] = eqs_x(a, v, t0 - 1 - tid);
    }
    double Z[2 * S], et[2 * S];
    eq_scan_staged<S>(a, c, xs, wt, Z, et, r, xm1, xm2);
    double* E = a.E + ((size_t)w * gridDim.x + blockIdx.x) * kEqDim;
#pragma unroll
    for (int i = 0; i < 2 * S; i++)
        if (tid == i) E[i] = et[i];
}

// stream launch 2: the tile's carry from the open tile's, the true run of every chunk, then y, the cast and the new state
template <int S>
__global__ __launch_bounds__(EQ_THREADS) void eq_stream_apply_kernel(EqArgs a) {
    constexpr int D = 2 * S;
    __shared__ float xs[EQ_LDS];
    __shared__ double wt[EQ_THREADS / 64][kEqDim];
    const int w = blockIdx.y, tid = threadIdx.x;
    const EqsView v = eqs_view(a, w);
    const long long t0 = v.t0e + (long long)blockIdx.x * EQ_TILE;
    if (t0 > v.o1) return;
    const int nt = (int)(v.o1 - t0 < EQ_TILE ? v.o1 - t0 : EQ_TILE);
    const long long hist0 = v.o1 - kEqsHist;            // the new ring holds y [max(0, hist0), o1)
    if (blockIdx.x == 0) {
        // y in front of the open tile comes out of the carried ring: the re-presented part of the range, and the part of the new ring
        const long long end = v.t0e < v.o1 ? v.t0e : v.o1;
        for (long long n = v.o0 + tid; n < end; n += EQ_THREADS) {
            const float f = v.sy[n & (kEqsHist - 1)];
            if (a.y) a.y[v.ybase + (n - v.o0)] = f;
            if (a.pcm && n >= v.j0 && n < v.j1) a.pcm[v.pdst + (n - v.j0)] = pcm_cast(f);
        }
        for (long long n = (hist0 > 0 ? hist0 : 0) + tid; n < end; n += EQ_THREADS) v.dy[n & (kEqsHist - 1)] = v.sy[n & (kEqsHist - 1)];
    }
    const EqTable* __restrict__ k = a.tab;
    double c[S][5];
    eq_load_coef<S>(a, c);
    int r; float xm1, xm2;
    eqs_stage(a, v, t0, nt, xs, r, xm1, xm2);
    double Z[D], et[D];
    eq_scan_staged<S>(a, c, xs, wt, Z, et, r, xm1, xm2);
    // S_t upwards from the open tile's carry (zero at the utterance's start), the whole call's loop from there on
    double St[D];
#pragma unroll
    for (int i = 0; i < D; i++) St[i] = v.e > 0 ? v.sS[i] : 0.0;
    const double* E = a.E + (size_t)w * gridDim.x * kEqDim;
    for (int q = 0; q < (int)blockIdx.x; q++) {
        double m[D];
        eq_mv<S>(k->Mp[8], St, m);
        const double* Eq = E + (size_t)q * kEqDim;
#pragma unroll
        for (int i = 0; i < D; i++) St[i] = m[i] + Eq[i];
    }
    if (nt < EQ_TILE) {
#pragma unroll
        for (int i = 0; i < D; i++)
            if (tid == i) v.dS[i] = St[i];
    }
    eq_mpow<S, 8>(k, tid, St);
#pragma unroll
    for (int i = 0; i < D; i++) St[i] += Z[i];
    eq_chunk<S, true>(c, xs + tid * (EQ_R + 1), r, xm1, xm2, St);
    __syncthreads();
    const int ylo = (int)(v.o0 - t0 < 0 ? 0 : (v.o0 - t0 < nt ? v.o0 - t0 : nt));
    if (a.y) eqs_store_f(xs, a.y, v.ybase + (t0 - v.o0), ylo, nt);
    if (a.pcm) {
        const int lo = (int)(v.j0 - t0 < 0 ? 0 : (v.j0 - t0 < nt ? v.j0 - t0 : nt)), hi = (int)(v.j1 - t0 < 0 ? 0 : (v.j1 - t0 < nt ? v.j1 - t0 : nt));
        eqs_store_pcm(xs, a.pcm, v.pdst + (t0 - v.j0), lo, hi);
    }
    const int hlo = (int)(hist0 - t0 < 0 ? 0 : (hist0 - t0 < nt ? hist0 - t0 : nt));
    for (int p = hlo + tid; p < nt; p += EQ_THREADS) v.dy[(t0 + p) & (kEqsHist - 1)] = xs[p + p / EQ_R];
}

template <int S>
static void eq_stream_launch(const EqArgs& a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(eq_stream_scan_kernel<S>, grid, dim3(EQ_THREADS), 0, st, a);
    hipLaunchKernelGGL(eq_stream_apply_kernel<S>, grid, dim3(EQ_THREADS), 0, st, a);
}

void eq_stream_run(const EqArgs& a, int nwin, long long max_tiles, hipStream_t st) {
    if (nwin <= 0 || max_tiles <= 0 || a.S < 1 || a.S > kEqMaxBands || !a.wtab || !a.state || !a.E) return;
    const dim3 grid((unsigned)max_tiles, nwin);
    switch (a.S) {
    case 1: eq_stream_launch<1>(a, grid, st); break;
    case 2: eq_stream_launch<2>(a, grid, st); break;
    case 3: eq_stream_launch<3>(a, grid, st); break;
    default: eq_stream_launch<4>(a, grid, st); break;
    }
}

}  // namespace sts
