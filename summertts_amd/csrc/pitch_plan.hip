// pitch_plan.hip -- per-phoneme pitch shift by a time warp of the float wave at the native rate (sts_set_pitch_plan; include/summertts_hip.h
// has the full definition, DESIGN.md 9l the kernel structure).  For one utterance of F = max(1, sum d) frames of `hop` samples, phoneme i
// with the Q32 step s_i (input samples per output sample) owning the samples of its d_i frames:
//   layout (pitch_layout.hpp, exact): phoneme i emits the outputs [o_i, o_i+1); output j of it sits at the Q32 input position
//   pos = (a_i << 32) + e_i + (j - o_i) s_i;  n0 = pos >> 32, f = frac(pos), c = 0.9 min(1, 2^32 / s_i), K = ceil(32 / c);
//   tap m of 2K reads x[n0 - K + 1 + m] (0 outside the utterance) with the coefficient g_m = the prototype h0 interpolated linearly at
//   512 c |f + K - 1 - m|;  y_j = float32(sum g_m x_m / sum g_m), float64 throughout, m ascending.
// One prototype serves every ratio (Smith's band-limited interpolation): h0[k] = sinc(k / 512) Kaiser_10(k / 16384), 16384 + 2 floats.
//
// One workgroup per (tile of PP_TILE outputs, member).  An output finds its phoneme by an upper-bound search of j in the inclusive output
// counts o_i+1 (a phoneme that emits nothing can never be the answer).  The tile's input span [n0_first - 51 + 1, n0_last + 51] (the
// widest K: a later output of the tile may reach further back than the first) -- consecutive outputs are at most step(+600) < 1.4143
// samples apart, whichever phonemes they belong to, so at most PP_TILE 1.4143 + 2 * 52 + 2 floats -- is staged in LDS with zeros outside
// the utterance.  A lane runs one output (coalesced stores); steps change inside a tile, so each output's loop ends at its own 2K.
// The prototype is read from global memory (64 KiB, L2-resident) or staged in LDS.
// Measured (one utterance of 185 k samples, microseconds per launch, LDS / global): tiles of 1024 outputs 48.8 / 62.6, of 512
// 29.3 / 34.5, of 256 30.2 / 22.6 -- the work is latency-bound, so what counts is workgroups in flight, and a workgroup that keeps 2 KiB of
// LDS instead of 66 runs eight to a CU: 256 outputs per workgroup, one per lane, the prototype from L2.  A member without a plan is copied.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/summertts_hip.h"
#include "devmath.hpp"
#include "kernels.hpp"

namespace sts {

constexpr int PP_THREADS = 256, PP_TILE = PP_THREADS;    // one output per lane
constexpr bool kPitchTableLds = false; // where the prototype is read from (the measurement above)
constexpr int PP_LDS = 480;         // >= (PP_TILE - 1) step(+600) / 2^32 + 2 kPitchMaxK + 2 = 464.7

bool pitch_plan_valid(int n, const int32_t* cents, const char** why) {
    if (n < 1) { *why = "pitch plan: every utterance needs n >= 1 phonemes"; return false; }
    if (cents)
        for (int i = 0; i < n; i++)
            if (cents[i] < -kPitchMaxCents || cents[i] > kPitchMaxCents) { *why = "pitch plan: cents must be in [-600, 600]"; return false; }
    return true;
}

void pitch_table(float* table) {
    const double pi = 3.14159265358979323846, beta = 10.0, i0b = bessel_i0(beta);
    for (int k = 0; k < kPitchProto; k++) {
        const double u = (double)k / kPitchRes, r = u / kPitchZC;
        const double sinc = k == 0 ? 1.0 : sin(pi * u) / (pi * u);
        table[k] = (float)(sinc * (bessel_i0(beta * sqrt(1.0 - r * r)) / i0b));
    }
    table[kPitchProto] = table[kPitchProto + 1] = 0.f;
}

const char* pitch_tables(int B, const int32_t* n, const int32_t* const* dur, const int64_t* const* step, const long long* xoff, int hop,
                         PitchTables* t) {
    long long TT = 0;
    for (int b = 0; b < B; b++) TT += step[b] ? n[b] : 0;
    t->TT = TT; t->total_out = 0; t->max_out = 0;
    t->nout.assign((size_t)B, 0);
    t->words.assign((size_t)6 * B + 5 * (size_t)TT, 0);
    long long* mem = t->words.data();
    long long *oend = mem + 6 * (size_t)B, *pos0 = oend + TT, *st = pos0 + TT, *cb = st + TT, *kk = cb + TT;
    std::vector<int64_t> o, e;
    long long toff = 0;
    for (int b = 0; b < B; b++) {
        long long frames = 0;
        for (int i = 0; i < n[b]; i++) {
            if (dur[b][i] < 0 || dur[b][i] > kPitchMaxDur) return "pitch plan: durations must be in [0, 100000]";
            frames += dur[b][i];
        }
        const long long N = (frames > 0 ? frames : 1) * hop;
        if (N >= kPitchMaxSamples) return "pitch plan: an utterance must hold fewer than 2^30 native samples";
        long long nout = N, np = 0;
        if (step[b]) {
            auto row = [&](long long i, long long oe, long long p0, int64_t s) {
                const double c = pitch_cutoff(s);
                oend[toff + i] = oe; pos0[toff + i] = p0; st[toff + i] = s; memcpy(&cb[toff + i], &c, 8); kk[toff + i] = pitch_reach(c);
            };
            if (frames > 0) {
                o.resize((size_t)n[b] + 1); e.resize((size_t)n[b] + 1);
                if (!pitch_layout(dur[b], step[b], n[b], hop, o.data(), e.data())) return "pitch plan: invalid layout";
                long long a = 0;
                for (int i = 0; i < n[b]; i++) { row(i, o[i + 1], ((a * hop) << 32) + e[i], step[b][i]); a += dur[b][i]; }
                nout = o[n[b]]; np = n[b];
            } else {                // the one frame nobody owns: step 2^32
                row(0, hop, 0, kPitchOne);
                nout = hop; np = 1;
            }
        }
        long long* m = mem + 6 * (size_t)b;
        m[0] = xoff[b]; m[1] = N; m[2] = t->total_out; m[3] = nout; m[4] = toff; m[5] = np;
        t->nout[b] = nout; t->total_out += nout; t->max_out = nout > t->max_out ? nout : t->max_out;
        toff += step[b] ? n[b] : 0;
    }
    return nullptr;
}

void pitch_args_carve(PitchArgs& a, const long long* dev_words, int B, long long TT) {
    a.mem = dev_words;
    a.oend = dev_words + 6 * (size_t)B; a.pos0 = a.oend + TT; a.step = a.pos0 + TT; a.c = (const double*)(a.step + TT); a.K = a.step + 2 * TT;
}

namespace {
struct PpOut { long long n0; double f, c; int K; };
// output j of a member with n phoneme rows at toff
__device__ __forceinline__ PpOut pp_locate(const PitchArgs& a, long long toff, int n, long long j) {
    const long long* oend = a.oend + toff;
    int l = 0, r = n - 1;
    while (l < r) { const int mid = (l + r) >> 1; if (oend[mid] > j) r = mid; else l = mid + 1; }
    const long long os = l ? oend[l - 1] : 0;
    const long long pos = a.pos0[toff + l] + (j - os) * a.step[toff + l];
    PpOut p;
    p.n0 = pos >> 32; p.f = (double)(pos & 0xffffffffll) * (1.0 / 4294967296.0); p.c = a.c[toff + l]; p.K = (int)a.K[toff + l];
    return p;
}
}  // namespace

// output j of a member whose staged input span starts at sample s0 in xs: the tap loop of the definition, m ascending, float64.  The
// whole-utterance kernel and the range kernel both run this one function, so a sample does not depend on which of them made it.
__device__ __forceinline__ float pp_output(const PitchArgs& a, long long toff, int n, long long j, const float* xs, long long s0, const float* h0) {
    const PpOut p = pp_locate(a, toff, n, j);
    const float* const xv = xs + (p.n0 - p.K + 1 - s0);               // taps [0, 2K) lie inside the span: n0 ascends with j and K <= kPitchMaxK
    const double f = p.f, c = p.c;
    const int T = 2 * p.K, K1 = p.K - 1;
    double num = 0.0, den = 0.0;
    for (int m = 0; m < T; m++) {
        const double dd = f + (double)(K1 - m);
        const double t = 512.0 * (c * fabs(dd));
        const int k = (int)t;                                         // t >= 0: floor
        double g = 0.0;
        if (k < kPitchProto) {
            const double ha = (double)h0[k], hb = (double)h0[k + 1];
            g = ha + (t - (double)k) * (hb - ha);
        }
        num += g * (double)xv[m];
        den += g;
    }
    return (float)(num / den);
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PP_THREADS) void pitch_plan_kernel(PitchArgs a) {
    __shared__ float xs[PP_LDS];
    __shared__ float hs[TAB_LDS ? kPitchTableFloats : 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long* mem = a.mem + 6 * (long long)b;
    const long long xoff = mem[0], N = mem[1], yoff = mem[2], nout = mem[3], toff = mem[4];
    const int n = (int)mem[5];
    const long long t0 = (long long)blockIdx.x * PP_TILE;
    if (t0 >= nout) return;
    const long long t1 = t0 + PP_TILE < nout ? t0 + PP_TILE : nout;
    const long long j = t0 + tid;
    if (n == 0) {                   // no plan: y = x, bit for bit (nout == N)
        if (j < t1) {
            const float v = a.x[xoff + j];
            if (a.y) a.y[yoff + j] = v;
            if (a.pcm) a.pcm[yoff + j] = pcm_cast(v);
        }
        return;
    }
    // the tile's input span, uniform across the workgroup: [s0, s1]
    const PpOut first = pp_locate(a, toff, n, t0), last = pp_locate(a, toff, n, t1 - 1);
    const long long s0 = first.n0 - kPitchMaxK + 1, s1 = last.n0 + kPitchMaxK;      // (a later output may reach further back than the first: the widest K)
    const int span = (int)(s1 - s0 + 1);
    if (span > PP_LDS) return;      // (never: consecutive outputs are at most step(+600) apart and K <= kPitchMaxK)
    for (int i = tid; i < span; i += PP_THREADS) {
        const long long p = s0 + i;
        xs[i] = (p >= 0 && p < N) ? a.x[xoff + p] : 0.f;
    }
    if (TAB_LDS)
        for (int i = tid; i < kPitchTableFloats; i += PP_THREADS) hs[i] = a.table[i];
    __syncthreads();
    const float y = pp_output(a, toff, n, j < t1 ? j : t0, xs, s0, TAB_LDS ? hs : a.table);      // (past the tile: output t0 again, stored nowhere)
    if (j < t1) {
        if (a.y) a.y[yoff + j] = y;
        if (a.pcm) a.pcm[yoff + j] = pcm_cast(y);
    }
}

// The range form (a stream through the warp, sts_pitch_apply_range): one workgroup per (tile of PP_TILE outputs, window), the tiles
// anchored at the window's yl0.  Window w reads its PsRow (pitch_stream.hpp): x[xbase ..) holds the samples [u0, u0 + xlen) of member
// `mem`; a staged position outside the utterance OR outside the window is 0 and is never read (the geometry keeps every tap that counts
// inside the window).  The float outputs [yl0, yl1) go to y[ybase ..); of them [y0, y1) go as int16 to pcm[pbase ..) when a.pcm is set.
__global__ __launch_bounds__(PP_THREADS) void pitch_range_kernel(PitchArgs a) {
    __shared__ float xs[PP_LDS];
    const int tid = threadIdx.x;
    const long long* row = a.rows + 10 * (long long)blockIdx.y;
    const long long xbase = row[0], u0 = row[1], u1 = row[1] + row[2], yl0 = row[4], yl1 = row[5], ybase = row[6], y0 = row[7], y1 = row[8], pbase = row[9];
    const long long* mem = a.mem + 6 * row[3];
    const long long N = mem[1], toff = mem[4];
    const int n = (int)mem[5];
    const long long t0 = yl0 + (long long)blockIdx.x * PP_TILE;
    if (t0 >= yl1) return;
    const long long t1 = t0 + PP_TILE < yl1 ? t0 + PP_TILE : yl1;
    const long long j = t0 + tid;
    float y;
    if (n == 0) {                   // no plan: y = x, bit for bit
        y = (j < t1 && j >= u0 && j < u1 && j < N) ? a.x[xbase + (j - u0)] : 0.f;
    } else {
        const PpOut first = pp_locate(a, toff, n, t0), last = pp_locate(a, toff, n, t1 - 1);
        const long long s0 = first.n0 - kPitchMaxK + 1, s1 = last.n0 + kPitchMaxK;
        const int span = (int)(s1 - s0 + 1);
        if (span > PP_LDS) return;  // (never, as above)
        for (int i = tid; i < span; i += PP_THREADS) {
            const long long p = s0 + i;
            xs[i] = (p >= 0 && p < N && p >= u0 && p < u1) ? a.x[xbase + (p - u0)] : 0.f;
        }
        __syncthreads();
        y = pp_output(a, toff, n, j < t1 ? j : t0, xs, s0, a.table);
    }
    if (j < t1) {
        if (a.y) a.y[ybase + (j - yl0)] = y;
        if (a.pcm && j >= y0 && j < y1) a.pcm[pbase + (j - y0)] = pcm_cast(y);
    }
}

bool pitch_table_in_lds() { return kPitchTableLds; }

void pitch_plan_run(const PitchArgs& a, int nmem, long long max_out, bool table_in_lds, hipStream_t st) {
    if (nmem <= 0 || max_out <= 0) return;
    const dim3 grid((unsigned)((max_out + PP_TILE - 1) / PP_TILE), nmem);
    if (table_in_lds) hipLaunchKernelGGL(pitch_plan_kernel<true>, grid, dim3(PP_THREADS), 0, st, a);
    else hipLaunchKernelGGL(pitch_plan_kernel<false>, grid, dim3(PP_THREADS), 0, st, a);
}

void pitch_range_run(const PitchArgs& a, int nwin, long long max_out, hipStream_t st) {
    if (nwin <= 0 || max_out <= 0) return;
    hipLaunchKernelGGL(pitch_range_kernel, dim3((unsigned)((max_out + PP_TILE - 1) / PP_TILE), nwin), dim3(PP_THREADS), 0, st, a);
}

}  // namespace sts
