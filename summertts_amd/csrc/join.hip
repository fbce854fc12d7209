// join.hip -- paragraph synthesis: the B sentences of a packed batch joined into ONE signal at the native rate (sts_infer_ids_joined;
// include/summertts_hip.h has the full definition, DESIGN.md 9i the kernel structure).  Sentence b holds N_b = F_b hop samples x_b and
// starts at start_b = (F_0 + .. + F_{b-1} + lead + gap_0 + .. + gap_{b-1}) hop of J; with the fade length h = floor(fade_ms 16 + 0.5):
//   e_b[t] = float32(float64(min(t + 1, N_b - t, h + 1)) / float64(h + 1));  J[start_b + t] = x_b[t] e_b[t];  every other J[i] = +0.0f.
// Everything downstream (resampler, loudness, limiter, cast) then sees J as one utterance.
//
// The launch is memory-bound (4 B in, 4 B + 2 B out per sample), so a workgroup owns a contiguous span of kJoinSpan samples of J and walks
// it region by region -- silence, then the part of a sentence inside the span, then the next silence ... -- every region handled by all
// of its lanes in groups of 4 samples (one 16-byte load, one 16-byte and one 8-byte store per lane).  Which sentence a span begins in is a
// wave-uniform binary search over the B-entry table (scalar loads: the table sits in registers, no lane diverges), and the walk reads one
// entry more per sentence the span touches.  Region edges are multiples of hop: with hop % 4 == 0 -- every decoder of the model format --
// all groups are aligned in x, J and the PCM; any other hop takes the sample-by-sample path.
// The envelope is evaluated only for groups within h samples of a sentence edge; elsewhere e == 1.0f and the sample is copied.  Near an
// edge e = float32(m r) with r = 1.0 / (h + 1) in float64, one division per lane: m / (h + 1) with m, h + 1 <= 801 is either a float32
// itself or at least 2^-35 (relative) away from every float32 rounding boundary, and m r is within 2^-52 of it, so the product rounds to
// the float32 the definition's quotient rounds to.
#include <math.h>
#include <stdint.h>

#include "../../include/summertts_hip.h"
#include "devmath.hpp"
#include "kernels.hpp"

namespace sts {

static constexpr int kJoinThreads = 256;
// samples of J one workgroup owns (tests/test_join_gpu.py reads the number from the next line: sentence lengths on both sides of it)
static constexpr int kJoinSpan = 4096;

bool join_valid(int B, const sts_join* j, const char** why) {
    if (B < 1) { *why = "join: B >= 1 sentences are required"; return false; }
    if (!j) return true;
    if (!(j->fade_ms >= 0.f && j->fade_ms <= 50.f)) { *why = "join: fade_ms must be finite and in [0, 50]"; return false; }
    if (j->lead_frames < 0 || j->lead_frames > kJoinMaxFrames || j->trail_frames < 0 || j->trail_frames > kJoinMaxFrames) {
        *why = "join: lead_frames and trail_frames must be in [0, 100000]"; return false;
    }
    if (j->gap_frames)
        for (int b = 0; b + 1 < B; b++)
            if (j->gap_frames[b] < 0 || j->gap_frames[b] > kJoinMaxFrames) { *why = "join: every gap must be in [0, 100000] frames"; return false; }
    return true;
}

int join_design(float fade_ms) { return (int)floor((double)fade_ms * 16.0 + 0.5); }

long long join_silence(int B, const sts_join* j, long long* sil) {
    long long s = j ? j->lead_frames : 0;
    for (int b = 0; b < B; b++) {
        if (sil) sil[b] = s;
        if (b + 1 < B && j && j->gap_frames) s += j->gap_frames[b];
    }
    return s + (j ? j->trail_frames : 0);
}

// sample t of a sentence of N samples under a fade of h samples, rinv = 1.0 / (h + 1): the one expression both kernels below evaluate
// (bit equality of a joined stream with the whole join rests on it)
__device__ __forceinline__ float join_faded(long long t, long long N, int h, double rinv, float v) {
    const long long m = t + 1 < N - t ? t + 1 : N - t;
    if (m > h) return v;                              // (e == 1.0f)
    return v * (float)((double)m * rinv);
}

__global__ __launch_bounds__(kJoinThreads) void join_kernel(JoinArgs a) {
    const int tid = threadIdx.x, hop = a.hop, B = a.B, h = a.h;
    const long long s0 = (long long)blockIdx.x * kJoinSpan;
    const long long s1 = s0 + kJoinSpan < a.NJ ? s0 + kJoinSpan : a.NJ;
    // sentence b: frames [off, off + len) of x, samples [start, start + len hop) of J
    auto off_of = [&](int b) -> long long { return a.wseg.off ? a.wseg.off[b] : a.wseg.ioff; };
    auto len_of = [&](int b) -> long long { return a.wseg.len ? a.wseg.len[b] : a.wseg.ilen; };
    auto start_of = [&](int b) -> long long { return (off_of(b) + (a.sil ? a.sil[b] : a.isil)) * hop; };
    // the first sentence that ends behind s0 (B: none does); the ends ascend
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (start_of(mid) + len_of(mid) * hop > s0) hi = mid; else lo = mid + 1;
    }
    int b = lo;
    const bool vec = (hop & 3) == 0;
    const double rinv = 1.0 / (double)(h + 1);
    const float* __restrict__ const x = a.x;
    float* __restrict__ const y = a.y;
    int16_t* __restrict__ const pcm = a.pcm;
    auto faded = [&](long long t, long long N, float v) -> float { return join_faded(t, N, h, rinv, v); };
    long long pos = s0;
    while (pos < s1) {
        long long st = a.NJ, en = a.NJ, xb = 0;
        if (b < B) { st = start_of(b); en = st + len_of(b) * hop; xb = off_of(b) * hop; }
        const long long z1 = st < s1 ? st : s1;
        if (pos < z1) {                                // silence [pos, z1)
            if (vec) {
                for (long long g = (pos >> 2) + tid; g < (z1 >> 2); g += kJoinThreads) {
                    if (y) *(float4*)(y + 4 * g) = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (pcm) *(uint2*)(pcm + 4 * g) = make_uint2(0u, 0u);
                }
            } else {
                for (long long i = pos + tid; i < z1; i += kJoinThreads) {
                    if (y) y[i] = 0.f;
                    if (pcm) pcm[i] = 0;
                }
            }
            pos = z1;
        }
        if (pos >= s1) break;
        // here b < B and st <= pos < en: the sentence's samples [pos, c1)
        const long long c1 = en < s1 ? en : s1, N = en - st;
        const float* const xs = x + xb;                // xs[t] = sample t of the sentence, J[st + t]
        if (vec) {
            for (long long g = (pos >> 2) + tid; g < (c1 >> 2); g += kJoinThreads) {
                const long long i = 4 * g, t = i - st;
                float4 v = *(const float4*)(xs + t);
                if (t < h || t + 4 > N - h) { v.x = faded(t, N, v.x); v.y = faded(t + 1, N, v.y); v.z = faded(t + 2, N, v.z); v.w = faded(t + 3, N, v.w); }
                if (y) *(float4*)(y + i) = v;
                if (pcm)
                    *(uint2*)(pcm + i) = make_uint2((uint32_t)(uint16_t)pcm_cast(v.x) | ((uint32_t)(uint16_t)pcm_cast(v.y) << 16),
                                                    (uint32_t)(uint16_t)pcm_cast(v.z) | ((uint32_t)(uint16_t)pcm_cast(v.w) << 16));
            }
        } else {
            for (long long i = pos + tid; i < c1; i += kJoinThreads) {
                const float v = faded(i - st, N, xs[i - st]);
                if (y) y[i] = v;
                if (pcm) pcm[i] = pcm_cast(v);
            }
        }
        pos = c1;
        if (en <= s1) b++;
    }
}

void join_run(const JoinArgs& a, hipStream_t st) {
    if (a.NJ <= 0 || a.B < 1) return;
    const unsigned spans = (unsigned)((a.NJ + kJoinSpan - 1) / kJoinSpan);
    hipLaunchKernelGGL(join_kernel, dim3(spans), dim3(kJoinThreads), 0, st, a);
}

// ---- the windowed join of a joined stream (sts_infer_ids_joined_stream, sts_join_apply_range): the samples [g0, g1) of J into the compact
// buffer y[i - g0], from the step's decoded windows -- row r of the table says that J[st, en) holds the samples [st - S, en - S) of a
// sentence of N samples that starts at S in J, to be read at x[xoff + (i - S)].  The rows ascend and do not overlap; everything between
// them is silence.  Where the join is the chain's writer, the cast of the kept range [k0, k1) goes to pcm[i - k0] as well.  The structure is
// join_kernel's: a contiguous span per workgroup, a wave-uniform search over the step's (small) table, a walk silence / sentence part /
// silence, groups of 4 samples when hop % 4 == 0 (g0, k0, k1, every st, en, S and xoff are multiples of hop: all groups are aligned in x,
// y and the PCM, and a group lies wholly inside or outside the kept range).  t and N of the envelope are the sentence's, not the window's.
__global__ __launch_bounds__(kJoinThreads) void join_window_kernel(JoinWinArgs a) {
    const int tid = threadIdx.x, nw = a.nw, h = a.h;
    const long long g0 = a.g0, k0 = a.k0, k1 = a.k1;
    const long long s0 = g0 + (long long)blockIdx.x * kJoinSpan;
    const long long s1 = s0 + kJoinSpan < a.g1 ? s0 + kJoinSpan : a.g1;
    const long long* __restrict__ const rows = a.rows;
    // the first row that ends behind s0 (nw: none does); the ends ascend
    int lo = 0, hi = nw;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rows[5 * mid + 1] > s0) hi = mid; else lo = mid + 1;
    }
    int r = lo;
    const bool vec = (a.hop & 3) == 0;
    const double rinv = 1.0 / (double)(h + 1);
    const float* __restrict__ const x = a.x;
    float* __restrict__ const y = a.y;
    int16_t* __restrict__ const pcm = a.pcm;
    long long pos = s0;
    while (pos < s1) {
        long long st = a.g1, en = a.g1, S = 0, N = 0, xoff = 0;
        if (r < nw) { st = rows[5 * r]; en = rows[5 * r + 1]; S = rows[5 * r + 2]; N = rows[5 * r + 3]; xoff = rows[5 * r + 4]; }
        const long long z1 = st < s1 ? st : s1;
        if (pos < z1) {                                // silence [pos, z1)
            if (vec) {
                for (long long g = (pos >> 2) + tid; g < (z1 >> 2); g += kJoinThreads) {
                    const long long i = 4 * g;
                    if (y) *(float4*)(y + (i - g0)) = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (pcm && i >= k0 && i < k1) *(uint2*)(pcm + (i - k0)) = make_uint2(0u, 0u);
                }
            } else {
                for (long long i = pos + tid; i < z1; i += kJoinThreads) {
                    if (y) y[i - g0] = 0.f;
                    if (pcm && i >= k0 && i < k1) pcm[i - k0] = 0;
                }
            }
            pos = z1;
        }
        if (pos >= s1) break;
        // here r < nw and st <= pos < en: the row's samples [pos, c1)
        const long long c1 = en < s1 ? en : s1;
        const float* const xs = x + xoff;              // xs[t] = sample t of the sentence, J[S + t]
        if (vec) {
            for (long long g = (pos >> 2) + tid; g < (c1 >> 2); g += kJoinThreads) {
                const long long i = 4 * g, t = i - S;
                float4 v = *(const float4*)(xs + t);
                if (t < h || t + 4 > N - h) {
                    v.x = join_faded(t, N, h, rinv, v.x); v.y = join_faded(t + 1, N, h, rinv, v.y);
                    v.z = join_faded(t + 2, N, h, rinv, v.z); v.w = join_faded(t + 3, N, h, rinv, v.w);
                }
                if (y) *(float4*)(y + (i - g0)) = v;
                if (pcm && i >= k0 && i < k1)
                    *(uint2*)(pcm + (i - k0)) = make_uint2((uint32_t)(uint16_t)pcm_cast(v.x) | ((uint32_t)(uint16_t)pcm_cast(v.y) << 16),
                                                           (uint32_t)(uint16_t)pcm_cast(v.z) | ((uint32_t)(uint16_t)pcm_cast(v.w) << 16));
            }
        } else {
            for (long long i = pos + tid; i < c1; i += kJoinThreads) {
                const float v = join_faded(i - S, N, h, rinv, xs[i - S]);
                if (y) y[i - g0] = v;
                if (pcm && i >= k0 && i < k1) pcm[i - k0] = pcm_cast(v);
            }
        }
        pos = c1;
        if (en <= s1) r++;
    }
}

void join_window_run(const JoinWinArgs& a, hipStream_t st) {
    if (a.g1 <= a.g0 || a.nw < 0) return;
    const unsigned spans = (unsigned)((a.g1 - a.g0 + kJoinSpan - 1) / kJoinSpan);
    hipLaunchKernelGGL(join_window_kernel, dim3(spans), dim3(kJoinThreads), 0, st, a);
}

}  // namespace sts
