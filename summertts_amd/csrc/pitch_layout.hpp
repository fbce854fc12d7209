// pitch_layout.hpp -- the host arithmetic of a pitch plan (sts_set_pitch_plan; include/summertts_hip.h has the definition): the design of a
// phoneme's step, the exact 64-bit layout of the warped signal, and the filter's cutoff and reach per step.  Plain C++ with no device code:
// pitch_plan.hip, the C API and tests/pitch_layout_check.cpp (built with -fsanitize=undefined) all read this one copy.
#pragma once
#include <math.h>
#include <stdint.h>

namespace sts {

constexpr int kPitchMaxCents = 600, kPitchZC = 32, kPitchRes = 512, kPitchProto = kPitchZC * kPitchRes, kPitchTableFloats = kPitchProto + 2;
constexpr int kPitchMaxK = 51, kPitchMaxDur = 100000, kPitchMaxHop = 1 << 20;
constexpr int64_t kPitchOne = (int64_t)1 << 32;
// step(-600) and step(+600): floor(2^(-+1/2) 2^32 + 0.5)
constexpr int64_t kPitchStepMin = 3037000500ll, kPitchStepMax = 6074001000ll;
constexpr int64_t kPitchMaxSamples = (int64_t)1 << 30;      // N < 2^30: positions (a << 32) + e + k step stay below 2^63

// step 1: input samples per output sample, as float32 and in Q32 (float64, rounded once)
inline float pitch_ratio(int cents) { return (float)pow(2.0, (double)cents / 1200.0); }
inline int64_t pitch_step(int cents) { return (int64_t)floor(pow(2.0, (double)cents / 1200.0) * 4294967296.0 + 0.5); }
// step 4: cutoff c = 0.9 min(1, 1 / rho) in units of the input Nyquist, and the reach K = ceil(32 / c) <= 51 of the 2K taps
inline double pitch_cutoff(int64_t step) { const double rho = (double)step / 4294967296.0; return 0.9 * fmin(1.0, 1.0 / rho); }
inline int pitch_reach(double c) { return (int)ceil(32.0 / c); }

// step 3 for one utterance: o[0 .. n] (first output of phoneme i; o[n] = the outputs the phonemes own) and e[0 .. n] (Q32 distance of
// phoneme i's first output behind its first sample), each optional.  False for n < 1, hop outside [1, 2^20], a duration outside
// [0, 100000], a step outside [step(-600), step(+600)] or max(1, sum d) hop >= 2^30.  Every intermediate is below 2^63: L_i < 2^62,
// e_i < step_i < 2^33, n_i step_i < L_i + step_i.
inline bool pitch_layout(const int32_t* d, const int64_t* step, int n, int hop, int64_t* o, int64_t* e) {
    if (n < 1 || hop < 1 || hop > kPitchMaxHop || !d || !step) return false;
    int64_t oo = 0, ee = 0, frames = 0;
    if (o) o[0] = 0;
    if (e) e[0] = 0;
    for (int i = 0; i < n; i++) {
        if (d[i] < 0 || d[i] > kPitchMaxDur || step[i] < kPitchStepMin || step[i] > kPitchStepMax) return false;
        frames += d[i];
        if (frames * hop >= kPitchMaxSamples) return false;
        const int64_t L = ((int64_t)d[i] * hop) << 32;
        const int64_t ni = L > ee ? (L - ee + step[i] - 1) / step[i] : 0;
        ee += ni * step[i] - L;
        oo += ni;
        if (o) o[i + 1] = oo;
        if (e) e[i + 1] = ee;
    }
    return true;
}

}  // namespace sts
