// capi_apply.hip -- the output stages and plans of include/summertts_hip.h on caller data, with no engine: each entry validates on the
// host, uploads through a DevScratch, launches the stage the engine launches, and copies the result back.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_common.hpp"
#include "dev_scratch.hpp"
#include "engine.hpp"
#include "eq_stream.hpp"
#include "join_stream.hpp"
#include "loud_stream.hpp"
#include "pitch_stream.hpp"

using namespace sts;

namespace {
// int64 lengths[B] -> int table, their sum and the longest one; null, or why the call cannot run
const char* signal_lengths(const int64_t* lengths, int B, int64_t max_total, const float* x, std::vector<int>& len, int64_t* total, int64_t* maxl) {
    len.resize(B); *total = 0; *maxl = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 0 || lengths[b] > (int64_t)1 << 30) return "lengths must be in [0, 2^30]";
        len[b] = (int)lengths[b]; *total += lengths[b]; *maxl = std::max<int64_t>(*maxl, lengths[b]);
    }
    if (*total > max_total) return "the signals must hold at most 2^30 samples in all";
    if (*total > 0 && !x) return "null signal";
    return nullptr;
}
// the step boundaries of a chunked entry and its overlap; stage: "loudness" or "eq"
int step_bounds_check(const char* stage, const int64_t* bounds, int n_steps, int back, int max_back) {
    const std::string s = std::string(stage) + " stream: ";
    if (n_steps < 1 || !bounds || bounds[0] != 0) return set_err(STS_EINVAL, s + "at least one step boundary, the first one 0");
    for (int k = 1; k < n_steps; k++)
        if (bounds[k] <= bounds[k - 1]) return set_err(STS_EINVAL, s + "the step boundaries must ascend");
    if (back < 0 || back > max_back) return set_err(STS_EINVAL, s + "the overlap must be in [0, 2048]");
    return STS_OK;
}
// the packed signals; an empty batch still hands the kernels a pointer
const float* up_signal(DevScratch& d, const float* x, int64_t total) { return total > 0 ? d.up(x, (size_t)total) : (const float*)d.raw(0); }
}  // namespace

extern "C" {

int sts_duration_plan_apply(int device, const float* w, const int32_t* fixed, const int32_t* lengths, int32_t B,
                            const int32_t* target_frames, int32_t* dur_out) {
    if (B < 1 || !w || !lengths || !dur_out) return set_err(STS_EINVAL, "B >= 1, w, lengths and dur_out are required");
    std::vector<int> tab(3 * (size_t)B);     // [offsets | lengths | targets]
    int64_t total = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 1 || total + lengths[b] > (1 << 24)) return set_err(STS_EINVAL, "lengths must be >= 1 and hold at most 2^24 weights in all");
        const char* why = nullptr;
        if (!dur_plan_valid(lengths[b], nullptr, fixed ? fixed + total : nullptr, target_frames ? target_frames[b] : 0, &why)) return set_err(STS_EINVAL, why);
        tab[b] = (int)total; tab[B + b] = lengths[b]; tab[2 * B + b] = target_frames ? target_frames[b] : 0;
        total += lengths[b];
    }
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    DurPlanArgs a{};
    a.w_in = d.up(w, (size_t)total); a.fixed = d.up(fixed, (size_t)total); a.forced = (int*)d.out((size_t)total);
    const int* dt = d.up(tab.data(), tab.size());
    a.target = dt + 2 * B; a.rem = (long long*)d.filled((size_t)total * 8, 0xFF);
    a.seg = SegView{dt, dt + B, 1, 0, 0, 0};
    if (d.ok) duration_plan(a, B, d.st);
    d.down(dur_out, a.forced, (size_t)total * 4);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the duration plan failed on the device");
}

int sts_speaker_blend(int device, const float* table, int32_t speaker_num, int32_t gin, int32_t B, const int32_t* sid,
                      const sts_speaker_mix* mixes, float* g_out) {
    if (B < 1 || B > (1 << 20) || !table || !g_out || speaker_num < 1 || gin < 1 || (int64_t)speaker_num * gin > (1 << 28) || (int64_t)B * gin > (1 << 28))
        return set_err(STS_EINVAL, "B >= 1, a table of speaker_num >= 1 rows of gin >= 1 floats and g_out are required");
    std::vector<sts_speaker_mix> none;
    if (!mixes) { none.assign((size_t)B, sts_speaker_mix{0, nullptr, nullptr, nullptr, 0.f}); mixes = none.data(); }
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (!speaker_mix_valid(speaker_num, gin, mixes[b], &why)) return set_err(STS_EINVAL, why);
    }
    std::vector<int32_t> words; int K = 0;
    speaker_mix_flatten(mixes, B, gin, words, &K);
    std::vector<int32_t> sidv((size_t)B, 0);
    if (sid) sidv.assign(sid, sid + B);
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    std::vector<float> g((size_t)B * gin);       // [gin][B], the engine's layout
    const float* dtab = d.up(table, (size_t)speaker_num * gin);
    const int* dsid = d.up(sidv.data(), (size_t)B);
    const int* dw = words.empty() ? (const int*)d.raw(0) : d.up(words.data(), words.size());
    float* dg = d.out(g.size());
    if (d.ok) speaker_blend(dtab, speaker_num, gin, dsid, B, speaker_mix_tab(dw, B, K), dg, d.st);
    d.down(g.data(), dg, g.size() * 4);
    if (!d.finish()) return set_err(STS_EDEVICE, "the speaker blend failed on the device");
    for (int b = 0; b < B; b++) for (int c = 0; c < gin; c++) g_out[(size_t)b * gin + c] = g[(size_t)c * B + b];
    return STS_OK;
}

int sts_gain_plan_apply(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                        const sts_gain_plan* plans, float* y, int16_t* pcm) {
    if (B < 1 || B > 65535 || !x || !dur_frames || !lengths || !plans || samples_per_frame < 1 || samples_per_frame > (1 << 20))      // (one grid row per signal)
        return set_err(STS_EINVAL, "1 <= B <= 65535 signals, their durations, phoneme counts and plans, and samples_per_frame >= 1 are required");
    const int hop = samples_per_frame;
    // host tables [offT B | lenT B | offF B | lenF B | h B | cum T | q T]: the geometry the engine keeps on the device
    int64_t T = 0;
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (lengths[b] < 1 || !gain_plan_valid(lengths[b], plans[b].gain_db, plans[b].ramp_ms, &why)) return set_err(STS_EINVAL, why ? why : "every utterance needs lengths[b] >= 1 phonemes");
        T += lengths[b];
        if (T > (1 << 24)) return set_err(STS_EINVAL, "batch too large");
    }
    std::vector<int32_t> tab((size_t)5 * B + 2 * (size_t)T);
    int32_t *offT = tab.data(), *lenT = offT + B, *offF = lenT + B, *lenF = offF + B, *hh = lenF + B, *cum = hh + B, *q = cum + T;
    int64_t t = 0, F = 0, maxF = 0;
    for (int b = 0; b < B; b++) {
        int64_t f = 0;
        for (int i = 0; i < lengths[b]; i++) {
            const int32_t dd = dur_frames[t + i];
            if (dd < 0 || dd > kDurMax) return set_err(STS_EINVAL, "durations must be in [0, 100000]");
            f += dd;
            if (f > ((int64_t)1 << 30)) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
            cum[t + i] = (int32_t)f;
        }
        if (f < 1) f = 1;
        gain_design(plans[b].gain_db, lengths[b], plans[b].ramp_ms, q + t, hh + b);
        offT[b] = (int32_t)t; lenT[b] = lengths[b]; offF[b] = (int32_t)F; lenF[b] = (int32_t)f;
        t += lengths[b]; F += f; maxF = std::max(maxF, f);
        if (F * hop > ((int64_t)1 << 30)) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
    }
    const int64_t total = F * hop;
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    const int* dt = d.up(tab.data(), tab.size());
    GainArgs a{};
    a.x = d.up(x, (size_t)total); a.y = y ? d.out((size_t)total) : nullptr; a.pcm = pcm ? d.out16((size_t)total) : nullptr;
    a.wseg = SegView{dt + 2 * B, dt + 3 * B, hop, 0, 0, 0}; a.hop = hop;
    a.tseg = SegView{dt, dt + B, 1, 0, 0, 0};
    a.h = dt + 4 * B; a.cum = dt + 5 * B; a.q = dt + 5 * B + T;
    if (d.ok) gain_plan_run(a, B, maxF * hop, d.st);
    d.down(y, a.y, (size_t)total * 4);
    d.down(pcm, a.pcm, (size_t)total * 2);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the gain plan failed on the device");
}

// the host side of the pitch entries: the batch's validity and the warp's tables (utterance b's signal at its offset in the packed x:
// the geometry the engine derives from its durations); *total = the samples of x.  STS_OK, or the error set
static int pitch_host_tables(const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame, const sts_pitch_plan* plans,
                             PitchTables& tab, int64_t* total_out) {
    if (B < 1 || B > 65535 || !dur_frames || !lengths || !plans || samples_per_frame < 1 || samples_per_frame > kPitchMaxHop)      // (one grid row per signal)
        return set_err(STS_EINVAL, "1 <= B <= 65535 signals, their durations, phoneme counts and plans, and samples_per_frame in [1, 2^20] are required");
    const int hop = samples_per_frame;
    int64_t T = 0;
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (lengths[b] < 1 || !pitch_plan_valid(lengths[b], plans[b].cents, &why)) return set_err(STS_EINVAL, why ? why : "every utterance needs lengths[b] >= 1 phonemes");
        T += lengths[b];
        if (T > (1 << 24)) return set_err(STS_EINVAL, "batch too large");
    }
    std::vector<int64_t> steps((size_t)T);
    std::vector<const int32_t*> dur((size_t)B);
    std::vector<const int64_t*> step((size_t)B);
    std::vector<long long> xoff((size_t)B);
    int64_t t = 0, total = 0;
    for (int b = 0; b < B; b++) {
        int64_t f = 0;
        for (int i = 0; i < lengths[b]; i++) {
            const int32_t dd = dur_frames[t + i];
            if (dd < 0 || dd > kDurMax) return set_err(STS_EINVAL, "durations must be in [0, 100000]");
            f += dd;
            if (plans[b].cents) steps[t + i] = pitch_step(plans[b].cents[i]);
        }
        dur[b] = dur_frames + t; step[b] = plans[b].cents ? steps.data() + t : nullptr; xoff[b] = total;
        t += lengths[b]; total += std::max<int64_t>(f, 1) * hop;
        if (total > ((int64_t)1 << 30)) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
    }
    if (const char* bad = pitch_tables(B, lengths, dur.data(), step.data(), xoff.data(), hop, &tab)) return set_err(STS_EINVAL, bad);
    *total_out = total;
    return STS_OK;
}

// table_mode: -1 the shipped placement of the prototype, 0 global memory, 1 LDS; iters > 0: that many more launches between two events,
// their mean in *ms (sts_debug_pitch_bench)
static int pitch_apply_impl(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                            const sts_pitch_plan* plans, int64_t* out_len, float* y, int16_t* pcm, int64_t capacity, int table_mode, int iters,
                            float* ms) {
    if (!x || capacity < 0) return set_err(STS_EINVAL, "1 <= B <= 65535 signals, their durations, phoneme counts and plans, and samples_per_frame in [1, 2^20] are required");
    PitchTables tab;
    int64_t total = 0;
    if (const int rc = pitch_host_tables(dur_frames, lengths, B, samples_per_frame, plans, tab, &total)) return rc;
    if (out_len) for (int b = 0; b < B; b++) out_len[b] = tab.nout[b];
    if ((y || pcm) && tab.total_out > capacity) return set_err(STS_EINVAL, "pitch plan: the outputs are too small for the warped signals (out_len has their lengths)");
    if (!y && !pcm) return STS_OK;
    std::vector<float> proto(kPitchTableFloats);
    pitch_table(proto.data());
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    PitchArgs a{};
    pitch_args_carve(a, d.up(tab.words.data(), tab.words.size()), B, tab.TT);
    a.table = d.up(proto.data(), proto.size());
    // (the outputs start out as NaN / 0x7FFF: a sample the kernel leaves out shows)
    a.x = d.up(x, (size_t)total); a.y = y ? d.out((size_t)tab.total_out) : nullptr; a.pcm = pcm ? d.out16((size_t)tab.total_out) : nullptr;
    const bool lds = table_mode < 0 ? pitch_table_in_lds() : table_mode != 0;
    if (d.ok) pitch_plan_run(a, B, tab.max_out, lds, d.st);
    if (d.ok && iters > 0 && ms) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        d.ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess && hipEventRecord(e0, d.st) == hipSuccess;
        for (int i = 0; i < iters && d.ok; i++) pitch_plan_run(a, B, tab.max_out, lds, d.st);
        d.ok = d.ok && hipEventRecord(e1, d.st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
        if (d.ok) *ms /= (float)iters;
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    d.down(y, a.y, (size_t)tab.total_out * 4);
    d.down(pcm, a.pcm, (size_t)tab.total_out * 2);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the pitch plan failed on the device");
}
int sts_pitch_apply(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                    const sts_pitch_plan* plans, int64_t* out_len, float* y, int16_t* pcm, int64_t capacity) {
    return pitch_apply_impl(device, x, dur_frames, lengths, B, samples_per_frame, plans, out_len, y, pcm, capacity, -1, 0, nullptr);
}
int sts_debug_pitch_bench(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                          const sts_pitch_plan* plans, float* y, int64_t capacity, int32_t table_in_lds, int32_t iters, float* ms_out) {
    if (!y || !ms_out || iters < 1 || table_in_lds < 0 || table_in_lds > 1) return set_err(STS_EINVAL, "pitch bench: y, ms_out, iters >= 1 and table_in_lds 0 or 1 are required");
    return pitch_apply_impl(device, x, dur_frames, lengths, B, samples_per_frame, plans, nullptr, y, nullptr, capacity, table_in_lds, iters, ms_out);
}

int sts_pitch_apply_range(int device, const float* x, int64_t x_len, const int32_t* dur_frames, const int32_t* lengths, int32_t B,
                          int32_t samples_per_frame, const sts_pitch_plan* plans, const sts_pitch_range* win, int32_t n_win, float* y,
                          int16_t* pcm, int64_t capacity) {
    if (!x || x_len < 1 || x_len > ((int64_t)1 << 30) || !win || n_win < 1 || n_win > 65535 || capacity < 0)
        return set_err(STS_EINVAL, "pitch range: a signal buffer of at most 2^30 samples and 1 <= n_win <= 65535 windows are required");
    PitchTables tab;
    int64_t total = 0;
    if (const int rc = pitch_host_tables(dur_frames, lengths, B, samples_per_frame, plans, tab, &total)) return rc;
    // every window: inside the caller's buffer, its range inside [0, N'], and the staged span of the range (clipped to the utterance)
    // inside the window -- the kernel reads nothing else, so nothing else needs to be there
    std::vector<PsRow> rows((size_t)n_win);
    long long ysum = 0, max_out = 0;
    for (int i = 0; i < n_win; i++) {
        const sts_pitch_range& w = win[i];
        if (w.utt < 0 || w.utt >= B) return set_err(STS_EINVAL, "pitch range: a window names no utterance of the batch");
        const PsUtt u = ps_utt(tab.words.data(), B, tab.TT, w.utt);
        if (w.xlen < 0 || w.xlen > x_len || w.xbase < 0 || w.xbase > x_len - w.xlen || w.u0 < 0 || w.u0 > u.N - w.xlen)
            return set_err(STS_EINVAL, "pitch range: a window lies outside the signal buffer or outside its utterance");
        if (w.y0 < 0 || w.y1 < w.y0 || w.y1 > u.Nw) return set_err(STS_EINVAL, "pitch range: outputs outside [0, N']");
        long long c0, c1;
        pitch_staged(u, w.y0, w.y1, &c0, &c1);
        if (c0 < c1 && (c0 < w.u0 || c1 > w.u0 + w.xlen)) return set_err(STS_EINVAL, "pitch range: a window does not cover the input span its outputs read");
        rows[(size_t)i] = PsRow{w.xbase, w.u0, w.xlen, w.utt, w.y0, w.y1, ysum, w.y0, w.y1, ysum};
        ysum += w.y1 - w.y0; max_out = std::max<long long>(max_out, w.y1 - w.y0);
    }
    if ((y || pcm) && ysum > capacity) return set_err(STS_EINVAL, "pitch range: the outputs are too small for the ranges");
    if ((!y && !pcm) || ysum == 0) return STS_OK;
    std::vector<float> proto(kPitchTableFloats);
    pitch_table(proto.data());
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    PitchArgs a{};
    pitch_args_carve(a, d.up(tab.words.data(), tab.words.size()), B, tab.TT);
    a.table = d.up(proto.data(), proto.size());
    a.rows = (const long long*)d.up(rows.data(), rows.size());
    a.x = d.up(x, (size_t)x_len); a.y = y ? d.out((size_t)ysum) : nullptr; a.pcm = pcm ? d.out16((size_t)ysum) : nullptr;
    if (d.ok) pitch_range_run(a, n_win, max_out, d.st);
    d.down(y, a.y, (size_t)ysum * 4);
    d.down(pcm, a.pcm, (size_t)ysum * 2);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the pitch range warp failed on the device");
}

int sts_join_apply(int device, const float* x, const int32_t* frames, int32_t B, int32_t samples_per_frame, const sts_join* join, float* y,
                   int16_t* pcm) {
    const char* why = nullptr;
    if (!join_valid(B, join, &why)) return set_err(STS_EINVAL, why);
    if (!x || !frames || samples_per_frame < 1 || samples_per_frame > (1 << 20) || B > (1 << 24))
        return set_err(STS_EINVAL, "1 <= B <= 2^24 signals, their frame counts and samples_per_frame >= 1 are required");
    const int hop = samples_per_frame;
    // host table [off B | len B | sil B]: the geometry the engine keeps on the device
    std::vector<long long> sil((size_t)B);
    const long long all = join_silence(B, join, sil.data());
    std::vector<int32_t> tab((size_t)3 * B);
    int64_t F = 0;
    for (int b = 0; b < B; b++) {
        if (frames[b] < 1) return set_err(STS_EINVAL, "join: every sentence has frames[b] >= 1");
        tab[b] = (int32_t)F; tab[B + b] = frames[b];
        F += frames[b];
        if ((F + sil[b]) * hop > ((int64_t)1 << 30)) return set_err(STS_EINVAL, "the signals and the joined signal must hold at most 2^30 samples each");
        tab[2 * (size_t)B + b] = (int32_t)sil[b];
    }
    const int64_t NX = F * hop, NJ = (F + all) * hop;
    if (NJ > ((int64_t)1 << 30)) return set_err(STS_EINVAL, "the signals and the joined signal must hold at most 2^30 samples each");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    const int* dt = d.up(tab.data(), tab.size());
    JoinArgs a{};
    // (the outputs start out as NaN / 0x7FFF: a sample the kernel leaves out shows)
    a.x = d.up(x, (size_t)NX); a.y = y ? d.out((size_t)NJ) : nullptr; a.pcm = pcm ? d.out16((size_t)NJ) : nullptr;
    a.wseg = SegView{dt, dt + B, hop, 0, 0, 0}; a.sil = dt + 2 * B;
    a.B = B; a.hop = hop; a.h = join ? join_design(join->fade_ms) : 0; a.NJ = NJ;
    if (d.ok) join_run(a, d.st);
    d.down(y, a.y, (size_t)NJ * 4);
    d.down(pcm, a.pcm, (size_t)NJ * 2);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the join failed on the device");
}

int sts_join_apply_range(int device, const float* x, const int32_t* frames, int32_t B, int32_t samples_per_frame, const sts_join* join,
                         int64_t first_frame, int64_t n_frames, float* y, int16_t* pcm) {
    const char* why = nullptr;
    if (!join_valid(B, join, &why)) return set_err(STS_EINVAL, why);
    if (!x || !frames || samples_per_frame < 1 || samples_per_frame > (1 << 20) || B > (1 << 24))
        return set_err(STS_EINVAL, "1 <= B <= 2^24 signals, their frame counts and samples_per_frame >= 1 are required");
    const int hop = samples_per_frame;
    std::vector<long long> sil((size_t)B);
    const long long all = join_silence(B, join, sil.data());
    int64_t F = 0;
    for (int b = 0; b < B; b++) {
        if (frames[b] < 1) return set_err(STS_EINVAL, "join: every sentence has frames[b] >= 1");
        F += frames[b];
        if ((F + all) * hop > ((int64_t)1 << 30)) return set_err(STS_EINVAL, "the signals and the joined signal must hold at most 2^30 samples each");
    }
    JsPlan js;                  // the layout and the window table the engine's step loop builds, with no decoder halo
    js.layout(B, frames, sil.data(), all);
    js.hop = hop;
    if (first_frame < 0 || n_frames < 1 || first_frame > js.FJ - n_frames) return set_err(STS_EINVAL, "join: the range must be n_frames >= 1 frames inside [0, F_J)");
    const long long g0 = first_frame, g1 = first_frame + n_frames;
    std::vector<JsWin> win; std::vector<JsRow> rows;
    long long Wtot = 0;
    js.windows(g0, g1, 0, win, &Wtot, nullptr);
    js.rows(g0, g1, win, rows);
    const int nw = (int)win.size();
    const int64_t NX = Wtot * hop, NY = n_frames * hop;
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    float* dx = (float*)d.raw((size_t)NX * 4 + 16);     // only the parts of x inside the range, packed
    std::vector<long long> tab((size_t)nw * 5 + 1);
    std::vector<int64_t> xoffF((size_t)B + 1, 0);       // sentence b's first frame in the caller's x
    for (int b = 0; b < B; b++) xoffF[b + 1] = xoffF[b] + frames[b];
    for (int i = 0; i < nw && d.ok; i++) {
        const JsWin& w = win[i]; const JsRow& r = rows[i];
        tab[5 * i] = r.st; tab[5 * i + 1] = r.en; tab[5 * i + 2] = r.S; tab[5 * i + 3] = r.N; tab[5 * i + 4] = r.xoff;
        d.put(dx + (size_t)w.coff * hop, x + (xoffF[w.b] + w.w0) * hop, (size_t)(w.w1 - w.w0) * hop * 4);
    }
    JoinWinArgs a{};
    // (the outputs start out as NaN / 0x7FFF: a sample the kernel leaves out shows)
    a.x = dx; a.y = y ? d.out((size_t)NY) : nullptr; a.pcm = pcm ? d.out16((size_t)NY) : nullptr;
    a.rows = d.up(tab.data(), tab.size()); a.nw = nw; a.hop = hop; a.h = join ? join_design(join->fade_ms) : 0;
    a.g0 = g0 * hop; a.g1 = g1 * hop; a.k0 = a.g0; a.k1 = a.g1;
    if (d.ok) join_window_run(a, d.st);
    d.down(y, a.y, (size_t)NY * 4);
    d.down(pcm, a.pcm, (size_t)NY * 2);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the join failed on the device");
}

int sts_loudness_measure(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float target_lufs, float peak_dbfs,
                         sts_loudness* out) {
    if (B < 1 || !lengths || !out) return set_err(STS_EINVAL, "B >= 1, lengths and out are required");
    if (!loudness_args_valid(2, target_lufs, peak_dbfs)) return set_err(STS_EINVAL, "target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS");
    LoudArgs a{};
    if (!loud_coef(rate, &a.k)) return set_err(STS_EINVAL, "rate must be an integer in [8000, 48000]");
    std::vector<int> len;
    int64_t total = 0, maxl = 0;
    if (const char* bad = signal_lengths(lengths, B, INT64_MAX, x, len, &total, &maxl)) return set_err(STS_EINVAL, bad);
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    const size_t ob = (size_t)B * sizeof(sts_loudness);
    a.x = up_signal(d, x, total); a.len = d.up(len.data(), (size_t)B); a.ilen = 0; a.scale = 1; a.P = 1; a.Q = 1;
    a.target = target_lufs; a.ceiling = peak_dbfs;
    a.out = (float*)d.filled(ob, 0xFF);
    loud_ws_carve(a, d.filled(loud_ws_bytes(B, total), 0xFF), B, total);
    if (d.ok) loudness_run(a, B, maxl, nullptr, d.st);
    d.down(out, a.out, ob);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "loudness measurement failed on the device");
}

int sts_loudness_measure_chunked(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float target_lufs, float peak_dbfs,
                                 const int64_t* bounds, int32_t n_steps, int32_t back, sts_loudness* out, sts_loudness* partial) {
    if (B < 1 || !lengths || !out) return set_err(STS_EINVAL, "B >= 1, lengths and out are required");
    if (!loudness_args_valid(2, target_lufs, peak_dbfs)) return set_err(STS_EINVAL, "target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS");
    LoudStreamArgs a{};
    if (!loud_coef(rate, &a.k)) return set_err(STS_EINVAL, "rate must be an integer in [8000, 48000]");
    if (const int rc = step_bounds_check("loudness", bounds, n_steps, back, 2048)) return rc;
    std::vector<int> len;
    int64_t total = 0, maxl = 0;
    if (const char* bad = signal_lengths(lengths, B, (int64_t)1 << 30, x, len, &total, &maxl)) return set_err(STS_EINVAL, bad);
    std::vector<int64_t> off(B + 1, 0);
    std::vector<long long> lenv(lengths, lengths + B);
    for (int b = 0; b < B; b++) off[b + 1] = off[b] + lengths[b];
    // every step's rows: the window [max(0, c_k - back), min(N_b, c_k+1 + back)) of every utterance with N_b > c_k, consumed [c_k, min(N_b, c_k+1));
    // and the gate's table behind every step (partial) and behind the last one (out): {0, samples consumed, first tile} per utterance
    LdsTrack track; track.begin(B);
    const long long tiles_all = track.layout(lenv.data());
    std::vector<LdsRow> rows; std::vector<int> row0(n_steps + 1, 0); std::vector<long long> tiles(n_steps, 1);
    std::vector<long long> utab((size_t)(n_steps + 1) * B * 3, 0);
    size_t ws = 0;
    for (int k = 0; k < n_steps; k++) {
        const int64_t c0 = bounds[k], c1 = k + 1 < n_steps ? bounds[k + 1] : INT64_MAX;
        for (int b = 0; b < B; b++) {
            const int64_t N = lengths[b];
            if (N <= c0) continue;
            const int64_t o0 = std::max<int64_t>(0, c0 - back), o1 = c1 > N - back ? N : c1 + back, j1 = std::min<int64_t>(N, c1);
            const LdsRow r = track.row(b, off[b] + o0, o0, o1 - o0, j1);
            if (const char* bad = lds_row_check(r, N)) return set_err(STS_EINVAL, bad);
            if (r.e != c0) return set_err(STS_EINVAL, "loudness stream: a step does not continue where the last one ended");
            tiles[k] = std::max(tiles[k], lds_tiles(r.e, r.j1));
            rows.push_back(r);
        }
        track.commit();
        row0[k + 1] = (int)rows.size();
        ws = std::max(ws, lds_ws_bytes(row0[k + 1] - row0[k], tiles[k]));
        for (int b = 0; b < B; b++) { utab[((size_t)k * B + b) * 3 + 1] = track.e[b]; utab[((size_t)k * B + b) * 3 + 2] = track.tbase[b]; }
    }
    for (int b = 0; b < B; b++) { utab[((size_t)n_steps * B + b) * 3 + 1] = track.e[b]; utab[((size_t)n_steps * B + b) * 3 + 2] = track.tbase[b]; }
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    a.x = up_signal(d, x, total);
    const char* dr = (const char*)d.up_bytes(rows.data(), rows.size() * sizeof(LdsRow));
    long long* du = (long long*)d.up(utab.data(), utab.size());
    // (results, state, workspace and tables start out as NaN: a word the kernels leave out, or a stale one they read, shows)
    float* dout = (float*)d.filled((size_t)(n_steps + 1) * B * sizeof(sts_loudness), 0xFF);
    a.state = (char*)d.filled(lds_state_bytes(B), 0xFF); a.E = (double*)d.filled(ws, 0xFF);
    a.tsum = (double*)d.filled((size_t)tiles_all * kLdsSlots * 8, 0xFF); a.tpeak = d.out((size_t)tiles_all);
    LoudArgs g{};
    g.k = a.k; g.target = target_lufs; g.ceiling = peak_dbfs; g.tsum = a.tsum; g.tpeak = a.tpeak; g.gain = d.out((size_t)B);
    if (d.ok) {
        int slot = 0;
        for (int k = 0; k < n_steps; k++) {
            const int nw = row0[k + 1] - row0[k];
            if (nw > 0) {
                a.wtab = (const long long*)(dr + (size_t)row0[k] * sizeof(LdsRow)); a.slot = slot;
                loud_stream_run(a, nw, tiles[k], d.st);
                slot ^= 1;
            }
            if (partial) {      // the result as if the call had stopped behind this step
                g.utab = du + (size_t)k * B * 3; g.out = dout + (size_t)k * B * 4;
                loud_gate_run(g, B, d.st);
            }
        }
        g.utab = du + (size_t)n_steps * B * 3; g.out = dout + (size_t)n_steps * B * 4;
        loud_gate_run(g, B, d.st);
    }
    d.down(out, g.out, (size_t)B * sizeof(sts_loudness));
    d.down(partial, dout, (size_t)n_steps * B * sizeof(sts_loudness));
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "loudness measurement failed on the device");
}

int sts_limiter_apply(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float gain_db, float ceiling_dbfs,
                      float lookahead_ms, float* y, int16_t* pcm, sts_limiter_stats* stats) {
    if (B < 1 || !lengths) return set_err(STS_EINVAL, "B >= 1 and lengths are required");
    LimiterDesign dsg;
    if (!limiter_design(rate, gain_db, ceiling_dbfs, lookahead_ms, &dsg))
        return set_err(STS_EINVAL, "rate in [8000, 48000], gain in [-40, 40] dB, ceiling in [-30, 0] dBFS, look-ahead in [0.25, 10] ms");
    std::vector<int> len;
    int64_t total = 0, maxl = 0;
    if (const char* bad = signal_lengths(lengths, B, (int64_t)1 << 30, x, len, &total, &maxl)) return set_err(STS_EINVAL, bad);
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    LimArgs a{};
    a.x = up_signal(d, x, total); a.len = d.up(len.data(), (size_t)B); a.ilen = 0; a.scale = 1; a.P = 1; a.Q = 1;
    a.H = dsg.H; a.c = dsg.c; a.G = dsg.G; a.gloud = nullptr;
    a.y = y ? d.out((size_t)total) : nullptr;
    a.pcm = pcm ? d.out16((size_t)total) : nullptr;
    a.stat = (unsigned*)d.filled((size_t)B * 16, 0xFF);
    std::vector<unsigned> raw((size_t)B * 4);
    if (d.ok) limiter_run(a, B, maxl, d.st);
    d.down(y, a.y, (size_t)total * 4);
    d.down(pcm, a.pcm, (size_t)total * 2);
    d.down(raw.data(), a.stat, (size_t)B * 16);
    if (!d.finish()) return set_err(STS_EDEVICE, "the limiter failed on the device");
    if (stats) limiter_stats_decode(raw.data(), B, stats);
    return STS_OK;
}

int sts_eq_apply(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, int32_t n_bands, const sts_eq_band* bands,
                 float* y, int16_t* pcm) {
    if (B < 1 || !lengths) return set_err(STS_EINVAL, "B >= 1 and lengths are required");
    const char* why = nullptr;
    if (!eq_valid(rate, n_bands, bands, &why)) return set_err(STS_EINVAL, why);
    if (n_bands < 1) return set_err(STS_EINVAL, "eq: at least one band to apply");
    std::vector<int> len;
    int64_t total = 0, maxl = 0;
    if (const char* bad = signal_lengths(lengths, B, (int64_t)1 << 30, x, len, &total, &maxl)) return set_err(STS_EINVAL, bad);
    double coef[5 * STS_EQ_MAX_BANDS];
    eq_design(rate, n_bands, bands, coef);
    EqTable tab;
    eq_table(n_bands, coef, &tab);
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    EqArgs a{};
    a.x = up_signal(d, x, total); a.len = d.up(len.data(), (size_t)B); a.ilen = 0; a.scale = 1; a.P = 1; a.Q = 1;
    a.S = n_bands; a.tab = (const EqTable*)d.up_bytes(&tab, sizeof(EqTable));
    // (the outputs start out as NaN / 0x7FFF: a sample the kernels leave out shows)
    a.y = y ? d.out((size_t)total) : nullptr; a.pcm = pcm ? d.out16((size_t)total) : nullptr;
    eq_ws_carve(a, d.filled(eq_ws_bytes(B, total), 0xFF), B, total);
    if (d.ok) eq_run(a, B, maxl, d.st);
    d.down(y, a.y, (size_t)total * 4);
    d.down(pcm, a.pcm, (size_t)total * 2);
    return d.finish() ? STS_OK : set_err(STS_EDEVICE, "the equaliser failed on the device");
}

int sts_eq_apply_chunked(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, int32_t n_bands, const sts_eq_band* bands,
                         const int64_t* bounds, int32_t n_steps, int32_t back, float* y, int16_t* pcm, float* win_y, int64_t win_capacity,
                         int64_t* win_off) {
    if (B < 1 || !lengths) return set_err(STS_EINVAL, "B >= 1 and lengths are required");
    const char* why = nullptr;
    if (!eq_valid(rate, n_bands, bands, &why)) return set_err(STS_EINVAL, why);
    if (n_bands < 1) return set_err(STS_EINVAL, "eq: at least one band to apply");
    if (const int rc = step_bounds_check("eq", bounds, n_steps, back, kEqsHist / 2)) return rc;
    std::vector<int> len;
    int64_t total = 0, maxl = 0;
    if (const char* bad = signal_lengths(lengths, B, (int64_t)1 << 30, x, len, &total, &maxl)) return set_err(STS_EINVAL, bad);
    std::vector<int64_t> off(B + 1, 0);
    for (int b = 0; b < B; b++) off[b + 1] = off[b] + lengths[b];
    // every step's rows: the window [max(0, c_k - back), min(N_b, c_k+1 + back)) of every utterance with N_b > c_k, kept [c_k, min(N_b, c_k+1))
    EqsTrack track; track.begin(B);
    std::vector<EqsRow> rows; std::vector<int> row0(n_steps + 1, 0); std::vector<long long> tiles(n_steps, 1);
    int64_t wtotal = 0; size_t ws = 0;
    for (int k = 0; k < n_steps; k++) {
        const int64_t c0 = bounds[k], c1 = k + 1 < n_steps ? bounds[k + 1] : INT64_MAX;
        for (int b = 0; b < B; b++) {
            if (win_off) win_off[(size_t)k * B + b] = -1;
            const int64_t N = lengths[b];
            if (N <= c0) continue;
            const int64_t o0 = std::max<int64_t>(0, c0 - back), o1 = c1 > N - back ? N : c1 + back, j1 = std::min<int64_t>(N, c1);
            const EqsRow r = track.row(b, off[b] + o0, o0, o1 - o0, o0, o1, wtotal, c0, j1, off[b] + c0);
            if (const char* bad = eqs_row_check(r, N)) return set_err(STS_EINVAL, bad);
            tiles[k] = std::max(tiles[k], eqs_tiles(r.e, r.o1));
            if (win_off) win_off[(size_t)k * B + b] = wtotal;
            wtotal += o1 - o0;
            rows.push_back(r);
        }
        track.commit();
        row0[k + 1] = (int)rows.size();
        ws = std::max(ws, eqs_ws_bytes(row0[k + 1] - row0[k], tiles[k]));
    }
    if (win_y && wtotal > win_capacity) return set_err(STS_EINVAL, "eq stream: win_y is too small for the steps' windows");
    double coef[5 * STS_EQ_MAX_BANDS];
    eq_design(rate, n_bands, bands, coef);
    EqTable tab;
    eq_table(n_bands, coef, &tab);
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DevScratch d;
    EqArgs a{};
    a.x = up_signal(d, x, total); a.S = n_bands; a.tab = (const EqTable*)d.up_bytes(&tab, sizeof(EqTable));
    const char* dr = (const char*)d.up_bytes(rows.data(), rows.size() * sizeof(EqsRow));
    // (outputs, state and workspace start out as NaN / 0x7FFF: a sample the kernels leave out, or a stale word they read, shows)
    a.y = d.out((size_t)wtotal); a.pcm = d.out16((size_t)total);
    a.state = (char*)d.filled(eqs_state_bytes(B), 0xFF); a.E = (double*)d.filled(ws, 0xFF);
    if (d.ok) {
        int slot = 0;
        for (int k = 0; k < n_steps; k++) {
            const int nw = row0[k + 1] - row0[k];
            if (nw == 0) continue;
            a.wtab = (const long long*)(dr + (size_t)row0[k] * sizeof(EqsRow)); a.slot = slot;
            eq_stream_run(a, nw, tiles[k], d.st);
            slot ^= 1;
        }
    }
    std::vector<float> hw(win_y ? 0 : (size_t)wtotal);
    float* wdst = win_y ? win_y : hw.data();
    d.down(wdst, a.y, (size_t)wtotal * 4);
    d.down(pcm, a.pcm, (size_t)total * 2);
    if (!d.finish()) return set_err(STS_EDEVICE, "the equaliser failed on the device");
    if (y)                      // each step's kept range out of its window
        for (const EqsRow& r : rows)
            if (r.j1 > r.j0) memcpy(y + r.pdst, wdst + r.ybase + (r.j0 - r.o0), (size_t)(r.j1 - r.j0) * 4);
    return STS_OK;
}

}  // extern "C"
