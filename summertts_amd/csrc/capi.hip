// capi.hip -- extern "C" surface declared in include/summertts_hip.h: everything that takes an engine, the host-only design and check
// functions and the error text.  The stages on caller data are in capi_apply.hip, the kernel-level sts_debug_* entries in capi_debug.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "capi_common.hpp"
#include "engine.hpp"
#include "eq_stream.hpp"
#include "join_stream.hpp"
#include "loud_stream.hpp"
#include "para_stream.hpp"
#include "pitch_stream.hpp"

using namespace sts;

struct sts_engine { Engine eng; };

thread_local std::string sts::g_capi_err;
// the setters that write an engine member themselves: what an open stream fixed stays fixed until sts_stream_close (engine.hpp stream_open)
#define STS_CAPI_NOT_WHILE_OPEN(e) \
    do { if ((e)->eng.stream_is_open()) return set_err(STS_ESTATE, "a stream or a paragraph is open on this engine (sts_stream_close / sts_para_close first)"); } while (0)

extern "C" {

const char* sts_last_error(void) { return g_capi_err.c_str(); }
void sts_free(void* p) { free(p); }

int sts_create(const float* blob, int64_t blob_bytes, int device, sts_engine** out) {
    if (!out) return set_err(STS_EINVAL, "sts_create: null out pointer");
    *out = nullptr;
    sts_engine* e = new (std::nothrow) sts_engine();
    if (!e) return set_err(STS_EDEVICE, "out of host memory");
    int rc = e->eng.init(blob, blob_bytes, device);
    if (rc != STS_OK) { set_err(rc, e->eng.error()); delete e; return rc; }
    *out = e;
    return STS_OK;
}

void sts_destroy(sts_engine* e) { delete e; }

int sts_speaker_num(const sts_engine* e) {
    if (!e) return 1;
    return e->eng.model.spk_num == 0 ? 1 : e->eng.model.spk_num;   // SynthesizerTrn.cpp:79-89
}

int sts_get_info(const sts_engine* e, sts_model_info* info) {
    if (!e || !info) return set_err(STS_EINVAL, "null argument");
    const Model& m = e->eng.model;
    info->is_multi_speaker = m.is_ms; info->lang_type = m.lang; info->dur_pred_type = m.dur_type; info->dec_type = m.dec_type;
    info->vocab = m.vocab; info->hidden = m.hidden; info->inter_channels = m.inter;
    info->speaker_num = m.spk_num == 0 ? 1 : m.spk_num; info->gin_channels = m.gin;
    info->samples_per_frame = m.hop_total; info->sample_rate = kNativeRate;   // (the model's native rate, whatever sts_set_output_rate selects)
    info->blob_floats_consumed = m.consumed;
    return STS_OK;
}

int sts_run_batch(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                  const float* length_scale, int32_t* n_out, int64_t* total_out) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    int rc = e->eng.run(B, ids, n, sid, length_scale);
    if (rc != STS_OK) return set_err(rc, e->eng.error());
    if (n_out) for (int b = 0; b < B; b++) n_out[b] = e->eng.n_samples[b];
    if (total_out) *total_out = e->eng.total_samples;
    return STS_OK;
}

int sts_copy_pcm_device(sts_engine* e, void* dst, int64_t cap) {
    if (!e || !dst) return set_err(STS_EINVAL, "null argument");
    if (cap < e->eng.total_samples || !e->eng.d_pcm) return set_err(STS_ESTATE, "destination too small or no run yet");
    // (d_pcm is the mapped pinned host buffer when the run's last kernel wrote the PCM there: Engine::pcm_in_host_)
    if (hipMemcpyAsync(dst, e->eng.pcm_in_host_ ? (const void*)e->eng.h_pcm : (const void*)e->eng.d_pcm, (size_t)e->eng.total_samples * 2,
                       e->eng.pcm_in_host_ ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, e->eng.stream) != hipSuccess ||
        hipStreamSynchronize(e->eng.stream) != hipSuccess)
        return set_err(STS_EDEVICE, "device copy failed");
    return STS_OK;
}

int sts_copy_pcm_host(sts_engine* e, int16_t* dst, int64_t cap) {
    if (!e || !dst) return set_err(STS_EINVAL, "null argument");
    if (cap < e->eng.total_samples || !e->eng.d_pcm) return set_err(STS_ESTATE, "destination too small or no run yet");
    if (e->eng.h_pcm) { memcpy(dst, e->eng.h_pcm, (size_t)e->eng.total_samples * 2); return STS_OK; }   // downloaded inside the run
    if (hipMemcpyAsync(dst, e->eng.d_pcm, (size_t)e->eng.total_samples * 2, hipMemcpyDeviceToHost, e->eng.stream) != hipSuccess ||
        hipStreamSynchronize(e->eng.stream) != hipSuccess)
        return set_err(STS_EDEVICE, "device-to-host copy failed");
    return STS_OK;
}

int sts_pcm_host_view(sts_engine* e, const int16_t** pcm, int64_t* count) {
    if (!e || !pcm || !count) return set_err(STS_EINVAL, "null argument");
    if (!e->eng.h_pcm || !e->eng.d_pcm) return set_err(STS_ESTATE, "no host copy of the PCM (sts_set_host_pcm(e, 1) before the run)");
    *pcm = e->eng.h_pcm; *count = e->eng.total_samples;
    return STS_OK;
}

int sts_infer_ids_batch(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                        const float* length_scale, int16_t** pcm_out, int32_t* n_out) {
    if (!pcm_out || !n_out) return set_err(STS_EINVAL, "null output");
    int64_t total = 0;
    if (!e) return set_err(STS_EINVAL, "null engine");
    const bool was = e->eng.host_pcm;
    e->eng.host_pcm = true;               // the PCM download rides at the end of the run: one stream sync for the whole call
    int rc = sts_run_batch(e, B, ids, n, sid, length_scale, n_out, &total);
    e->eng.host_pcm = was;
    if (rc != STS_OK) return rc;
    int16_t* all = (int16_t*)malloc((size_t)(total > 0 ? total : 1) * 2);
    if (!all) return set_err(STS_EDEVICE, "out of host memory");
    rc = sts_copy_pcm_host(e, all, total);
    if (rc != STS_OK) { free(all); return rc; }
    int64_t off = 0;
    for (int b = 0; b < B; b++) {
        if (B == 1) { pcm_out[0] = all; break; }   // single utterance: hand over the buffer itself
        pcm_out[b] = (int16_t*)malloc((size_t)(n_out[b] > 0 ? n_out[b] : 1) * 2);
        if (!pcm_out[b]) {
            for (int q = 0; q < b; q++) { free(pcm_out[q]); pcm_out[q] = nullptr; }
            free(all);
            return set_err(STS_EDEVICE, "out of host memory");
        }
        memcpy(pcm_out[b], all + off, (size_t)n_out[b] * 2);
        off += n_out[b];
    }
    if (B != 1) free(all);
    return STS_OK;
}

int sts_infer_ids(sts_engine* e, const int32_t* ids, int32_t n, int32_t sid, float length_scale, int16_t** pcm_out,
                  int32_t* n_out) {
    const int32_t* idp[1] = {ids};
    return sts_infer_ids_batch(e, 1, idp, &n, &sid, &length_scale, pcm_out, n_out);
}

int sts_infer_ids_stream(sts_engine* e, const int32_t* ids, int32_t n, int32_t sid, float length_scale, int32_t chunk_frames,
                         sts_chunk_cb cb, void* user, int32_t* n_total) {
    if (!e || !ids || !cb) return set_err(STS_EINVAL, "null argument");
    const int32_t* idp[1] = {ids};
    struct { sts_chunk_cb cb; void* user; } one{cb, user};      // the engine's callback names the utterance; this one has a single one
    using One = decltype(one);
    StreamSpec ss{chunk_frames, [](void* u, int32_t, const int16_t* pcm, int32_t ns, int32_t off) { return ((One*)u)->cb(((One*)u)->user, pcm, ns, off); }, &one};
    const int rc = e->eng.run(1, idp, &n, &sid, &length_scale, &ss);
    if (rc != STS_OK) return set_err(rc, e->eng.error());
    if (n_total) *n_total = (int32_t)e->eng.total_samples;
    return STS_OK;
}

int sts_infer_ids_batch_stream(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                               const float* length_scale, int32_t chunk_frames, sts_batch_chunk_cb cb, void* user, int32_t* n_total) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (B < 1 || !ids || !n || chunk_frames <= 0 || !cb) return set_err(STS_EINVAL, "B >= 1, ids, n, a positive chunk size and a callback are required");
    const int rc = e->eng.run_batch_stream(B, ids, n, sid, length_scale, chunk_frames, cb, user, n_total);
    if (rc != STS_OK) return set_err(rc, e->eng.error());
    return STS_OK;
}

int sts_stream_open(sts_engine* e, int32_t chunk_frames, int32_t max_live, int64_t capacity_frames) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.stream_open(chunk_frames, max_live, capacity_frames);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_stream_open_ex(sts_engine* e, int32_t chunk_frames, int32_t max_live, int64_t capacity_frames, int64_t capacity_phonemes) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (capacity_phonemes < 0 || capacity_phonemes > (1 << 24)) return set_err(STS_EINVAL, "capacity_phonemes is 0 (sts_stream_open) or in [1, 2^24]");
    const int rc = e->eng.stream_open(chunk_frames, max_live, capacity_frames, capacity_phonemes);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_stream_tables_info(const sts_engine* e, int32_t* planned, int64_t* capacity_phonemes, int64_t* free_phonemes) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const LiveStream* L = e->eng.live_;
    if (planned) *planned = L && L->planned() ? 1 : 0;
    if (capacity_phonemes) *capacity_phonemes = L ? L->capacity_phonemes : 0;
    if (free_phonemes) *free_phonemes = L ? L->free_phoneme_count() : 0;
    return STS_OK;
}
int sts_stream_get_loudness(sts_engine* e, int32_t* slot_out, sts_loudness* out, int64_t capacity) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (!e->eng.live_) return set_err(STS_ESTATE, "no stream is open on this engine (sts_stream_open first)");
    // (the two lists are filled and cleared together; the shorter one bounds the copy whatever happens)
    const int64_t n = (int64_t)std::min(e->eng.loud_slots.size(), e->eng.loud_res.size()), m = std::min<int64_t>(n, std::max<int64_t>(capacity, 0));
    if (slot_out && m > 0) memcpy(slot_out, e->eng.loud_slots.data(), (size_t)m * sizeof(int32_t));
    if (out && m > 0) memcpy(out, e->eng.loud_res.data(), (size_t)m * sizeof(sts_loudness));
    return (int)n;
}
int sts_stream_admit(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                     const float* length_scale, const sts_stream_noise* noise, int32_t* slot_out, int32_t* n_samples_out,
                     int32_t* admitted) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.stream_admit(B, ids, n, sid, length_scale, noise, slot_out, n_samples_out, admitted);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_stream_step(sts_engine* e, sts_batch_chunk_cb cb, void* user, int32_t* live_after) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.stream_step(cb, user, live_after);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_stream_info(const sts_engine* e, int32_t* open, int32_t* live, int32_t* free_slots, int64_t* free_frames, int64_t* steps) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const LiveStream* L = e->eng.live_;
    if (open) *open = L ? 1 : 0;
    if (live) *live = L ? L->live_count() : 0;
    if (free_slots) *free_slots = L ? L->free_slots() : 0;
    if (free_frames) *free_frames = L ? L->free_frames() : 0;
    if (steps) *steps = L ? L->steps : 0;
    return STS_OK;
}
int sts_stream_close(sts_engine* e) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.stream_close();
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}

// ---- open paragraphs (engine.hpp para_open; para_stream.hpp)
int sts_para_open(sts_engine* e, int32_t chunk_frames, int32_t max_resident, int64_t capacity_frames, int32_t lead_frames, float fade_ms) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.para_open(chunk_frames, max_resident, capacity_frames, lead_frames, fade_ms);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_para_append(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* length_scale,
                    const int32_t* gap_frames, int32_t* frames_out, int64_t* start_out, int32_t* appended) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.para_append(B, ids, n, sid, length_scale, gap_frames, frames_out, start_out, appended);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_para_finish(sts_engine* e, int32_t trail_frames) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.para_finish(trail_frames);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_para_step(sts_engine* e, sts_chunk_cb cb, void* user, int32_t* ready_after) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (!cb) return set_err(STS_EINVAL, "a step takes a callback");
    struct { sts_chunk_cb cb; void* user; } one{cb, user};      // the engine's callback names the utterance; a paragraph is a single one
    using One = decltype(one);
    const int rc = e->eng.para_step([](void* u, int32_t, const int16_t* pcm, int32_t ns, int32_t off) { return ((One*)u)->cb(((One*)u)->user, pcm, ns, off); },
                                    &one, ready_after);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_para_info(const sts_engine* e, int32_t* open, int32_t* finished, int64_t* sentences, int32_t* resident, int32_t* free_slots,
                  int64_t* free_frames, int64_t* frames_known, int64_t* frames_delivered, int64_t* steps) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const ParaStream* P = e->eng.para_;
    if (open) *open = P ? 1 : 0;
    if (finished) *finished = P && P->finished ? 1 : 0;
    if (sentences) *sentences = P ? P->sentences() : 0;
    if (resident) *resident = P ? P->resident() : 0;
    if (free_slots) *free_slots = P ? P->pool.free_slots() : 0;
    if (free_frames) *free_frames = P ? P->pool.free_frames() : 0;
    if (frames_known) *frames_known = P ? P->frames_known() : 0;
    if (frames_delivered) *frames_delivered = P ? P->frames_delivered() : 0;
    if (steps) *steps = P ? P->pool.steps : 0;
    return STS_OK;
}
int sts_para_close(sts_engine* e) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.para_close();
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}

int sts_stream_halo_frames(const sts_engine* e) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    return e->eng.stream_halo(e->eng.pitch_streaming && e->eng.pend.have_pitch);      // (the larger halo of a stream through the pitch warp)
}

int sts_set_forced_durations(sts_engine* e, const int32_t* dur, int64_t count) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (!(e->eng.live_ && e->eng.live_->planned())) STS_CAPI_NOT_WHILE_OPEN(e);     // (a planned open stream: for its next admission)
    e->eng.set_forced_durations(dur, count);
    return STS_OK;
}

int sts_set_duration_plan(sts_engine* e, int32_t B, const int32_t* n, const sts_dur_plan* plans) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_duration_plan(B, n, plans);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_get_phoneme_offsets(sts_engine* e, int64_t* start, int64_t capacity) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.phoneme_offsets(start, capacity);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_duration_fit(const float* w, const int32_t* fixed, int32_t n, int32_t target_frames, int32_t* dur_out) {
    if (!dur_out || n < 1) return set_err(STS_EINVAL, "n >= 1 and dur_out are required");
    const char* why = nullptr;
    if (!dur_plan_valid(n, nullptr, fixed, target_frames, &why)) return set_err(STS_EINVAL, why);
    if (!w) {            // (weights are read for the free phonemes only)
        for (int i = 0; i < n; i++) if (!fixed || fixed[i] < 0) return set_err(STS_EINVAL, "null weights with a free phoneme");
    }
    duration_fit(w, fixed, n, target_frames, dur_out);
    return STS_OK;
}

int sts_set_speaker_mix(sts_engine* e, int32_t B, const sts_speaker_mix* mixes) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_speaker_mix(B, mixes);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_speaker_mix_check(int32_t speaker_num, int32_t gin, int32_t B, const sts_speaker_mix* mixes) {
    if (B < 0 || (B > 0 && !mixes) || speaker_num < 0 || gin < 0) return set_err(STS_EINVAL, "speaker mix: B >= 0 entries, speaker_num >= 0 and gin >= 0 are required");
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (!speaker_mix_valid(speaker_num, gin, mixes[b], &why)) return set_err(STS_EINVAL, why);
    }
    return STS_OK;
}
int sts_get_speaker_embedding(const sts_engine* e, int32_t sid, float* out, int64_t capacity) {
    if (!e || !out) return set_err(STS_EINVAL, "null argument");
    const int rc = e->eng.speaker_embedding(sid, out, capacity);
    if (rc == STS_EINVAL) return set_err(rc, "speaker embedding: a multi-speaker model, sid in [0, speaker_num) and capacity >= gin_channels are required");
    return rc == STS_OK ? STS_OK : set_err(rc, "speaker embedding: the device copy failed");
}

int sts_set_gain_plan(sts_engine* e, int32_t B, const int32_t* n, const sts_gain_plan* plans) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_gain_plan(B, n, plans);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_gain_plan_check(int32_t B, const int32_t* n, const sts_gain_plan* plans) {
    if (B < 0 || (B > 0 && (!n || !plans))) return set_err(STS_EINVAL, "gain plan: B >= 0 plans and their phoneme counts are required");
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (!gain_plan_valid(n[b], plans[b].gain_db, plans[b].ramp_ms, &why)) return set_err(STS_EINVAL, why);
    }
    return STS_OK;
}
int sts_gain_design(const float* gain_db, int32_t n, float ramp_ms, int32_t* q, int32_t* h) {
    const char* why = nullptr;
    if (!gain_plan_valid(n, gain_db, ramp_ms, &why)) return set_err(STS_EINVAL, why);
    gain_design(gain_db, n, ramp_ms, q, h);
    return STS_OK;
}

int sts_set_pitch_plan(sts_engine* e, int32_t B, const int32_t* n, const sts_pitch_plan* plans) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_pitch_plan(B, n, plans);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_pitch_plan_check(int32_t B, const int32_t* n, const sts_pitch_plan* plans) {
    if (B < 0 || (B > 0 && (!n || !plans))) return set_err(STS_EINVAL, "pitch plan: B >= 0 plans and their phoneme counts are required");
    for (int b = 0; b < B; b++) {
        const char* why = nullptr;
        if (!pitch_plan_valid(n[b], plans[b].cents, &why)) return set_err(STS_EINVAL, why);
    }
    return STS_OK;
}
int sts_pitch_design(const int32_t* cents, int32_t n, float* ratio, int64_t* step) {
    const char* why = nullptr;
    if (!pitch_plan_valid(n, cents, &why)) return set_err(STS_EINVAL, why);
    for (int i = 0; i < n; i++) {
        if (ratio) ratio[i] = cents ? pitch_ratio(cents[i]) : 1.f;
        if (step) step[i] = cents ? pitch_step(cents[i]) : kPitchOne;
    }
    return STS_OK;
}
int sts_pitch_layout(const int32_t* dur_frames, const int64_t* step, int32_t n, int32_t samples_per_frame, int64_t* out_start, int64_t* resid) {
    if (!pitch_layout(dur_frames, step, n, samples_per_frame, out_start, resid))
        return set_err(STS_EINVAL, "pitch layout: n >= 1 durations in [0, 100000], steps in [step(-600), step(600)], samples_per_frame in [1, 2^20] and fewer than 2^30 samples are required");
    return STS_OK;
}
int sts_set_pitch_streaming(sts_engine* e, int enable) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    STS_CAPI_NOT_WHILE_OPEN(e);
    e->eng.pitch_streaming = enable != 0;
    return STS_OK;
}
int sts_pitch_chunk_starts(const int32_t* dur_frames, const int64_t* step, int32_t n, int32_t samples_per_frame, int32_t chunk_frames,
                           int64_t* out_first, int64_t capacity) {
    if (n < 1 || !dur_frames || samples_per_frame < 1 || samples_per_frame > kPitchMaxHop || chunk_frames < 1 || capacity < 0 || (capacity > 0 && !out_first))
        return set_err(STS_EINVAL, "pitch chunk starts: n >= 1 durations, samples_per_frame in [1, 2^20] and chunk_frames >= 1 are required");
    if (step)
        for (int i = 0; i < n; i++)
            if (step[i] < kPitchStepMin || step[i] > kPitchStepMax) return set_err(STS_EINVAL, "pitch chunk starts: steps must be in [step(-600), step(600)]");
    PitchTables tab;
    const long long xoff = 0;
    if (const char* bad = pitch_tables(1, &n, &dur_frames, &step, &xoff, samples_per_frame, &tab)) return set_err(STS_EINVAL, bad);
    const PsUtt u = ps_utt(tab.words.data(), 1, tab.TT, 0);
    const long long F = u.N / samples_per_frame, chunks = (F + chunk_frames - 1) / chunk_frames;
    if (chunks > 0x7fffffffll) return set_err(STS_EINVAL, "pitch chunk starts: too many chunks");
    if (out_first) {
        if (capacity < chunks + 1) return set_err(STS_EINVAL, "pitch chunk starts: out_first needs room for one entry per chunk and one more");
        for (long long k = 0; k < chunks; k++) out_first[k] = ps_Y(u, k * chunk_frames * samples_per_frame);
        out_first[chunks] = u.Nw;
    }
    return (int)chunks;
}
int sts_pitch_table(float* table, int64_t capacity_floats) {
    if (!table || capacity_floats < kPitchTableFloats) return set_err(STS_EINVAL, "pitch table: room for 16386 floats is required");
    pitch_table(table);
    return STS_OK;
}

int sts_join_check(int32_t B, const sts_join* join) {
    const char* why = nullptr;
    if (!join_valid(B, join, &why)) return set_err(STS_EINVAL, why);
    return STS_OK;
}
int sts_join_layout(int32_t B, const int32_t* frames, int32_t samples_per_frame, const sts_join* join, int64_t* start, int64_t* total, int32_t* h) {
    const char* why = nullptr;
    if (!join_valid(B, join, &why)) return set_err(STS_EINVAL, why);
    if (!frames || samples_per_frame < 1) return set_err(STS_EINVAL, "join: frames and samples_per_frame >= 1 are required");
    std::vector<long long> sil((size_t)B);
    const long long all = join_silence(B, join, sil.data());
    long long F = 0;
    for (int b = 0; b < B; b++) {
        if (frames[b] < 1) return set_err(STS_EINVAL, "join: every sentence has frames[b] >= 1");
        if (start) start[b] = (F + sil[b]) * samples_per_frame;
        F += frames[b];
    }
    if (total) *total = (F + all) * samples_per_frame;
    if (h) *h = join ? join_design(join->fade_ms) : 0;
    return STS_OK;
}
int sts_infer_ids_joined(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                         const float* length_scale, const sts_join* join, int16_t** pcm_out, int32_t* n_out) {
    if (!pcm_out || !n_out) return set_err(STS_EINVAL, "null output");
    if (!e) return set_err(STS_EINVAL, "null engine");
    const bool was = e->eng.host_pcm;
    e->eng.host_pcm = true;               // the PCM download rides at the end of the run: one stream sync for the whole call
    int rc = e->eng.run_joined(B, ids, n, sid, length_scale, join);
    e->eng.host_pcm = was;
    if (rc != STS_OK) return set_err(rc, e->eng.error());
    const int64_t total = e->eng.total_samples;
    int16_t* all = (int16_t*)malloc((size_t)(total > 0 ? total : 1) * 2);
    if (!all) return set_err(STS_EDEVICE, "out of host memory");
    rc = sts_copy_pcm_host(e, all, total);
    if (rc != STS_OK) { free(all); return rc; }
    *pcm_out = all; *n_out = (int32_t)total;
    return STS_OK;
}
int sts_infer_ids_joined_stream(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                                const float* length_scale, const sts_join* join, int32_t chunk_frames, sts_chunk_cb cb, void* user,
                                int32_t* n_total) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (B < 1 || !ids || !n || chunk_frames <= 0 || !cb) return set_err(STS_EINVAL, "B >= 1, ids, n, a positive chunk size and a callback are required");
    struct { sts_chunk_cb cb; void* user; } one{cb, user};      // the engine's callback names the utterance; J is the only one
    using One = decltype(one);
    const int rc = e->eng.run_joined_stream(B, ids, n, sid, length_scale, join, chunk_frames,
                                            [](void* u, int32_t, const int16_t* pcm, int32_t ns, int32_t off) { return ((One*)u)->cb(((One*)u)->user, pcm, ns, off); },
                                            &one, n_total);
    if (rc != STS_OK) return set_err(rc, e->eng.error());
    return STS_OK;
}
int sts_get_join_offsets(sts_engine* e, int64_t* start, int64_t capacity) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.join_offsets(start, capacity);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}

int sts_set_noise(sts_engine* e, float noise_scale, float noise_scale_w, uint64_t seed) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return set_err(STS_EINVAL, "noise scales must be finite and >= 0");
    e->eng.noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    return STS_OK;
}
int sts_get_noise(const sts_engine* e, float* noise_scale, float* noise_scale_w, uint64_t* seed) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (noise_scale) *noise_scale = e->eng.noise.ns;
    if (noise_scale_w) *noise_scale_w = e->eng.noise.nsw;
    if (seed) *seed = e->eng.noise.seed;
    return STS_OK;
}
int sts_set_record_taps(sts_engine* e, int enable) { if (!e) return set_err(STS_EINVAL, "null engine"); STS_CAPI_NOT_WHILE_OPEN(e); e->eng.record_taps = enable != 0; return STS_OK; }
int sts_set_conv_math(sts_engine* e, int mode) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (mode < 0 || mode > 3) return set_err(STS_EINVAL, "conv math: 0 = split-bf16 (default), 1 = exact fp32, 2 = split-bf16 wherever eligible, 3 = two-term fp16");
    STS_CAPI_NOT_WHILE_OPEN(e);
    e->eng.conv_math = mode;
    e->eng.h2_consecutive = 0; e->eng.h2_disabled = false;
    return STS_OK;
}
int sts_set_conv_mode(sts_engine* e, int mode) { if (!e) return set_err(STS_EINVAL, "null engine"); STS_CAPI_NOT_WHILE_OPEN(e); e->eng.conv_mode = mode; return STS_OK; }
int sts_debug_set(sts_engine* e, int key, int value) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (key != STS_DBG_STREAM_RETRY_STEP && key != STS_DBG_POISON) STS_CAPI_NOT_WHILE_OPEN(e);     // (the two test hooks of a step stay settable)
    switch (key) {
        case STS_DBG_ATTN_BLOCK_MIN_WGS: if (value < 1) return set_err(STS_EINVAL, "threshold must be >= 1"); e->eng.attn_block_min_wgs = value; return STS_OK;
        case STS_DBG_FLOW_FUSED: e->eng.flow_fused = value == 2 || value == 3 ? value : value != 0; return STS_OK;
        case STS_DBG_LAUNCH_AHEAD: if (value < 0 || value > 2) return set_err(STS_EINVAL, "launch_ahead must be 0, 1 or 2"); if ((value == 2) != (e->eng.launch_ahead == 2)) { e->eng.seen_tf_.clear(); e->eng.seen_order_.clear(); } e->eng.launch_ahead = value; return STS_OK;
        case STS_DBG_H2P: e->eng.h2p = value < 0 ? 0 : (value > 4 ? 4 : value); return STS_OK;
        case STS_DBG_H2P_TILE: e->eng.h2p_tile = value; return STS_OK;
        case STS_DBG_CHAIN_STREAMS: e->eng.chain_streams_dbg = value; return STS_OK;
        case STS_DBG_TAIL_FUSED: e->eng.tail_fused = value != 0; return STS_OK;
        case STS_DBG_UPS_ROWPH: e->eng.ups_rowph = value != 0; return STS_OK;
        case STS_DBG_MEMO_CLEAR: e->eng.seen_tf_.clear(); e->eng.seen_order_.clear(); return STS_OK;
        case STS_DBG_ATTN_REG: e->eng.attn_reg = value != 0; return STS_OK;
        case STS_DBG_DDS_TAIL: e->eng.dds_tail = value != 0; return STS_OK;
        case STS_DBG_PCM_DIRECT: e->eng.pcm_direct = value != 0; return STS_OK;
        case STS_DBG_STREAM_RETRY_STEP: e->eng.stream_retry_step = value == -2 ? -2 : (value < 0 ? -1 : value); return STS_OK;      // (-2: admissions, engine.hpp)
        case STS_DBG_STREAM_DIRECT: e->eng.stream_direct = value != 0; return STS_OK;
        case STS_DBG_POISON: e->eng.poison = (unsigned)value; return STS_OK;
        case STS_DBG_COL_PROJ: if (value < 0 || value > 3) return set_err(STS_EINVAL, "col_proj must be 0, 1, 2 or 3"); e->eng.col_proj_mode = value; return STS_OK;
        case STS_DBG_SDP_PRE_RIDE: e->eng.sdp_pre_ride = value != 0; return STS_OK;
        default: return set_err(STS_EINVAL, "unknown debug key");
    }
}
int sts_set_host_pcm(sts_engine* e, int enable) { if (!e) return set_err(STS_EINVAL, "null engine"); e->eng.host_pcm = enable != 0; return STS_OK; }
int sts_set_profiling(sts_engine* e, int enable) { if (!e) return set_err(STS_EINVAL, "null engine"); e->eng.profiling = enable == 2 ? 2 : (enable != 0 ? 1 : 0); return STS_OK; }

int sts_abi_version(void) { return STS_ABI_VERSION; }

int sts_set_output_rate(sts_engine* e, int32_t rate) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_output_rate(rate);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_get_output_rate(const sts_engine* e) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    return e->eng.out_rate;
}
int sts_resample_table(int32_t in_rate, int32_t out_rate, int32_t* P, int32_t* Q, int32_t* taps, float* table, int64_t capacity_floats) {
    ResampleDesign d;
    if (!resample_design(in_rate, out_rate, &d)) return set_err(STS_EINVAL, "rates must be integers in [8000, 48000] with P = out / gcd(in, out) <= 1024");
    const int64_t need = (int64_t)d.P * 2 * d.K;
    if (table && capacity_floats < need) return set_err(STS_EINVAL, "table capacity below P * taps floats");
    if (P) *P = d.P;
    if (Q) *Q = d.Q;
    if (taps) *taps = 2 * d.K;
    if (table) resample_table(d, in_rate, out_rate, table);
    return STS_OK;
}
int sts_set_loudness(sts_engine* e, int mode, float target_lufs, float peak_dbfs) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_loudness(mode, target_lufs, peak_dbfs);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_get_loudness_mode(const sts_engine* e, int* mode, float* target_lufs, float* peak_dbfs) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (mode) *mode = e->eng.loud_mode;
    if (target_lufs) *target_lufs = e->eng.loud_target;
    if (peak_dbfs) *peak_dbfs = e->eng.loud_peak;
    return STS_OK;
}
int sts_get_loudness(sts_engine* e, sts_loudness* out, int64_t capacity) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int64_t n = (int64_t)e->eng.loud_res.size();
    if (!out) return (int)n;              // (the count alone)
    if (capacity < n) return set_err(STS_EINVAL, "capacity below the last call's utterance count");
    if (n > 0) memcpy(out, e->eng.loud_res.data(), (size_t)n * sizeof(sts_loudness));
    return (int)n;
}
int sts_kweight_coeffs(int32_t rate, double coeffs[10]) {
    if (!coeffs) return set_err(STS_EINVAL, "null argument");
    if (!kweight_coeffs(rate, coeffs)) return set_err(STS_EINVAL, "rate must be an integer in [8000, 48000]");
    return STS_OK;
}
int sts_set_loudness_streaming(sts_engine* e, int enable) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    STS_CAPI_NOT_WHILE_OPEN(e);
    e->eng.loud_streaming = enable != 0;
    return STS_OK;
}
int sts_get_loudness_streaming(const sts_engine* e) { return e && e->eng.loud_streaming ? 1 : 0; }
int sts_set_limiter(sts_engine* e, int mode, float gain_db, float ceiling_dbfs, float lookahead_ms) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_limiter(mode, gain_db, ceiling_dbfs, lookahead_ms);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_get_limiter_mode(const sts_engine* e, int* mode, float* gain_db, float* ceiling_dbfs, float* lookahead_ms) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (mode) *mode = e->eng.lim_mode;
    if (gain_db) *gain_db = e->eng.lim_gain_db;
    if (ceiling_dbfs) *ceiling_dbfs = e->eng.lim_ceiling;
    if (lookahead_ms) *lookahead_ms = e->eng.lim_ms;
    return STS_OK;
}
int sts_get_limiter(sts_engine* e, sts_limiter_stats* out, int64_t capacity) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int64_t n = (int64_t)e->eng.lim_res.size();
    if (!out) return (int)n;              // (the count alone)
    if (capacity < n) return set_err(STS_EINVAL, "capacity below the last call's utterance count");
    if (n > 0) memcpy(out, e->eng.lim_res.data(), (size_t)n * sizeof(sts_limiter_stats));
    return (int)n;
}
int sts_limiter_design(int32_t rate, float gain_db, float ceiling_dbfs, float lookahead_ms, int32_t* H, double* c, double* G) {
    LimiterDesign d;
    if (!limiter_design(rate, gain_db, ceiling_dbfs, lookahead_ms, &d))
        return set_err(STS_EINVAL, "rate in [8000, 48000], gain in [-40, 40] dB, ceiling in [-30, 0] dBFS, look-ahead in [0.25, 10] ms");
    if (H) *H = d.H;
    if (c) *c = d.c;
    if (G) *G = d.G;
    return STS_OK;
}
int sts_set_eq(sts_engine* e, int32_t n_bands, const sts_eq_band* bands) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    const int rc = e->eng.set_eq(n_bands, bands);
    return rc == STS_OK ? STS_OK : set_err(rc, e->eng.error());
}
int sts_get_eq(const sts_engine* e, int32_t* n_bands, sts_eq_band* bands, int32_t capacity) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    if (n_bands) *n_bands = e->eng.eq_n;
    for (int i = 0; bands && i < e->eng.eq_n && i < capacity; i++) bands[i] = e->eng.eq_bands[i];
    return STS_OK;
}
int sts_set_eq_streaming(sts_engine* e, int enable) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    STS_CAPI_NOT_WHILE_OPEN(e);
    e->eng.eq_streaming = enable != 0;
    return STS_OK;
}
int sts_get_eq_streaming(const sts_engine* e) { return e && e->eng.eq_streaming ? 1 : 0; }
int sts_eq_check(int32_t rate, int32_t n_bands, const sts_eq_band* bands) {
    const char* why = nullptr;
    return eq_valid(rate, n_bands, bands, &why) ? STS_OK : set_err(STS_EINVAL, why);
}
int sts_eq_design(int32_t rate, int32_t n_bands, const sts_eq_band* bands, double* coeffs) {
    const char* why = nullptr;
    if (!eq_valid(rate, n_bands, bands, &why)) return set_err(STS_EINVAL, why);
    if (n_bands > 0 && !coeffs) return set_err(STS_EINVAL, "null argument");
    eq_design(rate, n_bands, bands, coeffs);
    return STS_OK;
}
int sts_build_flags(void) {
#ifdef STS_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}
int sts_get_profile_ex(const sts_engine* e, void* p, int64_t size_bytes) {
    if (!e || !p || size_bytes <= 0) return set_err(STS_EINVAL, "null argument");
    // the struct only grows at its end: a client built against an older header hands in its own sizeof and gets that prefix
    const size_t n = (size_t)size_bytes < sizeof(sts_profile) ? (size_t)size_bytes : sizeof(sts_profile);
    memcpy(p, &e->eng.prof, n);
    return STS_OK;
}
int sts_get_profile(const sts_engine* e, sts_profile* p) { return sts_get_profile_ex(e, p, (int64_t)sizeof(sts_profile)); }

int sts_get_tap(sts_engine* e, const char* name, float** data, int32_t* channels, int64_t* length) {
    if (!e || !name || !data || !channels || !length) return set_err(STS_EINVAL, "null argument");
    auto it = e->eng.taps.find(name);
    if (it == e->eng.taps.end()) return set_err(STS_ESTATE, std::string("tap not recorded: ") + name);
    const Tap& t = it->second;
    float* p = (float*)malloc(t.data.size() * sizeof(float) + 4);
    if (!p) return set_err(STS_EDEVICE, "out of host memory");
    memcpy(p, t.data.data(), t.data.size() * sizeof(float));
    *data = p; *channels = t.channels; *length = t.length;
    return STS_OK;
}

int sts_get_durations(sts_engine* e, int32_t* dur, int64_t cap) {
    if (!e || !dur) return set_err(STS_EINVAL, "null argument");
    if ((int64_t)e->eng.durations_h.size() > cap) return set_err(STS_ESTATE, "destination too small");
    memcpy(dur, e->eng.durations_h.data(), e->eng.durations_h.size() * sizeof(int32_t));
    return STS_OK;
}

// host only: the Winograd-domain copy of a conv's weights, as pack_wino and sts_debug_conv1d (mode 12) make it
int sts_debug_wino_pack(const float* w, int32_t Cout, int32_t k, int32_t Cin, float* out, int64_t out_floats) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || k < 2) return set_err(STS_EINVAL, "bad arguments");
    int n3, n2; wino_split(k, &n3, &n2);
    const int Cin_pad = (Cin + 15) / 16 * 16, Cout_pad = (Cout + 31) / 32 * 32;
    if (out_floats < (int64_t)(n3 + n2) * 4 * Cin_pad * Cout_pad) return set_err(STS_EINVAL, "output buffer too small");
    wino_pack(w, (long)k * Cin, Cin, 1, Cout, k, Cin, Cin_pad, Cout_pad, out);
    return n3 + n2;
}

}  // extern "C"
