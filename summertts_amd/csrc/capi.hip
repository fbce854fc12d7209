// capi.hip -- extern "C" surface declared in include/summertts_hip.h.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "engine.hpp"
#include "eq_stream.hpp"
#include "join_stream.hpp"
#include "loud_stream.hpp"
#include "para_stream.hpp"

using namespace sts;

struct sts_engine { Engine eng; };

static thread_local std::string g_err;
static int set_err(int code, const std::string& s) { g_err = s; return code; }
// the setters that write an engine member themselves: what an open stream fixed stays fixed until sts_stream_close (engine.hpp stream_open)
#define STS_CAPI_NOT_WHILE_OPEN(e) \
    do { if ((e)->eng.stream_is_open()) return set_err(STS_ESTATE, "a stream or a paragraph is open on this engine (sts_stream_close / sts_para_close first)"); } while (0)

extern "C" {

const char* sts_last_error(void) { return g_err.c_str(); }
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
    return e->eng.stream_halo();
}

int sts_set_forced_durations(sts_engine* e, const int32_t* dur, int64_t count) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    STS_CAPI_NOT_WHILE_OPEN(e);
    if (!dur || count <= 0) { e->eng.have_forced = false; return STS_OK; }
    e->eng.forced_dur.assign(dur, dur + count);
    e->eng.have_forced = true;
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
    const size_t wb = (((size_t)total * 4 + 255) & ~(size_t)255), tb = ((tab.size() * 4 + 255) & ~(size_t)255), rb = (((size_t)total * 8 + 255) & ~(size_t)255);
    char* d = nullptr;          // [w | fixed | out | tables | remainders]
    if (hipMalloc((void**)&d, 3 * wb + tb + rb) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    DurPlanArgs a{};
    a.w_in = (const float*)d; a.fixed = fixed ? (const int*)(d + wb) : nullptr; a.forced = (int*)(d + 2 * wb);
    const int* dt = (const int*)(d + 3 * wb);
    a.target = dt + 2 * B; a.rem = (long long*)(d + 3 * wb + tb);
    a.seg = SegView{dt, dt + B, 1, 0, 0, 0};
    ok = ok && hipMemcpyAsync(d, w, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         (!fixed || hipMemcpyAsync(d + wb, fixed, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemcpyAsync(d + 3 * wb, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        duration_plan(a, B, st);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(dur_out, a.forced, (size_t)total * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "the duration plan failed on the device");
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
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t tb = pad((size_t)speaker_num * gin * 4), sb = pad((size_t)B * 4), wb = pad(words.size() * 4), gb = pad((size_t)B * gin * 4);
    char* d = nullptr;          // [table | sid | term table | g]
    if (hipMalloc((void**)&d, tb + sb + wb + gb) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    std::vector<float> g((size_t)B * gin);       // [gin][B], the engine's layout
    ok = ok && hipMemcpyAsync(d, table, (size_t)speaker_num * gin * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d + tb, sidv.data(), (size_t)B * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d + tb + sb, words.data(), words.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        speaker_blend((const float*)d, speaker_num, gin, (const int*)(d + tb), B, speaker_mix_tab((const int*)(d + tb + sb), B, K), (float*)(d + tb + sb + wb), st);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(g.data(), d + tb + sb + wb, g.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    if (!ok) return set_err(STS_EDEVICE, "the speaker blend failed on the device");
    for (int b = 0; b < B; b++) for (int c = 0; c < gin; c++) g_out[(size_t)b * gin + c] = g[(size_t)c * B + b];
    return STS_OK;
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
            const int32_t d = dur_frames[t + i];
            if (d < 0 || d > kDurMax) return set_err(STS_EINVAL, "durations must be in [0, 100000]");
            f += d;
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
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t xb = pad((size_t)total * 4), tb = pad(tab.size() * 4), pb = pad((size_t)total * 2);
    char* d = nullptr;          // [x | tables | y | pcm]
    if (hipMalloc((void**)&d, 2 * xb + tb + pb) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    const int* dt = (const int*)(d + xb);
    GainArgs a{};
    a.x = (const float*)d; a.y = y ? (float*)(d + xb + tb) : nullptr; a.pcm = pcm ? (int16_t*)(d + 2 * xb + tb) : nullptr;
    a.wseg = SegView{dt + 2 * B, dt + 3 * B, hop, 0, 0, 0}; a.hop = hop;
    a.tseg = SegView{dt, dt + B, 1, 0, 0, 0};
    a.h = dt + 4 * B; a.cum = dt + 5 * B; a.q = dt + 5 * B + T;
    ok = ok && hipMemcpyAsync(d, x, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d + xb, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        gain_plan_run(a, B, maxF * hop, st);
        ok = hipGetLastError() == hipSuccess &&
             (!y || hipMemcpyAsync(y, a.y, (size_t)total * 4, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             (!pcm || hipMemcpyAsync(pcm, a.pcm, (size_t)total * 2, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "the gain plan failed on the device");
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
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t xb = pad((size_t)NX * 4), tb = pad(tab.size() * 4), yb = pad((size_t)NJ * 4), pb = pad((size_t)NJ * 2);
    char* d = nullptr;          // [x | table | y | pcm]
    if (hipMalloc((void**)&d, xb + tb + yb + pb) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    const int* dt = (const int*)(d + xb);
    JoinArgs a{};
    a.x = (const float*)d; a.y = y ? (float*)(d + xb + tb) : nullptr; a.pcm = pcm ? (int16_t*)(d + xb + tb + yb) : nullptr;
    a.wseg = SegView{dt, dt + B, hop, 0, 0, 0}; a.sil = dt + 2 * B;
    a.B = B; a.hop = hop; a.h = join ? join_design(join->fade_ms) : 0; a.NJ = NJ;
    // (the outputs start out as NaN / 0x7FFF: a sample the kernel leaves out shows)
    ok = ok && hipMemcpyAsync(d, x, (size_t)NX * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d + xb, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemsetAsync(d + xb + tb, 0xFF, yb, st) == hipSuccess &&
         hipMemsetD16Async((hipDeviceptr_t)(d + xb + tb + yb), 0x7FFF, pb / 2, st) == hipSuccess;
    if (ok) {
        join_run(a, st);
        ok = hipGetLastError() == hipSuccess &&
             (!y || hipMemcpyAsync(y, d + xb + tb, (size_t)NJ * 4, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             (!pcm || hipMemcpyAsync(pcm, d + xb + tb + yb, (size_t)NJ * 2, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "the join failed on the device");
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
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t xb = pad((size_t)NX * 4 + 16), tb = pad((size_t)nw * 5 * 8 + 8), yb = pad((size_t)NY * 4), pb = pad((size_t)NY * 2);
    char* d = nullptr;          // [x: only the parts inside the range, packed | table | y | pcm]
    if (hipMalloc((void**)&d, xb + tb + yb + pb) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    std::vector<long long> tab((size_t)nw * 5 + 1);
    std::vector<int64_t> xoffF((size_t)B + 1, 0);       // sentence b's first frame in the caller's x
    for (int b = 0; b < B; b++) xoffF[b + 1] = xoffF[b] + frames[b];
    for (int i = 0; i < nw && ok; i++) {
        const JsWin& w = win[i]; const JsRow& r = rows[i];
        tab[5 * i] = r.st; tab[5 * i + 1] = r.en; tab[5 * i + 2] = r.S; tab[5 * i + 3] = r.N; tab[5 * i + 4] = r.xoff;
        ok = hipMemcpyAsync(d + (size_t)w.coff * hop * 4, x + (xoffF[w.b] + w.w0) * hop, (size_t)(w.w1 - w.w0) * hop * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    }
    JoinWinArgs a{};
    a.x = (const float*)d; a.y = y ? (float*)(d + xb + tb) : nullptr; a.pcm = pcm ? (int16_t*)(d + xb + tb + yb) : nullptr;
    a.rows = (const long long*)(d + xb); a.nw = nw; a.hop = hop; a.h = join ? join_design(join->fade_ms) : 0;
    a.g0 = g0 * hop; a.g1 = g1 * hop; a.k0 = a.g0; a.k1 = a.g1;
    // (the outputs start out as NaN / 0x7FFF: a sample the kernel leaves out shows)
    ok = ok && hipMemcpyAsync(d + xb, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemsetAsync(d + xb + tb, 0xFF, yb, st) == hipSuccess &&
         hipMemsetD16Async((hipDeviceptr_t)(d + xb + tb + yb), 0x7FFF, pb / 2, st) == hipSuccess;
    if (ok) {
        join_window_run(a, st);
        ok = hipGetLastError() == hipSuccess &&
             (!y || hipMemcpyAsync(y, d + xb + tb, (size_t)NY * 4, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             (!pcm || hipMemcpyAsync(pcm, d + xb + tb + yb, (size_t)NY * 2, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipStreamSynchronize(st) == hipSuccess;
    } else if (st) (void)hipStreamSynchronize(st);
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "the join failed on the device");
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

int sts_debug_spline_step(int device, const float* h, int64_t n, float filter_sqrt, const float* r0, const float* r1, float* o0, float* o1) {
    if (!h || !o0 || !o1 || n < 1 || n > (1 << 24) || !(filter_sqrt > 0.f)) return set_err(STS_EINVAL, "h [29][n], 1 <= n <= 2^24, filter_sqrt > 0 and both outputs are required");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    // each output row is followed by a guard that reaches past the last 128-thread block of the launch; it must come back untouched
    const size_t guard = (size_t)((n + 127) / 128 * 128 - n) + 128;
    const size_t hb = pad((size_t)29 * n * 4), rb = pad((size_t)n * 4), ob = pad(((size_t)n + guard) * 4);
    char* d = nullptr;          // [h | r0 | r1 | o0 + guard | o1 + guard]
    if (hipMalloc((void**)&d, hb + 2 * rb + 2 * ob) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    float *d0 = (float*)(d + hb + 2 * rb), *d1 = (float*)(d + hb + 2 * rb + ob);
    std::vector<uint32_t> back0((size_t)n + guard), back1((size_t)n + guard);
    ok = ok && hipMemcpyAsync(d, h, (size_t)29 * n * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         (!r0 || hipMemcpyAsync(d + hb, r0, (size_t)n * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         (!r1 || hipMemcpyAsync(d + hb + rb, r1, (size_t)n * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemsetAsync(d0, 0xFF, 2 * ob, st) == hipSuccess;
    if (ok) {
        spline_step((const float*)d, (long)n, filter_sqrt, r0 ? (const float*)(d + hb) : nullptr, r1 ? (const float*)(d + hb + rb) : nullptr, d0, d1, (long)n, st);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(back0.data(), d0, back0.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipMemcpyAsync(back1.data(), d1, back1.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    if (!ok) return set_err(STS_EDEVICE, "the spline step failed on the device");
    for (size_t i = (size_t)n; i < back0.size(); i++)
        if (back0[i] != 0xFFFFFFFFu || back1[i] != 0xFFFFFFFFu) return set_err(STS_EDEVICE, "the spline step wrote past n");
    memcpy(o0, back0.data(), (size_t)n * 4);
    memcpy(o1, back1.data(), (size_t)n * 4);
    return STS_OK;
}

namespace {
// Exact-size device buffers of the kernel-level text-encoder entries: one allocation per tensor, freed on every return path.
struct DebugBufs {
    std::vector<void*> ptrs; hipStream_t st = nullptr; bool ok = true;
    DebugBufs() { ok = hipStreamCreate(&st) == hipSuccess; }
    ~DebugBufs() { if (st) (void)hipStreamDestroy(st); for (void* p : ptrs) (void)hipFree(p); }
    void* raw(size_t bytes) {
        void* d = nullptr;
        if (ok && hipMalloc(&d, bytes ? bytes : 4) == hipSuccess) { ptrs.push_back(d); return d; }
        ok = false; return nullptr;
    }
    const void* up4(const void* host, size_t words) {                   // null stays null
        if (!host) return nullptr;
        void* d = raw(words * 4);
        ok = ok && hipMemcpyAsync(d, host, words * 4, hipMemcpyHostToDevice, st) == hipSuccess;
        return d;
    }
    const float* up(const float* host, size_t count) { return (const float*)up4(host, count); }
    const int* up(const int* host, size_t count) { return (const int*)up4(host, count); }
    float* out(size_t count) {                                          // starts out as the sentinel 0xFFFFFFFF (a NaN)
        float* d = (float*)raw(count * 4);
        ok = ok && hipMemsetAsync(d, 0xFF, count * 4, st) == hipSuccess;
        return d;
    }
};
// lengths[B] -> device table [offsets | lengths]; returns L = sum(lengths) or -1
long debug_segments(const int32_t* lengths, int32_t B, std::vector<int>& tab, int* max_len) {
    if (!lengths || B < 1 || B > 65535) return -1;
    tab.assign(2 * (size_t)B, 0);
    long L = 0; *max_len = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 1 || L + lengths[b] > (1 << 24)) return -1;
        tab[b] = (int)L; tab[B + b] = lengths[b]; L += lengths[b];
        if (lengths[b] > *max_len) *max_len = lengths[b];
    }
    return L;
}
}  // namespace

int sts_debug_attention(int device, const float* q, const float* k, const float* v, const float* relk, const float* relv, int32_t nheads,
                        int32_t kc, int32_t win, const int32_t* lengths, int32_t B, int variant, float* o, int32_t o_rows,
                        int32_t* variant_out, int32_t* jpl_out) {
    if (variant_out) *variant_out = 0;
    if (jpl_out) *jpl_out = 0;
    if (!q || !k || !v || !o) return set_err(STS_EINVAL, "q, k, v and o are required");
    if (nheads < 1 || nheads > 65535 || kc < 1 || kc > 4096 || win < 0 || win > 4096) return set_err(STS_EINVAL, "1 <= nheads <= 65535, 1 <= kc <= 4096, 0 <= win <= 4096");
    if ((win > 0) != (relk != nullptr) || (win > 0) != (relv != nullptr)) return set_err(STS_EINVAL, "relk and relv [kc][2 win + 1] go with win > 0, null with win = 0");
    if (variant < 0 || variant > 3) return set_err(STS_EINVAL, "variant: 0 = the engine's choice, 1 = generic, 2 = register, 3 = matrix-core");
    const long rows = (long)nheads * kc;
    if (o_rows < rows) return set_err(STS_EINVAL, "o holds at least nheads * kc rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || (double)o_rows * (double)L > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= 2^24, o_rows * sum <= 2^30");
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.kc = kc; a.win = win; a.px = win > 0 ? 2 * win + 1 : 0; a.nheads = nheads; a.B = B; a.max_len = max_len; a.ld = L;
    a.block_min_wgs = 0; a.attn_reg = 1;            // the engine's defaults (engine.hpp)
    AttnPlan plan;
    if (variant == 0) plan = attention_choose(a);
    else attention_admits(a, variant, &plan);
    if (plan.kernel == ATTN_NONE) return set_err(STS_EINVAL, variant == 0 ? "no attention kernel admits this shape (utterance too long for the attention kernel)" : "the shape is outside the forced kernel's limits");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DebugBufs d;
    a.q = d.up(q, (size_t)rows * L); a.k = d.up(k, (size_t)rows * L); a.v = d.up(v, (size_t)rows * L);
    a.relk = d.up(relk, (size_t)kc * a.px); a.relv = d.up(relv, (size_t)kc * a.px);
    const int* dt = d.up(tab.data(), tab.size());
    a.o = d.out((size_t)o_rows * L);
    a.seg = SegView{dt, dt + B, 1, 0, 0, 0};
    if (d.ok) {
        attention_launch(a, plan, d.st);
        d.ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(o, a.o, (size_t)o_rows * L * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess &&
               hipStreamSynchronize(d.st) == hipSuccess;
    }
    if (!d.ok) return set_err(STS_EDEVICE, "the attention launch failed on the device");
    if (variant_out) *variant_out = plan.kernel;
    if (jpl_out) *jpl_out = plan.jpl;
    return STS_OK;
}

int sts_debug_layer_norm(int device, const float* a, const float* b, int32_t nb, int64_t b_stride, const float* res, const float* gamma,
                         const float* beta, int32_t C, int32_t pre_relu, int32_t post_gelu, const float* dw_w, const float* dw_b, int32_t dw_k,
                         int32_t dw_dil, int32_t dw_pad, const int32_t* lengths, int32_t B, float* y, int32_t y_rows) {
    if (!a || !gamma || !beta || !y) return set_err(STS_EINVAL, "a, gamma, beta and y are required");
    if (C < 1 || C > 65536 || y_rows < C) return set_err(STS_EINVAL, "1 <= C <= 65536 and y holds at least C rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || (double)y_rows * (double)L > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= 2^24, y_rows * sum <= 2^30");
    if (nb < 0 || nb > 8 || (nb > 0) != (b != nullptr)) return set_err(STS_EINVAL, "0 <= nb <= 8 partials in b (null with nb = 0)");
    if (nb > 1 && b_stride < (int64_t)C * L) return set_err(STS_EINVAL, "b_stride >= C * L floats between partials");
    if (dw_w && (dw_k < 1 || dw_k > 64 || dw_dil < 1 || dw_dil > 4096 || dw_pad < 0 || dw_pad > (1 << 20))) return set_err(STS_EINVAL, "depthwise conv: 1 <= k <= 64, 1 <= dil <= 4096, 0 <= pad <= 2^20");
    if (!dw_w && dw_b) return set_err(STS_EINVAL, "dw_b goes with dw_w");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    DebugBufs d;
    LnArgs g;
    memset(&g, 0, sizeof(g));
    const size_t n = (size_t)C * L;
    g.a = d.up(a, n); g.a_ld = L;
    g.nb = nb; g.b_stride = nb > 1 ? (long)b_stride : 0; g.b_ld = L;
    g.b = d.up(b, nb > 1 ? (size_t)(nb - 1) * (size_t)b_stride + n : n);
    g.res = d.up(res, n); g.res_ld = L;
    g.gamma = d.up(gamma, (size_t)C); g.beta = d.up(beta, (size_t)C);
    g.C = C; g.pre_relu = pre_relu != 0; g.post_gelu = post_gelu != 0;
    if (dw_w) { g.dw_w = d.up(dw_w, (size_t)dw_k * C); g.dw_b = d.up(dw_b, (size_t)C); g.dw_k = dw_k; g.dw_dil = dw_dil; g.dw_pad = dw_pad; g.dw_ld = C; }
    const int* dt = d.up(tab.data(), tab.size());
    g.y = d.out((size_t)y_rows * L); g.y_ld = L;
    g.seg = SegView{dt, dt + B, 1, 0, 0, 0}; g.B = B; g.max_len = max_len;
    if (d.ok) {
        layer_norm(g, d.st);
        d.ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(y, g.y, (size_t)y_rows * L * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess &&
               hipStreamSynchronize(d.st) == hipSuccess;
    }
    return d.ok ? STS_OK : set_err(STS_EDEVICE, "the LayerNorm launch failed on the device");
}

int sts_debug_resblock_layer(int device, const float* x, int32_t C, const int32_t* lengths, int32_t B, int64_t ld, int32_t n,
                             const float* const* w1, const float* const* b1, const int32_t* k1, const int32_t* dil1,
                             const float* const* w2, const float* const* b2, const int32_t* k2, float slope, int kind, int variant,
                             float* y, int32_t y_rows, uint32_t* ovf) {
    if (ovf) *ovf = 0;
    if (!x || !w1 || !k1 || !dil1 || !w2 || !k2 || !y) return set_err(STS_EINVAL, "x, y and the members' w1, k1, dil1, w2, k2 tables are required");
    if (kind < 1 || kind > 4) return set_err(STS_EINVAL, "kind: 1 = resblock_layer, 2 = resblock_wino, 3 = resblock_bf3 (bf16x3), 4 = resblock_bf3 (f16x2)");
    if (variant < -1 || variant > 1) return set_err(STS_EINVAL, "variant: -1 = automatic, 0 or 1");
    if (n < 1 || n > kMaxGroup) return set_err(STS_EINVAL, "1 <= n <= 4 members");
    if (C < 1 || C > 1024 || y_rows < C) return set_err(STS_EINVAL, "1 <= C <= 1024 and every y holds at least C rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || ld < L || (double)y_rows * (double)ld * n > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= ld, n * y_rows * ld <= 2^30");
    for (int j = 0; j < n; j++)
        if (!w1[j] || !w2[j] || k1[j] < 1 || k1[j] > 255 || k2[j] < 1 || k2[j] > 255 || dil1[j] < 1 || dil1[j] > 4096)
            return set_err(STS_EINVAL, "every member: w1, w2, 1 <= k1, k2 <= 255, 1 <= dil1 <= 4096");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    // the weights as the blob carries a ResBlock layer's convs, through the loader's packers
    HConv c1[kMaxGroup], c2[kMaxGroup];
    for (int j = 0; j < n; j++) {
        c1[j].out_ch = c1[j].in_ch = C; c1[j].k = k1[j]; c1[j].dil = dil1[j]; c1[j].pad = dil1[j] * (k1[j] - 1) / 2;
        c1[j].w = w1[j]; c1[j].b = b1 ? b1[j] : nullptr; c1[j].has_bias = c1[j].b ? 1 : 0;
        c2[j].out_ch = c2[j].in_ch = C; c2[j].k = k2[j]; c2[j].dil = 1; c2[j].pad = (k2[j] - 1) / 2;
        c2[j].w = w2[j]; c2[j].b = b2 ? b2[j] : nullptr; c2[j].has_bias = c2[j].b ? 1 : 0;
    }
    Model m;
    struct Freed { Model& m; ~Freed() { (void)hipDeviceSynchronize(); free_model(m); } } freed{m};     // (runs after the buffers' and the stream's release)
    if (!load_resblock_layer(c1, c2, n, m)) return set_err(STS_EDEVICE, "packing the layer's weights failed: " + m.error);
    DebugBufs d;
    const size_t yn = (size_t)y_rows * (size_t)ld;
    const float* dx = d.up(x, (size_t)C * (size_t)ld);
    const int* dt = d.up(tab.data(), tab.size());
    unsigned* dovf = (unsigned*)d.raw(4);
    d.ok = d.ok && hipMemsetAsync(dovf, 0, 4, d.st) == hipSuccess;
    float* dy[kMaxGroup] = {};
    for (int j = 0; j < n; j++) dy[j] = d.out(yn);
    if (!d.ok) return set_err(STS_EDEVICE, "device buffers of the layer");
    // the group as Engine::ResStage::fill_fused fills it: every member reads the same x and writes its own y
    ResLayerGroup R;
    memset(&R, 0, sizeof(R));
    R.n = n; R.C = C; R.ld = (long)ld; R.slope = slope; R.seg = SegView{dt, dt + B, 1, 0, 0, 0}; R.B = B; R.max_n = max_len;
    for (int j = 0; j < n; j++) {
        if (fill_res_member(m.rb[j].c1[0], m.rb[j].c2[0], dx, dy[j], kind == 4, R.g[j])) { R.math = 1; R.ovf = dovf; }
        else if (kind == 4) return set_err(STS_EINVAL, "shape has no two-term fp16 copy of its weights");
    }
    const bool eligible = kind == 1 ? resblock_layer_eligible(R) : kind == 2 ? resblock_wino_eligible(R) : resblock_bf3_eligible(R);
    if (!eligible) return set_err(STS_EINVAL, kind == 1 ? "shape not eligible for resblock_layer" : kind == 2 ? "shape not eligible for resblock_wino" : "shape not eligible for resblock_bf3");
    if (kind == 1) resblock_layer(R, d.st);
    else if (kind == 2) resblock_wino(R, d.st);
    else resblock_bf3(R, d.st, variant);
    d.ok = hipGetLastError() == hipSuccess;
    for (int j = 0; j < n && d.ok; j++) d.ok = hipMemcpyAsync(y + (size_t)j * yn, dy[j], yn * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess;
    uint32_t word = 0;
    d.ok = d.ok && hipMemcpyAsync(&word, dovf, 4, hipMemcpyDeviceToHost, d.st) == hipSuccess && hipStreamSynchronize(d.st) == hipSuccess;
    if (!d.ok) return set_err(STS_EDEVICE, "the ResBlock layer launch failed on the device");
    if (ovf) *ovf = word;
    return STS_OK;
}

int sts_debug_col_layer(int device, const float* x, int32_t C, const int32_t* lengths, int32_t B, int64_t ld, const float* xs_w,
                        const float* xs_b, const float* xr, const float* dw_w, const float* dw_b, int32_t dw_k, int32_t dw_dil, int32_t dw_pad,
                        const float* g1, const float* b1, const float* w, const float* bias, const float* add, const float* g2,
                        const float* b2, int32_t post_gelu, int32_t use_res, const float* tp_w, const float* tp_b, float tp_fs,
                        const float* tp_r0, const float* tp_r1, int32_t alias, float* y, int32_t y_rows, float* o0, float* o1) {
    if (!x || !w || !g2 || !b2 || !y) return set_err(STS_EINVAL, "x, w, g2, b2 and y are required");
    if (C < 1 || C > 4096 || y_rows < C) return set_err(STS_EINVAL, "1 <= C <= 4096 and y holds at least C rows");
    std::vector<int> tab; int max_len = 0;
    const long L = debug_segments(lengths, B, tab, &max_len);
    if (L < 0 || ld < L || (double)y_rows * (double)ld > (double)(1u << 30)) return set_err(STS_EINVAL, "lengths: B >= 1 entries, each >= 1, sum <= ld, y_rows * ld <= 2^30");
    if (dw_w && (dw_k < 1 || dw_k > 64 || dw_dil < 1 || dw_dil > 4096 || dw_pad < 0 || dw_pad > (1 << 20))) return set_err(STS_EINVAL, "depthwise conv: 1 <= k <= 64, 1 <= dil <= 4096, 0 <= pad <= 2^20");
    if (!dw_w && dw_b) return set_err(STS_EINVAL, "dw_b goes with dw_w");
    if (!xs_w && (xs_b || xr)) return set_err(STS_EINVAL, "xs_b and xr go with xs_w");
    if (tp_w ? (!o0 || !o1 || !(tp_fs > 0.f)) : (tp_b != nullptr)) return set_err(STS_EINVAL, "a tail needs o0, o1 and tp_fs > 0; tp_b goes with tp_w");
    if (alias < 0 || alias > 5 || (alias >= 2 && !tp_w) || ((alias == 2 || alias == 5) && !tp_r0) || ((alias == 3 || alias == 4) && !tp_r1))
        return set_err(STS_EINVAL, "alias: 0 none, 1 y = x, 2 o0 = r0, 3 o0 = r1, 4 o1 = r1, 5 o1 = r0 (2 - 5: a tail with that latent half)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    // the weights as the blob carries a ConvFlow's convs ([out][k][in]), through the loader's packers
    std::vector<float> dwt;
    HConv pre, sep, pw, proj; HLn n1, n2;
    pre.out_ch = C; pre.in_ch = 1; pre.k = 1; pre.w = xs_w; pre.b = xs_b; pre.has_bias = xs_b ? 1 : 0;
    if (dw_w) {
        dwt.resize((size_t)C * dw_k);
        for (int c = 0; c < C; c++) for (int j = 0; j < dw_k; j++) dwt[(size_t)c * dw_k + j] = dw_w[(size_t)j * C + c];
        sep.out_ch = C; sep.in_ch = 1; sep.k = dw_k; sep.dil = dw_dil; sep.pad = dw_pad; sep.w = dwt.data(); sep.b = dw_b; sep.has_bias = dw_b ? 1 : 0;
    }
    pw.out_ch = pw.in_ch = C; pw.k = 1; pw.w = w; pw.b = bias; pw.has_bias = bias ? 1 : 0;
    proj.out_ch = 29; proj.in_ch = C; proj.k = 1; proj.w = tp_w; proj.b = tp_b; proj.has_bias = tp_b ? 1 : 0;
    n1.size = C; n1.g = g1; n1.b = b1;
    n2.size = C; n2.g = g2; n2.b = b2;
    Model m;
    struct Freed { Model& m; ~Freed() { (void)hipDeviceSynchronize(); free_model(m); } } freed{m};     // (runs after the buffers' and the stream's release)
    if (!load_col_layer(xs_w ? &pre : nullptr, dw_w ? &sep : nullptr, (g1 && b1) ? &n1 : nullptr, pw, n2, tp_w ? &proj : nullptr, m))
        return set_err(STS_EDEVICE, "packing the layer's weights failed: " + m.error);
    const DConvFlow& cf = m.cf[0];
    DebugBufs d;
    const size_t xn = (size_t)C * (size_t)ld, yn = (size_t)y_rows * (size_t)ld;
    const float* dx = d.up(x, xn);
    const float* dadd = d.up(add, xn);
    const float* dxr = d.up(xr, (size_t)ld);
    const float* dr0 = d.up(tp_r0, (size_t)ld);
    const float* dr1 = d.up(tp_r1, (size_t)ld);
    const int* dt = d.up(tab.data(), tab.size());
    float* dy = d.out(yn);
    float* do0 = tp_w ? d.out((size_t)ld) : nullptr;
    float* do1 = tp_w ? d.out((size_t)ld) : nullptr;
    if (!d.ok) return set_err(STS_EDEVICE, "device buffers of the layer");
    Lvl lv;
    lv.seg = SegView{dt, dt + B, 1, 0, 0, 0}; lv.nb = B; lv.max_len = max_len; lv.total = L; lv.ld = (long)ld;
    // the kernarg block as the engine fills it; what the engine fixes per form and the entry leaves to the caller follows
    ColLayerArgs g;
    float* ydst = alias == 1 ? const_cast<float*>(dx) : dy;
    if (dw_w) fill_col_dds(cf.dds.sep[0], cf.dds.n1[0], cf.dds.pw[0], cf.dds.n2[0], dx, ydst, lv, g);
    else fill_col_oproj(cf.dds.pw[0], cf.dds.n2[0], dx, dadd, ydst, lv, g);
    g.C = C; g.add = dadd; g.add_ld = (long)ld; g.post_gelu = post_gelu != 0;
    g.res = use_res ? dx : nullptr; g.res_ld = (long)ld;
    if (xs_w) { fill_col_pre(cf.pre, dxr, dx, g); if (!use_res) g.res = nullptr; }
    if (tp_w)
        fill_col_tail(cf.proj, tp_fs, dr0, dr1, alias == 2 ? const_cast<float*>(dr0) : alias == 3 ? const_cast<float*>(dr1) : do0,
                      alias == 4 ? const_cast<float*>(dr1) : alias == 5 ? const_cast<float*>(dr0) : do1, g);
    if (!col_layer_eligible(g)) return set_err(STS_EINVAL, "shape not eligible for col_layer");
    col_layer(g, d.st);
    d.ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(y, dy, yn * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess &&
           (!tp_w || (hipMemcpyAsync(o0, g.tp_o0, (size_t)ld * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess &&
                      hipMemcpyAsync(o1, g.tp_o1, (size_t)ld * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess)) &&
           hipStreamSynchronize(d.st) == hipSuccess;
    return d.ok ? STS_OK : set_err(STS_EDEVICE, "the column-block layer launch failed on the device");
}

int sts_debug_adopt_z(int device, const float* src, int32_t C, int64_t ld_src, float* dst, int64_t ld_dst, const int64_t* src_off,
                      const int64_t* dst_off, const int32_t* len, int32_t B) {
    if (!src || !dst || !src_off || !dst_off || !len || B < 1 || B > 65535 || C < 1 || ld_src < 1 || ld_dst < 1 ||
        (double)C * (double)ld_src > (double)(1 << 28) || (double)C * (double)ld_dst > (double)(1 << 28))
        return set_err(STS_EINVAL, "src [C][ld_src], dst [C][ld_dst] (at most 2^28 floats each), the three tables and 1 <= B <= 65535 are required");
    std::vector<std::pair<int64_t, int64_t>> ranges;
    int max_len = 0;
    for (int b = 0; b < B; b++) {
        if (len[b] < 0 || src_off[b] < 0 || dst_off[b] < 0 || src_off[b] + len[b] > ld_src || dst_off[b] + len[b] > ld_dst)
            return set_err(STS_EINVAL, "a segment leaves its matrix");
        if (len[b] > 0) ranges.emplace_back(dst_off[b], dst_off[b] + len[b]);
        max_len = std::max(max_len, (int)len[b]);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++) if (ranges[i].first < ranges[i - 1].second) return set_err(STS_EINVAL, "destination ranges overlap");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    std::vector<long long> tab(((size_t)B * 20 + 7) / 8);       // long long src_off[B] | long long dst_off[B] | int len[B] (kernels.hpp adopt_z)
    for (int b = 0; b < B; b++) { tab[(size_t)b] = src_off[b]; tab[(size_t)B + b] = dst_off[b]; ((int*)(tab.data() + 2 * (size_t)B))[b] = len[b]; }
    DebugBufs d;
    const float* ds = d.up(src, (size_t)C * ld_src);
    float* dd = (float*)d.up4(dst, (size_t)C * ld_dst);
    const long long* dt = (const long long*)d.up4(tab.data(), tab.size() * 2);
    if (d.ok) {
        adopt_z(ds, ld_src, dd, ld_dst, C, dt, B, max_len, d.st);
        d.ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(dst, dd, (size_t)C * ld_dst * 4, hipMemcpyDeviceToHost, d.st) == hipSuccess &&
               hipStreamSynchronize(d.st) == hipSuccess;
    }
    return d.ok ? STS_OK : set_err(STS_EDEVICE, "the adoption launch failed on the device");
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
        case STS_DBG_STREAM_RETRY_STEP: e->eng.stream_retry_step = value < 0 ? -1 : value; return STS_OK;
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
int sts_loudness_measure(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float target_lufs, float peak_dbfs,
                         sts_loudness* out) {
    if (B < 1 || !lengths || !out) return set_err(STS_EINVAL, "B >= 1, lengths and out are required");
    if (!loudness_args_valid(2, target_lufs, peak_dbfs)) return set_err(STS_EINVAL, "target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS");
    LoudArgs a{};
    if (!loud_coef(rate, &a.k)) return set_err(STS_EINVAL, "rate must be an integer in [8000, 48000]");
    std::vector<int> len(B);
    int64_t total = 0, maxl = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 0 || lengths[b] > (int64_t)1 << 30) return set_err(STS_EINVAL, "lengths must be in [0, 2^30]");
        len[b] = (int)lengths[b]; total += lengths[b]; maxl = std::max<int64_t>(maxl, lengths[b]);
    }
    if (total > 0 && !x) return set_err(STS_EINVAL, "null signal");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    const size_t ws = loud_ws_bytes(B, total), xb = (((size_t)total * 4 + 255) & ~(size_t)255), lb = (((size_t)B * 4 + 255) & ~(size_t)255);
    const size_t ob = (size_t)B * sizeof(sts_loudness);
    char* d = nullptr;
    if (hipMalloc((void**)&d, xb + lb + ob + ws) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    a.x = (const float*)d; a.len = (const int*)(d + xb); a.ilen = 0; a.scale = 1; a.P = 1; a.Q = 1;
    a.target = target_lufs; a.ceiling = peak_dbfs;
    a.out = (float*)(d + xb + lb);
    loud_ws_carve(a, d + xb + lb + ob, B, total);
    ok = ok && (total == 0 || hipMemcpyAsync(d, x, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemcpyAsync(d + xb, len.data(), (size_t)B * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        loudness_run(a, B, maxl, nullptr, st);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(out, a.out, ob, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "loudness measurement failed on the device");
}
int sts_set_loudness_streaming(sts_engine* e, int enable) {
    if (!e) return set_err(STS_EINVAL, "null engine");
    STS_CAPI_NOT_WHILE_OPEN(e);
    e->eng.loud_streaming = enable != 0;
    return STS_OK;
}
int sts_get_loudness_streaming(const sts_engine* e) { return e && e->eng.loud_streaming ? 1 : 0; }
int sts_loudness_measure_chunked(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float target_lufs, float peak_dbfs,
                                 const int64_t* bounds, int32_t n_steps, int32_t back, sts_loudness* out, sts_loudness* partial) {
    if (B < 1 || !lengths || !out) return set_err(STS_EINVAL, "B >= 1, lengths and out are required");
    if (!loudness_args_valid(2, target_lufs, peak_dbfs)) return set_err(STS_EINVAL, "target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS");
    LoudStreamArgs a{};
    if (!loud_coef(rate, &a.k)) return set_err(STS_EINVAL, "rate must be an integer in [8000, 48000]");
    if (n_steps < 1 || !bounds || bounds[0] != 0) return set_err(STS_EINVAL, "loudness stream: at least one step boundary, the first one 0");
    for (int k = 1; k < n_steps; k++)
        if (bounds[k] <= bounds[k - 1]) return set_err(STS_EINVAL, "loudness stream: the step boundaries must ascend");
    if (back < 0 || back > 2048) return set_err(STS_EINVAL, "loudness stream: the overlap must be in [0, 2048]");
    std::vector<int64_t> off(B + 1, 0);
    std::vector<long long> lenv(B);
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 0 || lengths[b] > (int64_t)1 << 30) return set_err(STS_EINVAL, "lengths must be in [0, 2^30]");
        off[b + 1] = off[b] + lengths[b]; lenv[b] = lengths[b];
    }
    const int64_t total = off[B];
    if (total > (int64_t)1 << 30) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
    if (total > 0 && !x) return set_err(STS_EINVAL, "null signal");
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
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t xb = pad((size_t)total * 4), rb = pad(rows.size() * sizeof(LdsRow)), ub = pad(utab.size() * 8);
    const size_t sb = pad(lds_state_bytes(B)), wb = pad(ws), tsb = pad((size_t)tiles_all * kLdsSlots * 8), tpb = pad((size_t)tiles_all * 4);
    const size_t ob = pad((size_t)(n_steps + 1) * B * sizeof(sts_loudness)), gb = pad((size_t)B * 4);
    char* d = nullptr;          // [x | rows | gate tables | results | gains | state | workspace | tile sums | tile peaks]
    if (hipMalloc((void**)&d, xb + rb + ub + ob + gb + sb + wb + tsb + tpb + 256) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    char* dr = d + xb; char* du = dr + rb; char* dout = du + ub; char* dg = dout + ob; char* ds = dg + gb; char* dw = ds + sb;
    char* dts = dw + wb; char* dtp = dts + tsb;
    // (results, state, workspace and tables start out as NaN: a word the kernels leave out, or a stale one they read, shows)
    ok = ok && (total == 0 || hipMemcpyAsync(d, x, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         (rows.empty() || hipMemcpyAsync(dr, rows.data(), rows.size() * sizeof(LdsRow), hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemcpyAsync(du, utab.data(), utab.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemsetAsync(dout, 0xFF, ob + gb + sb + wb + tsb + tpb, st) == hipSuccess;
    if (ok) {
        a.x = (const float*)d; a.state = ds; a.E = (double*)dw; a.tsum = (double*)dts; a.tpeak = (float*)dtp;
        LoudArgs g{};
        g.k = a.k; g.target = target_lufs; g.ceiling = peak_dbfs; g.tsum = a.tsum; g.tpeak = a.tpeak; g.gain = (float*)dg;
        int slot = 0;
        for (int k = 0; k < n_steps; k++) {
            const int nw = row0[k + 1] - row0[k];
            if (nw > 0) {
                a.wtab = (const long long*)(dr + (size_t)row0[k] * sizeof(LdsRow)); a.slot = slot;
                loud_stream_run(a, nw, tiles[k], st);
                slot ^= 1;
            }
            if (partial) {      // the result as if the call had stopped behind this step
                g.utab = (long long*)du + (size_t)k * B * 3; g.out = (float*)dout + (size_t)k * B * 4;
                loud_gate_run(g, B, st);
            }
        }
        g.utab = (long long*)du + (size_t)n_steps * B * 3; g.out = (float*)dout + (size_t)n_steps * B * 4;
        loud_gate_run(g, B, st);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(out, g.out, (size_t)B * sizeof(sts_loudness), hipMemcpyDeviceToHost, st) == hipSuccess &&
             (!partial || hipMemcpyAsync(partial, dout, (size_t)n_steps * B * sizeof(sts_loudness), hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "loudness measurement failed on the device");
}
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
int sts_limiter_apply(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float gain_db, float ceiling_dbfs,
                      float lookahead_ms, float* y, int16_t* pcm, sts_limiter_stats* stats) {
    if (B < 1 || !lengths) return set_err(STS_EINVAL, "B >= 1 and lengths are required");
    LimiterDesign dsg;
    if (!limiter_design(rate, gain_db, ceiling_dbfs, lookahead_ms, &dsg))
        return set_err(STS_EINVAL, "rate in [8000, 48000], gain in [-40, 40] dB, ceiling in [-30, 0] dBFS, look-ahead in [0.25, 10] ms");
    std::vector<int> len(B);
    int64_t total = 0, maxl = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 0 || lengths[b] > (int64_t)1 << 30) return set_err(STS_EINVAL, "lengths must be in [0, 2^30]");
        len[b] = (int)lengths[b]; total += lengths[b]; maxl = std::max<int64_t>(maxl, lengths[b]);
    }
    if (total > (int64_t)1 << 30) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
    if (total > 0 && !x) return set_err(STS_EINVAL, "null signal");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    const size_t xb = (((size_t)total * 4 + 255) & ~(size_t)255), lb = (((size_t)B * 4 + 255) & ~(size_t)255);
    const size_t pb = (((size_t)total * 2 + 255) & ~(size_t)255), sb = (((size_t)B * 16 + 255) & ~(size_t)255);
    char* d = nullptr;
    if (hipMalloc((void**)&d, 2 * xb + lb + pb + sb + 256) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    LimArgs a{};
    a.x = (const float*)d; a.len = (const int*)(d + xb); a.ilen = 0; a.scale = 1; a.P = 1; a.Q = 1;
    a.H = dsg.H; a.c = dsg.c; a.G = dsg.G; a.gloud = nullptr;
    a.y = y ? (float*)(d + xb + lb) : nullptr;
    a.pcm = pcm ? (int16_t*)(d + 2 * xb + lb) : nullptr;
    a.stat = (unsigned*)(d + 2 * xb + lb + pb);
    std::vector<unsigned> raw((size_t)B * 4);
    ok = ok && (total == 0 || hipMemcpyAsync(d, x, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemcpyAsync(d + xb, len.data(), (size_t)B * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        limiter_run(a, B, maxl, st);
        ok = hipGetLastError() == hipSuccess &&
             (!y || total == 0 || hipMemcpyAsync(y, a.y, (size_t)total * 4, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             (!pcm || total == 0 || hipMemcpyAsync(pcm, a.pcm, (size_t)total * 2, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipMemcpyAsync(raw.data(), a.stat, (size_t)B * 16, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    if (!ok) return set_err(STS_EDEVICE, "the limiter failed on the device");
    if (stats) limiter_stats_decode(raw.data(), B, stats);
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
int sts_eq_apply(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, int32_t n_bands, const sts_eq_band* bands,
                 float* y, int16_t* pcm) {
    if (B < 1 || !lengths) return set_err(STS_EINVAL, "B >= 1 and lengths are required");
    const char* why = nullptr;
    if (!eq_valid(rate, n_bands, bands, &why)) return set_err(STS_EINVAL, why);
    if (n_bands < 1) return set_err(STS_EINVAL, "eq: at least one band to apply");
    std::vector<int> len(B);
    int64_t total = 0, maxl = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 0 || lengths[b] > (int64_t)1 << 30) return set_err(STS_EINVAL, "lengths must be in [0, 2^30]");
        len[b] = (int)lengths[b]; total += lengths[b]; maxl = std::max<int64_t>(maxl, lengths[b]);
    }
    if (total > (int64_t)1 << 30) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
    if (total > 0 && !x) return set_err(STS_EINVAL, "null signal");
    double coef[5 * STS_EQ_MAX_BANDS];
    eq_design(rate, n_bands, bands, coef);
    EqTable tab;
    eq_table(n_bands, coef, &tab);
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "no such device");
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t xb = pad((size_t)total * 4), lb = pad((size_t)B * 4), pb = pad((size_t)total * 2), tb = pad(sizeof(EqTable));
    const size_t wb = pad(eq_ws_bytes(B, total));
    char* d = nullptr;          // [x | lengths | tables | y | pcm | workspace]
    if (hipMalloc((void**)&d, 2 * xb + lb + tb + pb + wb + 256) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    EqArgs a{};
    a.x = (const float*)d; a.len = (const int*)(d + xb); a.ilen = 0; a.scale = 1; a.P = 1; a.Q = 1;
    a.S = n_bands; a.tab = (const EqTable*)(d + xb + lb);
    char* dy = d + xb + lb + tb; char* dp = dy + xb;
    a.y = y ? (float*)dy : nullptr; a.pcm = pcm ? (int16_t*)dp : nullptr;
    eq_ws_carve(a, dp + pb, B, total);
    // (the outputs start out as NaN / 0x7FFF: a sample the kernels leave out shows)
    ok = ok && (total == 0 || hipMemcpyAsync(d, x, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemcpyAsync(d + xb, len.data(), (size_t)B * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d + xb + lb, &tab, sizeof(EqTable), hipMemcpyHostToDevice, st) == hipSuccess &&
         (xb == 0 || hipMemsetAsync(dy, 0xFF, xb, st) == hipSuccess) &&
         (pb == 0 || hipMemsetD16Async((hipDeviceptr_t)dp, 0x7FFF, pb / 2, st) == hipSuccess);
    if (ok) {
        eq_run(a, B, maxl, st);
        ok = hipGetLastError() == hipSuccess &&
             (!y || total == 0 || hipMemcpyAsync(y, dy, (size_t)total * 4, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             (!pcm || total == 0 || hipMemcpyAsync(pcm, dp, (size_t)total * 2, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "the equaliser failed on the device");
}
int sts_eq_apply_chunked(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, int32_t n_bands, const sts_eq_band* bands,
                         const int64_t* bounds, int32_t n_steps, int32_t back, float* y, int16_t* pcm, float* win_y, int64_t win_capacity,
                         int64_t* win_off) {
    if (B < 1 || !lengths) return set_err(STS_EINVAL, "B >= 1 and lengths are required");
    const char* why = nullptr;
    if (!eq_valid(rate, n_bands, bands, &why)) return set_err(STS_EINVAL, why);
    if (n_bands < 1) return set_err(STS_EINVAL, "eq: at least one band to apply");
    if (n_steps < 1 || !bounds || bounds[0] != 0) return set_err(STS_EINVAL, "eq stream: at least one step boundary, the first one 0");
    for (int k = 1; k < n_steps; k++)
        if (bounds[k] <= bounds[k - 1]) return set_err(STS_EINVAL, "eq stream: the step boundaries must ascend");
    if (back < 0 || 2 * (int64_t)back > kEqsHist) return set_err(STS_EINVAL, "eq stream: the overlap must be in [0, 2048]");
    std::vector<int64_t> off(B + 1, 0);
    int64_t maxl = 0;
    for (int b = 0; b < B; b++) {
        if (lengths[b] < 0 || lengths[b] > (int64_t)1 << 30) return set_err(STS_EINVAL, "lengths must be in [0, 2^30]");
        off[b + 1] = off[b] + lengths[b]; maxl = std::max<int64_t>(maxl, lengths[b]);
    }
    const int64_t total = off[B];
    if (total > (int64_t)1 << 30) return set_err(STS_EINVAL, "the signals must hold at most 2^30 samples in all");
    if (total > 0 && !x) return set_err(STS_EINVAL, "null signal");
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
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t xb = pad((size_t)total * 4), tb = pad(sizeof(EqTable)), pb = pad((size_t)total * 2), yb = pad((size_t)wtotal * 4);
    const size_t rb = pad(rows.size() * sizeof(EqsRow)), sb = pad(eqs_state_bytes(B)), wb = pad(ws);
    char* d = nullptr;          // [x | tables | rows | window y | pcm | state | workspace]
    if (hipMalloc((void**)&d, xb + tb + rb + yb + pb + sb + wb + 256) != hipSuccess) return set_err(STS_EDEVICE, "out of device memory");
    hipStream_t st = nullptr;
    bool ok = hipStreamCreate(&st) == hipSuccess;
    char* dt = d + xb; char* dr = dt + tb; char* dy = dr + rb; char* dp = dy + yb; char* ds = dp + pb; char* dw = ds + sb;
    // (outputs, state and workspace start out as NaN / 0x7FFF: a sample the kernels leave out, or a stale word they read, shows)
    ok = ok && (total == 0 || hipMemcpyAsync(d, x, (size_t)total * 4, hipMemcpyHostToDevice, st) == hipSuccess) &&
         hipMemcpyAsync(dt, &tab, sizeof(EqTable), hipMemcpyHostToDevice, st) == hipSuccess &&
         (rows.empty() || hipMemcpyAsync(dr, rows.data(), rows.size() * sizeof(EqsRow), hipMemcpyHostToDevice, st) == hipSuccess) &&
         (yb == 0 || hipMemsetAsync(dy, 0xFF, yb, st) == hipSuccess) &&
         (pb == 0 || hipMemsetD16Async((hipDeviceptr_t)dp, 0x7FFF, pb / 2, st) == hipSuccess) &&
         hipMemsetAsync(ds, 0xFF, sb + wb, st) == hipSuccess;
    if (ok) {
        EqArgs a{};
        a.x = (const float*)d; a.S = n_bands; a.tab = (const EqTable*)dt;
        a.y = (float*)dy; a.pcm = (int16_t*)dp; a.E = (double*)dw; a.state = ds;
        int slot = 0;
        for (int k = 0; k < n_steps; k++) {
            const int nw = row0[k + 1] - row0[k];
            if (nw == 0) continue;
            a.wtab = (const long long*)(dr + (size_t)row0[k] * sizeof(EqsRow)); a.slot = slot;
            eq_stream_run(a, nw, tiles[k], st);
            slot ^= 1;
        }
        std::vector<float> hw((size_t)wtotal);
        float* wdst = win_y ? win_y : hw.data();
        ok = hipGetLastError() == hipSuccess &&
             (wtotal == 0 || hipMemcpyAsync(wdst, dy, (size_t)wtotal * 4, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             (!pcm || total == 0 || hipMemcpyAsync(pcm, dp, (size_t)total * 2, hipMemcpyDeviceToHost, st) == hipSuccess) &&
             hipStreamSynchronize(st) == hipSuccess;
        if (ok && y)            // each step's kept range out of its window
            for (const EqsRow& r : rows)
                if (r.j1 > r.j0) memcpy(y + r.pdst, wdst + r.ybase + (r.j0 - r.o0), (size_t)(r.j1 - r.j0) * 4);
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return ok ? STS_OK : set_err(STS_EDEVICE, "the equaliser failed on the device");
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

// ------------------------------------------------------------------------------------------------
// op-level entry for the parity tests: one conv on host arrays through the same kernels
int sts_debug_wino_pack(const float* w, int32_t Cout, int32_t k, int32_t Cin, float* out, int64_t out_floats) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || k < 2) return set_err(STS_EINVAL, "bad arguments");
    int n3, n2; wino_split(k, &n3, &n2);
    const int Cin_pad = (Cin + 15) / 16 * 16, Cout_pad = (Cout + 31) / 32 * 32;
    if (out_floats < (int64_t)(n3 + n2) * 4 * Cin_pad * Cout_pad) return set_err(STS_EINVAL, "output buffer too small");
    wino_pack(w, (long)k * Cin, Cin, 1, Cout, k, Cin, Cin_pad, Cout_pad, out);
    return n3 + n2;
}

static int debug_conv1d_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                             int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                             int32_t in_act, int mode, float** y_out, int32_t* Lout_out, int32_t iters, float* ms_out,
                             const int32_t* lengths, int32_t B, uint32_t* ovf_out);

int sts_debug_conv1d(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                     int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope, int32_t in_act,
                     int mode, float** y_out, int32_t* Lout_out) {
    return sts_debug_conv1d_bench(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode,
                                  y_out, Lout_out, 0, nullptr);
}

int sts_debug_conv1d_bench(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                           int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                           int32_t in_act, int mode, float** y_out, int32_t* Lout_out, int32_t iters, float* ms_out) {
    return debug_conv1d_impl(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode, y_out, Lout_out,
                             iters, ms_out, nullptr, 1, nullptr);
}

int sts_debug_conv1d_packed(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                            int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                            int32_t in_act, int mode, float** y_out, int32_t* Lout_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!lengths) return set_err(STS_EINVAL, "packed conv: null segment lengths");
    return debug_conv1d_impl(device, x, Cin, L, w, bias, Cout, k, pad, dil, stride_t, depthwise, in_slope, in_act, mode, y_out, Lout_out,
                             0, nullptr, lengths, B, ovf_out);
}

// lengths == null: one segment of L positions (the stand-alone entries); else B segments packed back to back, as the engine packs a batch
static int debug_conv1d_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout,
                             int32_t k, int32_t pad, int32_t dil, int32_t stride_t, int32_t depthwise, float in_slope,
                             int32_t in_act, int mode, float** y_out, int32_t* Lout_out, int32_t iters, float* ms_out,
                             const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!x || !w || !y_out || !Lout_out || Cin <= 0 || Cout <= 0 || L <= 0 || k <= 0) return set_err(STS_EINVAL, "bad conv arguments");
    const bool tr = stride_t > 0;
    const bool packed = lengths != nullptr;
    int maxlen = L;
    std::vector<int> tab;
    if (packed) {
        if (B <= 0 || dil < 1) return set_err(STS_EINVAL, "packed conv: B >= 1 segments and dil >= 1");
        int64_t total = 0;
        maxlen = 0;
        tab.assign((size_t)2 * B, 0);
        for (int b = 0; b < B; b++) {
            if (lengths[b] <= 0) return set_err(STS_EINVAL, "packed conv: every segment length must be positive");
            tab[b] = (int)total; tab[B + b] = lengths[b];
            total += lengths[b]; maxlen = std::max(maxlen, (int)lengths[b]);
        }
        if (total != L) return set_err(STS_EINVAL, "packed conv: L must equal the sum of the segment lengths");
        if (total * (tr ? stride_t : 1) > (int64_t)1 << 26) return set_err(STS_EINVAL, "packed conv: at most 2^26 output positions");
        // the geometries the engine launches on packed buffers: output segment = input segment (x stride)
        if (tr ? (k < stride_t || ((k - stride_t) & 1) || pad != (k - stride_t) / 2 || dil != 1) : (!(k & 1) || pad != dil * (k - 1) / 2))
            return set_err(STS_EINVAL, "packed conv: 'same' padding (odd k, pad = dil (k - 1) / 2) or a transposed conv with pad = (k - stride) / 2");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "hipSetDevice failed");
    const int Lout = tr ? (L - 1) * stride_t - 2 * pad + (k - 1) + 1 : L + 2 * pad - dil * (k - 1);
    if (Lout <= 0) return set_err(STS_EINVAL, "empty output");
    auto r_up = [](int v, int m) { return (v + m - 1) / m * m; };
    const int cin_eff = depthwise ? 1 : Cin;
    const int Cin_pad = r_up(cin_eff, 16), Cout_pad = r_up(Cout, 32);
    const int J = tr ? (k + stride_t - 1) / stride_t : 1;
    const size_t wn = depthwise ? (size_t)k * Cout_pad : (tr ? (size_t)stride_t * J : (size_t)k) * Cin_pad * Cout_pad;
    std::vector<float> wp(wn, 0.f), bp(Cout_pad, 0.f);
    if (depthwise) {
        for (int o = 0; o < Cout; o++) for (int t = 0; t < k; t++) wp[(size_t)t * Cout_pad + o] = w[(size_t)o * k + t];
    } else if (tr) {
        for (int ph = 0; ph < stride_t; ph++) for (int j = 0; j < J; j++) {
            int kk = ph + j * stride_t; if (kk >= k) continue;
            for (int ci = 0; ci < Cin; ci++) for (int o = 0; o < Cout; o++)
                wp[(((size_t)ph * J + j) * Cin_pad + ci) * Cout_pad + o] = w[((size_t)o * k + kk) * Cin + ci];
        }
    } else {
        for (int o = 0; o < Cout; o++) for (int t = 0; t < k; t++) for (int ci = 0; ci < Cin; ci++)
            wp[((size_t)t * Cin_pad + ci) * Cout_pad + o] = w[((size_t)o * k + t) * Cin + ci];
    }
    if (bias) memcpy(bp.data(), bias, sizeof(float) * Cout);
    // mode 12: the Winograd-domain kernel (weights transformed here the way load_model does it)
    std::vector<float> wu;
    int wn3 = 0, wn2 = 0;
    if (mode == 12 && !depthwise && !tr) {
        wino_split(k, &wn3, &wn2);
        wu.resize((size_t)(wn3 + wn2) * 4 * Cin_pad * Cout_pad);
        wino_pack(w, (long)k * Cin, Cin, 1, Cout, k, Cin, Cin_pad, Cout_pad, wu.data());
    }
    // mode + 100 (transposed convs of stride 2 / 4 / 8 through the split-operand kernels): the row-interleaved-phase packing (ConvArgs::rowph)
    const bool rowph = mode >= 100;
    if (rowph) {
        mode -= 100;
        if (!tr || depthwise || Cout != Cout_pad || (stride_t != 2 && stride_t != 4 && stride_t != 8)) return set_err(STS_EINVAL, "row-interleaved phases: transposed conv, stride 2 / 4 / 8, Cout % 32 == 0");
    }
    // modes 13 / 20..25 / 28..33: the split-bf16 kernel (conv_bf3.hip), automatic tile / tile code (mode - 20)
    const bool h2 = (mode == 50 || (mode >= 60 && mode < 85)) && !depthwise;       // the two-term fp16 form of the same kernel
    if (h2) mode = mode == 50 ? 13 : mode - 40;
    const bool bf3 = (mode == 13 || (mode >= 20 && mode < 45)) && !depthwise;
    std::vector<unsigned char> wb3;
    float h2_scale = 1.0f;
    if (rowph && !bf3) return set_err(STS_EINVAL, "row-interleaved phases: split-operand modes only");
    if (bf3 && rowph) {      // merged row rho = cout * stride + phase, one "phase" of J taps (as model.hip pack_bf3_rowph)
        const int rows = Cout_pad * stride_t;
        std::vector<float> wr((size_t)J * Cin_pad * rows, 0.f);
        for (int ph = 0; ph < stride_t; ph++) for (int j = 0; j < J; j++) for (int ci = 0; ci < Cin_pad; ci++) for (int o = 0; o < Cout_pad; o++)
            wr[((size_t)j * Cin_pad + ci) * rows + (size_t)o * stride_t + ph] = wp[(((size_t)ph * J + j) * Cin_pad + ci) * Cout_pad + o];
        wb3.resize(bf3_pack(wr.data(), 1, J, Cin_pad, rows, nullptr, false, h2 ? 1 : 0));
        bf3_pack(wr.data(), 1, J, Cin_pad, rows, wb3.data(), false, h2 ? 1 : 0, &h2_scale);
        std::vector<float> br((size_t)rows);
        for (int r = 0; r < rows; r++) br[r] = bp[r / stride_t];
        bp.swap(br);
    } else if (bf3) {
        wb3.resize(bf3_pack(wp.data(), tr ? stride_t : 1, tr ? J : k, Cin_pad, Cout_pad, nullptr, false, h2 ? 1 : 0));
        bf3_pack(wp.data(), tr ? stride_t : 1, tr ? J : k, Cin_pad, Cout_pad, wb3.data(), false, h2 ? 1 : 0, &h2_scale);
    }
    void* dwb3 = nullptr;
    float *dx = nullptr, *dw = nullptr, *db = nullptr, *dy = nullptr, *dwu = nullptr; int* dseg = nullptr;
    int seg[2] = {0, 1};
    bool ok = hipMalloc((void**)&dx, (size_t)Cin * L * 4) == hipSuccess && hipMalloc((void**)&dw, (wn + 1024) * 4) == hipSuccess &&
              hipMalloc((void**)&db, bp.size() * 4) == hipSuccess && hipMalloc((void**)&dy, (size_t)Cout * Lout * 4) == hipSuccess &&
              hipMalloc((void**)&dseg, 32 + tab.size() * 4) == hipSuccess;
    int rc = STS_OK;
    if (ok && !wu.empty()) ok = hipMalloc((void**)&dwu, (wu.size() + 1024) * 4) == hipSuccess;
    if (ok && bf3) ok = hipMalloc(&dwb3, wb3.size() + 4096) == hipSuccess;
    if (!ok) rc = set_err(STS_EDEVICE, "hipMalloc failed");
    if (rc == STS_OK) {
        (void)hipMemcpy(dx, x, (size_t)Cin * L * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(dw, wp.data(), wn * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(db, bp.data(), bp.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemset(dseg, 0, 32 + tab.size() * 4);
        (void)hipMemcpy(dseg, seg, 8, hipMemcpyHostToDevice);
        if (packed) (void)hipMemcpy(dseg + 8, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
        // packed: a NaN pattern instead of zeros, so that a position no workgroup writes cannot pass
        (void)hipMemset(dy, packed ? 0xFF : 0, (size_t)Cout * Lout * 4);
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.x = dx; a.x_ld = L; a.y = dy; a.y_ld = Lout; a.w = dw; a.bias = bias ? db : nullptr;
        a.Cin = cin_eff; a.Cout = Cout; a.Cin_pad = Cin_pad; a.Cout_pad = Cout_pad;
        a.depthwise = depthwise ? 1 : 0;
        if (tr) { a.ntap = J; a.tap_step = -1; a.tap_off = 0; a.out_stride = stride_t; a.out_off = -pad; a.transposed = 1; a.n_extra = J - 1; a.max_n = L + J - 1; }
        else { a.ntap = k; a.tap_step = dil; a.tap_off = -pad; a.out_stride = 1; a.out_off = 0; a.max_n = Lout; }
        a.in_act = in_act; a.in_slope = in_slope; a.epi = EPI_STORE;
        // segment lengths in base units: in = L, out = Lout -> two views over the same {off=0,len=1} table
        a.in_seg = SegView{dseg, dseg + 1, L, 0}; a.out_seg = SegView{dseg, dseg + 1, Lout, 0}; a.B = 1;
        if (packed) {     // real offset / length tables of B entries (behind the overflow word), output scale = stride
            a.in_seg = SegView{dseg + 8, dseg + 8 + B, 1, 0}; a.out_seg = SegView{dseg + 8, dseg + 8 + B, tr ? stride_t : 1, 0}; a.B = B;
            a.max_n = tr ? maxlen + J - 1 : maxlen;
        }
        if (dwu) { (void)hipMemcpy(dwu, wu.data(), wu.size() * 4, hipMemcpyHostToDevice); a.wu = dwu; a.wino_n3 = wn3; a.wino_n2 = wn2; }
        if (dwb3) { (void)hipMemcpy(dwb3, wb3.data(), wb3.size(), hipMemcpyHostToDevice); a.wb3 = dwb3; }
        if (h2) { a.math = 1; a.wscale = h2_scale; a.ovf = (unsigned*)dseg + 4; }     // (overflow word: behind the segment table)
        if (rowph) { a.rowph = stride_t; a.Cout = a.Cout_pad = Cout_pad * stride_t; }
        auto launch = [&]() {
            if (bf3) conv_bf3(a, nullptr, mode == 13 ? -1 : mode - 20);
            else if (mode == 12) conv_wino(a, nullptr);
            else if (mode != 1 && conv_mfma_eligible(a)) conv_mfma(a, nullptr, mode >= 2 ? mode - 2 : -1);
            else conv_generic(a, nullptr);
        };
        if (bf3 && !conv_bf3_eligible(a)) rc = set_err(STS_EINVAL, "shape not eligible for the split-bf16 kernel");
        else if (mode == 12 && !conv_wino_eligible(a)) rc = set_err(STS_EINVAL, "shape not eligible for the Winograd kernel");
        else if (!bf3 && mode >= 2 && mode != 12 && !conv_mfma_eligible(a)) rc = set_err(STS_EINVAL, "shape not eligible for the matrix-core kernel");
        else launch();
        if (rc == STS_OK && iters > 0 && ms_out) {   // steady-state timing of the same launch (HIP events, null stream)
            hipEvent_t e0, e1;
            (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
            (void)hipDeviceSynchronize();
            (void)hipEventRecord(e0, nullptr);
            for (int it = 0; it < iters; it++) launch();
            (void)hipEventRecord(e1, nullptr);
            (void)hipEventSynchronize(e1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            *ms_out = ms / (float)iters;
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        }
        if (rc == STS_OK && (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)) rc = set_err(STS_EDEVICE, "conv kernel failed");
        if (rc == STS_OK) {
            float* y = (float*)malloc((size_t)Cout * Lout * 4);
            (void)hipMemcpy(y, dy, (size_t)Cout * Lout * 4, hipMemcpyDeviceToHost);
            *y_out = y; *Lout_out = Lout;
            if (ovf_out) { *ovf_out = 0; if (h2) (void)hipMemcpy(ovf_out, dseg + 4, 4, hipMemcpyDeviceToHost); }
        }
    }
    (void)hipFree(dx); (void)hipFree(dw); (void)hipFree(db); (void)hipFree(dy); (void)hipFree(dseg); if (dwu) (void)hipFree(dwu); if (dwb3) (void)hipFree(dwb3);
    return rc;
}

// One "same"-padded conv through the pre-split path (conv_h2p.hip): x fp32 [Cin][L] -> split_planes -> conv_h2p_group (`members` identical
// members in one grid; member 0 is returned) -> all three output forms decoded to fp32 [Cout][L] on the host.
static int debug_conv_h2p_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                              const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                              int32_t iters, float* ms_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out);

int sts_debug_conv_h2p(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                       const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                       int32_t iters, float* ms_out) {
    return debug_conv_h2p_impl(device, x, Cin, L, w, bias, Cout, k, dil, res, in_slope, out_slope, tile, members, y_out, y16_out, yp_out, iters, ms_out,
                               nullptr, 1, nullptr);
}

// The same conv on B segments packed back to back (L = their sum): split_planes and conv_h2p_group both get the B-entry segment table and
// max_n = the longest segment; the plane and output buffers start out as a NaN pattern.
int sts_debug_conv_h2p_packed(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                              const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                              const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!lengths) return set_err(STS_EINVAL, "packed conv: null segment lengths");
    return debug_conv_h2p_impl(device, x, Cin, L, w, bias, Cout, k, dil, res, in_slope, out_slope, tile, members, y_out, y16_out, yp_out, 0, nullptr,
                               lengths, B, ovf_out);
}

static int debug_conv_h2p_impl(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k, int32_t dil,
                              const float* res, float in_slope, float out_slope, int tile, int members, float* y_out, float* y16_out, float* yp_out,
                              int32_t iters, float* ms_out, const int32_t* lengths, int32_t B, uint32_t* ovf_out) {
    if (!x || !w || Cin <= 0 || Cout <= 0 || L <= 0 || k <= 0 || !(k & 1) || dil < 1 || members < 1 || members > kMaxGroup) return set_err(STS_EINVAL, "bad conv arguments");
    if (Cin % 16 || Cout % 32) return set_err(STS_EINVAL, "pre-split conv: Cin % 16 == 0 and Cout % 32 == 0");
    const bool packed = lengths != nullptr;
    int maxlen = L;
    std::vector<int> tab;
    if (packed) {
        if (B <= 0) return set_err(STS_EINVAL, "packed conv: B >= 1 segments");
        int64_t total = 0;
        maxlen = 0;
        tab.assign((size_t)2 * B, 0);
        for (int b = 0; b < B; b++) {
            if (lengths[b] <= 0) return set_err(STS_EINVAL, "packed conv: every segment length must be positive");
            tab[b] = (int)total; tab[B + b] = lengths[b];
            total += lengths[b]; maxlen = std::max(maxlen, (int)lengths[b]);
        }
        if (total != L) return set_err(STS_EINVAL, "packed conv: L must equal the sum of the segment lengths");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "hipSetDevice failed");
    const int pad = dil * (k - 1) / 2;
    std::vector<float> wp((size_t)k * Cin * Cout, 0.f);
    for (int o = 0; o < Cout; o++) for (int t = 0; t < k; t++) for (int ci = 0; ci < Cin; ci++)
        wp[((size_t)t * Cin + ci) * Cout + o] = w[((size_t)o * k + t) * Cin + ci];
    std::vector<unsigned char> wb(bf3_pack(wp.data(), 1, k, Cin, Cout, nullptr, true, 1));
    float wscale = 1.0f;
    bf3_pack(wp.data(), 1, k, Cin, Cout, wb.data(), true, 1, &wscale);
    const size_t in_b = (size_t)Cin * L * 4, out_b = (size_t)Cout * L * 4;
    float *dx = nullptr, *db = nullptr, *dres = nullptr, *dres16 = nullptr; void *dxp = nullptr, *dwb = nullptr, *dtmp = nullptr; unsigned* dovf = nullptr;
    float* dy[kMaxGroup] = {}; float* dy16[kMaxGroup] = {}; void* dyp[kMaxGroup] = {}; int* dtab = nullptr;
    bool ok = hipMalloc((void**)&dx, in_b) == hipSuccess && hipMalloc(&dxp, in_b) == hipSuccess && hipMalloc(&dwb, wb.size() + 8192) == hipSuccess &&
              hipMalloc((void**)&db, (size_t)Cout * 4) == hipSuccess && hipMalloc((void**)&dovf, 64) == hipSuccess;
    if (ok && packed) ok = hipMalloc((void**)&dtab, tab.size() * 4) == hipSuccess;
    if (ok && res) ok = hipMalloc((void**)&dres, out_b) == hipSuccess && hipMalloc((void**)&dres16, out_b) == hipSuccess && hipMalloc(&dtmp, out_b) == hipSuccess;
    for (int m = 0; m < members && ok; m++)
        ok = hipMalloc((void**)&dy[m], out_b) == hipSuccess && hipMalloc((void**)&dy16[m], out_b) == hipSuccess && hipMalloc(&dyp[m], out_b) == hipSuccess;
    int rc = ok ? STS_OK : set_err(STS_EDEVICE, "hipMalloc failed");
    if (rc == STS_OK) {
        (void)hipMemcpy(dx, x, in_b, hipMemcpyHostToDevice);
        (void)hipMemset(dwb, 0, wb.size() + 8192);
        (void)hipMemcpy(dwb, wb.data(), wb.size(), hipMemcpyHostToDevice);
        (void)hipMemset(db, 0, (size_t)Cout * 4);
        if (bias) (void)hipMemcpy(db, bias, (size_t)Cout * 4, hipMemcpyHostToDevice);
        (void)hipMemset(dovf, 0, 64);
        SegView whole{nullptr, nullptr, 1, 0, 0, L};
        int nb = 1;
        if (packed) {     // a real table of B entries; every buffer the kernels write starts out as NaNs (fp32 and fp16 alike)
            (void)hipMemcpy(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
            whole = SegView{dtab, dtab + B, 1, 0, 0, 0};
            nb = B;
            (void)hipMemset(dxp, 0xFF, in_b);
            if (res) { (void)hipMemset(dres16, 0xFF, out_b); (void)hipMemset(dtmp, 0xFF, out_b); }
            for (int m = 0; m < members; m++) { (void)hipMemset(dy[m], 0xFF, out_b); (void)hipMemset(dy16[m], 0xFF, out_b); (void)hipMemset(dyp[m], 0xFF, out_b); }
        }
        split_planes(dx, L, Cin, whole, nb, maxlen, in_slope, dxp, nullptr, L, dovf, nullptr);
        if (res) {
            (void)hipMemcpy(dres, res, out_b, hipMemcpyHostToDevice);
            split_planes(dres, L, Cout, whole, nb, maxlen, 1.0f, dtmp, dres16, L, nullptr, nullptr);
        }
        H2PGroup G;
        memset(&G, 0, sizeof(G));
        G.n = members; G.seg = whole; G.B = nb; G.max_n = maxlen; G.ovf = dovf;
        for (int m = 0; m < members; m++) {
            H2PArgs& a = G.g[m];
            a.xp = dxp; a.xp_ld = L; a.wb = dwb; a.wscale = wscale; a.bias = bias ? db : nullptr; a.res16 = dres16; a.res_ld = L;
            a.y = iters < 0 ? nullptr : dy[m]; a.y_ld = L; a.y16 = dy16[m]; a.y16_ld = L; a.yp = dyp[m]; a.yp_ld = L; a.yp_slope = out_slope;    // (iters < 0: timing with a layer's second conv's outputs only)
            a.Cin = Cin; a.Cout = Cout; a.ntap = k; a.tap_step = dil; a.tap_off = -pad;
        }
        if (!conv_h2p_group_eligible(G)) rc = set_err(STS_EINVAL, "shape not eligible for the pre-split kernel");
        else {
            conv_h2p_group(G, nullptr, tile);
            if (iters != 0 && ms_out) {
                if (iters < 0) iters = -iters;
                hipEvent_t e0, e1;
                (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
                (void)hipDeviceSynchronize();
                (void)hipEventRecord(e0, nullptr);
                for (int it = 0; it < iters; it++) conv_h2p_group(G, nullptr, tile);
                (void)hipEventRecord(e1, nullptr);
                (void)hipEventSynchronize(e1);
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e0, e1);
                *ms_out = ms / (float)iters;
                (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
            }
            if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) rc = set_err(STS_EDEVICE, "conv kernel failed");
        }
        if (rc == STS_OK) {
            if (y_out) (void)hipMemcpy(y_out, dy[0], out_b, hipMemcpyDeviceToHost);
            if (ovf_out) (void)hipMemcpy(ovf_out, dovf, 4, hipMemcpyDeviceToHost);
            std::vector<float> t16((size_t)Cout * L);
            std::vector<uint16_t> tp((size_t)Cout * L * 2);
            (void)hipMemcpy(t16.data(), dy16[0], out_b, hipMemcpyDeviceToHost);
            (void)hipMemcpy(tp.data(), dyp[0], out_b, hipMemcpyDeviceToHost);
            const size_t ps = (size_t)Cout * L;       // fp16 values per plane
            for (int c = 0; c < Cout / 16; c++) for (long t = 0; t < L; t++) for (int h = 0; h < 2; h++) for (int e = 0; e < 8; e++) {
                const int ch = 16 * c + 8 * (e >> 2) + 4 * h + (e & 3);
                const size_t u = ((size_t)c * L + t) * 16 + h * 8 + e;
                if (y16_out) y16_out[(size_t)ch * L + t] = t16[u];
                if (yp_out) {
                    _Float16 hi, lo;
                    memcpy(&hi, &tp[u], 2); memcpy(&lo, &tp[ps + u], 2);
                    yp_out[(size_t)ch * L + t] = (float)hi + (float)lo * (1.0f / 2048.0f);
                }
            }
        }
    }
    (void)hipFree(dx); (void)hipFree(dxp); (void)hipFree(dwb); (void)hipFree(db); (void)hipFree(dovf); if (dtab) (void)hipFree(dtab);
    if (dres) (void)hipFree(dres); if (dres16) (void)hipFree(dres16); if (dtmp) (void)hipFree(dtmp);
    for (int m = 0; m < kMaxGroup; m++) { if (dy[m]) (void)hipFree(dy[m]); if (dy16[m]) (void)hipFree(dy16[m]); if (dyp[m]) (void)hipFree(dyp[m]); }
    return rc;
}

// One "same"-padded conv through the Winograd-domain lab path (conv_h2w.hip): x fp32 [C][L] -> to_x16 -> conv_h2w_group (`members` identical
// members) -> member 0's fp32 [C][L] output and its x16 output (lrelu(out, out_slope)) decoded to fp32 [C][L].
int sts_debug_conv_h2w(int device, const float* x, int32_t C, int32_t L, const float* w, const float* bias, int32_t k, int32_t dil, const float* res,
                       float in_slope, float out_slope, int members, float* y_out, float* y16_out, int32_t iters, float* ms_out) {
    if (!x || !w || C <= 0 || L <= 0 || k <= 0 || !(k & 1) || dil < 1 || members < 1 || members > kMaxGroup || C % 128) return set_err(STS_EINVAL, "bad conv arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return set_err(STS_EDEVICE, "no HIP device visible (no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return set_err(STS_EDEVICE, "hipSetDevice failed");
    std::vector<float> wp((size_t)k * C * C, 0.f);
    for (int o = 0; o < C; o++) for (int t = 0; t < k; t++) for (int ci = 0; ci < C; ci++) wp[((size_t)t * C + ci) * C + o] = w[((size_t)o * k + t) * C + ci];
    int n3, n2; wino_split(k, &n3, &n2);
    const int ntapw = 4 * n3 + 3 * n2;
    std::vector<float> wu((size_t)ntapw * C * C);
    h2w_transform_weights(wp.data(), k, C, C, wu.data());
    std::vector<unsigned char> wb(bf3_pack(wu.data(), 1, ntapw, C, C, nullptr, true, 1));
    float wscale = 1.0f;
    bf3_pack(wu.data(), 1, ntapw, C, C, wb.data(), true, 1, &wscale);
    const size_t tb = (size_t)C * L * 4;
    float *dx = nullptr, *dx16 = nullptr, *db = nullptr, *dres = nullptr, *dres16 = nullptr; void* dwb = nullptr; unsigned* dovf = nullptr;
    float* dy[kMaxGroup] = {}; float* dy16[kMaxGroup] = {};
    bool ok = hipMalloc((void**)&dx, tb) == hipSuccess && hipMalloc((void**)&dx16, tb) == hipSuccess && hipMalloc(&dwb, wb.size() + 8192) == hipSuccess &&
              hipMalloc((void**)&db, (size_t)C * 4) == hipSuccess && hipMalloc((void**)&dovf, 64) == hipSuccess;
    if (ok && res) ok = hipMalloc((void**)&dres, tb) == hipSuccess && hipMalloc((void**)&dres16, tb) == hipSuccess;
    for (int m = 0; m < members && ok; m++) ok = hipMalloc((void**)&dy[m], tb) == hipSuccess && hipMalloc((void**)&dy16[m], tb) == hipSuccess;
    int rc = ok ? STS_OK : set_err(STS_EDEVICE, "hipMalloc failed");
    if (rc == STS_OK) {
        (void)hipMemcpy(dx, x, tb, hipMemcpyHostToDevice);
        (void)hipMemset(dwb, 0, wb.size() + 8192);
        (void)hipMemcpy(dwb, wb.data(), wb.size(), hipMemcpyHostToDevice);
        (void)hipMemset(db, 0, (size_t)C * 4);
        if (bias) (void)hipMemcpy(db, bias, (size_t)C * 4, hipMemcpyHostToDevice);
        (void)hipMemset(dovf, 0, 64);
        to_x16(dx, L, C, L, dx16, L, nullptr);
        if (res) { (void)hipMemcpy(dres, res, tb, hipMemcpyHostToDevice); to_x16(dres, L, C, L, dres16, L, nullptr); }
        H2WGroup G;
        memset(&G, 0, sizeof(G));
        G.n = members; G.seg = SegView{nullptr, nullptr, 1, 0, 0, L}; G.B = 1; G.max_n = L; G.ovf = dovf;
        for (int m = 0; m < members; m++) {
            H2WArgs& a = G.g[m];
            a.x16 = dx16; a.x_ld = L; a.wu = dwb; a.wscale = wscale; a.bias = bias ? db : nullptr; a.res16 = dres16; a.res_ld = L;
            a.y16 = dy16[m]; a.y16_ld = L; a.y = iters < 0 ? nullptr : dy[m]; a.y_ld = L; a.in_slope = in_slope; a.out_slope = out_slope; a.C = C; a.k = k; a.dil = dil;
        }
        if (!conv_h2w_group_eligible(G)) rc = set_err(STS_EINVAL, "shape not eligible for the Winograd-domain kernel");
        else {
            conv_h2w_group(G, nullptr);
            if (iters != 0 && ms_out) {
                if (iters < 0) iters = -iters;
                hipEvent_t e0, e1;
                (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
                (void)hipDeviceSynchronize();
                (void)hipEventRecord(e0, nullptr);
                for (int it = 0; it < iters; it++) conv_h2w_group(G, nullptr);
                (void)hipEventRecord(e1, nullptr);
                (void)hipEventSynchronize(e1);
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e0, e1);
                *ms_out = ms / (float)iters;
                (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
            }
            if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) rc = set_err(STS_EDEVICE, "conv kernel failed");
        }
        if (rc == STS_OK) {
            if (y_out) (void)hipMemcpy(y_out, dy[0], tb, hipMemcpyDeviceToHost);
            if (y16_out) {
                std::vector<float> t16((size_t)C * L);
                (void)hipMemcpy(t16.data(), dy16[0], tb, hipMemcpyDeviceToHost);
                for (int c = 0; c < C / 16; c++) for (long t = 0; t < L; t++) for (int h = 0; h < 2; h++) for (int e = 0; e < 8; e++)
                    y16_out[(size_t)(16 * c + 8 * (e >> 2) + 4 * h + (e & 3)) * L + t] = t16[((size_t)c * L + t) * 16 + h * 8 + e];
            }
        }
    }
    (void)hipFree(dx); (void)hipFree(dx16); (void)hipFree(dwb); (void)hipFree(db); (void)hipFree(dovf);
    if (dres) (void)hipFree(dres); if (dres16) (void)hipFree(dres16);
    for (int m = 0; m < kMaxGroup; m++) { if (dy[m]) (void)hipFree(dy[m]); if (dy16[m]) (void)hipFree(dy16[m]); }
    return rc;
}

}  // extern "C"
