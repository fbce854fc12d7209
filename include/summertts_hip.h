/* summertts_hip.h -- C ABI of libsummertts_hip.so, the MI355X (gfx950) acoustic + vocoder engine.
 *
 * This is the drop-in boundary for the hot path of huakunyang/SummerTTS: everything that
 * SynthesizerTrn::infer does AFTER the text frontend has produced phoneme ids
 * (/root/reference/src/models/SynthesizerTrn.cpp:357-400) and the model construction it depends on
 * (SynthesizerTrn.cpp:91-163).  Plain pointers and sizes only -- no C++/torch types -- so the
 * reference's C++ class (include/SynthesizerTrn.h in this repo keeps the reference's exact class
 * surface) or any other host language binds to it directly.  See INTEGRATION.md for the binding a
 * SummerTTS maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative STS_E* code; sts_last_error()
 * returns a static, thread-local description.  Buffers returned through `**` out-parameters are
 * malloc()'d and owned by the caller (free with sts_free == the reference's tts_free_data,
 * /root/reference/src/utils/utils.cpp:34-37).  An engine is not re-entrant (neither is the
 * reference instance); use one engine per host thread / per GPU.
 */
#ifndef SUMMERTTS_HIP_H_
#define SUMMERTTS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sts_engine sts_engine;

enum {
    STS_OK = 0,
    STS_EINVAL = -1,   /* bad argument (null pointer, phoneme id outside the vocabulary, n <= 0 ...) */
    STS_EMODEL = -2,   /* the blob does not parse as a SummerTTS model */
    STS_EDEVICE = -3,  /* HIP runtime failure (no gfx950 device, out of memory ...) */
    STS_ESTATE = -4    /* call sequence error (e.g. asking for a tap that was not recorded) */
};

/* Replaces SynthesizerTrn::SynthesizerTrn(float* modelData, int32_t modelSize)
 * (/root/reference/src/models/SynthesizerTrn.cpp:91-163): parses the float-stream blob (size in BYTES,
 * as ttsLoadModel returns it), repacks and uploads the weights to HIP device `device`.  The blob is
 * copied; the caller may free it afterwards (as test/main.cpp:144-145 does). */
int sts_create(const float* blob, int64_t blob_bytes, int device, sts_engine** out);
void sts_destroy(sts_engine* e);

/* Replaces SynthesizerTrn::getSpeakerNum (SynthesizerTrn.cpp:79-89): 1 for single-speaker models. */
int sts_speaker_num(const sts_engine* e);

/* Model facts the host side needs (vocabulary size for id validation, samples per frame, ...). */
typedef struct sts_model_info {
    int32_t is_multi_speaker, lang_type, dur_pred_type, dec_type;
    int32_t vocab, hidden, inter_channels, speaker_num, gin_channels;
    int32_t samples_per_frame;      /* total upsampling factor */
    int32_t sample_rate;            /* the model's NATIVE rate, 16000 (/root/reference/test/main.cpp:13,16) -- unchanged by sts_set_output_rate */
    int64_t blob_floats_consumed;   /* floats consumed by the acoustic sections (frontend sections follow) */
} sts_model_info;
int sts_get_info(const sts_engine* e, sts_model_info* info);

/* Replaces the post-frontend part of SynthesizerTrn::infer (SynthesizerTrn.cpp:357-400) for one
 * utterance: ids[n] -> int16 PCM.  Out-of-range sid -> 0 (SynthesizerTrn.cpp:366-369).
 * *pcm_out is malloc()'d; *n_out = sample count. */
int sts_infer_ids(sts_engine* e, const int32_t* ids, int32_t n, int32_t sid, float length_scale,
                  int16_t** pcm_out, int32_t* n_out);

/* Streaming form (no reference counterpart: SynthesizerTrn::infer returns the whole utterance,
 * SynthesizerTrn.cpp:389-400).  Text encoder, duration predictor and flow run once; the decoder then runs
 * chunk by chunk (chunk_frames acoustic frames each, decoded with the receptive-field halo on both sides) and
 * `cb` receives every chunk's PCM as soon as it is on the host: first audio after one chunk instead of after
 * the whole utterance, decoder workspace bounded by the chunk size.  The concatenated chunks equal
 * sts_infer_ids' output bit for bit when the kernel variant is pinned (sts_set_conv_mode) and to within 1 LSB
 * under the automatic choice (a chunk is a smaller launch and may be routed to the split-K kernel, which sums
 * K in a different order).  `pcm` is only valid during the callback; a non-zero return stops the stream.
 * *n_total = samples delivered. */
typedef int (*sts_chunk_cb)(void* user, const int16_t* pcm, int32_t n_samples, int32_t sample_offset);
int sts_infer_ids_stream(sts_engine* e, const int32_t* ids, int32_t n, int32_t sid, float length_scale,
                         int32_t chunk_frames, sts_chunk_cb cb, void* user, int32_t* n_total);
/* frames of context the streaming decoder adds on each side of a chunk (a property of the loaded model and, at a non-native output rate,
 * of the resampler: see sts_set_output_rate) */
int sts_stream_halo_frames(const sts_engine* e);

/* Batched streaming (ABI 10): B utterances streamed together, chunk by chunk.  Text encoder, duration predictor and flow run once as
 * a packed batch of B (as sts_infer_ids_batch; forced durations likewise; sampling noise: utterance b uses seed + b).  Then step k decodes
 * chunk k of every utterance still live -- frames [k C, min((k + 1) C, F_b)) of utterance b, C = chunk_frames, F_b its frame count -- each
 * from the window [max(0, f0 - halo), min(F_b, f1 + halo)) (halo = sts_stream_halo_frames), all windows of the step in one decode pass.
 * The decoder's workspace holds sum_b min(F_b, C + 2 halo) frames, not the whole batch.
 *   Delivery: step by step; within a step in ascending `utt`; all chunks of a step reach the caller before the next step starts.  An
 *   utterance leaves the steps once its last chunk is delivered.  sample_offset counts output samples of that utterance at the current
 *   output rate: chunk k starts at ceil(k C hop P / Q) (k C hop at the native rate), as in sts_infer_ids_stream.  `pcm` is only valid
 *   during the callback.  A non-zero return stops THAT utterance only: it receives nothing more, the others go on unchanged.
 *   n_total (may be NULL): [B] samples delivered per utterance.  sid and length_scale may be NULL (0 and 1.0).
 *   Equality: each utterance's concatenated chunks equal its sts_infer_ids_stream output and member b of sts_infer_ids_batch bit for bit
 *   when the kernel variant is pinned (sts_set_conv_mode), and to within 1 LSB under the automatic choice.  B == 1 is
 *   sts_infer_ids_stream itself, bit for bit in every mode.
 *   conv math 3: an activation beyond fp16's range before anything was delivered repeats the whole call in form 0; at a later step that
 *   step is decoded again in form 0 for all of its windows, and so are the steps after it.  No chunk is delivered twice, and
 *   sts_profile.conv_math_fallbacks counts the call once.
 *   B < 1, chunk_frames <= 0, a NULL callback or NULL ids / n: STS_EINVAL, nothing runs. */
typedef int (*sts_batch_chunk_cb)(void* user, int32_t utt, const int16_t* pcm, int32_t n_samples, int32_t sample_offset);
int sts_infer_ids_batch_stream(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                               const float* length_scale, int32_t chunk_frames, sts_batch_chunk_cb cb, void* user,
                               int32_t* n_total);

/* Open streams: a batched stream that admits new utterances between its steps.  One per engine; nothing here is on by default.
 *   sts_stream_open fixes the chunk size C = chunk_frames, the output rate, the limiter setting, the conv mode and the conv math, and
 *   allocates a latent pool of capacity_frames frames for at most max_live utterances at a time (1 <= max_live <= 1024;
 *   capacity_frames * inter_channels and capacity_frames * samples_per_frame at most 2 10^9).  STS_EINVAL while EQ bands are set without
 *   sts_set_eq_streaming, the loudness mode is 1 without sts_set_loudness_streaming or is 2, or record taps are on (with the stream
 *   modes on the EQ and the measurement run from per-slot state: "Per-slot filter state" below), or while a duration plan, speaker mix,
 *   gain plan or forced durations are pending (a pending table belongs to a next run, and open is not a run); STS_ESTATE when a stream is
 *   open.  sts_stream_open is the capacity_phonemes == 0 case of sts_stream_open_ex (below), which admits utterances WITH those tables.
 *   sts_stream_admit runs text encoder, duration predictor and flow of B newcomers as the packed batch a sts_infer_ids_batch_stream call
 *   of those B would, and moves their latents into the pool.  All or nothing: *admitted = B, or 0 when slots or frames do not suffice now
 *   (nothing has changed; retry after a retirement).  slot_out[b] = the slot of utterance b, the `utt` its chunks arrive with (-1: it has
 *   no frames and receives nothing); n_samples_out[b] = its total output samples at the current rate, so that the caller can tell a slot's
 *   last chunk.  Both may be NULL; sid and length_scale may be NULL (0 and 1.0).  noise: NULL = the engine's setting with seed + b for
 *   utterance b of the admission, as utterance b of a batch call; otherwise [B] settings used as given.  B > max_live: STS_EINVAL.
 *   sts_stream_step is ONE step: every live slot, in ascending slot order, decodes its next chunk -- frames [f_s, min(f_s + C, F_s)) of
 *   slot s from its own position f_s -- all windows in one decode pass, and the chunks reach `cb` (utt = slot) before the call returns.  A
 *   slot retires, and its index and its frames become free, behind its last chunk or when its callback returns non-zero.  *live_after (may
 *   be NULL) = slots still live.  With no live slot it does nothing.
 *   sts_stream_info: any output may be NULL; *steps = sts_stream_step calls since open that decoded.  sts_stream_close drops the live
 *   slots without delivering and frees the pool; sts_destroy closes an open stream.  No entry of an open stream may be called from a
 *   chunk callback.
 *   While a stream is open every other run entry of the engine and every setter of what open fixed (output rate, limiter, EQ, loudness,
 *   conv mode, conv math, plans, mixes, forced durations, record taps, the debug switches other than STS_DBG_STREAM_RETRY_STEP and
 *   STS_DBG_POISON) returns STS_ESTATE; sts_set_noise stays allowed.  (A planned stream, below, lets the four table setters through.)
 *   Equality: whatever the admission schedule, the list of chunks of every utterance and their sample offsets equal its
 *   sts_infer_ids_stream chunks with the same chunk_frames bit for bit when the kernel variant is pinned (sts_set_conv_mode), and its PCM
 *   is within 1 LSB of that under the automatic choice.
 *   conv math 3: an activation beyond fp16's range during an admission repeats that admission alone in form 0 (nothing of it has been
 *   delivered); raised in a step, that step is decoded again in form 0 and the stream stays in form 0 until it is closed.  No chunk is
 *   delivered twice; sts_profile.conv_math_fallbacks counts the steps of one open stream once.  STS_DBG_STREAM_RETRY_STEP = k applies to
 *   the k-th sts_stream_step since open. */
typedef struct sts_stream_noise { float noise_scale, noise_scale_w; uint64_t seed; } sts_stream_noise;
int sts_stream_open(sts_engine* e, int32_t chunk_frames, int32_t max_live, int64_t capacity_frames);
int sts_stream_admit(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                     const float* length_scale, const sts_stream_noise* noise, int32_t* slot_out, int32_t* n_samples_out,
                     int32_t* admitted);
int sts_stream_step(sts_engine* e, sts_batch_chunk_cb cb, void* user, int32_t* live_after);
int sts_stream_info(const sts_engine* e, int32_t* open, int32_t* live, int32_t* free_slots, int64_t* free_frames, int64_t* steps);
int sts_stream_close(sts_engine* e);
/* Planned open streams: sts_stream_open_ex with capacity_phonemes in [1, 2^24] opens a stream whose admissions take the per-call tables of
 * a closed stream.  capacity_phonemes == 0 is sts_stream_open exactly (same refusals, same setters refused while open, same bits);
 * negative or larger: STS_EINVAL.  A planned stream refuses at open what sts_stream_open refuses (EQ bands or loudness mode 1 without
 * their stream modes, loudness mode 2, record taps, and a plan, mix, gain plan or forced durations pending AT open).
 *   While a planned stream is open sts_set_duration_plan, sts_set_speaker_mix, sts_set_gain_plan and sts_set_forced_durations return
 *   STS_OK, and what they set applies to the NEXT sts_stream_admit only, whatever its outcome (one that finds no room, *admitted = 0, and
 *   one that fails included).  That admission must have the B and n[b] the tables were set for: otherwise STS_EINVAL, nothing is admitted
 *   and the tables are dropped.  A duration plan together with forced durations: STS_EINVAL, both dropped, as in a run.  The conv-math-3
 *   repeat of an admission applies the same tables again.  Every other setter stays STS_ESTATE.
 *   An admitted utterance carries: its planned durations (n_samples_out[b] and its chunks follow from them); its blended speaker vector,
 *   through its last chunk; its gain plan -- an utterance whose sts_gain_plan entry has gain_db != NULL takes n[b] columns of a phoneme pool
 *   of capacity_phonemes columns (first fit, returned when it retires), one without takes none.  Admission is all or nothing over slots,
 *   frames AND phonemes.  A step runs the gain stage only when a live slot carries a gain plan; in such a step a slot without one keeps its
 *   samples bit for bit.  Equality: every utterance's chunks equal those of sts_infer_ids_stream with the same tables set just before
 *   it, under the terms of an unplanned stream.  After an admission sts_get_durations and sts_get_phoneme_offsets report the admitted
 *   utterances, packed as after sts_infer_ids_batch_stream (so for a plain stream too).
 *   Still refused or unsupported: loudness mode 2 and record taps in an open stream, the EQ, loudness and plans in open paragraphs
 *   (sts_para_*), and sts_multi_*.
 *   sts_stream_tables_info: any output may be NULL; *planned = 1 for an open planned stream, the pool's capacity and its free columns
 *   (zeros otherwise).
 *   These entries were added without a new STS_ABI_VERSION: detect them by symbol. */
int sts_stream_open_ex(sts_engine* e, int32_t chunk_frames, int32_t max_live, int64_t capacity_frames, int64_t capacity_phonemes);
int sts_stream_tables_info(const sts_engine* e, int32_t* planned, int64_t* capacity_phonemes, int64_t* free_phonemes);
/* (The EQ and loudness in an open stream -- per-slot filter state -- and sts_stream_get_loudness: below, behind sts_get_loudness.) */
/* The kernel that moves an admission's latents into the pool, on caller data (host pointers in and out): B column segments of the
 * channel-major src [C][ld_src] into dst [C][ld_dst]; segment b is len[b] columns from src_off[b] to dst_off[b].  dst comes back with
 * every element outside the destination ranges unchanged.  Ranges outside either matrix, overlapping destination ranges, B outside
 * [1, 65535] or C < 1: STS_EINVAL. */
int sts_debug_adopt_z(int device, const float* src, int32_t C, int64_t ld_src, float* dst, int64_t ld_dst, const int64_t* src_off,
                      const int64_t* dst_off, const int32_t* len, int32_t B);
/* The kernel that moves an admission's tables into a planned stream's pools, on caller data (host pointers in and out).  For newcomer
 * b < B with slot[b] >= 0: column b of g [gin][B] -> column slot[b] of gpool [gin][max_live] (gin 0: g and gpool NULL, nothing moves);
 * n[b] > 0: cum[src_off[b] .. + n[b]) and q[..] (arrays of n_src entries) -> rows 0 and 1 of pool [2][capacity_phonemes + 1] at column
 * dst_off[b], and the words of its slot in slot_words [3][max_live] (rows off | n | h) = {dst_off[b], n[b], h[b]}; n[b] == 0 (it carries
 * no phonemes): its words = {capacity_phonemes, 1, 0}, the pool's shared neutral column.  slot[b] == -1: nothing.  gpool, pool and
 * slot_words come back with everything else unchanged.  Ranges outside either array, overlapping destination ranges, a slot named
 * twice or outside [-1, max_live), B outside [1, 65535]: STS_EINVAL. */
int sts_debug_adopt_tables(int device, const float* g, int32_t gin, int32_t B, float* gpool, int32_t max_live, const int32_t* cum,
                           const int32_t* q, int64_t n_src, int32_t* pool, int64_t capacity_phonemes, int32_t* slot_words,
                           const int32_t* slot, const int32_t* src_off, const int32_t* n, const int32_t* dst_off, const int32_t* h);

/* Batched form (new capability; the reference processes exactly one utterance per call).  The B
 * utterances are packed along time on the device and run through every kernel together.
 * pcm_out[b] is malloc()'d per utterance. */
int sts_infer_ids_batch(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n,
                        const int32_t* sid, const float* length_scale, int16_t** pcm_out, int32_t* n_out);

/* Same, but leaves the PCM on the device (packed back to back, utterance order) for a following
 * RCCL gather; n_out[b] = samples of utterance b, *total_out = sum.  Copy out with
 * sts_copy_pcm_device (device-to-device, asynchronous on the engine stream then synchronised). */
int sts_run_batch(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                  const float* length_scale, int32_t* n_out, int64_t* total_out);
/* sts_set_host_pcm(e, 1): sts_run_batch also downloads the PCM into an engine-owned pinned host buffer as the last step of
 * the run (one stream synchronisation per call instead of two); sts_copy_pcm_host then copies from that buffer.  Leave it
 * off (default) when the PCM stays on the device for an RCCL gather. */
int sts_set_host_pcm(sts_engine* e, int enable);
int sts_copy_pcm_device(sts_engine* e, void* device_dst, int64_t capacity_samples);
int sts_copy_pcm_host(sts_engine* e, int16_t* host_dst, int64_t capacity_samples);
/* Zero-copy form of sts_copy_pcm_host for a caller that consumes the PCM before its next call on this engine: *pcm points into
 * the engine-owned pinned host buffer the last run downloaded into (needs sts_set_host_pcm(e, 1); STS_ESTATE otherwise), *count =
 * samples of all utterances back to back.  The pointer is valid until the next run / destroy on this engine. */
int sts_pcm_host_view(sts_engine* e, const int16_t** pcm, int64_t* count);

/* Parity/diagnostic controls (test infrastructure hooks; defaults reproduce the reference):
 *   forced durations: per-phoneme frame counts that override ceil(exp(logw)*lengthScale) for the NEXT
 *   run only (the ceil is discontinuous, so waveform parity is checked with the
 *   oracle's durations).  Packed for the whole batch (sum of n entries). */
int sts_set_forced_durations(sts_engine* e, const int32_t* dur, int64_t count);
/* ---- sampling noise (VITS inference noise; the reference's SynthesizerTrn::infer fixes both scales at 0, which stays the default).
 *   noise_scale      scales the prior sample  z_p = m + eps * logs * noise_scale          (SynthesizerTrn.cpp:383: logs, NOT exp(logs))
 *   noise_scale_w    scales the stochastic duration predictor's latent  z = eps * noise_scale_w  (StochasticDurationPredictor.cpp:129;
 *                    accepted and ignored by models with the Fix duration predictor, as in the reference)
 *   seed             utterance b of a call samples with seed + b; the engine never advances it (same call + same seed = same PCM)
 * eps is a counter-based Philox4x64-10 stream per (seed, utterance element): results do not depend on batching, devices or chunking.
 * The setting persists and applies to sts_infer_ids, sts_infer_ids_stream, sts_infer_ids_batch and sts_run_batch.  A negative or
 * non-finite scale answers STS_EINVAL and changes nothing. */
int sts_set_noise(sts_engine* e, float noise_scale, float noise_scale_w, uint64_t seed);
int sts_get_noise(const sts_engine* e, float* noise_scale, float* noise_scale_w, uint64_t* seed);
/* ---- output sample rate (no reference counterpart: every model produces 16 kHz).  sts_set_output_rate(e, rate): 0 or 16000 = native
 * (the default; no extra work, bit-identical to an engine that never set a rate), otherwise an integer rate in [8000, 48000]: the decoder's
 * float wave is resampled on the device and every call form -- sts_infer_ids, sts_infer_ids_batch, sts_run_batch (counts, offsets,
 * sts_copy_pcm_device / _host, sts_pcm_host_view), sts_infer_ids_stream -- returns int16 PCM at that rate.  The setting persists, like
 * sts_set_noise.  An invalid rate answers STS_EINVAL and changes nothing.  sts_get_output_rate returns the effective rate (16000 = native).
 *   The filter (in = 16000, out = the rate; exactly what sts_resample_table returns):
 *     g = gcd(in, out), P = out / g, Q = in / g; P > 1024 is rejected (e.g. 47999).  L_out = ceil(L_in P / Q) per utterance.
 *     Output j sits at input position j Q / P: phase phi = (j Q) mod P, base n0 = (j Q) div P.
 *     c = 0.9 min(1, out / in) (cutoff in units of the input Nyquist), W = 32 / c, K = ceil(W): 2K taps per phase.
 *     Tap m (0 <= m < 2K) of phase phi reads input n0 - K + 1 + m at offset d = phi / P + K - 1 - m, coefficient
 *     h = c sinc(c d) I0(beta sqrt(1 - (d / W)^2)) / I0(beta) for |d| < W, else 0; beta = 10, sinc(x) = sin(pi x) / (pi x).
 *     Designed in float64, every phase normalised to sum 1, rounded to float32: table [P][2K].  Input outside the utterance is 0.
 *     y_j = the fp32 FMA chain over m = 0 .. 2K-1; PCM = the reference's cast (int16)(int32)(y_j * 32737).
 *   Streaming: a chunk covering native samples [a, b) emits the outputs ceil(a P / Q) <= j < ceil(b P / Q) (the last one through L_out);
 *   sample_offset counts output samples.  The decode halo grows by ceil(K / samples_per_frame) frames (sts_stream_halo_frames reports the
 *   halo at the current rate).  Taps: "wave" stays the native float wave; "wave_out" (non-native rate only) is y before the cast. */
int sts_set_output_rate(sts_engine* e, int32_t rate);
int sts_get_output_rate(const sts_engine* e);
/* Host only (no device): the design above for in_rate -> out_rate (both integers in [8000, 48000]).  *P, *Q, *taps (= 2K) are set when
 * non-null; table == NULL asks for the sizes only, otherwise it receives the float32 [P][taps] table the kernel uses (capacity_floats
 * below P * taps: STS_EINVAL). */
int sts_resample_table(int32_t in_rate, int32_t out_rate, int32_t* P, int32_t* Q, int32_t* taps, float* table, int64_t capacity_floats);
/* ---- loudness (ABI 11; no reference counterpart: SynthesizerTrn.cpp:389-396 casts whatever level the model produces, and wraps
 * around past |o| > 1.0009).  sts_set_loudness(e, mode, target_lufs, peak_dbfs) selects, per engine (the setting persists):
 *   STS_LOUD_OFF (0, default): no extra work; PCM bit-identical to an engine that never set it.
 *   STS_LOUD_MEASURE (1): every utterance of a whole-utterance call (sts_infer_ids, sts_infer_ids_batch, sts_run_batch) is measured;
 *     the PCM is bit-identical to mode 0.  sts_get_loudness reads the results afterwards.
 *   STS_LOUD_NORMALIZE (2): measures, then casts each utterance with its own gain.
 * The measurement applies to the float wave at the output rate (sts_set_output_rate): the native wave at 16 kHz, otherwise the
 * resampled wave (y before the cast; the "wave_out" tap).  For one utterance x[0 .. N) at rate fs:
 *   1 K-weighting, two biquads in cascade from zero state (y = the filtered x), coefficients as sts_kweight_coeffs returns them:
 *     high shelf  f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *                 Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2:  b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0,
 *                 a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0];
 *     high-pass   f0 = 38.13547087602444, Q = 0.5003270373238773, same K and a0:  b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0].
 *   2 Blocks: S = floor(fs / 10 + 0.5); block j = y[jS, jS + 4S) for j = 0 .. floor((N - 4S) / S) (none if N < 4S);
 *     z_j = sum y^2 / (4S), l_j = -0.691 + 10 log10 z_j.
 *   3 Gating (BS.1770-4, one channel, weight 1): keep l_j > -70; Gr = -0.691 + 10 log10(mean z of those) - 10; the final set has
 *     l_j > -70 and l_j > Gr; L = -0.691 + 10 log10(mean z of the final set).  An empty final set (shorter than 400 ms, silent, or all
 *     gated out): L = -inf, the utterance is unmeasured.
 *   4 Peak p = max |x| (sample peak of the float signal).
 *   5 Gain, with target T in [-70, 0] LUFS and ceiling C in [-30, 0] dBFS: g_L = 10^((T - L) / 20) if L is finite, else 1;
 *     g = p > 0 ? min(g_L, 10^(C / 20) / p) : g_L, computed in float64 and rounded to float32 (|x g 32737| <= 32737: mode 2 never wraps).
 *   6 Mode 2: pcm[i] = the reference's cast (int16)(int32)(x[i] g * 32737), one fp32 multiply in front of it.
 *   7 Results per utterance of the last whole-utterance call, in call order: lufs (L, -INFINITY when unmeasured), peak (p), gain (g; mode 1
 *     reports it too), blocks (size of the final set).
 * An utterance's results are a function of its own x only, bit for bit (not of its batch companions, its position, or repetition).
 * Streaming needs the whole utterance before normalizing: while the mode is not 0, sts_infer_ids_stream and sts_infer_ids_batch_stream
 * answer STS_EINVAL (the engine stays usable) -- unless, for mode 1, sts_set_loudness_streaming (below) is on.  Bad arguments (unknown mode, NaN or out-of-range target / ceiling): STS_EINVAL, nothing
 * changes.  sts_get_loudness returns the count of the last call's results (0 after a call in mode 0, a failure, or a
 * streaming call that did not measure) and
 * copies them to out; out == NULL asks for the count alone, a capacity below it answers STS_EINVAL. */
#define STS_LOUD_OFF 0
#define STS_LOUD_MEASURE 1
#define STS_LOUD_NORMALIZE 2
typedef struct sts_loudness { float lufs; float peak; float gain; int32_t blocks; } sts_loudness;
int sts_set_loudness(sts_engine* e, int mode, float target_lufs, float peak_dbfs);
int sts_get_loudness_mode(const sts_engine* e, int* mode, float* target_lufs, float* peak_dbfs);
int sts_get_loudness(sts_engine* e, sts_loudness* out, int64_t capacity);
/* Per-slot filter state: an open stream (planned or not) opened with EQ bands set and sts_set_eq_streaming on runs the streamed EQ on every
 * slot, and one opened under loudness mode 1 with sts_set_loudness_streaming on measures every slot -- each slot from a carried state of
 * its own, kept in pools the stream allocates at open for the stages that are on (per stream slot: 98.8 KB of EQ state, 66 KB of
 * loudness state; and 132 bytes per tile of 8192 output samples for capacity_frames' samples / 8192 + max_live tiles).  An utterance of N
 * output samples owns N / 8192 + 1 tiles from its admission to its retirement: admission is all or nothing over slots, frames, phonemes
 * AND tiles (any one utterance that fits the empty frame pool fits the empty tile pool; a fragmented one may answer *admitted = 0).  Equality: every
 * slot's chunks equal its sts_infer_ids_stream chunks under the same settings, under the terms above.  The four setters (sts_set_eq,
 * sts_set_eq_streaming, sts_set_loudness, sts_set_loudness_streaming) return STS_ESTATE while the stream is open.
 *   sts_stream_get_loudness: the slots retired by the most recent sts_stream_step of a measuring stream, in ascending slot order: their
 *   count is returned, and min(count, capacity) entries are copied to slot_out / out (either may be NULL).  Each entry is what
 *   sts_get_loudness reports after a closed stream of that utterance -- one its callback stopped: over what was delivered.  0 after a step
 *   that retired nothing; STS_ESTATE with no stream open.  sts_get_loudness returns the same entries without the slots.
 *   Added without a new STS_ABI_VERSION: detect it by symbol. */
int sts_stream_get_loudness(sts_engine* e, int32_t* slot_out, sts_loudness* out, int64_t capacity);
/* Host only (no device), like sts_resample_table: the K-weighting above for rate in [8000, 48000] as float64 {b0, b1, b2, a1, a2} of the
 * shelf, then of the high-pass. */
int sts_kweight_coeffs(int32_t rate, double coeffs[10]);
/* The same kernels on caller signals: B float signals at `rate` packed back to back in x (host memory), lengths[b] samples each (0
 * allowed); out[b] receives the results defined above for the given target / ceiling. */
int sts_loudness_measure(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate,
                         float target_lufs, float peak_dbfs, sts_loudness* out);
/* ---- loudness in a stream (ABI number unchanged).  sts_set_loudness_streaming(e, 1) lets every streaming call (sts_infer_ids_stream,
 * sts_infer_ids_batch_stream, sts_infer_ids_joined_stream, the engine side of a streamed pool request) run under STS_LOUD_MEASURE; 0
 * (default) keeps the refusal above for modes 1 and 2, word for word, and sts_get_loudness then reports count 0 after a stream.  The
 * switch persists until changed; it has no effect in a whole-utterance call or under mode 0 (with it off, or under mode 0, a stream
 * allocates, uploads and launches exactly what it always did).  sts_get_loudness_streaming returns it (0 for a null engine).  Under
 * STS_LOUD_NORMALIZE a stream stays refused with the switch on as well: the gain needs the integrated loudness of the whole utterance
 * before its first sample leaves.  The remedy is a loop across calls: measure in a stream, then set the limiter's make-up gain
 * (sts_set_limiter) for the next calls of that voice.  sts_stream_halo_frames does not change.
 *   Definition: every chunk is the chunk of the same stream under mode 0, bit for bit (measuring never writes PCM).  Step k of utterance
 *   b consumes exactly the samples it delivers -- [j0, j1) at the output rate -- of the float signal loudness reads in a whole call: the
 *   nearest running float stage in front of it (tail, gain plan, join, resampler, or the streamed EQ's y when sts_set_eq_streaming is on).
 *   Samples a step re-presents below j0 or looks ahead to beyond j1 (the limiter's widened range) are not consumed.  After the call,
 *   sts_get_loudness returns B entries (a joined stream: 1, for the signal J); utterance b's entry is steps 1 to 5 and 7 above applied to
 *   x[0 .. e_b), e_b = the samples delivered.  For an utterance that ran to its end that is the whole call's entry (sts_infer_ids,
 *   sts_infer_ids_batch per utterance, sts_infer_ids_joined), bit for bit with the conv mode pinned and for EVERY chunk_frames: the kernels
 *   K-weight in chunks of 32 samples and tiles of 8192, both anchored at the utterance's first sample, the carry-in of a chunk depends
 *   only on its tile's carry and the chunks in front of it in that tile, and the engine keeps the open tile's carry and input per
 *   utterance and every tile's sums per call.  For an utterance whose callback stopped it, it is the measurement of what was delivered.
 *   gain is reported as in mode 1 of a whole call (under the limiter: g_L).  A step the engine decodes twice (the split-bf16 repeat)
 *   starts both times from the same state. */
int sts_set_loudness_streaming(sts_engine* e, int enable);
int sts_get_loudness_streaming(const sts_engine* e);
/* The stream-mode kernels on caller signals: signals, rate, target and ceiling as sts_loudness_measure.  bounds, n_steps and back follow
 * sts_eq_apply_chunked: bounds[0 .. n_steps) ascending step boundaries, bounds[0] = 0, common to all utterances; step k consumes
 * [bounds[k], bounds[k+1]) (the last one: to the end), clipped to each length, and an utterance with lengths[b] <= bounds[k] takes no
 * part in it.  back in [0, 2048]: step k presents the window [max(0, bounds[k] - back), min(lengths[b], bounds[k+1] + back)); only the
 * part behind the previous step's end and below bounds[k+1] is consumed.  out[B]: the final results.  partial (may be NULL; n_steps x B
 * entries): partial[k B + b] = the result as if the call had stopped behind step k, i.e. of x_b[0 .. min(lengths[b], bounds[k+1])) -- the
 * only place where the gate runs per step.  Malformed step lists: STS_EINVAL.  (On the device results, state, workspace and the tile
 * tables start out as NaN.) */
int sts_loudness_measure_chunked(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float target_lufs,
                                 float peak_dbfs, const int64_t* bounds, int32_t n_steps, int32_t back, sts_loudness* out,
                                 sts_loudness* partial);
/* ---- look-ahead peak limiter (ABI 13; no reference counterpart).  sts_set_limiter(e, mode, gain_db, ceiling_dbfs, lookahead_ms): mode
 * STS_LIMITER_OFF (0, default: nothing extra runs, PCM bit-identical to an engine that never set it) or STS_LIMITER_ON (1).  Valid:
 * gain_db in [-40, 40], ceiling_dbfs in [-30, 0], lookahead_ms in [0.25, 10]; NaN, anything outside, or an unknown mode: STS_EINVAL,
 * nothing changes.  The setting persists like sts_set_noise; sts_get_limiter_mode returns the four values.
 * The limiter works on the float wave at the output rate fs (the native wave at 16 kHz, else the resampler's output: the signal
 * loudness measures).  For one utterance x[0 .. N):
 *   1 Design (host, float64; exactly what sts_limiter_design returns): H = floor(lookahead_ms fs / 1000 + 0.5) (1 <= H <= 480),
 *     c = 10^(ceiling_dbfs / 20), G = 10^(gain_db / 20).
 *   2 Static gain g0 = float32(G g_loud) (one float64 product, rounded once); g_loud = 1, or under loudness mode 2 the utterance's
 *     loudness gain as float32.  While the limiter is on, step 5 of the loudness definition drops its peak clamp: g = g_L (the limiter
 *     holds the ceiling instead; sts_loudness.gain reports g_L, peak_dbfs is accepted and unused).  Loudness mode 1 is unchanged.
 *   3 v[n] = float32(x[n] g0); a[n] = |v[n]| as float64.
 *   4 Required gain in fixed point: q[n] = floor(min(1, c / a[n]) 2^30), division and product in float64 (a[n] <= c: q = 2^30; a[n]
 *     infinite or NaN: q = 0).  Outside the utterance (n < 0 or n >= N): q = 2^30.
 *   5 Sliding minimum: m[k] = min q[k - H .. k + H] for -H <= k < N + H.
 *   6 Sliding mean of the minimum, exact: S[n] = sum m[n - H .. n + H] in 64-bit integers; s[n] = float32(float64(S[n]) /
 *     float64((2H + 1) 2^30)).
 *   7 y[n] = float32(v[n] s[n]); pcm[n] = the reference's cast (int16)(int32)(y[n] * 32737).
 * Every window of step 6 contains a window of step 5 that contains n, so s[n] <= c / a[n] and |pcm| <= floor(32737 c) + 1: the cast never
 * wraps.  Where no sample within 2H exceeds the ceiling, s[n] = 1.0f exactly and y[n] = v[n].  y[n] depends on x[n - 2H .. n + 2H] only,
 * and steps 4-6 are integer arithmetic: an utterance's result is a function of its own samples, bit for bit.
 * Whole-utterance calls (sts_infer_ids, sts_infer_ids_batch, sts_run_batch) limit after the resampler and the loudness kernels; the tap
 * "wave_lim" is y ("wave" / "wave_out" stay the unlimited signals).  sts_get_limiter (conventions of sts_get_loudness; count 0 after a
 * call with the limiter off, a streaming call or a failure) returns per utterance: gain = g0, min_gain = min s[n] (1.0 when untouched),
 * peak_out = max |y[n]| over the samples whose y is not NaN, limited = the number of samples with S[n] < (2H + 1) 2^30.
 * Streaming (sts_infer_ids_stream, sts_infer_ids_batch_stream, sts_pool_submit_stream) is allowed with the limiter on while the loudness
 * mode is 0: a chunk that emits outputs [j0, j1) is limited from the float signal over [j0 - 2H, j1 + 2H) clipped to the utterance, so
 * the decode window grows and sts_stream_halo_frames reports the halo at the current rate and limiter setting.  Concatenated chunks
 * equal the whole-utterance PCM (bit for bit under a pinned conv mode: the streaming contract).  Streaming calls report no stats. */
#define STS_LIMITER_OFF 0
#define STS_LIMITER_ON 1
typedef struct sts_limiter_stats { float gain; float min_gain; float peak_out; int32_t limited; } sts_limiter_stats;
int sts_set_limiter(sts_engine* e, int mode, float gain_db, float ceiling_dbfs, float lookahead_ms);
int sts_get_limiter_mode(const sts_engine* e, int* mode, float* gain_db, float* ceiling_dbfs, float* lookahead_ms);
int sts_get_limiter(sts_engine* e, sts_limiter_stats* out, int64_t capacity);
/* Host only (no device), like sts_resample_table: step 1 above for rate in [8000, 48000]; each of H, c, G is set when non-null. */
int sts_limiter_design(int32_t rate, float gain_db, float ceiling_dbfs, float lookahead_ms, int32_t* H, double* c, double* G);
/* The same kernel on caller signals: B float signals at `rate` packed back to back in x (host memory), lengths[b] samples each (0
 * allowed), g_loud = 1.  y (float) and pcm (int16) receive the limited signals packed like x, stats[b] the results above; each of the
 * three may be NULL. */
int sts_limiter_apply(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, float gain_db, float ceiling_dbfs,
                      float lookahead_ms, float* y, int16_t* pcm, sts_limiter_stats* stats);
/* ---- duration plans (ABI 14; no reference counterpart: SynthesizerTrn::infer has one lengthScale per call).  sts_set_duration_plan(e, B, n,
 * plans) gives utterance b of the NEXT call (n[b] phonemes) the plan plans[b]; each field may be absent:
 *   rate [n[b]] or NULL      per-phoneme multiplier on the utterance's length_scale (SSML <prosody rate> over a span: rate = 1 / speed)
 *   fixed [n[b]] or NULL     >= 0: exactly this many frames (a <break time> on a pause phoneme); -1: predicted
 *   target_frames            0: none; > 0: the utterance is exactly this many frames (target_frames * samples_per_frame native samples) long
 * The plan is copied and applies to the next run only, whatever that run's outcome (the lifetime of forced durations), in every call form:
 * sts_infer_ids, sts_infer_ids_batch, sts_run_batch, sts_infer_ids_stream, sts_infer_ids_batch_stream.  That run must have the same B and
 * n[b]: otherwise it answers STS_EINVAL and nothing runs.  B == 0 or plans == NULL drops a pending plan.  A plan and forced durations both
 * pending at a run: STS_EINVAL, and both are dropped.  An utterance whose plan has all fields NULL / 0 is synthesised as without a plan, bit
 * for bit; a call with no plan pending launches and uploads nothing new.
 * Valid (checked at the set call; otherwise STS_EINVAL and nothing changes): rate finite and in [1/64, 64]; fixed in [-1, 100000];
 * target_frames 0 or in [1, 2^20]; with a target, target_frames - sum fixed >= #free (free: fixed < 0 or fixed == NULL), and with no free
 * phoneme sum fixed == target_frames.
 * For one utterance, lw_i the "logw" tap:
 *   1 u_i = expf(lw_i) * length_scale (fp32: the expression of a call without a plan).
 *   2 w_i = u_i * rate_i, one fp32 multiply (rate == NULL: w_i = u_i bit for bit).  The tap "dur_w" ([1][total phonemes]; recorded when taps
 *     are on and the run had a plan) is w.
 *   3 No target: d_i = fixed_i if fixed_i >= 0, else the clamp of a call without a plan: min(ceilf(w_i), 100000), 0 for NaN or w_i <= 0.
 *   4 Target F: fixed phonemes keep fixed_i.  R' = F - sum fixed - #free.  Each free phoneme gets d_i = 1 + a_i + e_i, in 64-bit integers:
 *       k_i = (int64) floorf(fminf(w_i, 4096.f) * 1048576.f); 0 when w_i is NaN or not above 0.
 *       K = sum k_i over the free phonemes; K == 0: every k_i = 1 and K = #free.
 *       a_i = (R' k_i) div K, r_i = (R' k_i) mod K (products below 2^54).  L = R' - sum a_i, so 0 <= L < #free.
 *       e_i = 1 for the L free phonemes that come first in the order (r_i descending, then i ascending), else 0.
 *     So sum d_i == F exactly, every free phoneme is heard (d_i >= 1), |d_i - 1 - R' k_i / K| < 1, and the result is a function of the
 *     utterance's own w only (not of its batch companions, its position, or the device).
 * A run with a plan neither reads nor feeds the launch-ahead memo (STS_DBG_LAUNCH_AHEAD).  From milliseconds: frames = round(ms * 16 /
 * samples_per_frame) at the model's 16 kHz. */
typedef struct sts_dur_plan {
    const float*   rate;          /* [n] or NULL: per-phoneme multiplier on the utterance's length_scale */
    const int32_t* fixed;         /* [n] or NULL: >= 0 exactly this many frames, -1 = predicted */
    int32_t        target_frames; /* 0 = none; > 0: the utterance is exactly this many frames long */
} sts_dur_plan;
int sts_set_duration_plan(sts_engine* e, int32_t B, const int32_t* n, const sts_dur_plan* plans);
/* Host only (no device), like sts_resample_table: steps 3-4 above on caller weights w[n] (fixed may be NULL; target_frames 0 = step 3).
 * STS_EINVAL for an invalid or infeasible plan (the rules above). */
int sts_duration_fit(const float* w, const int32_t* fixed, int32_t n, int32_t target_frames, int32_t* dur_out);
/* The same kernel on caller weights, like sts_limiter_apply: B utterances packed back to back in w (host memory), lengths[b] >= 1 weights
 * each; fixed (packed like w) and target_frames ([B]) may be NULL.  dur_out receives the durations packed like w. */
int sts_duration_plan_apply(int device, const float* w, const int32_t* fixed, const int32_t* lengths, int32_t B,
                            const int32_t* target_frames, int32_t* dur_out);
/* Phoneme start offsets of the last run in output samples, packed like sts_get_durations (same count, same capacity convention): phoneme i
 * with f frames before it in its utterance starts at ceil(f * samples_per_frame * P / Q) at the current output rate (sts_set_output_rate; f *
 * samples_per_frame at the native rate) -- the convention of a streaming chunk's sample_offset.  Host arithmetic; after any call form, with
 * or without a plan.  After sts_infer_ids_joined the positions are those in the joined output (see there). */
int sts_get_phoneme_offsets(sts_engine* e, int64_t* start, int64_t capacity);
/* ---- speaker blending (no reference counterpart: SynthesizerTrn::infer takes one sid, a row of emb_g).  sts_set_speaker_mix(e, B, mixes)
 * gives utterance b of the NEXT call the conditioning vector g of mixes[b] instead of row sid[b] of the model's table.  With
 * E[s][c] = emb_g[c * speaker_num + s] (the blob's layout, [gin_channels][speaker_num]) and gin = gin_channels, for every channel c:
 *     acc_c = 0.0 (float64)
 *     for k = 0 .. K-1 in order:  acc_c += (double)weight[k] * (double)E[sid[k]][c]
 *     if vector != NULL:          acc_c += (double)vector_weight * (double)vector[c]
 *     g_c = (float)acc_c          (one rounding, to nearest even)
 * Each product of two fp32 values is exact in float64, so the result does not depend on whether the compiler contracts to an FMA.
 * K = 1, weight = 1, vector = NULL gives g = E[sid[0]] exactly: the plain-sid result, bit for bit.  K = 0, vector_weight = 1 gives g = vector
 * exactly.  Weights are used as given: not normalised, negative weights (an extrapolation) allowed.  Denormal results are not part of the
 * contract.
 * The mix is copied and applies to the next run only, whatever that run's outcome (the lifetime of a duration plan), in every call form:
 * sts_infer_ids, sts_infer_ids_batch, sts_run_batch, sts_infer_ids_stream, sts_infer_ids_batch_stream.  That run must have the same B:
 * otherwise it answers STS_EINVAL, nothing runs and the mix is dropped.  B == 0 or mixes == NULL drops a pending mix.  An invalid mix (the
 * rules in the struct below; sts_speaker_mix_check) answers STS_EINVAL at the set call and changes nothing; a single-speaker model answers
 * STS_EINVAL for any non-empty mix.  An utterance whose entry is empty (k == 0, vector == NULL) is synthesised with its sid[b] as without a
 * mix, bit for bit; a call with no mix pending launches and uploads nothing new.  A mixed call launches the blend kernel in place of the
 * speaker gather and its term table rides in the run's one upload.  A mix is independent of forced durations, duration plans, noise,
 * output rate, loudness and limiter; a run with a mix neither reads nor feeds the launch-ahead memo (STS_DBG_LAUNCH_AHEAD). */
typedef struct sts_speaker_mix {
    int32_t        k;              /* 0..16 table terms; k == 0 and vector == NULL: no mix, the call's sid[b] applies */
    const int32_t* sid;            /* [k] rows, each in [0, speaker_num) -- out of range is STS_EINVAL here, not "-> 0" */
    const float*   weight;         /* [k] finite, |w| <= 16 */
    const float*   vector;         /* NULL or [gin_channels] finite: a caller's own embedding */
    float          vector_weight;  /* finite, |w| <= 16; read only when vector != NULL */
} sts_speaker_mix;
int sts_set_speaker_mix(sts_engine* e, int32_t B, const sts_speaker_mix* mixes);
/* Host only (no device): the validity rules above for B entries against a table of speaker_num rows of gin floats (speaker_num 0 = a
 * single-speaker model: only empty entries pass). */
int sts_speaker_mix_check(int32_t speaker_num, int32_t gin, int32_t B, const sts_speaker_mix* mixes);
/* Row sid of the model's table as gin_channels floats (what a mix with k = 1, weight 1 produces).  STS_EINVAL: a single-speaker model, sid
 * outside [0, speaker_num), capacity below gin_channels. */
int sts_get_speaker_embedding(const sts_engine* e, int32_t sid, float* out, int64_t capacity);
/* The same kernel on a caller's table (host memory, the blob's layout [gin][speaker_num]), like sts_limiter_apply: g_out [B][gin] receives
 * utterance b's vector.  sid ([B] or NULL = all 0): the row an EMPTY entry takes (outside [0, speaker_num) -> 0, as a plain call);
 * mixes == NULL: every entry is empty. */
int sts_speaker_blend(int device, const float* table, int32_t speaker_num, int32_t gin, int32_t B, const int32_t* sid,
                      const sts_speaker_mix* mixes, float* g_out);
/* ---- gain plans (no reference counterpart: SynthesizerTrn::infer has no volume control).  sts_set_gain_plan(e, B, n, plans) gives utterance b
 * of the NEXT call (n[b] phonemes) the plan plans[b]: a gain per phoneme and the width of the transition across a phoneme boundary -- SSML
 * <prosody volume> and <emphasis> over a span, ducking, muting one word.
 * Valid (checked at the set call; otherwise STS_EINVAL and nothing changes): gain_db[i] is -INFINITY or finite in [-96, 24]; ramp_ms is
 * finite and in [0, 50]; NaN anywhere is invalid.
 * For one utterance, with the run's final durations d_i (after forced durations or a duration plan, if any) and hop = samples_per_frame:
 * F = max(1, sum d_i) frames, N = F hop native samples, x[0 .. N) the decoder's float wave at the native 16 kHz (the tap "wave").
 *   1 Design (host, float64; exactly what sts_gain_design returns): q_i = floor(10^(gain_db_i / 20) 2^20 + 0.5) as int32, q_i = 0 for
 *     -INFINITY, q_i = 2^20 when gain_db == NULL; h = floor(ramp_ms 8 + 0.5), so 0 <= h <= 400: the transition is 2h + 1 native samples wide.
 *   2 Step function: Q[t] = q_i for the phoneme i whose span [s_i hop, (s_i + d_i) hop) contains t, s_i = sum_{j < i} d_j.  A phoneme with
 *     d_i = 0 owns nothing.  A sample no phoneme owns (the single frame of an utterance whose durations are all 0) has Q = 2^20.  Outside
 *     the utterance Q[t] = Q[0] for t < 0 and Q[N - 1] for t >= N: no fade at the edges.
 *   3 Sliding sum, exact: S[t] = sum Q[t - h .. t + h] in 64-bit integers (S < 2^34; the same in any evaluation order).
 *   4 Envelope: env[t] = float32(float64(S[t]) / float64((2h + 1) 2^20)).
 *   5 y[t] = x[t] * env[t], one fp32 multiply.  Where every Q of the window is 2^20, env = 1.0f exactly and y[t] = x[t] bit for bit.
 * y replaces x as the input of everything downstream: decoder wave -> gain envelope -> resampler -> loudness -> limiter -> cast.  With
 * nothing downstream (native rate, loudness mode 0 or 1, limiter off) the gain kernel writes the PCM itself with the reference's cast
 * (int16)(int32)(y * 32737).  A positive gain can take |y| past 1.0009, where that cast wraps around as the reference's does: the limiter
 * (sts_set_limiter) is the remedy.
 * Taps: "wave" stays the un-gained signal; "wave_gain" is y (recorded only by a one-pass run that had a plan); "wave_out" and "wave_lim"
 * are computed from y.
 * The plan is copied and applies to the next run only, whatever that run's outcome (the lifetime of a duration plan), in every call form:
 * sts_infer_ids, sts_infer_ids_batch, sts_run_batch, sts_infer_ids_stream, sts_infer_ids_batch_stream.  That run must have the same B and
 * n[b]: otherwise it answers STS_EINVAL, nothing runs and the plan is dropped.  B == 0 or plans == NULL drops a pending plan.  An utterance
 * whose entry has gain_db == NULL is synthesised as without a plan, bit for bit; a call with no plan pending launches, allocates and uploads
 * nothing new.  A planned call launches one kernel behind the decoder's last one; its q table rides in the run's one upload, and nothing
 * waits on the host: the durations stay on the device.  The plan is independent of forced durations, duration plans, speaker mixes, noise,
 * output rate, loudness, limiter and conv math (the split-bf16 repeat of a call applies the same plan again); a run with a gain plan
 * neither reads nor feeds the launch-ahead memo (STS_DBG_LAUNCH_AHEAD).
 * Streaming: a window's decoded native samples are gained at their absolute positions t before the resampler or the limiter reads them,
 * the halo samples those two read beyond a chunk included.  The envelope is pointwise in t: sts_stream_halo_frames does not change, and
 * concatenated chunks equal the whole-utterance PCM (bit for bit under a pinned conv mode, within 1 LSB otherwise). */
typedef struct sts_gain_plan {
    const float* gain_db;   /* [n] or NULL: per-phoneme gain in dB; -INFINITY = mute */
    float        ramp_ms;   /* width of the transition across a phoneme boundary */
} sts_gain_plan;
int sts_set_gain_plan(sts_engine* e, int32_t B, const int32_t* n, const sts_gain_plan* plans);
/* Host only (no device): the validity rules above for B plans of n[b] >= 1 phonemes each. */
int sts_gain_plan_check(int32_t B, const int32_t* n, const sts_gain_plan* plans);
/* Host only (no device), like sts_limiter_design: step 1 above for one utterance of n >= 1 phonemes (gain_db may be NULL); each of q ([n])
 * and h is set when non-null.  STS_EINVAL for an invalid plan. */
int sts_gain_design(const float* gain_db, int32_t n, float ramp_ms, int32_t* q, int32_t* h);
/* The same kernel on caller signals, like sts_limiter_apply: B float signals packed back to back in x (host memory); utterance b has
 * lengths[b] >= 1 phonemes with the durations dur_frames (>= 0, packed for the whole batch) and its signal is max(1, sum d)
 * samples_per_frame samples long (samples_per_frame >= 1; B <= 65535).  y (float) and pcm (int16) receive the gained signals packed like x; each may
 * be NULL. */
int sts_gain_plan_apply(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                        const sts_gain_plan* plans, float* y, int16_t* pcm);
/* ---- pitch plans (no reference counterpart: VITS has no F0 input).  sts_set_pitch_plan(e, B, n, plans) gives utterance b of the NEXT call
 * (n[b] phonemes) a pitch shift per phoneme in cents -- SSML <prosody pitch> over a span -- by a time warp: a phoneme shifted by the ratio
 * r = 2^(cents / 1200) is synthesised r times as long and read back r times as fast through a band-limited interpolator.  Its duration
 * stays, its pitch is multiplied by r.  THE FORMANTS MOVE WITH THE PITCH (the spectral envelope is scaled by r like everything else: a
 * large upward shift sounds smaller / younger, a downward one larger); that is why the range ends at +-600 cents.  A formant-preserving
 * shift is not offered.
 * Valid (checked at the set call; otherwise STS_EINVAL and nothing changes): every cents[i] in [-600, 600].
 * For one utterance, with the run's final durations d_i, hop = samples_per_frame, F = max(1, sum d_i) frames, N = F hop < 2^30 native
 * samples, x[0 .. N) the float wave the warp reads (the gain plan's output if one ran, otherwise the decoder's):
 *   1 Design (host, float64; exactly what sts_pitch_design returns): ratio_i = (float) 2^(cents_i / 1200); step_i = floor(2^(cents_i /
 *     1200) 2^32 + 0.5) as int64, the input samples per output sample in Q32.  step(0) = 2^32.
 *   2 Duration compensation: the run behaves as a run with a duration plan whose rate_i is the pending duration plan's rate_i (1.0f
 *     without one) times ratio_i, one fp32 multiply on the host; all cents 0 multiply by 1.0f, so the durations are those of a call
 *     without a pitch plan.  A phoneme with fixed_i >= 0 must have cents_i == 0 (breaks are silent), and a duration plan with
 *     target_frames > 0 admits no non-zero cents: otherwise the run answers STS_EINVAL.  FORCED DURATIONS (sts_set_forced_durations) ARE
 *     USED AS GIVEN AND NOT COMPENSATED: the caller who forces d_i states the length of the span that is then read r_i times as fast.
 *   3 Layout (exact, 64-bit integers; sts_pitch_layout): o_0 = 0, e_0 = 0, L_i = (d_i hop) << 32; n_i = L_i > e_i ?
 *     ceil((L_i - e_i) / step_i) : 0; e_i+1 = e_i + n_i step_i - L_i; o_i+1 = o_i + n_i.  Output j in [o_i, o_i+1) sits at the Q32 position
 *     pos = (a_i << 32) + e_i + (j - o_i) step_i, a_i = hop sum_{k < i} d_k.  The warped length is N' = o_n.  A phoneme shorter than the
 *     step that reaches it emits nothing (n_i = 0) and e carries on.  An utterance whose durations are all 0: the one frame nobody owns
 *     takes step 2^32, so N' = hop.
 *   4 Filter, one prototype for every ratio (Smith's band-limited interpolation; exactly what sts_pitch_table returns):
 *     h0[k] = float32(sinc(k / 512) I0(10 sqrt(1 - (k / 16384)^2)) / I0(10)), k = 0 .. 16383; h0[16384] = h0[16385] = 0 (float64, rounded
 *     once).  For output j: n0 = pos >> 32, f = (pos & 0xffffffff) / 2^32, rho = step_i / 2^32, c = 0.9 min(1, 1 / rho), K = ceil(32 / c)
 *     <= 51.  Tap m in [0, 2K) reads x[n0 - K + 1 + m] -- 0 outside [0, N), never a batch neighbour -- with dd = f + K - 1 - m,
 *     t = 512 c |dd|, k = floor(t), g_m = h0[k] + (t - k) (h0[k + 1] - h0[k]) (0 when k >= 16384).
 *     y_j = float32(sum g_m x_m / sum g_m): coefficients, both sums (m ascending) and the division in float64.
 *   5 An utterance whose entry has cents == NULL in a run that has a plan is copied bit for bit (y = x, N' = N); one with cents is
 *     filtered everywhere, also where cents are 0.
 * An output's value depends on its utterance alone: not on batch companions, the position in the packed buffer or the tile.
 * PCM is the reference's cast (int16)(int32)(y * 32737) of y_j.
 * The warp runs at the native rate directly behind the gain kernel: decoder wave -> gain envelope -> warp -> resampler -> EQ -> loudness
 * -> limiter -> cast.  Everything behind it sees utterance b as N'_b native samples: the returned counts are ceil(N'_b P / Q), and
 * sts_get_phoneme_offsets answers ceil(o_i P / Q).  Taps: "wave" and "wave_gain" stay the unwarped signals, "wave_pitch" is the warped one
 * (all utterances back to back), "wave_out" / "wave_eq" / "wave_lim" are computed from it.
 * The plan is copied and applies to the next run only, whatever that run's outcome (the lifetime of a gain plan): sts_infer_ids,
 * sts_infer_ids_batch, sts_run_batch, sts_pool_submit_pitch, sts_multi_set_pitch_plan.  That run must have the same B and n[b]: otherwise
 * it answers STS_EINVAL, nothing runs and the plan is dropped.  B == 0 or plans == NULL drops a pending plan.  A run with a pitch plan is
 * never launched ahead and neither reads nor feeds the launch-ahead memo; its layout is made on the host when the durations arrive (they
 * come with the frame counts) and uploaded without a further wait; the split-bf16 repeat of a call applies the same plan again.  A call
 * with no plan pending launches, allocates and uploads nothing new.
 * NOT AVAILABLE with a plan pending -- each answers STS_EINVAL, runs nothing and drops the plan: sts_infer_ids_stream and
 * sts_infer_ids_batch_stream (unless sts_set_pitch_streaming is on, below), sts_stream_open / sts_stream_open_ex, sts_stream_admit, sts_infer_ids_joined, sts_infer_ids_joined_stream,
 * sts_para_open, sts_para_append (while a paragraph or an unplanned stream is open the setter itself answers STS_ESTATE).
 * Added without a new STS_ABI_VERSION: detect the entries by symbol. */
typedef struct sts_pitch_plan {
    const int32_t* cents;   /* [n] or NULL: per-phoneme shift in cents, each in [-600, 600] */
} sts_pitch_plan;
int sts_set_pitch_plan(sts_engine* e, int32_t B, const int32_t* n, const sts_pitch_plan* plans);
/* Host only (no device): the validity rules above for B plans of n[b] >= 1 phonemes each. */
int sts_pitch_plan_check(int32_t B, const int32_t* n, const sts_pitch_plan* plans);
/* Host only: step 1 for one utterance of n >= 1 phonemes (cents == NULL: ratio 1.0f, step 2^32); each of ratio ([n]) and step ([n]) is set
 * when non-null.  STS_EINVAL for an invalid plan. */
int sts_pitch_design(const int32_t* cents, int32_t n, float* ratio, int64_t* step);
/* Host only: step 3 for one utterance: out_start[0 .. n] = o_i and resid[0 .. n] = e_i, each set when non-null (the all-zero utterance
 * answers o_n = 0 here: the hop samples of step 4's rule belong to no phoneme).  STS_EINVAL: n < 1, a duration outside [0, 100000], a
 * step outside [step(-600), step(600)], samples_per_frame outside [1, 2^20], or max(1, sum d) samples_per_frame >= 2^30. */
int sts_pitch_layout(const int32_t* dur_frames, const int64_t* step, int32_t n, int32_t samples_per_frame, int64_t* out_start, int64_t* resid);
/* Host only: the prototype h0 of step 4, 16386 floats (a smaller capacity answers STS_EINVAL). */
int sts_pitch_table(float* table, int64_t capacity_floats);
/* The warp kernel on caller signals, like sts_gain_plan_apply: B float signals packed back to back in x (host memory); utterance b has
 * lengths[b] >= 1 phonemes with the durations dur_frames (packed for the whole batch) and its signal is max(1, sum d) samples_per_frame
 * samples long (B <= 65535).  out_len[b] (optional) receives N'_b; y (float) and pcm (int16) receive the warped signals packed back to back
 * by N'_b, each may be NULL (both NULL: only out_len is computed, on the host).  capacity: the samples y and pcm have room for; a smaller
 * one than sum N'_b answers STS_EINVAL with out_len set. */
int sts_pitch_apply(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                    const sts_pitch_plan* plans, int64_t* out_len, float* y, int16_t* pcm, int64_t capacity);
/* Lab (tools/pitch_cost.py): sts_pitch_apply's float output with the prototype read from global memory (table_in_lds 0) or staged in
 * LDS (1), then iters >= 1 more launches between two events: *ms_out = their mean time in milliseconds. */
int sts_debug_pitch_bench(int device, const float* x, const int32_t* dur_frames, const int32_t* lengths, int32_t B, int32_t samples_per_frame,
                          const sts_pitch_plan* plans, float* y, int64_t capacity, int32_t table_in_lds, int32_t iters, float* ms_out);
/* ---- a pitch plan in a stream (ABI number unchanged: detect the entries by symbol).  The warp's layout is exact integer arithmetic on
 * durations that are known before a stream's first step, and output j depends on nothing but j and its taps: so a chunk of decoder frames
 * maps to a range of warped outputs.  sts_set_pitch_streaming(e, 1) lets sts_infer_ids_stream and sts_infer_ids_batch_stream run with a
 * plan pending: the steps and the chunk grid are those of a duration-planned stream with the compensated rates, every step warps its
 * decode windows with the range form of the warp kernel, and the concatenated chunks of utterance b are the PCM of sts_infer_ids /
 * sts_infer_ids_batch with the same plan bit for bit (under a pinned conv mode, as for every stream), for every chunk size, at every
 * output rate, with the limiter, a gain plan, a duration plan, a speaker mix and sampling noise.  The callback's n and first-output index,
 * delivered[b] and sts_get_phoneme_offsets carry the warped counts at the output rate; a chunk that owns no output (possible when a chunk
 * is a single sample) is not delivered.  sts_stream_halo_frames reports the larger halo of such a stream while a plan is pending:
 * dec_halo + ceil((ceil(extra step(+600) / 2^32) + 52) / hop), extra = the resampler's K plus the limiter's reach in native samples.
 * Off by default and persistent; STS_ESTATE while a stream or a paragraph is open.  With the switch off every call does what it did.  With
 * it on and a plan pending, a stream still answers STS_EINVAL, runs nothing and drops the plan while the streamed EQ has bands set
 * (sts_set_eq_streaming), streamed loudness measures (sts_set_loudness_streaming under mode 1) or record taps are on; and every other
 * form of the NOT AVAILABLE list above refuses as before: open streams, joined runs and joined streams, open paragraphs, the pool's
 * streaming requests and sts_multi_*.
 * With pos(j) the Q32 position of step 3 (strictly increasing; a member without a plan: j << 32),
 *   Y(f) = #{j : pos(j) < (f hop) << 32}, Y(F) = N';
 * chunk k of an utterance of F frames, C = chunk_frames, owns the warped outputs [Y(k C), Y(min(F, (k + 1) C))) and, at the output rate
 * P / Q, the samples [ceil(Y(k C) P / Q), ceil(Y(min(F, (k + 1) C)) P / Q)) of ceil(N' P / Q): the chunks partition the signal in order.
 * sts_pitch_chunk_starts (host only) returns the number of chunks ceil(F / C) -- or a negative STS_E* code -- and, when out_first is
 * non-null, out_first[k] = Y(k C) for every chunk and out_first[chunks] = N' (capacity below chunks + 1: STS_EINVAL).  step == NULL is the
 * member without a plan (Y(f) = f hop); otherwise the steps of sts_pitch_design.  Arguments as sts_pitch_layout. */
int sts_set_pitch_streaming(sts_engine* e, int enable);
int sts_pitch_chunk_starts(const int32_t* dur_frames, const int64_t* step, int32_t n, int32_t samples_per_frame, int32_t chunk_frames,
                           int64_t* out_first, int64_t capacity);
/* The range form of the warp kernel on caller data: what a step of a stream through the warp launches.  The batch (dur_frames, lengths, B,
 * samples_per_frame, plans) is sts_pitch_apply's and fixes every utterance's layout.  Window i computes the outputs [y0, y1) of utterance
 * utt from the native samples [u0, u0 + xlen) of that utterance, which stand at x[xbase .. xbase + xlen) of the caller's buffer of x_len
 * floats; the kernel reads nothing else of x and takes every other sample of the utterance as 0.  The window must therefore cover the span
 * its outputs read, clipped to the utterance: [max(0, n0(y0) - 50), min(N, n0(y1 - 1) + 52)) with n0 of step 4 (an utterance without a
 * plan: [y0, y1) itself) -- otherwise STS_EINVAL, as for a window outside x or outside [0, N), a range outside [0, N'], n_win outside
 * [1, 65535] or a capacity below sum (y1 - y0).  y (float) and pcm (int16) receive the ranges packed back to back in window order, each
 * may be NULL.  Every sample equals sts_pitch_apply's sample j of that utterance bit for bit. */
typedef struct sts_pitch_range {
    int32_t utt;            /* the utterance of the batch, [0, B) */
    int64_t xbase;          /* where the window's first sample stands in x */
    int64_t u0, xlen;       /* the window: native samples [u0, u0 + xlen) of the utterance */
    int64_t y0, y1;         /* the warped outputs to compute */
} sts_pitch_range;
int sts_pitch_apply_range(int device, const float* x, int64_t x_len, const int32_t* dur_frames, const int32_t* lengths, int32_t B,
                          int32_t samples_per_frame, const sts_pitch_plan* plans, const sts_pitch_range* win, int32_t n_win, float* y,
                          int16_t* pcm, int64_t capacity);
/* ---- paragraph synthesis (no reference counterpart: SynthesizerTrn::infer runs a whole line as ONE utterance, at quadratic attention cost and
 * without batching).  sts_infer_ids_joined runs B sentences as exactly the packed batch sts_infer_ids_batch would run and joins their float
 * waves on the device into ONE signal -- in front of the resampler, loudness, the limiter and the cast, which then see the paragraph as the
 * single utterance it is: one loudness gain, a limiter look-ahead and resampler taps that reach across the joins, faded sentence edges.
 * Native 16 kHz float domain, exact; hop = samples_per_frame.  Sentence b has F_b = max(1, sum d) frames and the native float wave
 * x_b[0 .. N_b), N_b = F_b hop: the tap "wave_gain" if a gain plan applies, else "wave".
 * Valid (checked before anything runs; otherwise STS_EINVAL and nothing changes): B >= 1; every gap, lead_frames and trail_frames in
 * [0, 100000]; fade_ms finite and in [0, 50] (NaN is invalid).  From milliseconds: frames = round(ms * 16 / samples_per_frame), the
 * convention of the duration plans.
 *   1 Design (host): h = floor(fade_ms * 16 + 0.5), so 0 <= h <= 800.
 *   2 Layout (host, 64-bit): start_0 = lead_frames hop; start_{b+1} = start_b + N_b + gap_b hop; N_J = start_{B-1} + N_{B-1} + trail_frames hop.
 *     Every start_b and N_J is a multiple of hop; F_J = N_J / hop.  (sts_join_layout returns exactly this.)
 *   3 Envelope of sentence b at local t in [0, N_b): e_b[t] = float32(float64(min(t + 1, N_b - t, h + 1)) / float64(h + 1)): a linear
 *     fade-in over the first h samples and fade-out over the last h.  h = 0 gives 1.0f everywhere; a sentence shorter than 2h simply
 *     never reaches 1.
 *   4 Joined signal: J[start_b + t] = x_b[t] * e_b[t], one fp32 multiply; where e = 1.0f the sample is x_b[t] bit for bit.  Every other
 *     J[t] is +0.0f.
 *   5 Downstream J is ONE utterance of F_J frames: the resampler gives L_out = ceil(N_J P / Q) samples, loudness one measurement and one
 *     gain, the limiter one set of stats, and the cast comes last.  With nothing downstream (native rate, loudness mode 0 or 1, limiter
 *     off) the join kernel writes the PCM itself with the reference's cast (int16)(int32)(J * 32737).  N_J > 2 10^9 or L_out > 2^31 - 1
 *     answers STS_EINVAL before the decoder runs.
 * The join is one kernel launch behind the decoder's last one (behind the gain kernel when a gain plan applies); it writes the silence
 * too (no memset), and its B-entry table rides in the run's one upload.  A call without a join launches, allocates and uploads nothing
 * new. */
typedef struct sts_join {
    const int32_t* gap_frames;   /* [B-1] or NULL (= all 0): silence between sentence b and b+1, in frames */
    int32_t lead_frames, trail_frames;   /* silence in front of the first / behind the last sentence, in frames */
    float   fade_ms;             /* edge fade of every sentence */
} sts_join;
/* Host only (no device): the validity rules above (join == NULL = all zeros: only B is checked). */
int sts_join_check(int32_t B, const sts_join* join);
/* Host only (no device): steps 1-2 above for B sentences of frames[b] >= 1 frames of samples_per_frame >= 1 samples each.  start ([B], native
 * samples), total (N_J) and h are each set when non-null.  STS_EINVAL for an invalid join or frame count. */
int sts_join_layout(int32_t B, const int32_t* frames, int32_t samples_per_frame, const sts_join* join, int64_t* start, int64_t* total,
                    int32_t* h);
/* The same kernel on caller signals, like sts_gain_plan_apply: B float signals of frames[b] samples_per_frame samples packed back to back
 * in x (host memory; at most 2^30 samples in x and in J).  y (float) and pcm (int16) receive J and its cast, N_J samples each; each may be
 * NULL.  On the device both start out as a NaN / 0x7FFF pattern, so a sample the kernel did not write shows. */
int sts_join_apply(int device, const float* x, const int32_t* frames, int32_t B, int32_t samples_per_frame, const sts_join* join, float* y,
                   int16_t* pcm);
/* The B sentences as the packed batch of sts_infer_ids_batch -- the same sid rule, noise seed + b, forced durations, and a pending
 * duration plan, speaker mix or gain plan applied per sentence (their B and n[b] must match, as for any call) -- joined as defined above.
 * *pcm_out is ONE malloc()'d buffer of *n_out = L_out samples.  join == NULL means all zeros: the sentences back to back, no fade.  The
 * call neither reads nor feeds the launch-ahead memo (STS_DBG_LAUNCH_AHEAD).  B == 1 with an all-zero join returns sts_infer_ids' PCM bit
 * for bit.
 * Afterwards: sts_get_durations is unchanged (packed per phoneme); sts_get_phoneme_offsets reports positions in the joined output, phoneme
 * i of sentence b with f frames before it in its sentence at ceil((start_b + f hop) P / Q); sts_get_join_offsets the sentence starts
 * ceil(start_b P / Q); sts_get_loudness and sts_get_limiter report count 1.  Taps: "wave" and "wave_gain" stay per sentence (packed);
 * "wave_join" is J; "wave_out" and "wave_lim" are computed from J.
 * The streaming form is sts_infer_ids_joined_stream below.  Out of scope: sts_multi_*, and per-request plans through the pool. */
int sts_infer_ids_joined(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                         const float* length_scale, const sts_join* join, int16_t** pcm_out, int32_t* n_out);
/* Sentence starts of the last call in output samples, ceil(start_b P / Q): [B] entries (capacity below B: STS_EINVAL).  STS_ESTATE when the
 * last call was not a joined one. */
int sts_get_join_offsets(sts_engine* e, int64_t* start, int64_t capacity);
/* The joined signal of sts_infer_ids_joined, streamed: chunked PCM of the ONE signal, in order.
 *   Front, duration predictor and flow run once as the packed batch of B, exactly as in sts_infer_ids_joined: the same sid rule, noise
 *   seed + b and forced durations; a pending duration plan, speaker mix or gain plan applies per sentence.
 *   Layout: sts_join_layout's start_b, N_J, F_J = N_J / hop and h.  N_J > 2 10^9 or L_out > 2^31 - 1 answers STS_EINVAL before the decoder
 *   runs, as there.
 *   Chunks: with C = chunk_frames, step k delivers the frames [k C, min((k + 1) C, F_J)) of the JOINED signal -- at the output rate the
 *   samples [ceil(k C hop P / Q), ceil(min((k + 1) C, F_J) hop P / Q)); sample_offset is the first of them.  There are exactly
 *   ceil(F_J / C) callbacks, in order, one per step; a step that lies wholly in silence is one of them (and launches no decoder kernel).
 *   A non-zero return ends the call with STS_OK; *n_total (optional) is the samples delivered.  `pcm` is only valid inside the callback.
 *   Each step decodes, of every sentence within reach of the chunk, one window (the chunk, the resampler's and limiter's reach, the
 *   decoder's halo), joins the windows into a window of J and runs resampler and limiter on J as one utterance: the decoder workspace is
 *   bounded by the chunk, not by the paragraph.
 *   Equality: the concatenated chunks equal sts_infer_ids_joined's PCM of the same call bit for bit when the kernel variant is pinned
 *   (sts_set_conv_mode), and agree within 1 LSB under the automatic choice -- the streaming contract of sts_infer_ids_stream.  With
 *   B == 1 and an all-zero join the chunks equal sts_infer_ids_stream's.
 *   The limiter may be on: the chunks concatenate to the whole joined PCM, and its look-ahead reaches across the joins.  Loudness mode
 *   != 0 or EQ bands set answers STS_EINVAL, as for every stream.
 *   B < 1, chunk_frames <= 0, a NULL callback, NULL ids / n or an invalid join answers STS_EINVAL: nothing runs and nothing changes.
 *   Afterwards sts_get_join_offsets, sts_get_phoneme_offsets and sts_get_durations answer as after sts_infer_ids_joined.
 *   Conv math 3: the overflow word follows sts_infer_ids_batch_stream's rule -- raised at step 0 the whole call is repeated in the
 *   split-bf16 form, raised later that step and the steps after it are decoded in that form, and no chunk leaves twice
 *   (STS_DBG_STREAM_RETRY_STEP applies).  The call neither reads nor feeds the launch-ahead memo. */
int sts_infer_ids_joined_stream(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                                const float* length_scale, const sts_join* join, int32_t chunk_frames, sts_chunk_cb cb, void* user,
                                int32_t* n_total);
/* The windowed join kernel of a joined stream on caller signals, like sts_join_apply: y (float) and pcm (int16) receive
 * J[first_frame hop, (first_frame + n_frames) hop) and its cast, n_frames samples_per_frame samples each; each may be NULL.  The range must lie
 * inside [0, F_J) with n_frames >= 1.  Only the parts of each sentence inside the range are uploaded, packed compactly, with the window
 * table the engine's step builds.  On the device both outputs start out as a NaN / 0x7FFF pattern, as in sts_join_apply. */
int sts_join_apply_range(int device, const float* x, const int32_t* frames, int32_t B, int32_t samples_per_frame, const sts_join* join,
                         int64_t first_frame, int64_t n_frames, float* y, int16_t* pcm);
/* Open paragraphs: a joined stream whose sentences are appended while it plays (a service that voices a language model's output gets its
 * text sentence by sentence).  One per engine; nothing here is on by default.  Every delivered chunk is a chunk of the ONE joined signal
 * J that sts_infer_ids_joined_stream would deliver for the finished paragraph: the same chunk grid, the same faded edges, one limiter,
 * resampler taps that reach across the joins, offsets on one time axis.
 *   sts_para_open fixes C = chunk_frames, the output rate, the limiter setting, the conv mode and the conv math, and the join's
 *   lead_frames and fade_ms (sts_join_check's rules), and allocates a latent pool of capacity_frames frames for at most max_resident
 *   sentences at a time, under sts_stream_open's bounds.  STS_ESTATE while an open stream or an open paragraph exists (and while a
 *   paragraph is open sts_stream_open answers STS_ESTATE too); STS_EINVAL under the conditions that make sts_stream_open refuse.
 *   sts_para_append runs text encoder, duration predictor and flow of the B new sentences as the packed batch a joined call of those B
 *   would, and moves their latents into the pool.  gap_frames[b] (NULL = zeros, each in [0, 100000]) is the silence between the sentence
 *   before and sentence b; for the paragraph's first sentence it must be 0 (the lead was given at open).  The layout is sts_join_layout's,
 *   continued: the sentence with global index i starts at start_i = start_{i-1} + N_{i-1} + gap hop and has F_i = max(1, sum d) frames.
 *   frames_out[b] = its frames, start_out[b] = its start in output samples, ceil(start P / Q) (sts_get_join_offsets' rule); both may be
 *   NULL, as may sid and length_scale (0 and 1.0).  Sampling noise: global sentence i uses seed + i, the setting read at every append.
 *   All or nothing: *appended = B, or 0 when slots or frames do not suffice now (nothing has changed; retry after steps have retired
 *   sentences) or the paragraph was stopped.  STS_EINVAL: an append that would carry N_J past 2 10^9 native samples or L_out past
 *   2^31 - 1, B > max_resident, bad arguments, an append after finish.
 *   sts_para_finish: no more sentences will come; F_J = the end of the last sentence + trail_frames.  STS_EINVAL with no sentence
 *   appended, twice, or with trail_frames outside [0, 100000].
 *   sts_para_step is ONE step: the next chunk of J, if it is deliverable, decoded as the closed joined stream's step decodes it and handed
 *   to `cb` before the call returns.  With Ho = the resampler's and limiter's reach in frames (sts_stream_halo_frames minus the decoder's
 *   own halo) and E = the end of the last sentence appended so far, chunk k = frames [k C, (k + 1) C) is deliverable before finish iff
 *   (k + 1) C + Ho <= E; after finish every remaining chunk is, the short last one included.  So a stalled writer costs at most C + Ho
 *   frames of withheld audio behind the last sentence.  *ready_after (may be NULL) = chunks deliverable now without a further append.
 *   With nothing deliverable it launches nothing and delivers nothing.  A silent chunk (lead, a known gap) leaves without a decode.  A
 *   non-zero callback return stops the paragraph: later steps and appends do nothing, only sts_para_info and sts_para_close remain useful.
 *   A sentence's slot and frames become free once no later step reads it: when the next undelivered chunk k has
 *   k C - halo >= start frame + F_i (halo = sts_stream_halo_frames).
 *   sts_para_info: any output may be NULL; *steps = chunks delivered.  sts_para_close frees the pool and drops what was not delivered;
 *   sts_destroy closes an open paragraph.  No entry of an open paragraph may be called from a chunk callback.
 *   While a paragraph is open every other run entry of the engine and every setter of what open fixed returns STS_ESTATE, as while a
 *   stream is open; sts_set_noise stays allowed.
 *   Equality: whatever the schedule of appends and steps, the list of chunks (count, sample offsets, sizes, samples) equals
 *   sts_infer_ids_joined_stream's for the same sentences, gaps, lead, trail and fade bit for bit when the kernel variant is pinned
 *   (sts_set_conv_mode), and the PCM is within 1 LSB of sts_infer_ids_joined's under the automatic choice.
 *   Conv math 3: an activation beyond fp16's range during an append repeats that append alone in form 0; raised in a step, that step is
 *   decoded again in form 0 and the paragraph stays there until it is closed.  No chunk leaves twice.  STS_DBG_STREAM_RETRY_STEP = k names
 *   the step that delivers chunk k. */
int sts_para_open(sts_engine* e, int32_t chunk_frames, int32_t max_resident, int64_t capacity_frames, int32_t lead_frames, float fade_ms);
int sts_para_append(sts_engine* e, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* length_scale,
                    const int32_t* gap_frames, int32_t* frames_out, int64_t* start_out, int32_t* appended);
int sts_para_finish(sts_engine* e, int32_t trail_frames);
int sts_para_step(sts_engine* e, sts_chunk_cb cb, void* user, int32_t* ready_after);
int sts_para_info(const sts_engine* e, int32_t* open, int32_t* finished, int64_t* sentences, int32_t* resident, int32_t* free_slots,
                  int64_t* free_frames, int64_t* frames_known, int64_t* frames_delivered, int64_t* steps);
int sts_para_close(sts_engine* e);
/* ---- parametric equaliser (no reference counterpart; ABI number unchanged).  sts_set_eq(e, n_bands, bands) puts a tone stage of 0 to
 * STS_EQ_MAX_BANDS biquad sections in front of loudness and the limiter: an "audio profile" (telephone band, rumble and DC removal, a
 * presence lift) that loudness mode 2 and the limiter then measure and limit as played.  n_bands = 0 (default) switches the stage off:
 * nothing extra is allocated, uploaded or launched and the PCM is bit-identical to an engine that never set it.  The setting persists
 * like sts_set_limiter; sts_get_eq returns it (n_bands always; the first min(n_bands, capacity) bands when bands is non-null).
 *   Band {type, freq_hz, gain_db, q}: type STS_EQ_PEAK, _LOWSHELF, _HIGHSHELF, _HIGHPASS or _LOWPASS; gain_db is ignored by the two
 *   passes but must be finite.  Valid at output rate fs: type in 1..5, freq_hz in [20, 0.45 fs], q in [0.1, 8], gain_db in [-24, 24],
 *   q fs / freq_hz <= 6400 (alpha below is then at least 4.9e-4 and every pole lies at least 1.2e-4 inside the unit circle: the bound
 *   on which the numerical tolerance below rests), everything finite.  Anything else: STS_EINVAL, nothing changes.  sts_set_eq checks against the engine's current
 *   output rate; a run checks again (sts_set_output_rate may have been called since) and answers STS_EINVAL before anything is enqueued
 *   when a band no longer fits.
 *   1 Coefficients (host, float64; exactly what sts_eq_design returns, 5 per band): the Audio-EQ-Cookbook biquad with
 *     w0 = 2 pi f0 / fs, alpha = sin w0 / (2 q), A = 10^(gain_db / 40), the shelves in the Q form 2 sqrt(A) alpha:
 *       peak       b = {1 + alpha A, -2 cos w0, 1 - alpha A}                          a = {1 + alpha / A, -2 cos w0, 1 - alpha / A}
 *       high-pass  b = {(1 + cos w0) / 2, -(1 + cos w0), (1 + cos w0) / 2}            a = {1 + alpha, -2 cos w0, 1 - alpha}
 *       low-pass   b = {(1 - cos w0) / 2, 1 - cos w0, (1 - cos w0) / 2}               a = {1 + alpha, -2 cos w0, 1 - alpha}
 *       low shelf  b = {A (A+1 - (A-1) cos w0 + s), 2 A (A-1 - (A+1) cos w0), A (A+1 - (A-1) cos w0 - s)}
 *                  a = {A+1 + (A-1) cos w0 + s, -2 (A-1 + (A+1) cos w0), A+1 + (A-1) cos w0 - s},   s = 2 sqrt(A) alpha
 *       high shelf b = {A (A+1 + (A-1) cos w0 + s), -2 A (A-1 + (A+1) cos w0), A (A+1 + (A-1) cos w0 - s)}
 *                  a = {A+1 - (A-1) cos w0 + s, 2 (A-1 - (A+1) cos w0), A+1 - (A-1) cos w0 - s}
 *     normalised by a0 to (b0, b1, b2, a1, a2).
 *   2 Signal, for one utterance x[0 .. N) (float32) at the output rate, N unchanged, no tail: u_0 = float64(x); section s in band order,
 *     direct form I from zero state at the utterance's first sample,
 *       u_s[n] = b0 u_{s-1}[n] + b1 u_{s-1}[n-1] + b2 u_{s-1}[n-2] - a1 u_s[n-1] - a2 u_s[n-2]      (float64);
 *     y = float32(u_S), pcm = the reference's cast (int16)(int32)(y * 32737).  An utterance's output depends on its own samples only.
 *   The kernels (eq.hip) evaluate the recurrence as a scan over chunks, which associates it differently: y equals the definition within
 *   2^-24 |u_S[n]| + 2^-26 max |u_S| per sample (tests/eq_ref.py holds the definition and the scan's order, both in float64).
 * Place in the chain: decoder tail -> gain plan -> join -> resampler -> EQ -> loudness -> limiter -> cast.  The EQ runs at the output
 * rate; after sts_infer_ids_joined it sees the ONE joined signal.  With nothing downstream (loudness mode 0 or 1, limiter off) the EQ
 * kernel writes the PCM itself; loudness and the limiter read the EQ's float output.  Tap "wave_eq": that output ("wave", "wave_gain",
 * "wave_join", "wave_out" stay the signals in front of it).
 * Streaming (sts_infer_ids_stream, sts_infer_ids_batch_stream, sts_infer_ids_joined_stream, sts_pool_submit_stream) answers STS_EINVAL
 * while an EQ is set: an IIR has no finite halo, and the sequential state carried from chunk to chunk would make the PCM depend on the
 * chunking -- unless sts_set_eq_streaming (below) is on. */
#define STS_EQ_MAX_BANDS 4
#define STS_EQ_PEAK 1
#define STS_EQ_LOWSHELF 2
#define STS_EQ_HIGHSHELF 3
#define STS_EQ_HIGHPASS 4
#define STS_EQ_LOWPASS 5
typedef struct sts_eq_band { int32_t type; float freq_hz; float gain_db; float q; } sts_eq_band;
int sts_set_eq(sts_engine* e, int32_t n_bands, const sts_eq_band* bands);
int sts_get_eq(const sts_engine* e, int32_t* n_bands, sts_eq_band* bands, int32_t capacity);
/* Host only (no device): the validity rules above at output rate `rate` (STS_OK or STS_EINVAL with the reason in sts_last_error). */
int sts_eq_check(int32_t rate, int32_t n_bands, const sts_eq_band* bands);
/* Host only (no device): step 1 for valid bands; coeffs receives 5 float64 per band, {b0, b1, b2, a1, a2}. */
int sts_eq_design(int32_t rate, int32_t n_bands, const sts_eq_band* bands, double* coeffs);
/* The same kernels on caller signals, like sts_limiter_apply: B float signals at `rate` packed back to back in x (host memory),
 * lengths[b] samples each (0 allowed), n_bands >= 1.  y (float) and pcm (int16) receive the equalised signals packed like x; each may be
 * NULL.  (On the device both start out as NaN / 0x7FFF, so a sample the kernels left out shows.) */
int sts_eq_apply(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, int32_t n_bands,
                 const sts_eq_band* bands, float* y, int16_t* pcm);
/* ---- the equaliser in a stream (ABI number unchanged).  sts_set_eq_streaming(e, 1) lets every streaming call run while bands are set;
 * 0 (default) keeps the refusal above.  The switch persists until changed; it has no effect without bands or in a whole-utterance call
 * (with it off, or without bands, a stream allocates, uploads and launches exactly what it always did).  sts_get_eq_streaming returns
 * it (0 for a null engine).  Streaming under loudness mode 1 or 2 stays refused (mode 1 runs with sts_set_loudness_streaming: loudness
 * then measures the streamed EQ's y), and sts_stream_halo_frames does not change: an IIR needs
 * no look-ahead, and the carried state replaces the look-back.
 *   Definition: in a streaming call the signal of utterance b (of a joined stream: the one signal J) is y of step 2 above, the float64
 *   DF-I cascade from zero state over the ENTIRE utterance at the output rate, evaluated in eq.hip's fixed order -- chunks of 32
 *   samples, tiles of 8192, both anchored at the utterance's first sample.  Each callback delivers its range of that y: cast, or limited
 *   and then cast.  The carry-in of a chunk depends only on its tile's carry and on the chunks in front of it in that tile, so the
 *   engine keeps, per utterance, the open tile's carry and input (and the last y the limiter's window reaches back into) and continues
 *   from there: the concatenated chunks are the PCM of the corresponding whole call (sts_infer_ids, sts_infer_ids_batch per utterance,
 *   sts_infer_ids_joined) for EVERY chunk_frames -- bit for bit with the conv mode pinned, as for a stream without an EQ.  A step the
 *   engine decodes twice (the split-bf16 repeat) starts both times from the same state. */
int sts_set_eq_streaming(sts_engine* e, int enable);
int sts_get_eq_streaming(const sts_engine* e);
/* The stream-mode kernels on caller signals: signals, rate and bands as sts_eq_apply.  bounds[0 .. n_steps): ascending step boundaries,
 * bounds[0] = 0, common to all utterances; step k covers [bounds[k], bounds[k+1]) (the last one: to the end), clipped to each length, and
 * an utterance with lengths[b] <= bounds[k] takes no part in it.  back in [0, 2048]: step k presents the window
 * [max(0, bounds[k] - back), min(lengths[b], bounds[k+1] + back)) -- what the limiter's widened range does in the engine; the input behind
 * the previous window's end is consumed, the part in front of it is answered from the carried state.  y / pcm (each may be NULL): every
 * step's [bounds[k], bounds[k+1]), packed like x.  win_y (may be NULL; win_capacity floats): every step's WHOLE window output, step by
 * step and utterance by utterance, and win_off[k B + b] (may be NULL; n_steps x B entries) its offset there, -1 where the utterance takes
 * no part.  (On the device outputs, state and workspace start out as NaN / 0x7FFF.) */
int sts_eq_apply_chunked(int device, const float* x, const int64_t* lengths, int32_t B, int32_t rate, int32_t n_bands,
                         const sts_eq_band* bands, const int64_t* bounds, int32_t n_steps, int32_t back, float* y, int16_t* pcm,
                         float* win_y, int64_t win_capacity, int64_t* win_off);
/*   record intermediate tensors of the next run: "x_enc","m","logs","logw","z_p","z","wave","wave_out" ("logs": the second half of the
 *   encoder projection, computed only by runs that record taps or sample the prior; "wave_out": the resampled float wave, only at a
 *   non-native output rate, one-pass calls; "dur_w": the planned duration weights, only a run with a duration plan; "wave_gain": the
 *   gained native float wave, only a one-pass run with a gain plan; "wave_join": the joined native float wave J, only
 *   sts_infer_ids_joined; "wave_eq": the equaliser's float output at the output rate, only a one-pass run with sts_set_eq) */
int sts_set_record_taps(sts_engine* e, int enable);
/*   fetch a tap: malloc()'d copy, channel-major [channels][total_len] (== the reference's column-major
 *   MatrixXf [time, channels]); for batches the utterances are packed along time. */
int sts_get_tap(sts_engine* e, const char* name, float** data, int32_t* channels, int64_t* length);
/*   durations of the last run, packed (sum of n entries) */
int sts_get_durations(sts_engine* e, int32_t* dur, int64_t capacity);
/*   conv dispatch: 0 = automatic, 1 = force the generic VALU kernel everywhere, 2..7 = force LDS-staged
 *   matrix-core tile (idx-2), 8 / 9 = force the split-K matrix-core kernel (32 / 64 columns per workgroup) */
int sts_set_conv_mode(sts_engine* e, int mode);
/*   arithmetic of the decoder trunk's matrix-core convs (upsamplers + ResBlock convs, ~95 % of the FLOPs):
 *   0 = fp32 operands split exactly into three bf16 terms each, six bf16 MFMA products per fp32 product, fp32 accumulation
 *       (conv_bf3.hip; as accurate as 1 against float64, 6/16 of its matrix-pipe time);
 *   1 = the exact-fp32 MFMA instruction (v_mfma_f32_32x32x2_f32) everywhere;
 *   2 = as 0, and also for every other eligible matrix-core conv (flow, text encoder) regardless of its grid size -- by default
 *       those switch to the split form only from the batch size on at which they stop being launch-latency-bound (tests).
 *   3 = "f16x2": fp32 operands as TWO fp16 terms (the small one pre-scaled by 2^11, weights by a per-conv power of two), three
 *       fp16 MFMA products per fp32 product -- half the matrix-pipe time of 0, 22-23 instead of 24 operand bits (measured error
 *       against float64: docs/HISTORY.md 5f) -- the default.  An activation beyond fp16's range raises a flag and the call (a
 *       streaming call: the chunk, before it is handed out) is repeated in form 0; sts_profile.conv_math_fallbacks counts these.
 *       After two such calls in a row the engine stays in form 0 until sts_set_conv_math is called again
 *       (sts_profile.conv_math_pinned).  The first repeat of an engine and the pinning are reported through tts_log.
 *   The default can also be chosen with the environment variable STS_CONV_MATH = f16x2 | bf16x3 | f32; any other value is
 *   reported through tts_log and ignored (the default applies). */
int sts_set_conv_math(sts_engine* e, int mode);

/*   test hooks (per engine, never read from the environment): force a kernel family that the automatic choice would not pick
 *   at the size of a test.  key: STS_DBG_ATTN_BLOCK_MIN_WGS -- the matrix-core block attention kernel engages from this many
 *   workgroups on (default 96; 1 = always).
 *   (Keys 2-4 selected the two persistent-kernel families of round 3; both lost their A/B against the launch path and were deleted
 *   in round 5 -- the numbers stay retired and answer STS_EINVAL.) */
enum { STS_DBG_ATTN_BLOCK_MIN_WGS = 1,
       STS_DBG_TAIL_FUSED = 14 /* MB-iSTFT / MS-iSTFT decoders: 1 (default) the tail (spectrum, inverse DFT + overlap-add, synthesis filter, int16 cast) as one launch, 0 three */,
       STS_DBG_UPS_ROWPH = 15 /* upsamplers (transposed convs, stride 2 / 4 / 8): 1 (default) phases interleaved along the packed rows -> whole-sector stores, 0 phase-major rows */,
       STS_DBG_CHAIN_STREAMS = 13 /* lab: bit i = the ResBlock chains of decoder stage i as per-chain launches on three prioritised streams instead of one grouped launch per layer (-1: off) */,
       STS_DBG_H2P = 11 /* decoder stages of 128 k channels under the two-term fp16 arithmetic: 1 (default) pre-split channel-minor activations (conv_h2p.hip) from ~8 tiles of 128 x 128 per CU on, 2 always (tests), 0 the staged kernels */,
       STS_DBG_H2P_TILE = 12 /* lab: tile code of conv_h2p_group, -1 automatic */,
       STS_DBG_MEMO_CLEAR = 10 /* any value: forget the launch-ahead memo (bench.py: every timed request is then one the engine has not served before) */,
       STS_DBG_PCM_DIRECT = 9 /* sts_set_host_pcm(1), one utterance: 1 (default) the decoder's last kernel writes the PCM into the pinned host buffer itself, 0 a download behind it */,
       STS_DBG_DDS_TAIL = 8 /* stochastic duration predictor: 1 (default) a ConvFlow's projection + spline step ride in its last DDSConv layer's launch, 0 three launches */,
       STS_DBG_ATTN_REG = 7 /* one-query attention: 1 (default) operands in registers (attention_reg_kernel), 0 the round-1 kernel */,
       STS_DBG_LAUNCH_AHEAD = 6 /* one-utterance calls and packed batches: 1 (default) a request the engine has served before (same ids, speaker, length scale: the frame count is a pure function of them) enqueues flow + decoder before the count reaches the host, 0 the host always waits for it, 2 (tests) the memo is keyed by the phoneme count alone -- provokes the repeat that answers a hash collision */,
       STS_DBG_FLOW_FUSED = 5 /* reverse flow: 1 (default) one launch per WaveNet layer (wn_flow.hip, under the two-term fp16 arithmetic) where the grid is one round of workgroups, with 16 output frames per workgroup where 32 would leave half the compute units without one; 0 one launch per conv; 2 / 3 (tests, A/B) one launch per layer at any size with 32 / 16 frames per workgroup -- 1, 2 and 3 return the same bits */ };
/* ABI 10, sts_infer_ids_batch_stream: STS_DBG_STREAM_RETRY_STEP (tests) -- under conv math 3 the overflow word counts as raised after step k
 * (value k; -1 = off), which takes the split-bf16 repeat of that step (k > 0) or of the whole call (k = 0); -2: it counts as raised in
 * every sts_stream_admit instead, which takes the repeat of that admission; STS_DBG_STREAM_DIRECT -- 1 the
 * last kernel of a step writes the step's chunks into mapped pinned host memory itself, 0 (default) one download per step */
enum { STS_DBG_STREAM_RETRY_STEP = 16, STS_DBG_STREAM_DIRECT = 17 };
/* ABI 12, STS_DBG_POISON (tests): value = a 32-bit fill pattern, 0 = off (default).  While it is on, every call fills each workspace arena
 * with the pattern on the engine's stream right after laying it out (before any upload or kernel writes into it; once per layout, never
 * between the stages or stream steps of one call), and the host fills the output regions the call will write (the pinned PCM or chunk
 * buffer up to the call's capacity with the pattern's low 16 bits, the loudness results of its utterances) before the first kernel that
 * writes them is enqueued.  No result may depend on what the arenas held before: a poisoned call returns what an unpoisoned engine returns, bit for bit.
 * sts_profile.poison_bytes reports the bytes the last call filled. */
enum { STS_DBG_POISON = 18 };
/* STS_DBG_COL_PROJ (tests, A/B; no ABI change) -- the text encoder's q/k/v projection and the producer of its input (the embedding, or the
 * previous layer's second LayerNorm): 1 (default) one launch, with all three passes in one workgroup per 16 phonemes from 24 such column
 * blocks on and one workgroup per (column block, pass) below; 0 the producer and the conv as two launches at any size; 2 / 3 one launch at
 * any size with the passes in one workgroup / one workgroup per pass -- 1, 2 and 3 return the same bits.
 * STS_DBG_SDP_PRE_RIDE (tests, A/B) -- the stochastic duration predictor's `pre` conv (1x1, hidden -> hidden) of a single-speaker model:
 * 1 (default) one more workgroup per column block in the launch of the encoder's output projection, 0 a conv launch of its own. */
enum { STS_DBG_COL_PROJ = 19, STS_DBG_SDP_PRE_RIDE = 20 };
int sts_debug_set(sts_engine* e, int key, int value);

/* Per-stage device timing of the last run, measured with HIP events on the engine's own stream. */
typedef struct sts_profile {
    float ms_text_encoder, ms_duration, ms_flow, ms_decoder, ms_total_device;
    float ms_decoder_mfma;          /* time of the pure conv_mfma launch sequence inside the decoder */
    int32_t decoder_mfma_launches;
    double flops_text_encoder, flops_duration, flops_flow, flops_decoder;   /* algorithmic (true-tap) FLOPs */
    double flops_decoder_mfma;      /* FLOPs executed by the launches timed in ms_decoder_mfma */
    double bytes_decoder_min;       /* algorithmic HBM bytes of the decoder (weights once + act in/out per conv) */
    int64_t frames, samples, phonemes;
    double flops_decoder_mfma_executed;   /* matrix-core FLOPs the timed launches actually execute: the Winograd-domain layer
                                             kernels need (4 n3 + 3 n2) / (2 k) of a k-tap conv's direct-form products */
    double bytes_text_encoder, bytes_duration, bytes_flow;   /* algorithmic HBM bytes per stage (as bytes_decoder_min) */
    float ms_sync_wait_host;        /* host time blocked on the frame-count download (the one data-dependent sync) */
    double flops_decoder_bf16_issued;     /* bf16 matrix-core FLOPs issued by the timed launches that run on split operands
                                             (6 x their algorithmic FLOPs; 3 x with sts_set_conv_math(3)); 0 with sts_set_conv_math(1) */
    int64_t conv_math_fallbacks;          /* sts_set_conv_math(3): calls of this engine so far that were repeated in the split-bf16 form */
    int32_t conv_math_pinned;             /* 1: after two such calls in a row the engine now stays in the split-bf16 form (until sts_set_conv_math) */
    int32_t launch_ahead;                 /* 1: this run enqueued flow + decoder before the frame count reached the host (one utterance or a packed batch whose members the engine has all served before; ms_sync_wait_host ~ 0) */
    int64_t launch_ahead_misses;          /* launch-ahead runs of this engine so far (one utterance or a batch) whose remembered frame counts turned out wrong -- a hash collision of the memo -- so that flow + decoder were repeated the waiting way */
    float us_host_setup;                  /* host time from the entry of the run to the first launch being enqueued (input checks, tables, the one upload) */
    float us_host_enqueue;                /* host time from the entry of the run to the last launch being enqueued (the GPU runs behind it) */
    float us_host_tail;                   /* host time from the return of the run's last stream synchronisation to the return of the call */
    int64_t poison_bytes;                 /* ABI 12: bytes of workspace and host outputs the last call filled under STS_DBG_POISON (0 when it is off) */
} sts_profile;
/* enable: 0 off; 1 HIP events at all eight stage boundaries of a run (ms_text_encoder ... ms_decoder_mfma); 2 only the two events around the
 * decoder's matrix-core region (ms_decoder_mfma; the per-stage times read 0) -- every event is a barrier packet between two kernels
 * (5-10 us of idle GPU each), so a caller who wants the dominant kernel family timed inside a step it also times uses 2. */
int sts_set_profiling(sts_engine* e, int enable);
/* The struct only ever grows at its end (STS_ABI_VERSION counts the revisions).  sts_get_profile_ex copies min(size_bytes,
 * sizeof(sts_profile)) bytes, so a client compiled against an older header passes ITS sizeof and is never overrun;
 * sts_get_profile(e, p) == sts_get_profile_ex(e, p, sizeof(sts_profile)) of the header this library was built from -- use it only
 * when client and library are built together. */
/* (Stays 18 with the planned open streams: sts_stream_open_ex, sts_stream_tables_info, sts_pool_submit_stream_ex and
 * sts_debug_adopt_tables are additive and are detected by symbol, not by version.) */
#define STS_ABI_VERSION 18
int sts_abi_version(void);
/* bit 0: lab build (-DSTS_EXPERIMENTS: environment knobs of knobs.hpp, every conv tile code);
 * 0 for the shipped library */
int sts_build_flags(void);
int sts_get_profile(const sts_engine* e, sts_profile* p);
int sts_get_profile_ex(const sts_engine* e, void* p, int64_t size_bytes);

/* Stand-alone conv entry for op-level parity tests: y = conv1d(x) with x [Cin][L] on the host.
 * w is the reference layout [out][k][in] (transposed: same).  mode as sts_set_conv_mode; 13 / 20.. = the split-bf16 kernel
 * (automatic tile / tile code mode - 20), 50 / 60.. = the two-term fp16 kernel (automatic tile / tile code mode - 60). */
int sts_debug_conv1d(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias,
                     int32_t Cout, int32_t k, int32_t pad, int32_t dil, int32_t stride_transposed,
                     int32_t depthwise, float in_slope, int32_t in_act, int mode, float** y, int32_t* Lout);

/* Same conv, additionally timed: `iters` back-to-back launches between two HIP events; *ms_out = mean
 * milliseconds per launch (kernel micro-benchmarks, tools/conv_bench.py). */
int sts_debug_conv1d_bench(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias,
                           int32_t Cout, int32_t k, int32_t pad, int32_t dil, int32_t stride_transposed,
                           int32_t depthwise, float in_slope, int32_t in_act, int mode, float** y, int32_t* Lout,
                           int32_t iters, float* ms_out);

/* sts_debug_conv1d_packed (ABI 15): the same conv on B utterances packed back to back along the time axis, as the engine packs a batch:
 * x [Cin][L] with L = sum(lengths), every lengths[b] >= 1.  The kernels get device offset / length tables of B entries (B = 1 included)
 * and a grid sized by the longest segment; halos are zero at every segment's edges.  Geometries: "same" padding (odd k, pad =
 * dil (k - 1) / 2; output segment = input segment) or a transposed conv with pad = (k - stride) / 2 (output segment = input segment x
 * stride); anything else is STS_EINVAL.  mode as above.  The output buffer starts out as a NaN pattern, so a position no workgroup
 * writes reads as NaN.  *ovf (optional): the overflow word of the two-term fp16 kernels after the launch (0 for every other mode). */
int sts_debug_conv1d_packed(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias,
                            int32_t Cout, int32_t k, int32_t pad, int32_t dil, int32_t stride_transposed,
                            int32_t depthwise, float in_slope, int32_t in_act, int mode, float** y, int32_t* Lout,
                            const int32_t* lengths, int32_t B, uint32_t* ovf);

/* sts_debug_conv1d_epi (detected by symbol, ABI 18): sts_debug_conv1d_packed with the epilogues and operand forms the engine gives its
 * convs (kernels.hpp ConvArgs).  opts null: sts_debug_conv1d_packed, bit for bit (gap must then be 0).
 *   epi        0 STORE  y = v | 1 RESADD  y = v + res | 3 SUB  y = y_init - v | 4 GATE  y[c] = tanh(v[c]) sigmoid(v[c + H]), Cout = 2 H |
 *              5 RESSKIP  Cout = 2 H: y = y_init + v[:H], aux = (epi_flag & 1 ? 0 : aux_init) + v[H:]; Cout = H: every row goes to aux |
 *              6 TANH_PCM  aux (the wave, optional) = tanh(v), pcm = trunc(wave * 32737), Cout = 1;   v = conv + bias + ubias[:, b]
 *   gate_perm  1 (GATE, H % 16 == 0): the weights, the bias and ubias are packed with the loader's (tanh16, sigmoid16) row order
 *   in_reflect 1: the logical input of segment b is its reflect-pad-left-1 view (len + 1 positions: p reads x[p - 1], p = 0 reads x[1]);
 *              output segment b is len + 1 long and starts at off[b] + b
 *   nsum       0, or 2 / 3: the logical input is ((x + xs1) [+ xs2]) / nsum, formed by the kernel while it stages its input
 *   kslices    1, or 2 / 4 / 8 (STORE on the split-K modes 8 / 9): y holds kslices partial planes [kslices][Cout][Lout], bias on plane 0
 *   ubias      [Cout][B] in source row order, or null;  res / y_init / aux_init: the shape of the tensor they belong to;  xs1, xs2: as x
 * gap: segment b starts at off[b] = sum_{i < b} (lengths[i] + gap), so L = sum(lengths) + B gap (gap 0: the engine's packing); output
 * segment b starts at off[b] * stride (+ b with in_reflect) and Lout = L * stride (+ B).  y has Cout rows (GATE and RESSKIP: H), aux H
 * rows (TANH_PCM: 1), pcm one.  Every column of y / aux / pcm outside the output segments holds the sentinel 0xFFFFFFFF (pcm: 0x7FFF)
 * before the launch, and so does a whole tensor without an initial value; a tensor WITH an initial value (the target of a
 * read-modify-write epilogue) holds the finite sentinel 0x2F5A5A5A (1.99e-10) there instead, whatever y_init / aux_init hold in those
 * columns, so that an update running into them changes their bits; all columns come back.
 * Everything a kernel family does not take is STS_EINVAL (nothing falls back to another kernel), decided before any device call. */
typedef struct sts_conv_epi_opts {
    int32_t size_bytes;         /* sizeof(sts_conv_epi_opts) */
    int32_t epi, epi_flag, H, gate_perm, in_reflect, nsum, kslices;
    const float* ubias;
    const float* res;
    const float* y_init;
    const float* aux_init;
    const float* xs1;
    const float* xs2;
    float* aux_out;             /* caller-allocated [H or 1][Lout] */
    int16_t* pcm_out;           /* caller-allocated [Lout] */
} sts_conv_epi_opts;
int sts_debug_conv1d_epi(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias,
                         int32_t Cout, int32_t k, int32_t pad, int32_t dil, int32_t stride_transposed,
                         int32_t depthwise, float in_slope, int32_t in_act, int mode, float** y, int32_t* Lout,
                         const int32_t* lengths, int32_t B, uint32_t* ovf, const sts_conv_epi_opts* opts, int32_t gap);

/* One "same"-padded conv (odd k, pad = dil (k - 1) / 2) through the pre-split path of the wide decoder stages (conv_h2p.hip): x fp32
 * [Cin][L] -> split_planes(in_slope) -> conv_h2p_group with `members` identical members -> member 0's three output forms, each decoded to
 * fp32 [Cout][L] (null: not wanted): y = the channel-major fp32 output, y16 = the channel-minor fp32 copy, yp = the two fp16 planes of
 * lrelu(out, out_slope) recombined.  res: optional residual [Cout][L].  tile < 0: automatic. */
int sts_debug_conv_h2p(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k,
                       int32_t dil, const float* res, float in_slope, float out_slope, int tile, int members, float* y, float* y16,
                       float* yp, int32_t iters, float* ms_out);

/* sts_debug_conv_h2p_packed (ABI 15): sts_debug_conv_h2p on B packed utterances (x, res and the outputs [C][L], L = sum(lengths), every
 * lengths[b] >= 1): split_planes and conv_h2p_group both get the B-entry segment table and max_n = the longest segment.  The plane and
 * output buffers start out as a NaN pattern.  *ovf (optional): the overflow word after the launch. */
int sts_debug_conv_h2p_packed(int device, const float* x, int32_t Cin, int32_t L, const float* w, const float* bias, int32_t Cout, int32_t k,
                              int32_t dil, const float* res, float in_slope, float out_slope, int tile, int members, float* y, float* y16,
                              float* yp, const int32_t* lengths, int32_t B, uint32_t* ovf);

/* The same conv through the Winograd-domain lab kernel (conv_h2w.hip: segmented F(2,3) / F(2,2) on two-term fp16 operands): y = fp32 [C][L],
 * y16 = its channel-minor output of lrelu(out, out_slope) decoded to [C][L].  C % 128 == 0, odd k >= 3, (k - 1) dil <= 64. */
int sts_debug_conv_h2w(int device, const float* x, int32_t C, int32_t L, const float* w, const float* bias, int32_t k, int32_t dil, const float* res,
                       float in_slope, float out_slope, int members, float* y, float* y16, int32_t iters, float* ms_out);

/* One reverse ConvFlow step of the stochastic duration predictor on caller data, launched exactly as the engine launches it where the
 * projection runs as its own conv (misc_kernels.hip spline_step: one thread per position, 128 per workgroup): (r0, r1) -> (o0, o1) =
 * (inverse rational-quadratic spline of r1 under the 29 parameters h[.][i], r0).  h is [29][n] with row stride n (10 widths, 10 heights,
 * 9 inner derivatives, all unnormalised); filter_sqrt divides the first 20 rows.  r0 / r1: n floats each, either may be NULL = all zeros,
 * as the kernel allows.  o0 / o1 receive n floats each.  On the device every output row is followed by a guard that covers the rest of the
 * launch's last workgroup and 128 positions more; a guard word the kernel changed is STS_EDEVICE.  1 <= n <= 2^24. */
int sts_debug_spline_step(int device, const float* h, int64_t n, float filter_sqrt, const float* r0, const float* r1, float* o0, float* o1);

/* sts_debug_attention (ABI 16): the text encoder's windowed relative-position attention on caller data, between the q / k / v convs and the
 * output conv.  q, k, v: [nheads * kc][L], L = sum(lengths), B utterances packed back to back as the engine packs them (every lengths[b]
 * >= 1).  relk / relv: [kc][2 win + 1], null exactly when win = 0.  nheads is free here (the engine pins 2).
 * variant: 0 = the kernel the engine's dispatcher picks for this shape with the engine's defaults; 1 = attention_kernel (generic, any shape
 * whose LDS row fits the device); 2 = attention_reg_kernel (kc <= 96, 2 win + 1 <= 16, longest utterance <= 256); 3 = attention_mfma_kernel
 * (kc % 16 == 0, kc <= 128, 2 win + 1 <= 32, LDS <= 150 KiB).  A forced variant whose limits the shape does not meet, or a shape no kernel
 * admits, is STS_EINVAL and nothing is launched.
 * o: [o_rows][L] floats, o_rows >= nheads * kc.  The device buffers have exactly these sizes; the output starts out as the word 0xFFFFFFFF
 * everywhere and all of it is copied back, so an element no workgroup wrote -- and a row past nheads * kc that one did -- shows.
 * *variant_out (optional): the kernel launched (1 | 2 | 3); *jpl_out (optional): keys per lane of the register kernel (2 | 4), else 0. */
int sts_debug_attention(int device, const float* q, const float* k, const float* v, const float* relk, const float* relv, int32_t nheads,
                        int32_t kc, int32_t win, const int32_t* lengths, int32_t B, int variant, float* o, int32_t o_rows,
                        int32_t* variant_out, int32_t* jpl_out);

/* sts_debug_layer_norm (ABI 16): the text encoder's / duration predictors' LayerNorm launch on caller data, all of its fused forms:
 *   v = [depthwise conv of] a (+ b_0 + ... + b_{nb-1}) ; relu(v) if pre_relu ; y = LN_C(v) * gamma + beta ; gelu(y) if post_gelu ; res + y.
 * a, res (optional), y: [C][L] (y: [y_rows][L], y_rows >= C), L = sum(lengths) as above.  b: nb in 0..8 partials [C][L], b_stride floats
 * apart (>= C L; read only when nb > 1), null exactly when nb = 0.  dw_w (optional) [k][C] with dw_b (optional) [C]: tap j reads position
 * pos + j dil - pad of the SAME utterance, zero outside it.  The output starts out as the word 0xFFFFFFFF and is copied back whole. */
int sts_debug_layer_norm(int device, const float* a, const float* b, int32_t nb, int64_t b_stride, const float* res, const float* gamma,
                         const float* beta, int32_t C, int32_t pre_relu, int32_t post_gelu, const float* dw_w, const float* dw_b, int32_t dw_k,
                         int32_t dw_dil, int32_t dw_pad, const int32_t* lengths, int32_t B, float* y, int32_t y_rows);

/* sts_debug_resblock_layer (ABI 17): ONE fused ResBlock layer launch of the decoder's narrow stages on caller data,
 *   y_j = x + conv2_j(lrelu(conv1_j(lrelu(x)))),   conv1_j: k1[j] taps of dilation dil1[j], conv2_j: k2[j] taps of dilation 1, "same" padding,
 * for the n members (ResBlock chains) j of one grid; the intermediate is zero outside every utterance, whatever b1 is.
 * x: [C][ld]; B utterances of lengths[b] >= 1 packed back to back from column 0 (L = sum(lengths) <= ld), as the engine packs them.  Every
 * member reads the same x and writes its own y.  w1[j] [C][k1[j]][C], w2[j] [C][k2[j]][C] in the blob's [out][k][in] order; b1 / b2: null, or
 * n pointers to [C] each of which may be null.  The weights go through the loader's own packers and the group is filled as the decoder fills it.
 * kind: 1 = resblock_layer (exact fp32, direct form), 2 = resblock_wino (exact fp32, Winograd domain), 3 = resblock_bf3 on three bf16 terms,
 * 4 = resblock_bf3 on two fp16 terms.  variant (kinds 3 / 4): -1 = the shipped tile shape, 0 / 1 = resblock_bf3's two shapes per width.
 * The kind's own eligibility function judges the filled group; what it refuses is STS_EINVAL and nothing is launched.  The kernels admit
 * C = 32 / 64 / 128, 1 <= n <= 4, odd k1 and k2, dil1 (k1 - 1) <= 64, k2 <= 33; kind 2 moreover dil1 in {1, 2, 3, 5, 6}, k1 >= 2, 2 <= k2 <= 15.
 * y: n x [y_rows][ld] floats, y_rows >= C.  The device buffers have exactly these sizes; every y starts out as the word 0xFFFFFFFF and is
 * copied back whole, so an element no workgroup wrote -- and a row past C or a column past L that one did -- shows.
 * *ovf (optional): the overflow word of the two-term fp16 form after the launch (0 for kinds 1 to 3). */
int sts_debug_resblock_layer(int device, const float* x, int32_t C, const int32_t* lengths, int32_t B, int64_t ld, int32_t n,
                             const float* const* w1, const float* const* b1, const int32_t* k1, const int32_t* dil1,
                             const float* const* w2, const float* const* b2, const int32_t* k2, float slope, int kind, int variant,
                             float* y, int32_t y_rows, uint32_t* ovf);

/* sts_debug_col_layer (ABI 18): ONE launch of the fused column-block layer (col_layer.hip) on caller data, in each of its forms:
 *   h = x, or (xs_w given) h[c][t] = (xs_w[c] xr[t] + xs_b[c]) + x[c][t], each step rounded to float (the ConvFlow's folded 1 -> C input conv)
 *   u = gelu(LN_C(dw_b + dwconv(h)) g1 + b1) with dw_w given (tap j reads position pos + j dw_dil - dw_pad of the SAME utterance of h, zero
 *       outside it), else u = h
 *   v = add + (conv1x1(u) + bias) ;  y = LN_C(v) g2 + b2 ;  gelu(y) if post_gelu ;  y = h + y if use_res
 *   with tp_w: p = tp_w y + tp_b (29 rows), o0[t] = inverse spline of r1[t] under p[:, t] (tp_fs = sqrt(filter channels)), o1 = r0; y is
 *       then not written.
 * x, add (optional): [C][ld]; B utterances of lengths[b] >= 1 packed back to back from column 0 (sum(lengths) <= ld).  xs_w [C], xs_b [C]
 * (optional), xr [ld] (optional: the all-zero latent); dw_w [dw_k][C], dw_b [C] (optional); g1, b1, g2, b2, bias (optional) [C]; w [C][C]
 * and tp_w [29][C] in the blob's [out][1][in] order, tp_b [29]; tp_r0 / tp_r1 [ld] (optional: zeros).  The convs go through the loader's own
 * packers (load_col_layer) and the kernel arguments are filled by the functions the engine fills them with.
 * col_layer_eligible judges the filled arguments; what it refuses is STS_EINVAL and nothing is launched.  The kernel admits C = 32 / 64 /
 * 192 / 256 (a tail: not 256), 1 <= dw_k <= 3, g1 and b1 with dw_w, xs_w only with dw_w and use_res, tp_b with tp_w.
 * alias (the refusals of overlapping buffers): 0 = none, 1 = y is x, 2 = o0 is r0, 3 = o0 is r1, 4 = o1 is r1 -- all refused -- and 5 = o1
 * is r0, which is admitted (o1 then comes back as that buffer: r0's own values in the columns past sum(lengths)).
 * y: [y_rows][ld], y_rows >= C; o0, o1: [ld], required with tp_w.  The device buffers have exactly these sizes; y, o0 and o1 start out as
 * the word 0xFFFFFFFF and are copied back whole, so an element no workgroup wrote -- and a row past C or a column past sum(lengths) that
 * one did -- shows. */
int sts_debug_col_layer(int device, const float* x, int32_t C, const int32_t* lengths, int32_t B, int64_t ld, const float* xs_w,
                        const float* xs_b, const float* xr, const float* dw_w, const float* dw_b, int32_t dw_k, int32_t dw_dil, int32_t dw_pad,
                        const float* g1, const float* b1, const float* w, const float* bias, const float* add, const float* g2,
                        const float* b2, int32_t post_gelu, int32_t use_res, const float* tp_w, const float* tp_b, float tp_fs,
                        const float* tp_r0, const float* tp_r1, int32_t alias, float* y, int32_t y_rows, float* o0, float* o1);

void sts_free(void* p);
const char* sts_last_error(void);

/* Host-only diagnostic: the Winograd-domain weight transform the loader applies to the decoder's ResBlock convs
 * (segmented F(2,3), summertts_amd/csrc/kernels.hpp: wino_pack).  w is [Cout][k][Cin] (the blob's order); out must
 * hold n_seg * 4 * Cin_pad * Cout_pad floats, laid out [seg][4][Cin_pad][Cout_pad] (Cin_pad = Cin rounded up to 16,
 * Cout_pad to 32).  Returns n_seg (>= 1) or a negative STS_E* code.  No GPU needed. */
int sts_debug_wino_pack(const float* w, int32_t Cout, int32_t k, int32_t Cin, float* out, int64_t out_floats);

/* ---- request pool (no reference counterpart: SynthesizerTrn::infer is one blocking call per
 * utterance, SynthesizerTrn.cpp:323).  n_engines engines on one GPU, one worker thread each, one FIFO; a free
 * worker folds up to max_batch queued requests into ONE packed variable-length batch.  submit() returns a
 * ticket (> 0) or a negative STS_E* code; wait() blocks until that request is done and hands back a
 * malloc()'d PCM buffer (release with sts_free).  Thread-safe: any thread may submit / wait. */
typedef struct sts_pool sts_pool;
int sts_pool_create(const float* blob, int64_t blob_bytes, int device, int n_engines, int max_batch, sts_pool** out);
void sts_pool_destroy(sts_pool* p);
int64_t sts_pool_submit(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale);
int sts_pool_wait(sts_pool* p, int64_t ticket, int16_t** pcm_out, int32_t* n_out);
int sts_pool_stats(sts_pool* p, int64_t* batches, int64_t* requests);
const char* sts_pool_last_error(void);
/*   sts_pool_submit_ex: sts_pool_submit with this request's own sampling noise (sts_set_noise; the request's seed is used as given).
 *   Requests with different noise settings share one packed batch. */
int64_t sts_pool_submit_ex(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                           float noise_scale_w, uint64_t seed);
/*   sts_pool_set_output_rate: sts_set_output_rate on every engine of the pool.  STS_ESTATE while any request is outstanding (submitted and
 *   not yet collected by sts_pool_wait), so that one batch never mixes rates. */
int sts_pool_set_output_rate(sts_pool* p, int32_t rate);
/*   sts_pool_submit_stream (ABI 10): a streaming request.  A worker that takes one from the head of the FIFO folds in further queued
 *   streaming requests with the same chunk_frames (up to max_batch) and runs them as one batched stream (sts_infer_ids_batch_stream);
 *   streaming and whole-utterance requests never share a batch.  `cb` receives this request's chunks ON THE WORKER THREAD (it must not
 *   wait on its own ticket, nor on any other of the pool's tickets); a non-zero return stops this request only.  sts_pool_wait returns
 *   after its last chunk (or its stop) with *pcm_out = NULL and *n_out = samples delivered.  A failure before any chunk of the batch has
 *   left re-runs its members one by one; a failure after that completes every unfinished member's ticket with the error.  Returns a
 *   ticket or a negative STS_E* code (STS_EINVAL: bad ids, chunk_frames <= 0, a NULL callback). */
int64_t sts_pool_submit_stream(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                               float noise_scale_w, uint64_t seed, int32_t chunk_frames, sts_chunk_cb cb, void* user);
/*   sts_pool_set_loudness (ABI 11): sts_set_loudness on every engine of the pool, modes 0 and 2 only (STS_EINVAL for 1).  STS_ESTATE while any
 *   request is outstanding, as sts_pool_set_output_rate.  While the mode is 2, sts_pool_submit_stream answers STS_EINVAL. */
int sts_pool_set_loudness(sts_pool* p, int mode, float target_lufs, float peak_dbfs);
/*   sts_pool_set_limiter (ABI 13): sts_set_limiter on every engine of the pool.  STS_ESTATE while any request is outstanding, as
 *   sts_pool_set_output_rate.  Streaming requests are limited chunk by chunk. */
int sts_pool_set_limiter(sts_pool* p, int mode, float gain_db, float ceiling_dbfs, float lookahead_ms);
/*   sts_pool_set_eq: sts_set_eq on every engine of the pool (one setting for every request; no per-request EQ).  STS_ESTATE while any
 *   request is outstanding.  While bands are set, sts_pool_submit_stream answers STS_EINVAL unless sts_pool_set_eq_streaming is on. */
int sts_pool_set_eq(sts_pool* p, int32_t n_bands, const sts_eq_band* bands);
/*   sts_pool_set_eq_streaming: sts_set_eq_streaming on every engine of the pool.  STS_ESTATE while any request is outstanding. */
int sts_pool_set_eq_streaming(sts_pool* p, int enable);
/*   sts_pool_set_stream_admission (default off): on, a worker runs a group of streaming requests as an OPEN stream (sts_stream_open: the
 *   group's chunk size, max_live = max_batch, capacity = max_batch * 1024 frames) and looks at the FIFO between steps: while its head is a
 *   streaming request of the same chunk size and slots are free, it takes up to the free count and admits them into the running stream, so
 *   a client that arrives late hears its first chunk after one admission and one step, not after the group has drained.  A head of any
 *   other kind is left for another worker or for after the drain; FIFO order is kept.  An admission that fails with more than one request
 *   is retried one by one (a bad request fails alone); one that finds no room goes back to the head of the FIFO.  Tickets complete as
 *   without it.  With the pool's EQ or loudness set, and for a group that does not fit the empty pool, streamed groups run the closed way.
 *   STS_ESTATE while any request is outstanding.  sts_pool_stream_stats: groups = streamed groups run as open streams, admitted_midstream =
 *   requests admitted into a running one (either may be NULL). */
int sts_pool_set_stream_admission(sts_pool* p, int enable);
int sts_pool_get_stream_admission(const sts_pool* p);
int sts_pool_stream_stats(sts_pool* p, int64_t* groups, int64_t* admitted_midstream);
/*   sts_pool_submit_plan (ABI 14): sts_pool_submit_ex with this request's own duration plan (sts_set_duration_plan: rate and fixed hold n
 *   entries each or are NULL, target_frames 0 = none; an invalid plan answers STS_EINVAL).  Whole-utterance requests only.  Requests with and
 *   without a plan share one packed batch: the plan is per utterance. */
int64_t sts_pool_submit_plan(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                             float noise_scale_w, uint64_t seed, const float* rate, const int32_t* fixed, int32_t target_frames);
/*   sts_pool_submit_mix: sts_pool_submit_ex with this request's own speaker mix (sts_set_speaker_mix; copied; NULL or an empty entry = the
 *   plain sid; an invalid mix answers STS_EINVAL).  Whole-utterance requests only.  Mixed and plain requests share one packed batch. */
int64_t sts_pool_submit_mix(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                            float noise_scale_w, uint64_t seed, const sts_speaker_mix* mix);
/*   sts_pool_submit_gain: sts_pool_submit_ex with this request's own gain plan (sts_set_gain_plan: gain_db holds n entries or is NULL;
 *   copied; NULL or an entry with gain_db == NULL = no plan; an invalid plan answers STS_EINVAL).  Whole-utterance requests only.  Requests
 *   with and without a plan share one packed batch: the plan is per utterance, and a member without one keeps its samples bit for bit. */
int64_t sts_pool_submit_gain(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                             float noise_scale_w, uint64_t seed, const sts_gain_plan* plan);
/*   sts_pool_submit_pitch: sts_pool_submit_ex with this request's own pitch plan (sts_set_pitch_plan; copied; plan == NULL or cents == NULL:
 *   a plain request; an invalid plan answers STS_EINVAL).  Whole-utterance requests only.  Requests with and without a plan share one
 *   packed batch: a member without one keeps its samples bit for bit. */
int64_t sts_pool_submit_pitch(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                              float noise_scale_w, uint64_t seed, const sts_pitch_plan* plan);
/*   sts_pool_submit_stream_ex: sts_pool_submit_stream with this request's own duration plan, speaker mix and gain plan, each optional
 *   (copied; validated at submit as sts_pool_submit_plan / _mix / _gain validate theirs: STS_EINVAL).  All three NULL is
 *   sts_pool_submit_stream.  Planned and plain streaming requests of one chunk size share a group; with admission on
 *   (sts_pool_set_stream_admission) the group is a planned open stream (sts_stream_open_ex) and a planned request is admitted into it
 *   midstream like a plain one. */
int64_t sts_pool_submit_stream_ex(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                                  float noise_scale_w, uint64_t seed, int32_t chunk_frames, sts_chunk_cb cb, void* user,
                                  const sts_dur_plan* plan, const sts_speaker_mix* mix, const sts_gain_plan* gain);

/*   sts_pool_submit_joined: a paragraph (sts_infer_ids_joined) as ONE request: one ticket, one PCM.  Sentence b samples with seed + b.  It
 *   runs as its own packed batch of B, whatever max_batch is, and is never folded with other requests; the pool's output rate, loudness
 *   and limiter apply to the joined signal.  The ids and the join are copied.  An invalid join or request answers STS_EINVAL.  A joined
 *   request carries no duration plan, speaker mix or gain plan. */
int64_t sts_pool_submit_joined(sts_pool* p, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                               const float* length_scale, float noise_scale, float noise_scale_w, uint64_t seed, const sts_join* join);

/* ---- multi-device batch (no reference counterpart).  One host process drives n_devices GPUs:
 * one engine (weights replicated) and one worker thread per entry of `devices` (HIP device indices; an index may repeat,
 * e.g. {0, 0} = two engines on one GPU).  sts_multi_infer_ids_batch shards the B utterances by utterance -- longest first,
 * greedy, balanced by phoneme count, no exchange between devices -- runs every shard as one packed batch on its device
 * concurrently, and returns the PCM in INPUT order: pcm_out[b] is malloc()'d per utterance (release with sts_free),
 * n_out[b] = its sample count.  On any failure every output is released and a negative STS_E* code is returned.
 * The handle is not re-entrant (one batch at a time), like an engine. */
typedef struct sts_multi sts_multi;
int sts_multi_create(const float* blob, int64_t blob_bytes, const int32_t* devices, int32_t n_devices, sts_multi** out);
/*   How the PCM comes home.  STS_MULTI_AUTO (= sts_multi_create) and STS_MULTI_DOWNLOAD: every device downloads its own shard over
 *   PCIe.  STS_MULTI_RCCL (opt-in): one RCCL communicator rank per device (ncclCommInitAll; distinct devices required, one is
 *   allowed): sample counts and a "rank 0 can receive" word by ncclAllGather, the int16 PCM of ranks > 0 by ncclSend / grouped
 *   ncclRecv into a gather buffer on devices[0] (over xGMI), then ONE download.  A failure or a 60 s timeout inside a collective
 *   aborts all communicators of the handle (ncclCommAbort): that call returns STS_EDEVICE -- it never hangs -- and the handle
 *   continues with per-device downloads.  The RCCL path is not part of the automatic mode because it has not been run on N > 1 real
 *   devices yet.  sts_multi_gather_mode reports which one a handle uses (1 = RCCL). */
enum { STS_MULTI_AUTO = 0, STS_MULTI_RCCL = 1, STS_MULTI_DOWNLOAD = 2 };
int sts_multi_create_ex(const float* blob, int64_t blob_bytes, const int32_t* devices, int32_t n_devices, int32_t flags, sts_multi** out);
int sts_multi_gather_mode(const sts_multi* m);
/*   sts_multi_rccl_ranks: the size of the handle's communicator as RCCL reports it (ncclCommCount; 0 = no RCCL gather on this handle,
 *   -1 = the RCCL library has no ncclCommCount).  sts_multi_last_gather_ms: wall time rank 0 spent inside the last call's RCCL gather
 *   (count exchange, ready round, transfers, the one download; 0 in download mode).  sts_multi_set_conv_math: sts_set_conv_math on
 *   every engine of the handle. */
int sts_multi_rccl_ranks(sts_multi* m);
double sts_multi_last_gather_ms(const sts_multi* m);
int sts_multi_set_conv_math(sts_multi* m, int mode);
/*   sts_multi_set_noise: sts_set_noise for the handle; utterance b of a batch samples with seed + b (b = its index in the caller's
 *   batch, not within a device's shard: the PCM does not depend on the number of devices). */
int sts_multi_set_noise(sts_multi* m, float noise_scale, float noise_scale_w, uint64_t seed);
/*   sts_multi_set_output_rate: sts_set_output_rate on every engine of the handle; both gathers then exchange counts in output samples. */
int sts_multi_set_output_rate(sts_multi* m, int32_t rate);
/*   sts_multi_set_loudness (ABI 11): sts_set_loudness on every engine of the handle, modes 0 and 2 only (STS_EINVAL for 1). */
int sts_multi_set_loudness(sts_multi* m, int mode, float target_lufs, float peak_dbfs);
/*   sts_multi_set_limiter (ABI 13): sts_set_limiter on every engine of the handle. */
int sts_multi_set_limiter(sts_multi* m, int mode, float gain_db, float ceiling_dbfs, float lookahead_ms);
/*   sts_multi_set_eq: sts_set_eq on every engine of the handle. */
int sts_multi_set_eq(sts_multi* m, int32_t n_bands, const sts_eq_band* bands);
/*   sts_multi_set_duration_plan (ABI 14): sts_set_duration_plan for the NEXT sts_multi_infer_ids_batch of the handle, which must have the
 *   same B and n[b] (otherwise STS_EINVAL and nothing runs).  plans[b] belongs to utterance b of the caller's batch and follows it into its
 *   device's shard: the PCM does not depend on the number of devices. */
int sts_multi_set_duration_plan(sts_multi* m, int32_t B, const int32_t* n, const sts_dur_plan* plans);
/*   sts_multi_set_speaker_mix: sts_set_speaker_mix for the NEXT sts_multi_infer_ids_batch of the handle, which must have the same B
 *   (otherwise STS_EINVAL, nothing runs and the mix is dropped).  mixes[b] belongs to utterance b of the caller's batch and follows it into
 *   its device's shard: the PCM does not depend on the number of devices. */
int sts_multi_set_speaker_mix(sts_multi* m, int32_t B, const sts_speaker_mix* mixes);
/*   sts_multi_set_gain_plan: sts_set_gain_plan for the NEXT sts_multi_infer_ids_batch of the handle, which must have the same B and n[b]
 *   (otherwise STS_EINVAL, nothing runs and the plan is dropped).  plans[b] belongs to utterance b of the caller's batch and follows it into
 *   its device's shard: the PCM does not depend on the number of devices. */
int sts_multi_set_gain_plan(sts_multi* m, int32_t B, const int32_t* n, const sts_gain_plan* plans);
/*   sts_multi_set_pitch_plan: sts_set_pitch_plan for the NEXT sts_multi_infer_ids_batch of the handle, sharded like the gain plan. */
int sts_multi_set_pitch_plan(sts_multi* m, int32_t B, const int32_t* n, const sts_pitch_plan* plans);
/*   test hook: the shared library that provides the nccl* entry points (NULL / "" = librccl.so.1) and whether STS_MULTI_RCCL may list
 *   one device several times (tests/fake_rccl: N emulated ranks on one GPU; real RCCL refuses duplicates).  Only before the first
 *   STS_MULTI_RCCL handle of the process is created.  TEST-ONLY: refused with STS_ESTATE unless the process environment carries
 *   STS_TEST_HOOKS=1, so that no caller of the drop-in library substitutes the collective library or lifts the distinct-device check
 *   by accident. */
int sts_multi_set_rccl_library(const char* path, int allow_repeated_devices);
/*   layout of the gather buffer (host arithmetic only): rank r's block starts at offsets[r] samples (256-byte aligned);
 *   returns the buffer's extent in samples */
int64_t sts_multi_gather_layout(const int64_t* counts, int32_t n_ranks, int64_t* offsets);
void sts_multi_destroy(sts_multi* m);
int sts_multi_device_count(const sts_multi* m);
int sts_multi_speaker_num(const sts_multi* m);
int sts_multi_infer_ids_batch(sts_multi* m, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                              const float* length_scale, int16_t** pcm_out, int32_t* n_out);
/* the placement sts_multi_infer_ids_batch would use: device_slot_out[b] = index into `devices` (host logic only) */
int sts_multi_shard_of(const sts_multi* m, int32_t B, const int32_t* n, int32_t* device_slot_out);
const char* sts_multi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
