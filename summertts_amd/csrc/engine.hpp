// engine.hpp -- the batched acoustic pipeline on one MI355X: owns the HIP stream, the device-resident
// model, two workspace arenas (phoneme-level and frame-level) and a pinned staging buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <string.h>

#include <deque>
#include <map>
#include <unordered_map>
#include <string>
#include <vector>

#include "../../include/summertts_hip.h"
#include "kernels.hpp"
#include "live_stream.hpp"
#include "model.hpp"

namespace sts {

struct Arena {
    char* base = nullptr; size_t cap = 0, used = 0; bool measuring = false;
    void* alloc(size_t bytes) {
        size_t a = (used + 255) & ~(size_t)255;
        used = a + bytes;
        if (measuring) return nullptr;
        return base + a;
    }
    template <typename T> T* get(size_t count) { return (T*)alloc(count * sizeof(T)); }
};

// One member of a fused ResBlock layer's kernarg block from the layer's two packed convs: the one place that knows which copy of the weights
// each fused kernel reads (Engine::ResStage::fill_fused; sts_debug_resblock_layer).  h2: the two-term fp16 copies where both exist -- returns
// whether it took them (the caller then sets ResLayerGroup::math = 1 and its overflow word).
inline bool fill_res_member(const DConv& c1, const DConv& c2, const float* x, float* y, bool h2, ResLayerArgs& g) {
    g.x = x; g.y = y; g.w1 = c1.w; g.b1 = c1.bias; g.w2 = c2.w; g.b2 = c2.bias;
    g.k1 = c1.k; g.dil1 = c1.dil; g.k2 = c2.k; g.wu1 = c1.wu; g.wu2 = c2.wu;
    g.wb1 = c1.wb3; g.wb2 = c2.wb3p;
    if (!(h2 && c1.wh2 && c2.wh2p)) return false;
    g.wb1 = c1.wh2; g.wb2 = c2.wh2p; g.ws1 = c1.h2_scale; g.ws2 = c2.h2_scale;
    return true;
}

// one packed level of the pipeline: which segments, how long, how many positions in total
struct Lvl {
    SegView seg; int nb = 0; int max_len = 0; long total = 0; long ld = 0;
};

// The kernarg block of a column-block layer launch (col_layer.hip) in each of its forms: the one place that knows which copy of a packed
// conv the kernel reads (Engine::dds, the text encoder's output projection; sts_debug_col_layer).
// A DDSConv layer x -> y = x + gelu(LN2(conv1x1(gelu(LN1(dwconv(x))))))
inline void fill_col_dds(const DConv& sep, const DLn& n1, const DConv& pw, const DLn& n2, const float* x, float* y, const Lvl& lv, ColLayerArgs& g) {
    memset(&g, 0, sizeof(g));
    g.x = x; g.x_ld = lv.ld;
    g.dw_w = sep.w; g.dw_b = sep.bias; g.dw_k = sep.k; g.dw_dil = sep.dil; g.dw_pad = sep.pad; g.dw_ld = sep.Cout_pad;
    g.g1 = n1.g; g.b1 = n1.b;
    g.wc = pw.wc; g.bias = pw.bias;
    g.g2 = n2.g; g.b2 = n2.b; g.post_gelu = 1;
    g.res = x; g.res_ld = lv.ld; g.y = y; g.y_ld = lv.ld; g.C = pw.Cin;
    g.seg = lv.seg; g.B = lv.nb; g.max_len = lv.max_len;
}
// ... with the ConvFlow's 1 -> C input conv folded in: h = (w r + b) + g is the layer's input and residual; x = res = g, the rank-1 term
// from the conv's single input row (pre_in == null: the all-zero latent)
inline void fill_col_pre(const DConv& pre, const float* pre_in, const float* pre_res, ColLayerArgs& g) {
    g.x = pre_res; g.res = pre_res; g.xs_w = pre.w; g.xs_b = pre.bias; g.xr = pre_in;
}
// ... with the 29-row projection and the reverse spline step behind the layer
inline void fill_col_tail(const DConv& proj, float filter_sqrt, const float* r0, const float* r1, float* o0, float* o1, ColLayerArgs& g) {
    g.tp_w = proj.w; g.tp_b = proj.bias; g.tp_fs = filter_sqrt;
    g.tp_r0 = r0; g.tp_r1 = r1; g.tp_o0 = o0; g.tp_o1 = o1;
}
// The attention output projection with its residual and LayerNorm: y = LN(add + conv1x1(x))
inline void fill_col_oproj(const DConv& o, const DLn& n, const float* x, const float* add, float* y, const Lvl& lv, ColLayerArgs& g) {
    memset(&g, 0, sizeof(g));
    g.x = x; g.x_ld = lv.ld; g.wc = o.wc; g.bias = o.bias;
    g.add = add; g.add_ld = lv.ld; g.g2 = n.g; g.b2 = n.b; g.y = y; g.y_ld = lv.ld; g.C = o.Cin;
    g.seg = lv.seg; g.B = lv.nb; g.max_len = lv.max_len;
}

struct ConvOpt {
    int in_act = 0; float slope = 0.f; int reflect = 0;
    int epi = EPI_STORE, epi_flag = 0; float epi_scale = 1.f;
    const float* res = nullptr; long res_ld = 0;
    float* aux = nullptr; long aux_ld = 0;
    int16_t* pcm = nullptr;
    const float* ubias = nullptr;
    int pad_l = -1;            // override the left padding (FFN same_padding)
    int tile = -1;             // force a kernel variant for this conv (as sts_set_conv_mode - 2); -1 = automatic
    int kslices = 1; long kslice_stride = 0;   // cross-workgroup split of K into partial outputs (kernels.hpp ConvArgs::kslices)
    // the conv's input is the mean ((x + sum1) [+ sum2]) / nsum of tensors of x's geometry (kernels.hpp ConvArgs::nsum); where the kernel
    // the conv is routed to cannot form it while staging, Engine::conv materialises it into sum_dst (sum_n floats) first
    const float* sum1 = nullptr; const float* sum2 = nullptr; int nsum = 0; float* sum_dst = nullptr; long sum_n = 0;
};

// streaming decode (Engine::run_stream_steps): the PCM of every utterance is handed to `cb` chunk by chunk; cb returns non-zero to stop
// that utterance only.  delivered (optional, [B]): samples handed to cb per utterance
struct StreamSpec {
    int chunk_frames; int (*cb)(void* user, int32_t utt, const int16_t* pcm, int32_t n_samples, int32_t sample_offset); void* user;
    int32_t* delivered = nullptr;
};
int decoder_halo_frames(const Model& M);   // decoder.hip
struct WinGeom;                             // the windows of one decode pass (decoder.hip)
struct StreamRun;                           // what the steps of one streaming call share (engine.hip)
struct StreamTail;                          // the windows the output side of a step sees (engine.hip)
struct ParaStream;                          // the host side of an open paragraph (para_stream.hpp)
inline bool noise_scale_valid(float s) { return s >= 0.f && s <= 3.0e38f; }   // (false for NaN and +inf)
// sts_set_loudness: mode 0, 1 or 2, target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS (false for NaN)
inline bool loudness_args_valid(int mode, float target, float peak) {
    return mode >= 0 && mode <= 2 && target >= -70.f && target <= 0.f && peak >= -30.f && peak <= 0.f;
}
// sts_limiter_stats of B utterances from the limiter kernel's raw words [B][4] (limiter.hip)
void limiter_stats_decode(const unsigned* raw, int B, sts_limiter_stats* out);

struct Tap { std::vector<float> data; int channels = 0; long length = 0; };
// What the setters left for the NEXT call only, whatever its outcome, each kind as the run uploads it (Engine::run_setup):
struct PendingTables {
    // forced durations (sts_set_forced_durations): consumed by the duration stage of the run that uses them
    std::vector<int32_t> forced_dur; bool have_forced = false;
    // duration plan (duration_plan.hip), materialised for the whole batch: an utterance without a plan has rate 1 (w * 1.0f == w bit for
    // bit), fixed -1, target 0.  plan_n: the phoneme counts the next call must have
    std::vector<int32_t> plan_n, plan_fixed, plan_target; std::vector<float> plan_rate; bool have_plan = false;
    // speaker mix (misc_kernels.hip speaker_blend): the flattened term table (kernels.hpp SpeakerMixTab) for mix_B utterances with mix_K
    // terms in all
    std::vector<int32_t> mix_words; int mix_B = 0, mix_K = 0; bool have_mix = false;
    // gain plan (gain_plan.hip): q per phoneme of the whole batch (an utterance without a plan: 2^20 throughout, env == 1.0f), then h per
    // utterance.  gain_has[b]: entry b came with gain_db -- a planned open stream gives only those utterances columns of its phoneme pool
    std::vector<int32_t> gain_n, gain_words; std::vector<char> gain_has; bool have_gain = false;
    // pitch plan (pitch_plan.hip): the cents of the whole batch (0 for an utterance without a plan); pitch_has[b]: entry b came with cents
    std::vector<int32_t> pitch_n, pitch_cents; std::vector<char> pitch_has; bool have_pitch = false;
    void drop_call_tables() { have_plan = have_mix = have_gain = have_pitch = false; }      // (forced durations stay: their run consumes them)
    void drop_all() { drop_call_tables(); have_forced = false; }
};
// The split-bf16 repeat of a run sets up again from the same pending tables; the forced durations, which the first attempt's duration
// stage consumed, are pending again behind again()
struct KeepForced {
    PendingTables& t; const bool had;
    explicit KeepForced(PendingTables& tables) : t(tables), had(tables.have_forced) {}
    void again() { t.have_forced = had; }
};
class Engine;
// The tables of nb utterances (phoneme counts n, members[i] the tables of utterance i) on `eng` for its next run or admission, in the
// order duration plan, speaker mix, gain plan, pitch plan.  kinds < 0: a kind is set when a member carries it; otherwise the kinds of
// the mask (kTab*) are set.  A member without a kind that is set gets its empty entry.  On a failure nothing stays pending and the
// error is eng.error()
enum : int { kTabDuration = 1, kTabMix = 2, kTabGain = 4, kTabPitch = 8 };
int apply_utt_tables(Engine& eng, int nb, const int32_t* n, const UttTables* const* members, int kinds = -1);
constexpr int kNativeRate = 16000;   // every model of the reference produces 16 kHz (test/main.cpp:13,16)

class Engine {
public:
    ~Engine();
    int init(const float* blob, int64_t bytes, int device);
    int run(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const StreamSpec* ss = nullptr);
    int run_once(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const StreamSpec* ss);
    // streaming (sts_infer_ids_batch_stream; sts_infer_ids_stream is its B == 1): B utterances, chunk k of every live one decoded as the
    // windows of one pass per step.  n_total (optional, [B]): samples delivered per utterance
    int run_batch_stream(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, int chunk_frames,
                         int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* n_total);
    const std::string& error() const { return err_; }

    Model model;
    int device = 0;
    // results of the last run
    std::vector<int32_t> n_samples;    // per utterance
    int64_t total_samples = 0;
    int16_t* d_pcm = nullptr;          // device, packed (the mapped pinned HOST buffer when pcm_in_host_: use pcm_hbm() where a true device buffer is required)
    // the last run's PCM in HBM, or null when no HBM copy exists (pcm_in_host_: the kernels wrote it over the host link) -- what RCCL
    // transfers and device-to-device copies must use (xGMI / D2D traffic out of host memory by accident)
    const int16_t* pcm_hbm() const { return pcm_in_host_ ? nullptr : d_pcm; }
    float host_us_setup_ = 0, host_us_enq_ = 0;
    double host_t0_ = 0, host_t_sync_ = 0;   // steady-clock microseconds: entry of the run, return of its last stream synchronisation
    bool pcm_in_host_ = false;         // this run's PCM was written by the kernels into the pinned host buffer (d_pcm is its device-side address; no HBM copy exists)
    const int16_t* h_pcm = nullptr;    // host copy of the last run's PCM (pinned, engine-owned) when host_pcm is set, else null
    bool host_pcm = false;             // download the PCM as part of run(): one stream sync per call instead of two
    std::vector<int32_t> durations_h;  // packed
    std::map<std::string, Tap> taps;
    sts_profile prof{};
    // controls
    // sampling noise (sts_set_noise): prior scale ns, SDP latent scale nsw, seed of utterance 0 (utterance b of a call: seed + b)
    struct Noise { float ns = 0.f, nsw = 0.f; uint64_t seed = 0; };
    Noise noise;
    std::vector<Noise> noise_utt;      // when it holds B entries: the per-utterance settings of a B-utterance run instead (sts_pool, sts_multi)
    // output sample rate (sts_set_output_rate): kNativeRate = the decoder's own samples, nothing extra runs; otherwise every call's PCM is
    // the decoder's float wave resampled on the device (resample.hip).  rs: the filter; d_rs_table: its [P][2K] table, uploaded by set
    int out_rate = kNativeRate;
    ResampleDesign rs;
    float* d_rs_table = nullptr;
    bool resampling() const { return out_rate != kNativeRate; }
    long long out_count(long long native) const { return resampling() ? (native * rs.P + rs.Q - 1) / rs.Q : native; }   // L_out = ceil(L_in P / Q)
    int set_output_rate(int rate);
    int stream_halo(bool warped = false) const;           // decoder halo frames of a streaming chunk at the current rate (+ the resampler's K samples)
    // loudness (sts_set_loudness, loudness.hip): 0 off (nothing extra runs), 1 measure every utterance of a whole-utterance call, 2 measure
    // and cast each utterance with its own gain.  Measured on the float wave at the output rate; loud_res: the last call's results, one per
    // utterance (empty after a call in mode 0, a streaming call or a failure)
    int loud_mode = 0; float loud_target = -16.f, loud_peak = -1.f;
    std::vector<sts_loudness> loud_res;
    int set_loudness(int mode, float target, float peak);
    // look-ahead peak limiter (sts_set_limiter, limiter.hip): 0 off (nothing extra runs), 1 every utterance of a whole-utterance call is
    // scaled by G (times its loudness gain under loudness mode 2, which then drops its peak clamp) and held under the ceiling; the limiter
    // writes the PCM.  lim_res: the last call's results, one per utterance (empty after a call with it off, a streaming call or a failure)
    int lim_mode = 0; float lim_gain_db = 0.f, lim_ceiling = -1.f, lim_ms = 5.f;
    std::vector<sts_limiter_stats> lim_res;
    int set_limiter(int mode, float gain_db, float ceiling_dbfs, float lookahead_ms);
    // the tables of the NEXT call only, whatever its outcome (sts_set_forced_durations, sts_set_duration_plan, sts_set_speaker_mix,
    // sts_set_gain_plan, sts_set_pitch_plan): run() drops them when the call returns, so the conv-math-3 repeat of a call applies them
    // again.  A setter validates and materialises here; an invalid table changes nothing; B == 0 or null drops a pending one.  A pitch
    // plan is for whole-utterance calls only: the run multiplies its duration plan's rates by the ratios (run_setup), lays the warp out
    // on the host when the durations arrive (pitch_geometry) and launches the warp kernel behind the gain kernel (decode_end)
    PendingTables pend;
    void set_forced_durations(const int32_t* dur, int64_t count);
    int set_duration_plan(int B, const int32_t* n, const sts_dur_plan* plans);
    int set_speaker_mix(int B, const sts_speaker_mix* mixes);
    int set_gain_plan(int B, const int32_t* n, const sts_gain_plan* plans);
    int set_pitch_plan(int B, const int32_t* n, const sts_pitch_plan* plans);
    void drop_tables() { pend.drop_all(); }
    // a pending pitch plan and a call form that cannot apply one: the plan is dropped and the call refused
    bool refuse_pitch(const char* what) {
        if (!pend.have_pitch) return false;
        pend.have_pitch = false; err_ = std::string("a pitch plan is pending: ") + what + " cannot apply one (the plan is dropped)";
        return true;
    }
    int speaker_embedding(int sid, float* out, int64_t capacity) const;
    // paragraph join (sts_infer_ids_joined, join.hip): run_joined() runs the B sentences as run() would and joins their native float waves
    // into one signal in front of the resampler, loudness, the limiter and the cast.  join_on: the run in progress joins; join_sil: silence
    // frames in front of each sentence (kernels.hpp join_silence), join_total_sil: lead + every gap + trail; join_h: the fade in samples.
    // last_join_start: sentence starts of the last run in native samples (empty: it was not a joined run)
    bool join_on = false; std::vector<int32_t> join_sil; long long join_total_sil = 0; int join_h = 0;
    std::vector<int64_t> last_join_start;
    int run_joined(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const sts_join* join, const StreamSpec* ss = nullptr);
    int join_offsets(int64_t* start, int64_t capacity);
    // phoneme start offsets of the last run in output samples, packed like durations_h (sts_get_phoneme_offsets); last_n: its phoneme counts
    std::vector<int32_t> last_n;
    int phoneme_offsets(int64_t* start, int64_t capacity);
    bool record_taps = false; int profiling = 0;       // profiling: 0 off, 1 all stage events, 2 the matrix-core region's two events only (sts_set_profiling)
    int conv_mode = 0;
    int conv_math = 3;                 // 0 = split-bf16 trunk convs (conv_bf3.hip), 1 = exact-fp32 MFMA, 3 = two-term fp16 (sts_set_conv_math)
    long h2_fallbacks = 0;             // runs repeated in split-bf16 because an activation left fp16's range (conv_math 3)
    int h2_consecutive = 0; bool h2_disabled = false;   // two repeats in a row: the engine stays on split-bf16 until sts_set_conv_math
    double products() const { return conv_math == 3 ? 3.0 : 6.0; }     // 16-bit matrix products per fp32 product
    int pcm_direct = 1;                // 1: with host_pcm, a one-utterance call's last kernel writes the PCM into the pinned host buffer itself (no download behind it) (STS_DBG_PCM_DIRECT)
    int dds_tail = 1;                  // 1: a ConvFlow's 29-row projection and spline step ride in its last DDSConv layer's launch (col_layer.hip tail) (STS_DBG_DDS_TAIL)
    int attn_reg = 1;                  // 1: one-query attention with its operands in registers (attention_reg_kernel) where the shape allows (STS_DBG_ATTN_REG)
    int attn_block_min_wgs = 96;       // attention_mfma_kernel from this many workgroups on (sts_debug_set)
    int launch_ahead = 1;              // 1: a one-utterance call the engine has served before enqueues flow + decoder before the frame count is on the host; 2 (tests): the memo is keyed by the phoneme count alone (sts_debug_set STS_DBG_LAUNCH_AHEAD)
    long ahead_misses = 0;             // launch-ahead calls whose count fell outside the predicted 64-frame bucket (a hash collision; repeated the waiting way)
    // the launch-ahead memo: hash of an utterance's (ids, speaker, length scale [, nsw, seed when nsw != 0]) -> its frame count (a pure
    // function of them); the last kMemoEntries distinct utterances, FIFO
    static constexpr size_t kMemoEntries = 1024;
    std::unordered_map<unsigned long long, long> seen_tf_; std::deque<unsigned long long> seen_order_;
    // Host waits of a run (the frame counts of a request the engine has not served before; the run's final stream synchronisation).  A direct
    // caller's thread polls them (lowest latency: it asked for one utterance now).  sts_pool / sts_multi workers set polite_wait: their thread
    // SLEEPS through ~80 % of the expected wait and polls only the tail, so N engines do not cost N host cores.  The
    // expectation is a running estimate per size class (log2 of the batch's phoneme count), scaled down for a smaller request of the class.
    bool polite_wait = false;
    struct WaitEst { double us = 0.0; long phonemes = 0; };
    WaitEst wait_est_[2][24];              // [0] frame counts, [1] final synchronisation
    void nap_before_wait(int which, long phonemes);
    void note_wait(int which, long phonemes, double waited_us, bool was_ready_at_wake);
    int final_sync(long phonemes);
    int ups_rowph = 1;                 // upsamplers: 1 the row-interleaved-phase copies (ConvArgs::rowph: whole-sector stores), 0 phase-major rows (sts_debug_set)
    int tail_fused = 1;                // MB-iSTFT / MS-iSTFT tail: 1 spectrum + inverse DFT / overlap-add + synthesis filter + int16 cast as one launch, 0 three (sts_debug_set)
    int chain_streams_dbg = -1;        // lab: stage mask -- the chains of the masked decoder stages as per-chain launches on three prioritised streams instead of grouped launches
    int h2p = 1;                       // 1: the wide ResBlock stages (C % 128 == 0) on pre-split channel-minor activations (conv_h2p.hip; two-term fp16 arithmetic only), 0: the staged kernels
    int h2p_tile = -1;                 // lab: tile code of conv_h2p_group (-1: automatic)
    int flow_fused = 1;                // 1: the reverse flow as one launch per WaveNet layer where eligible (wn_flow.hip; two-term fp16 arithmetic only),
                                       // 16-frame tiles where 32-frame tiles would leave half the CUs without a workgroup; 0: one launch per conv;
                                       // 2 / 3: one launch per layer at any size, 32- / 16-frame tiles (sts_debug_set STS_DBG_FLOW_FUSED)
    int col_proj_mode = 1;                  // text encoder, the q/k/v projection and the producer of its input (col_layer.hip col_proj_kernel): 1 one launch -- all
                                       // passes in one workgroup from 24 column blocks on, one workgroup per (column block, pass) below; 0: the producer and
                                       // the conv as two launches; 2 / 3: one launch at any size, passes in one workgroup / split (sts_debug_set STS_DBG_COL_PROJ)
    int sdp_pre_ride = 1;              // 1: the stochastic duration predictor's `pre` conv as one more workgroup per column block of the encoder's output
                                       // projection launch where eligible, 0: a conv launch of its own (sts_debug_set STS_DBG_SDP_PRE_RIDE)
    int n_cus = 0;                     // compute units of the device (init)
    int stream_retry_step = -1;        // tests (STS_DBG_STREAM_RETRY_STEP): a stream (of one utterance or several) under conv_math 3 treats the overflow word as raised after step k; -2: every admission into an open stream does (it is repeated in form 0)
    int stream_direct = 0;             // streaming, any B: 1 the pack / resample / limiter kernel writes each step's chunks into mapped pinned host memory, 0 one download (STS_DBG_STREAM_DIRECT)
    unsigned poison = 0;               // tests (STS_DBG_POISON): 32-bit pattern every call fills its workspace arenas and host outputs with; 0 = off
    int64_t poison_bytes_ = 0;         // bytes the current call has filled so far (sts_profile.poison_bytes)
    hipStream_t stream = nullptr;

private:
    int fail(int code, const std::string& msg) { err_ = msg; return code; }
    bool ensure(Arena& a, size_t bytes);
    bool ensure_pinned(size_t bytes);
    void poison_arena(const Arena& a);                 // STS_DBG_POISON: the arena's laid-out extent, on the engine's stream
    void poison_host16(void* p, size_t samples);       // STS_DBG_POISON: host-visible int16 output, the pattern's low 16 bits
    void poison_host32(void* p, size_t words);         // STS_DBG_POISON: host-visible 32-bit output words
    ConvArgs conv_args(const DConv& c, const float* x, const Lvl& lin, float* y, const Lvl& lout, const ConvOpt& o, double* flops);
    void conv(const DConv& c, const float* x, const Lvl& lin, float* y, const Lvl& lout, const ConvOpt& o);
    void ln(const DLn& l, const float* a, const float* b, const float* res, float* y, const Lvl& lv, int pre_relu, int post_gelu, int nb = 1, long b_stride = 0);
    int pick_kslices(const DConv& c, const Lvl& lout) const;
    // (tail: the ConvFlow's projection + reverse spline step, run inside the last layer's launch when it can take them; *tail_done says so)
    struct SplineTail { const DConv* proj; float filter_sqrt; const float* r0; const float* r1; float* o0; float* o1; };
    float* dds(const DDds& d, float* h, float* t1, float* t2, const Lvl& lv, const DConv* pre = nullptr, const float* pre_in = nullptr,
               const float* pre_res = nullptr, const SplineTail* tail = nullptr, bool* tail_done = nullptr);
    int run_any_math(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const StreamSpec* ss);
    struct RunCtx;                  // what the stages of one run share (run_ctx.hpp)
    struct ResStage;                // the ResBlock chains of one decoder stage (decoder.hip)
    int run_setup(RunCtx& c);
    int run_text_encoder(RunCtx& c);
    int run_durations(RunCtx& c);
    int run_frame_workspace(RunCtx& c);
    int run_flow(RunCtx& c);
    int run_decode(RunCtx& c, int nw, long Wtot, int maxW, int zoff0, int wlen0);
    int decode_end(RunCtx& c, const float* wave, const WinGeom& win, long Wtot, int maxW);
    int wait_frame_counts(RunCtx& c);
    int plan_output(RunCtx& c);
    int frame_geometry(RunCtx& c);
    int run_output(RunCtx& c);
    int run_stream_steps(RunCtx& c);
    int stream_host_buffers(RunCtx& c, StreamRun& s);                        // the pinned table room and the chunks' host buffer
    void stream_tail(RunCtx& c, const StreamRun& s, const StreamTail& t);    // a step's launches behind the decoder (the join)
    int stream_loud_gate(RunCtx& c, StreamRun& s);                           // a measuring stream's gate, once behind the last step
    int live_loud_gate(RunCtx& c, StreamRun& s, int n);                      // a measuring open stream's gate over n retiring slots of a step
    int stream_admit_once(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, int32_t* slot_out,
                          int32_t* n_samples_out, int32_t* admitted);
    int para_append_once(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const long long* gap,
                         int32_t* frames_out, int64_t* start_out, int32_t* appended);
    int ensure_overflow_word();
    template <typename Valid>       // what the four table setters share (engine.hip)
    bool table_begin(const char* what, bool given, bool& have, int B, const int32_t* n, bool with_n, int max_B, const char* over, long* total, int* rc,
                     Valid&& valid);
    void tap(const char* name, const float* d, int channels, long ld, long length);
    void stage_begin(int s);
    void mark(int i);

    std::string err_;
    Arena arenaT_, arenaF_;
    char* pinned_ = nullptr; size_t pinned_cap_ = 0;
    char* pinned_pcm_ = nullptr; size_t pinned_pcm_cap_ = 0;
    int16_t* pinned_pcm_dev_ = nullptr;   // the same buffer as the GPU sees it (mapped): the last kernel of a small call writes the PCM straight into it
    unsigned* ovf_host_ = nullptr; unsigned* ovf_ = nullptr;              // conv_math 3: overflow word (host-mapped) and its device address
    int* hmap_ = nullptr; int* hmap_dev_ = nullptr; size_t hmap_cap_ = 0;   // host-mapped result block of the durations kernel
    unsigned* arrive_ = nullptr; int seq_ = 0;
    float* loud_host_ = nullptr; float* loud_dev_ = nullptr; int loud_cap_ = 0;   // host-mapped sts_loudness[loud_cap_]: the gating kernel's results
    LoudCoef loud_k_{}; int loud_k_rate_ = 0;                                     // the kernels' filter tables for loud_k_rate_
    unsigned* lim_host_ = nullptr; int lim_cap_ = 0;                              // pinned: the limiter's raw result words [lim_cap_][4], downloaded behind its launch
    hipEvent_t ev_[8] = {};
    static constexpr int kAux = 3;            // ResBlock chains of one decoder stage run concurrently
    hipStream_t aux_[kAux] = {};
    hipEvent_t ev_fork_ = nullptr, ev_join_[kAux] = {};
    hipEvent_t ev_setup_ = nullptr;      // behind run_setup's upload of the pinned staging block (batches)
    hipStream_t cur_ = nullptr;               // stream the conv()/ln() helpers launch on
    bool have_events_ = false;
    int cur_stage_ = 0;
    double flops_[4] = {0, 0, 0, 0};
    double bytes_[4] = {0, 0, 0, 0};
    double bytes_w_[4] = {0, 0, 0, 0};       // the weight share of bytes_ (does not scale with the positions)
    double mfma_flops_ = 0, mfma_exec_ = 0, bf16_exec_ = 0, sync_wait_ms_ = 0; int mfma_launches_ = 0; bool in_mfma_region_ = false;
    EqTable* d_eq_ = nullptr; int eq_tab_rate_ = 0; bool eq_dirty_ = true;        // the EQ's tables on the device, the rate they were built for
    int eq_prepare();                                                             // a run with an EQ: the bands against the current rate, the tables
    float* d_pitch_table_ = nullptr;   // the prototype on the device, uploaded by the first run with a pitch plan
    int pitch_geometry(RunCtx& c);     // a run with a pitch plan, when its durations are on the host: the layout, its upload, the counts
public:
    // parametric equaliser (sts_set_eq, eq.hip): eq_n bands, 0 = off (nothing extra runs).  Every whole-utterance call filters the float
    // wave at the output rate in front of loudness and the limiter; with neither downstream the EQ kernel writes the PCM.  The device
    // tables are built and uploaded by the first run after a change of the bands or the output rate (eq_prepare), not per call
    int eq_n = 0; sts_eq_band eq_bands[STS_EQ_MAX_BANDS] = {};
    int set_eq(int n_bands, const sts_eq_band* bands);
    // a joined stream (sts_infer_ids_joined_stream): run_joined with a StreamSpec -- front and flow once as the packed batch, then
    // run_stream_steps walks the JOINED time axis (join_stream.hpp): the callback's utterance is always 0, a non-zero return ends the call.
    // n_total (optional): samples delivered
    int run_joined_stream(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const sts_join* join,
                          int chunk_frames, int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* n_total);
    // an open stream (sts_stream_open .. sts_stream_close; live_stream.hpp, DESIGN.md 9c "Open streams"): one per engine.  stream_open fixes
    // the chunk size, the output rate, the limiter setting, the conv mode and the conv math, and allocates the latent pool
    // [inter_channels][capacity_frames] by its own hipMalloc (never in arenaF_: every later run lays that out again and may reallocate it).
    // stream_admit runs front and flow of B newcomers as the packed batch a sts_infer_ids_batch_stream call of them would, and moves their z
    // into the pool (adopt_z); all or nothing (*admitted = B, or 0: no room now).  stream_step is ONE step of run_stream_steps over every
    // live slot in ascending slot order, each at its own next frame; a slot retires behind its last chunk or when its callback returns
    // non-zero.  While a stream is open every other run and every setter of what open fixed returns STS_ESTATE.  With eq_streaming the
    // EQ, and with loud_streaming loudness mode 1, run from per-slot state in pools allocated at open (live_stream.hpp "per-slot filter
    // state"); the slots a step retires are gated inside it, their results in loud_res with their slots in loud_slots.  Refused by
    // stream_open: EQ bands and mode 1 without their stream modes, mode 2, record taps, and a duration plan / speaker mix / gain plan /
    // forced durations pending AT OPEN (a pending table belongs to a next run, and open is not one).  Not to be called from a chunk callback.
    // capacity_phonemes > 0: a PLANNED stream (sts_stream_open_ex; live_stream.hpp, DESIGN.md 9c "Planned open streams").  Its four table
    // setters work while it is open and apply to the next stream_admit only, whatever its outcome; what a step needs of them (each slot's
    // conditioning vector, a gain-planned slot's cum / q columns and {off, n, h}) moves into pools of the stream's own at admission
    // (adopt_tables, one launch next to adopt_z), and a step reads them by slot.  0: exactly the stream above.
    int stream_open(int chunk_frames, int max_live, long long capacity_frames, long long capacity_phonemes = 0);
    int stream_admit(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const sts_stream_noise* noise,
                     int32_t* slot_out, int32_t* n_samples_out, int32_t* admitted);
    int stream_step(int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* live_after);
    int stream_close();
    bool stream_is_open() const { return live_ != nullptr || para_ != nullptr; }      // "open": an open stream or an open paragraph
    LiveStream* live_ = nullptr;       // null: no stream is open
    // an open paragraph (sts_para_open .. sts_para_close; para_stream.hpp, DESIGN.md 9i "Open paragraphs"): ONE joined stream per engine
    // whose sentences are appended between its steps.  para_open fixes what stream_open fixes and the join's lead and fade, and allocates
    // the latent pool; para_append runs front and flow of B new sentences as the packed batch a joined call of those B would (global
    // sentence i samples with seed + i) and moves their z into the pool; para_step is ONE step of run_stream_steps with the join and the
    // pool both set -- the next chunk of J if the frontier rule lets it leave, its callback's utterance always 0.  While a paragraph is open
    // the engine refuses what it refuses while a stream is open, and sts_stream_open too.  Not to be called from a chunk callback.
    int para_open(int chunk_frames, int max_resident, long long capacity_frames, int lead_frames, float fade_ms);
    int para_append(int B, const int32_t* const* ids, const int32_t* n, const int32_t* sid, const float* ls, const int32_t* gap_frames,
                    int32_t* frames_out, int64_t* start_out, int32_t* appended);
    int para_finish(int trail_frames);
    int para_step(int (*cb)(void*, int32_t, const int16_t*, int32_t, int32_t), void* user, int32_t* ready_after);
    int para_close();
    ParaStream* para_ = nullptr;       // null: no paragraph is open
    // a measuring open stream: the slots retired by the most recent step that measured, ascending -- loud_res holds their results in
    // this order (sts_stream_get_loudness)
    std::vector<int32_t> loud_slots;
    // first output of every phoneme of the last run in native samples of the WARPED signal, packed like durations_h (empty: the last run
    // had no pitch plan): what sts_get_phoneme_offsets converts instead of frames * hop
    std::vector<int64_t> last_pitch_start;
    // a pitch plan in a closed stream (sts_set_pitch_streaming; pitch_plan.hip's range form, pitch_stream.hpp): off, a stream with a plan
    // pending is refused; on, sts_infer_ids_stream and sts_infer_ids_batch_stream run it through the range warp
    bool pitch_streaming = false;
    // loudness in a stream (sts_set_loudness_streaming; loudness.hip's stream mode, loud_stream.hpp): off, a stream under mode 1 or 2 is
    // refused; on, mode 1 measures what each step delivers from a state carried per utterance in the frame arena (mode 2 stays refused)
    bool loud_streaming = false;
    // the equaliser in a stream (sts_set_eq_streaming; eq.hip's stream mode, eq_stream.hpp): off, a stream with bands set is refused; on,
    // every step runs the EQ behind the resampler on its windows from a state carried per utterance in the frame arena
    bool eq_streaming = false;
};

}  // namespace sts
