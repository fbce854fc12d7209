// run_ctx.hpp -- internal to the engine's translation units (engine.hip, decoder.hip): the workspace pointers and the context the stages
// of one run share.
#pragma once
#include "engine.hpp"
#include "eq_stream.hpp"
#include "loud_stream.hpp"
#include "out_chain.hpp"
#include "join_stream.hpp"
#include "stream_step.hpp"

namespace sts {

#define HIPCK(call)                                                                           \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) return fail(STS_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

struct BufT {
    int *meta_i; float* ls; float *ns, *nsw; uint64_t* seed; int* ids; int* forced;
    float *x, *qkv, *att, *y, *x1, *ffh, *m, *logs;
    float *dh, *dt1, *dt2, *dc, *dhh, *dp29, *dr[4], *dlogw;
    int *dur, *cum, *frames;
    float *g, *cond_dp, *cond_dec, *cond_wn;
    // a run with a duration plan only (null otherwise): the uploaded plan [rate Ttot | fixed Ttot | target B] between ids and forced, the
    // plan kernel's remainder scratch, w for the "dur_w" tap
    float* plan_rate; int *plan_fixed, *plan_target; long long* plan_rem; float* dur_w;
    // a run with a speaker mix only (null otherwise): the uploaded term table (kernels.hpp SpeakerMixTab) right behind the ids
    int* mix;
    // a run with a gain plan only (null otherwise): the uploaded table [q Ttot | h B] behind the mix
    int *gain_q, *gain_h;
    // a joined run only (null otherwise): the uploaded silence table [B] behind the gain plan's (JoinArgs::sil)
    int* join_sil;
    // a run with a pitch plan only (null otherwise): the warp's tables (kernels.hpp PitchTables::words, sized at setup for the planned
    // members' phonemes) and, behind them, the window table of the warped signals [off B | off B | N' B] (decoder.hip WinGeom)
    long long* pitch_words; int* pitch_win;
};
struct BufF {
    float *z, *h, *acts, *out, *x0, *regA, *regB, *tailA, *tailB, *tailC, *wave, *fliptmp;
    float *ff_h[2], *ff_part[2], *ff_macc[2], *ff_alt;        // one-launch-per-layer flow (wn_flow.hip): channel-minor h / partial sums / -m slices, alternate home of a z half
    // the output chain (out_chain.hpp): a buffer exists iff a stage of this run reads or writes it, and is null otherwise.  pcm: the returned
    // PCM; pcm_nat / pcm_rs: the tail's / the resampler's int16 samples (pcm when that stage is the writer, else scratch); wave_*: the
    // stages' float outputs (wave above: the tail's); lws / limws / eqws: stage workspaces; streaming: the step tables (stream_step.hpp StepTab),
    // stream_pack's packed chunk buffer, the per-window speaker vectors and conditioning of a multi-speaker HiFi-GAN decoder
    // (members in the order they were added: the layout every earlier build measured with)
    int16_t* pcm;
    int16_t* pcm_nat; float* wave_out;
    int16_t* pcm_rs; char* lws;
    char* limws; float* wave_lim;
    float* wave_gain;
    float* wave_join;
    char* stab; int16_t* spack; float *gwin, *cond_win;
    float* wave_eq; char* eqws;
    float* wave_pitch;         // a run with a pitch plan only (null otherwise): the warped signals, packed back to back
    // a stream that runs the EQ only (null otherwise): the carried state [B][2] slots (eq_stream.hpp) and the step's tile end states
    char* eqst; double* eqsE;
    // a stream that measures loudness only (null otherwise): the carried state [B][2] slots (loud_stream.hpp), the step's tile end states,
    // the call's result tables (lds_res_bytes)
    char* ldst; double* ldsE; char* ldres;
};
// Everything a run's stages share: batch geometry, workspace pointers, host / device tables.  Engine::run() fills it stage by
// stage; the stage functions below see its fields under the names the pipeline has always used (RUN_ALIASES).
struct Engine::RunCtx {
    int B = 0; const int32_t* const* ids = nullptr; const int32_t* n = nullptr; const int32_t* sid = nullptr; const float* ls = nullptr;
    const StreamSpec* ss = nullptr;
    std::vector<int> offT, lenT; long Ttot = 0; int maxT = 0;
    int H = 0, C = 0, FF = 0, fdp = 0, wnH = 0, wnL = 0, ffn2_slices = 1;
    Lvl lvT, lvB, lv1;
    BufT bt; BufF bf;
    size_t up_bytes = 0;
    int *pm = nullptr, *p_offT = nullptr, *p_lenT = nullptr, *p_sid = nullptr, *p_offF = nullptr, *p_lenF = nullptr, *p_one = nullptr;
    int *d_offT = nullptr, *d_lenT = nullptr, *d_sid = nullptr, *d_offF = nullptr, *d_lenF = nullptr, *d_one = nullptr, *d_win = nullptr;
    bool inl = false, no_inline_seg = false, ms = false;
    bool dh_in_enc = false;         // the stochastic duration predictor's `pre` conv ran inside the text encoder's last launch (bt.dh is written)
    long Ftot = 0; int maxF = 0, hop = 0;
    // One utterance (the reference's own call shape): buffers, leading dimensions and every dispatch decision use the frame CAPACITY
    // Fld = the count rounded up to a bucket of 64 frames, so that a call which launches the flow and the decoder AHEAD of the frame count
    // (ahead: the count is predicted, the kernels read the real one from device memory) makes exactly the dispatch decisions of a call
    // that waited for it -- and returns bit-identical samples.  Batches: Fld == Ftot, nothing changes.
    long Fld = 0; int maxFld = 0; bool ahead = false, ahead_b = false, mapped = false, forced = false;
    bool plan = false;              // this run applies a duration plan (sts_set_duration_plan): never launched ahead, never in the memo
    bool gain = false;              // this run applies a gain plan (sts_set_gain_plan): the gain kernel runs behind the decoder's tail; never launched ahead, never in the memo
    bool join = false;              // this run joins its sentences into one signal (sts_infer_ids_joined): the join kernel runs behind the decoder's tail (and the gain kernel); never launched ahead, never in the memo
    long long FJ = 0;               // a joined run: frames of the joined signal (sum of the sentences' + lead + gaps + trail)
    // this run applies a pitch plan (sts_set_pitch_plan): the warp kernel runs behind the gain kernel; never launched ahead, never in the
    // memo.  Made by pitch_geometry when the durations are on the host: pitch_rows (the tables' per-phoneme length), every utterance's
    // warped sample count, their sum and maximum
    bool pitch = false; long long pitch_rows = 0, pitch_total = 0, pitch_max = 0; std::vector<long long> pitch_nout;
    std::vector<long long> pitch_words_h;     // a stream through the warp: the tables on the host, for every step's geometry (pitch_stream.hpp)
    bool mix = false;               // this run blends speakers (sts_set_speaker_mix): bt.g comes from speaker_blend; never launched ahead, never in the memo
    std::vector<Engine::Noise> nz; bool any_ns = false, any_nsw = false;   // per-utterance sampling noise (engine.hpp Noise), which of the two is used
    std::vector<unsigned long long> req_keys; std::vector<long> predF;      // launch-ahead memo: per-utterance request hashes, remembered frame counts (empty: not all known)
    int halo = 0; long Wcap = 0; int upS = 1; long Lsb = 0; int sbC = 0;
    long long Ocap = 0;             // PCM capacity in output samples (== Wcap * hop at the native rate)
    bool bstream = false;           // a stream of several utterances: window i of a step is not utterance i (run_decode gathers the conditioning per window)
    bool use_ff = false; int ffG = 0, ffNT = 32;     // the one-launch-per-layer flow: taken, its channel groups, output frames per workgroup (32 / 16)
    // the output chain of this run (Engine::plan_output), and next to it the limiter's design, the resampler's ratio (1 / 1: native rate)
    // and the EQ's band count
    OutChain oc{}; LimiterDesign limd; int rsP = 1, rsQ = 1, eqS = 0;
    const float* stage_out(int s) const {      // the float output of stage s (null: it has none in this run)
        const float* const o[OS_COUNT] = {bf.wave, bf.wave_gain, bf.wave_join, bf.wave_out, nullptr, bf.wave_eq, nullptr, bf.wave_lim};
        return s < 0 ? nullptr : o[s];
    }
    // (behind everything else) a joined stream: its step geometry, made when the frame counts arrive
    JsPlan js;
    // (and behind that) one step of an open stream (Engine::stream_step, live_stream.hpp): "utterance" b of this context is the live slot
    // live_slots[b], its z lies at its own offset in the stream's pool (bf.z, leading dimension Fld = the pool's capacity), and its chunk
    // starts at its own next frame.  Null: a closed call
    LiveStream* live = nullptr; std::vector<int> live_slots;
    // an admission into an open stream (Engine::stream_admit_once): front and flow alone -- no output stage runs, so the frame workspace
    // holds no carried EQ / loudness state, step workspace or result tables
    bool admission = false;
    // (and behind that) one step of an open paragraph (Engine::para_step, para_stream.hpp): `join` and `live` are both set.  js is the
    // paragraph's plan as far as it is known, the step is chunk para_k of it alone, sentence b's z lies at para_zoff[b] of the pool and
    // speaks as para_sid[b] (b: the plan's index); para_stop: the chunk's callback ended the paragraph.  para_k < 0: no paragraph
    long long para_k = -1; const int* para_zoff = nullptr; const int* para_sid = nullptr; bool para_stop = false;
};
#define RUN_ALIASES(c)                                                                                                              \
    [[maybe_unused]] Model& M = model;                                                                                              \
    [[maybe_unused]] const int B = (c).B; [[maybe_unused]] const StreamSpec* const ss = (c).ss;                                     \
    [[maybe_unused]] const long Ttot = (c).Ttot; [[maybe_unused]] const int maxT = (c).maxT;                                        \
    [[maybe_unused]] const int H = (c).H, C = (c).C, FF = (c).FF, fdp = (c).fdp, wnH = (c).wnH, wnL = (c).wnL, ffn2_slices = (c).ffn2_slices; \
    [[maybe_unused]] Lvl &lvT = (c).lvT, &lvB = (c).lvB, &lv1 = (c).lv1;                                                            \
    [[maybe_unused]] BufT& bt = (c).bt; [[maybe_unused]] BufF& bf = (c).bf;                                                         \
    [[maybe_unused]] const size_t up_bytes = (c).up_bytes;                                                                          \
    [[maybe_unused]] int* const pm = (c).pm; [[maybe_unused]] int* const p_offF = (c).p_offF; [[maybe_unused]] int* const p_lenF = (c).p_lenF; \
    [[maybe_unused]] int* const d_sid = (c).d_sid; [[maybe_unused]] int* const d_offF = (c).d_offF; [[maybe_unused]] int* const d_lenF = (c).d_lenF; \
    [[maybe_unused]] int* const d_win = (c).d_win;                                                                                  \
    [[maybe_unused]] const bool inl = (c).inl, no_inline_seg = (c).no_inline_seg, ms = (c).ms;                                      \
    [[maybe_unused]] const long Ftot = (c).Ftot; [[maybe_unused]] const int maxF = (c).maxF, hop = (c).hop;                         \
    [[maybe_unused]] const long Fld = (c).Fld; [[maybe_unused]] const int maxFld = (c).maxFld; [[maybe_unused]] const bool ahead = (c).ahead; \
    [[maybe_unused]] const int halo = (c).halo; [[maybe_unused]] const long Wcap = (c).Wcap, Lsb = (c).Lsb;                         \
    [[maybe_unused]] const int upS = (c).upS, sbC = (c).sbC;                                                                        \
    [[maybe_unused]] const bool use_ff = (c).use_ff; [[maybe_unused]] const int ffG = (c).ffG;

}  // namespace sts
