// out_chain.hpp -- the output chain behind the decoder's trunk, decided once per run.  Plain C++: no HIP, no engine type.
//
// The stages, in their fixed order: tail, gain, join, resample, pack, eq, loud, limit.  A running stage reads the float output of the
// nearest running stage in front of it that has one, and the last running stage that can cast to int16 writes the PCM the caller
// gets; every other int16 result goes to scratch.  A streaming run decodes tail and gain per step and runs resample / pack / limit on
// each step's windows; loud runs in one only with the fact loud_stream under mode 1 (sts_set_loudness_streaming; the engine refuses every
// other such call): it then measures each step's windows of the nearest running float stage in front of it, which writes its float
// output for it, and changes nothing else of the plan -- it never writes PCM.  eq runs only with the fact eq_stream (sts_set_eq_streaming):
// it then runs on each step's windows behind the resampler from a state carried per utterance, pack never runs, and the EQ is the writer
// when the limiter is off.  A joined stream (sts_infer_ids_joined_stream) joins
// each step's windows into a window of the ONE signal J: pack never runs, and the join is the writer when nothing runs behind it.
// A stream through the pitch warp (the fact pitch_stream, sts_set_pitch_streaming) runs the range warp in the gain stage on each step's
// windows: pack never runs and nothing is downloaded in place -- the warp is the writer when nothing runs behind it.
#pragma once

namespace sts {

enum OutStage { OS_TAIL, OS_GAIN, OS_JOIN, OS_RESAMPLE, OS_PACK, OS_EQ, OS_LOUD, OS_LIMIT, OS_COUNT };

struct OutFacts {
    bool stream; int B;
    bool resample, gain, join, eq; int loud_mode; bool limit;
    bool taps, stream_direct;
    bool eq_stream = false;     // (behind the others, which older callers initialise in order) a stream runs the EQ: sts_set_eq_streaming
    bool loud_stream = false;   // (behind that one) a stream under loudness mode 1 measures: sts_set_loudness_streaming
    bool pitch_stream = false;  // (behind that one) a stream through the pitch warp (sts_set_pitch_streaming): the range warp packs its chunks
};

struct OutChain {
    bool run[OS_COUNT];     // the stage runs
    int src[OS_COUNT];      // the stage whose float output it reads (-1: none -- the tail, pack, a stage that does not run)
    bool wave[OS_COUNT];    // it writes a float output: a later stage reads it, or the taps record it
    int writer;             // the stage that writes the returned PCM
    bool pcm_nat, pcm_rs;   // the tail's / the resampler's int16 samples go to scratch (they are not the writer)
    bool loud_cast, loud_no_clamp, lim_gloud;   // loudness casts with its gain; leaves the peak to the limiter; the limiter takes its gain
    bool lws, limws, spack, stab;   // workspaces: loudness, the limiter's result words, the packed chunk buffer, the step tables
    bool chunk_in_place;    // streaming: nothing packs the step's one chunk, it is downloaded from its offset in the PCM
    bool eqws, eqst;        // the EQ's workspaces: the whole call's tile table; a stream's carried state, step workspace and table rows
    bool lst;               // a stream that measures loudness: its carried state, step workspace, result tables and table rows (lws stays false)
};

inline OutChain plan_out_chain(const OutFacts& f) {
    OutChain p{};
    const bool whole = !f.stream, eqs = f.stream && f.eq && f.eq_stream, lds = f.stream && f.loud_stream && f.loud_mode == 1;
    p.run[OS_TAIL] = true; p.run[OS_GAIN] = f.gain; p.run[OS_JOIN] = f.join; p.run[OS_RESAMPLE] = f.resample;
    p.run[OS_PACK] = f.stream && !f.join && !f.resample && !f.limit && !eqs && !f.pitch_stream && (f.B > 1 || f.stream_direct);
    p.run[OS_EQ] = f.eq && (whole || eqs); p.run[OS_LOUD] = (f.loud_mode != 0 && whole) || lds; p.run[OS_LIMIT] = f.limit;
    const bool normalise = p.run[OS_LOUD] && f.loud_mode == 2;
    int cur = -1;           // the current float signal
    for (int s = 0; s < OS_COUNT; s++) {
        p.src[s] = p.run[s] && s != OS_PACK ? cur : -1;     // (pack moves int16 samples)
        if (!p.run[s] || s == OS_PACK) continue;
        if (p.src[s] >= 0) p.wave[p.src[s]] = true;
        if (s != OS_LOUD) cur = s;                          // (loudness measures: the limiter reads what it read)
        if (s != OS_LOUD || normalise) p.writer = s;
    }
    // the gain, join and EQ kernels always write their float output; the others only for a reader (above) or the taps
    p.wave[OS_GAIN] = p.run[OS_GAIN]; p.wave[OS_JOIN] = p.run[OS_JOIN]; p.wave[OS_EQ] = p.run[OS_EQ];
    if (f.taps) p.wave[OS_TAIL] = true;
    if (f.taps && whole) { p.wave[OS_RESAMPLE] = p.run[OS_RESAMPLE]; p.wave[OS_LIMIT] = p.run[OS_LIMIT]; }
    p.pcm_nat = p.writer != OS_TAIL; p.pcm_rs = p.run[OS_RESAMPLE] && p.writer != OS_RESAMPLE;
    p.loud_cast = p.writer == OS_LOUD; p.loud_no_clamp = p.run[OS_LIMIT]; p.lim_gloud = normalise;
    p.lws = p.run[OS_LOUD] && whole; p.limws = p.run[OS_LIMIT] && whole; p.spack = p.run[OS_PACK] && f.B > 1; p.stab = f.stream;
    p.chunk_in_place = f.stream && !f.join && !p.run[OS_RESAMPLE] && !p.run[OS_LIMIT] && !p.run[OS_PACK] && !eqs && !f.pitch_stream;
    p.eqws = p.run[OS_EQ] && whole; p.eqst = eqs; p.lst = lds;
    return p;
}

}  // namespace sts
