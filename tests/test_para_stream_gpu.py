"""An open paragraph on the MI355X (sts_para_open .. sts_para_close): whatever the schedule of appends and steps, the chunks are those of
sts_infer_ids_joined_stream over the finished paragraph -- count, offsets, sizes and bits with the kernel variant pinned
(set_conv_mode(6)), within 1 LSB of sts_infer_ids_joined under the automatic choice; what the frontier holds back and releases; silent
steps without a decode; a pool too small for the paragraph; speakers and sampling noise per sentence; the conv-math-3 repeat of a step;
states and arguments."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import para_stream_ref as psr
from summertts_amd import engine, synth_blob as sb
from test_join_gpu import _tiny
from test_join_stream_gpu import _cat, _check_stream, _frames_of, _lsb

pytestmark = pytest.mark.gpu

STS_OK, STS_EINVAL, STS_ESTATE = 0, -1, -4
LENS = (3, 7, 12, 5)
JOIN = {"gap_frames": [0, 3, 1], "lead_frames": 2, "trail_frames": 1, "fade_ms": 5.0}
CAP = 4096


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _ids(cfg, lens=LENS):
    return [sb.synthetic_ids(n, cfg.vocab, salt=3 * n + 1) for n in lens]


def _gaps(join, n):
    g = list((join or {}).get("gap_frames") or [0] * (n - 1))
    return [0] + g


def _drive(syn, ids, chunk, join, schedule, sid=None, ls=None, max_res=8, cap=CAP, log=None):
    """An open paragraph through `schedule`: ("a", i0, i1) appends the sentences [i0, i1) as one batch, "s" steps once, "d" drains what is
    deliverable, "f" finishes.  -> the chunks [(sample_offset, pcm)]; `log` collects (frames, starts) of every append and the info at the end"""
    join = join or {}
    gaps = _gaps(join, len(ids))
    syn.para_open(chunk, max_res, cap, join.get("lead_frames", 0), join.get("fade_ms", 0.0))
    out = []
    try:
        for op in schedule:
            if op == "s":
                c, _ = syn.para_step()
                if c is not None:
                    out.append(c)
            elif op == "d":
                while True:
                    c, ready = syn.para_step()
                    if c is None:
                        assert ready == 0
                        break
                    out.append(c)
            elif op == "f":
                syn.para_finish(join.get("trail_frames", 0))
            else:
                _, i0, i1 = op
                got = syn.para_append(ids[i0:i1], None if sid is None else sid[i0:i1], None if ls is None else ls[i0:i1], gaps[i0:i1])
                assert got is not None, op
                if log is not None:
                    log.append(got)
        if log is not None:
            log.append(syn.para_info())
    finally:
        syn.para_close()
    return out


def _same_chunks(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(got, want))


def _schedules(n):
    return {"all at once": [("a", 0, n), "f", "d"],
            "one by one, drained": [x for i in range(n) for x in (("a", i, i + 1), "d")] + ["f", "d"],
            "single steps between": [x for i in range(n) for x in (("a", i, i + 1), "s", "s")] + ["s", "f", "d"],
            "finish before draining": [("a", 0, n - 1), "s", ("a", n - 1, n), "f", "d"]}


CONFIGS = [(16000, None), (8000, None), (44100, None), (16000, 1.0), (8000, 1.0), (44100, 1.0)]      # (rate, limiter look-ahead in ms)


# ---- 1. equality with the closed stream --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,look", CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix"])
def test_every_schedule_delivers_the_closed_streams_chunks(kind, rate, look):
    cfg, blob = _tiny(kind)
    ids = _ids(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if look:
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, look)
    whole = syn.infer_joined(ids, join=JOIN)
    frames, FJ = _frames_of(syn, ids, JOIN)
    starts = syn.join_offsets(len(ids)).tolist()
    halo = syn.stream_halo_frames()
    for chunk in (1, 7, halo, 3 * halo + 1):
        closed = syn.infer_joined_stream(ids, chunk, join=JOIN)
        _check_stream(closed, whole, FJ, chunk, (kind, rate, look, chunk))
        for name, sched in _schedules(len(ids)).items():
            log = []
            got = _drive(syn, ids, chunk, JOIN, sched, log=log)
            assert _same_chunks(got, closed), (kind, rate, look, chunk, name, len(got), len(closed))
            info = log.pop()
            assert [f for a in log for f in a[0]] == frames and [s for a in log for s in a[1]] == starts, name
            assert info["finished"] and info["sentences"] == len(ids) and info["resident"] == 0 and info["free_frames"] == CAP
            assert info["frames_known"] == info["frames_delivered"] == FJ and info["steps"] == len(closed)
    assert np.array_equal(syn.infer_joined(ids, join=JOIN), whole)                        # and the engine is what it was
    syn.close()


# ---- 2. held back and released -----------------------------------------------------------------------------------------------------------
def test_the_frontier_holds_back_and_releases():
    cfg, blob = _tiny("hifigan_fix")
    ids = _ids(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    Hd = syn.stream_halo_frames()                       # native rate, no limiter: the decoder's own halo
    syn.set_output_rate(44100)
    syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
    Ho = syn.stream_halo_frames() - Hd
    assert Ho > 0
    for chunk in (1, 7):
        closed = syn.infer_joined_stream(ids, chunk, join=JOIN)
        frames, FJ = _frames_of(syn, ids, JOIN)
        syn.para_open(chunk, 8, CAP, JOIN["lead_frames"], JOIN["fade_ms"])
        assert syn.para_step() == (None, 0)                                               # nothing appended: nothing leaves
        syn.para_append(ids[:1])
        E = JOIN["lead_frames"] + frames[0]
        want = max(0, (E - Ho) // chunk)                                                  # chunks k with (k + 1) C + Ho <= E
        assert want < len(closed) and syn.para_info()["frames_known"] == E
        got = []
        for k in range(want):
            c, ready = syn.para_step()
            assert c is not None and ready == want - k - 1, (chunk, k, ready)
            got.append(c)
        assert syn.para_step() == (None, 0) and syn.para_info()["frames_delivered"] == want * chunk
        assert (want + 1) * chunk + Ho > E
        syn.para_append(ids[1:], gap_frames=_gaps(JOIN, len(ids))[1:])
        released = (want + 1) * chunk + Ho <= FJ - JOIN["trail_frames"]                   # against the end of the last sentence now
        assert released and (syn.para_step()[0] is not None) == released
        syn.para_close()
        # the whole list through the same points
        sched = [("a", 0, 1), "d", ("a", 1, len(ids)), "d", "f", "d"]
        assert _same_chunks(_drive(syn, ids, chunk, JOIN, sched), closed), chunk
        assert _same_chunks(got, closed[:want]), chunk
    syn.close()


def test_silent_steps_launch_no_decoder_kernel():
    """native rate, no limiter: the J window of a step is its chunk, so a lead or gap longer by whole chunks adds silent steps only -- the
    decoder's matrix-core launches of the paragraph (sts_profile.decoder_mfma_launches, summed over its steps) stay what they were"""
    cfg, blob = _tiny("hifigan_fix", 9)
    ids = _ids(cfg, (3, 7, 12))
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    halo = syn.stream_halo_frames()
    lead, gap = 3 * halo + 5, 7 + 2 * halo + 9
    base = None
    for join in ({"gap_frames": [gap, 0], "lead_frames": lead, "fade_ms": 1.0}, {"gap_frames": [gap, 0], "lead_frames": lead + 7 * 40, "fade_ms": 1.0},
                 {"gap_frames": [gap + 21, 0], "lead_frames": lead, "fade_ms": 1.0}):
        closed = syn.infer_joined_stream(ids, 7, join=join)
        syn.para_open(7, 4, CAP, join["lead_frames"], 1.0)
        syn.para_append(ids[:2], gap_frames=[0, join["gap_frames"][0]])
        got = []
        while True:
            c, _ = syn.para_step()
            if c is None:
                break
            got.append(c)
        assert len(got) >= join["lead_frames"] // 7 and all(not p.any() for _, p in got[:join["lead_frames"] // 7])
        syn.para_append(ids[2:], gap_frames=[0])
        syn.para_finish(0)
        while True:
            c, _ = syn.para_step()
            if c is None:
                break
            got.append(c)
        launches = syn.profile()["decoder_mfma_launches"]
        syn.para_close()
        assert _same_chunks(got, closed)
        if base is None:
            base = (launches, len(got))
            assert launches > 0
        else:
            assert launches == base[0] and len(got) > base[1], join
    syn.close()


# ---- 3. residency ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [0, 0x7FC00000], ids=hex)
def test_a_pool_too_small_for_the_paragraph(poison):
    cfg, blob = _tiny("mbb_fix")
    lens = (12, 15, 9, 14, 11, 13)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=5 * n + 2) for n in lens]
    join = {"gap_frames": [2, 0, 5, 1, 0], "lead_frames": 3, "trail_frames": 4, "fade_ms": 2.0}
    gaps = _gaps(join, len(ids))
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    if poison:
        syn.debug_set("poison", poison)
    chunk = 7
    closed = syn.infer_joined_stream(ids, chunk, join=join)
    frames, FJ = _frames_of(syn, ids, join)
    Hd = syn.stream_halo_frames()

    def play(max_res, cap, real):
        """append one sentence at a time, stepping while there is no room -> (chunks, refusals); real: on the engine, else the restatement"""
        m = psr.Para(chunk, Hd, 0, join["lead_frames"], max_res, cap)
        out, refused = [], 0
        for i in range(len(ids)):
            while True:
                ok = (syn.para_append(ids[i:i + 1], gap_frames=gaps[i:i + 1]) if real else m.append(frames[i:i + 1], gaps[i:i + 1])) is not None
                if ok:
                    break
                refused += 1
                if real:
                    c, _ = syn.para_step()
                    assert c is not None, "no room and nothing to deliver"
                    out.append(c)
                else:
                    if m.ready() == 0:
                        return None, refused
                    m.delivered()
        return out, refused

    # the smallest pool of at least two sentences with which the restatement gets through, and it must refuse on the way
    for max_res in range(2, len(ids)):
        cap = sum(sorted(frames)[-max_res:])
        model = play(max_res, cap, False)
        if model[0] is not None:
            break
    assert model[0] is not None and model[1] > 0 and max_res < len(ids) and cap < sum(frames), (frames, Hd)
    syn.para_open(chunk, max_res, cap, join["lead_frames"], join["fade_ms"])
    got, refused = play(max_res, cap, True)
    assert refused == model[1]
    syn.para_finish(join["trail_frames"])
    while True:
        c, _ = syn.para_step()
        if c is None:
            break
        got.append(c)
    info = syn.para_info()
    syn.para_close()
    assert _same_chunks(got, closed) and info["resident"] == 0 and info["free_frames"] == cap and info["free_slots"] == max_res
    syn.close()


# ---- 4. per-sentence speaker and noise -----------------------------------------------------------------------------------------------------
def test_speakers_and_sampling_noise_per_sentence():
    cfg, blob = _tiny("ms_hifigan_fix", 5)
    ids = _ids(cfg)
    sid = [0, 2, 1, 2]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(22050)
    quiet = syn.infer_joined_stream(ids, 5, sid, None, JOIN)
    syn.set_noise(0.667, 0.8, 77)
    closed = syn.infer_joined_stream(ids, 5, sid, None, JOIN)
    assert _cat(closed).tobytes() != _cat(quiet).tobytes()                                # the noise is audible in the reference itself
    for sched in ([("a", 0, 1), "s", ("a", 1, 3), "d", ("a", 3, 4), "f", "d"], [("a", 0, 2), ("a", 2, 4), "f", "d"]):
        assert _same_chunks(_drive(syn, ids, 5, JOIN, sched, sid=sid), closed), sched      # seed + GLOBAL index, speaker per sentence
    other = _drive(syn, ids, 5, JOIN, [("a", 0, 4), "f", "d"], sid=[0, 0, 0, 0])
    assert len(other) == len(closed) and _cat(other).tobytes() != _cat(closed).tobytes()
    syn.close()


# ---- 5. conv math 3: the repeat of a step ------------------------------------------------------------------------------------------------
def test_the_split_bf16_repeat_of_a_step():
    """STS_DBG_STREAM_RETRY_STEP = 2 under conv math 3 (the automatic kernel choice): chunks 0 and 1 are the two-term fp16 ones, chunk 2 and
    every later one are decoded in split-bf16 (appends behind it too), no chunk arrives twice and conv_math_fallbacks rises by one.  Forced
    durations are not available to an open paragraph: both maths must agree on the frame counts, which the test checks first."""
    cfg, blob = _tiny("hifigan_fix")
    ids = _ids(cfg)
    sched = [("a", 0, 2), "s", "s", "s", ("a", 2, 4), "f", "d"]
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_conv_math("f16x2")
    la, lb, lc = [], [], []
    plain = _drive(syn, ids, 4, JOIN, sched, log=la)
    syn.set_conv_math("bf16x3")
    bf3 = _drive(syn, ids, 4, JOIN, sched, log=lb)
    assert la[:-1] == lb[:-1], "the two arithmetics disagree on a frame count: choose other sentences"
    syn.set_conv_math("f16x2")
    before = syn.profile()["conv_math_fallbacks"]
    syn.debug_set("stream_retry_step", 2)
    got = _drive(syn, ids, 4, JOIN, sched, log=lc)
    assert syn.profile()["conv_math_fallbacks"] == before + 1
    syn.debug_set("stream_retry_step", -1)
    assert lc[:-1] == la[:-1] and len(got) == len(plain) == len(bf3) > 4
    assert [o for o, _ in got] == list(np.cumsum([0] + [p.size for _, p in got])[:-1]) == [o for o, _ in plain]      # every chunk once, in order
    for i in range(2):
        assert np.array_equal(got[i][1], plain[i][1]), i
    worst = max(_lsb(got[i][1], bf3[i][1]) for i in range(2, len(got)))
    print("retry at step 2: max |paragraph - split-bf16 paragraph| =", worst, "LSB")
    assert worst <= 1
    syn.close()


# ---- 6. states and arguments -------------------------------------------------------------------------------------------------------------
def test_states_and_arguments():
    cfg, blob = _tiny("hifigan_fix", 3)
    ids = _ids(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    lib = syn.lib
    cb = engine.CHUNK_CB(lambda user, pcm, n, off: 0)
    whole = syn.infer_ids(ids[2])
    # refused at open: an equaliser, loudness, record taps, pending per-call tables
    syn.set_eq([(engine.EQ_PEAK, 1000.0, 3.0, 1.0)])
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL
    syn.set_eq(None)
    syn.set_loudness(engine.LOUD_MEASURE)
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL
    syn.set_loudness(engine.LOUD_OFF)
    syn.set_record_taps(True)
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL
    syn.set_record_taps(False)
    syn.set_gain_plan([len(ids[0])], [{"gain_db": [0.0] * len(ids[0])}])
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL
    syn.set_gain_plan(None)
    syn.set_forced_durations([1] * len(ids[0]))
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL
    syn.set_forced_durations(None)
    syn.set_duration_plan([len(ids[0])], [{"rate": [1.5] * len(ids[0])}])
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL
    syn.set_duration_plan(None)
    ms = engine.Synthesizer(_tiny("ms_hifigan_fix", 5)[1])                                # a speaker mix needs a model with speakers
    ms.set_speaker_mix([{"sid": [0, 2], "weight": [0.5, 0.5]}])
    assert ms.lib.sts_para_open(ms.h, 8, 2, 1000, 0, 0.0) == STS_EINVAL and not ms.para_info()["open"]
    ms.set_speaker_mix(None)
    ms.para_open(8, 2, 1000, 0, 0.0)                                                      # (dropped: nothing else stood in the way)
    with pytest.raises(engine.StsError, match="sts error -4"):
        ms.set_speaker_mix([{"sid": [0, 2], "weight": [0.5, 0.5]}])
    ms.para_close()
    ms.close()
    assert not syn.para_info()["open"]
    # an open stream stands in the way of a paragraph, as a paragraph in the way of a stream (below)
    syn.stream_open(8, 2, 1000)
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_ESTATE
    assert syn.stream_info()["open"] and not syn.para_info()["open"]
    syn.stream_close()
    for args in ((0, 2, 1000, 0, 0.0), (8, 0, 1000, 0, 0.0), (8, 1025, 1000, 0, 0.0), (8, 2, 0, 0, 0.0), (8, 2, 1 << 40, 0, 0.0), (8, 2, 1000, -1, 0.0),
                 (8, 2, 1000, 100001, 0.0), (8, 2, 1000, 0, 50.5), (8, 2, 1000, 0, float("nan"))):
        assert lib.sts_para_open(syn.h, *args) == STS_EINVAL, args
    # nothing is open
    assert lib.sts_para_close(syn.h) == STS_ESTATE and lib.sts_para_finish(syn.h, 0) == STS_ESTATE
    assert lib.sts_para_step(syn.h, cb, None, None) == STS_ESTATE
    with pytest.raises(engine.StsError):
        syn.para_append(ids[:1])
    assert not syn.para_info()["open"]
    # open: one at a time, and no open stream next to it
    syn.para_open(8, 2, 1000, 1, 1.0)
    assert lib.sts_para_open(syn.h, 8, 2, 1000, 0, 0.0) == STS_ESTATE and lib.sts_stream_open(syn.h, 8, 2, 1000) == STS_ESTATE
    assert syn.para_info()["open"] and not syn.stream_info()["open"]
    # every other run entry and every setter of what open fixed
    for call in (lambda: syn.infer_ids(ids[0]), lambda: syn.infer_joined(ids), lambda: syn.infer_joined_stream(ids, 4), lambda: syn.infer_ids_stream(ids[0], 4),
                 lambda: syn.set_output_rate(8000), lambda: syn.set_limiter(engine.LIMITER_ON), lambda: syn.set_conv_mode(0), lambda: syn.set_conv_math("bf16x3"),
                 lambda: syn.set_loudness(engine.LOUD_MEASURE), lambda: syn.set_eq([(engine.EQ_PEAK, 1000.0, 3.0, 1.0)]), lambda: syn.set_record_taps(True),
                 lambda: syn.set_forced_durations([1]), lambda: syn.set_duration_plan([len(ids[0])], [{"rate": [1.5] * len(ids[0])}]), lambda: syn.set_gain_plan([len(ids[0])], [{"gain_db": [0.0] * len(ids[0])}])):
        with pytest.raises(engine.StsError, match="sts error -4"):
            call()
    syn.set_noise(0.0, 0.0, 0)                                                            # stays allowed
    # bad appends, finish before a sentence
    assert lib.sts_para_finish(syn.h, 0) == STS_EINVAL
    p = engine.PreparedBatch(ids[:3], None, None)
    app = C.c_int32(-7)
    gap = np.asarray([3, 0, 0], np.int32)
    assert lib.sts_para_append(syn.h, 3, p.ptrs, p.n_p, None, None, None, None, None, C.addressof(app)) == STS_EINVAL and app.value == 0     # B > max_resident
    assert lib.sts_para_append(syn.h, 2, p.ptrs, p.n_p, None, None, gap.ctypes.data, None, None, C.addressof(app)) == STS_EINVAL              # a gap in front of the first
    assert lib.sts_para_append(syn.h, 0, p.ptrs, p.n_p, None, None, None, None, None, C.addressof(app)) == STS_EINVAL
    assert lib.sts_para_append(syn.h, 1, None, p.n_p, None, None, None, None, None, C.addressof(app)) == STS_EINVAL
    assert lib.sts_para_append(syn.h, 1, p.ptrs, p.n_p, None, None, None, None, None, None) == STS_EINVAL
    gap[1] = 100001
    assert lib.sts_para_append(syn.h, 2, p.ptrs, p.n_p, None, None, (gap[1:]).ctypes.data, None, None, C.addressof(app)) == STS_EINVAL
    assert syn.para_info()["sentences"] == 0
    assert lib.sts_para_step(syn.h, C.cast(None, engine.CHUNK_CB), None, None) == STS_EINVAL
    syn.para_close()
    # an append after finish, a second finish; a stop through the callback
    syn.para_open(4, 4, 1000, 1, 1.0)
    syn.para_append(ids[:2])
    seen = []
    first, _ = syn.para_step(on_chunk=lambda pcm, off: seen.append(off) or True)
    assert first is not None and seen == [0]
    assert syn.para_step() == (None, 0) and syn.para_append(ids[2:3]) is None            # stopped: later steps and appends do nothing
    info = syn.para_info()
    assert info["open"] and info["resident"] == 0 and info["steps"] == 1
    syn.para_close()
    syn.para_open(4, 4, 1000, 1, 1.0)
    syn.para_append(ids[:2])
    assert lib.sts_para_finish(syn.h, 100001) == STS_EINVAL and lib.sts_para_finish(syn.h, -1) == STS_EINVAL and not syn.para_info()["finished"]
    syn.para_finish(2)
    assert lib.sts_para_finish(syn.h, 2) == STS_EINVAL
    with pytest.raises(engine.StsError, match="sts error -1"):
        syn.para_append(ids[2:3])
    # close with live sentences, then a plain call as before
    assert syn.para_info()["resident"] == 2
    syn.para_close()
    assert np.array_equal(syn.infer_ids(ids[2]), whole)
    # sts_destroy with an open paragraph
    syn.para_open(4, 4, 1000, 0, 0.0)
    syn.para_append(ids[:2])
    syn.close()
    fresh = engine.Synthesizer(blob)
    fresh.set_conv_mode(6)
    assert np.array_equal(fresh.infer_ids(ids[2]), whole)
    fresh.close()


@pytest.mark.parametrize("rate", [0, 44100], ids=["native samples", "output samples"])
def test_an_append_past_the_length_limit_is_refused(rate):
    """N_J <= 2 10^9 native samples and L_out <= 2^31 - 1 output samples: a full-size model (256 samples per frame), a lead and gaps of
    100000 frames, sentences of 3 phonemes appended until the limit answers -- about 78 appends at the native rate, where N_J binds, and
    about 30 at 44.1 kHz, where the output count binds long before N_J does; no step, nothing decoded"""
    cfg = sb.full_cfg("hifigan_sdp")
    syn = engine.Synthesizer(sb.make_blob(cfg, 5))
    hop = syn.info.samples_per_frame
    if rate:
        syn.set_output_rate(rate)
    up = Fraction(rate or syn.info.sample_rate, syn.info.sample_rate)

    def fits(frames):
        return frames * hop <= 2000000000 and -(-frames * hop * up.numerator // up.denominator) <= 2147483647
    ids = [sb.synthetic_ids(3, cfg.vocab, salt=1)]
    p = engine.PreparedBatch(ids, None, None)
    app = C.c_int32(-7)
    far = np.full(1, 100000, np.int32)
    bound = 2000000000 // (100000 * hop) + 2
    assert bound <= 128
    syn.para_open(8, 128, 65536, 100000, 0.0)
    f0 = syn.para_append(ids)[0][0]
    for n_far in range(bound):
        rc = syn.lib.sts_para_append(syn.h, 1, p.ptrs, p.n_p, None, None, far.ctypes.data, None, None, C.addressof(app))
        if rc != STS_OK:
            break
        assert app.value == 1
    info = syn.para_info()
    E = info["frames_known"]
    assert rc == STS_EINVAL and app.value == 0 and fits(E) and not fits(E + 100000 + f0) and info["sentences"] == n_far + 1
    assert ((E + 100000 + f0) * hop <= 2000000000) == bool(rate)                          # at 44.1 kHz the output count alone refused
    assert info["resident"] == n_far + 1                                                 # the refused append took nothing
    assert not fits(E + 100000), "test set-up: the sentence's own frames decided the refusal"
    assert syn.lib.sts_para_finish(syn.h, 100000) == STS_EINVAL and not syn.para_info()["finished"]     # finish answers to the same limit
    syn.para_finish(0)
    syn.para_close()
    syn.close()


# ---- 7. the automatic kernel choice, and the generator -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix"])
def test_the_automatic_kernel_choice_agrees_within_one_lsb(kind):
    cfg, blob = _tiny(kind)
    ids = _ids(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(0)
    whole = syn.infer_joined(ids, join=JOIN)
    frames, FJ = _frames_of(syn, ids, JOIN)
    for chunk in (7, 3 * syn.stream_halo_frames() + 1):
        got = _drive(syn, ids, chunk, JOIN, _schedules(len(ids))["single steps between"])
        pcm = _cat(got)
        assert len(got) == -(-FJ // chunk) and pcm.size == whole.size
        worst = _lsb(pcm, whole)
        print(kind, chunk, "max |paragraph - whole| =", worst, "LSB")
        assert worst <= 1, (kind, chunk)
    syn.close()


def test_the_generator_appends_what_its_iterator_yields():
    cfg, blob = _tiny("hifigan_fix")
    ids = _ids(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    join = {"gap_frames": [3, 3, 3], "lead_frames": 2, "trail_frames": 1, "fade_ms": 5.0}
    closed = syn.infer_joined_stream(ids, 7, join=join)
    asked = []

    def sentences():
        for i, s in enumerate(ids):
            asked.append(i)
            yield s
    got = list(syn.stream_paragraph(sentences(), 7, gap_frames=3, lead_frames=2, trail_frames=1, fade_ms=5.0))
    assert _same_chunks(got, closed) and asked == [0, 1, 2, 3] and not syn.para_info()["open"]
    with pytest.raises(ValueError, match="sid_iter ran out"):                             # fewer speaker ids than sentences: said so, and closed
        list(syn.stream_paragraph(iter(ids), 7, sid_iter=[0, 0]))
    assert not syn.para_info()["open"]
    syn.close()
