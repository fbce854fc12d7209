"""A joined stream on the MI355X (sts_infer_ids_joined_stream, sts_join_apply_range): the windowed join kernel on caller signals against
the NumPy restatement of tests/join_ref.py, bit for bit; an engine's concatenated chunks against sts_infer_ids_joined of the same call --
bit for bit with the kernel variant pinned (set_conv_mode(6)), within 1 LSB under the automatic choice, the contract of every stream;
one sentence against sts_infer_ids_stream; long silences; speakers and plans per sentence; a stopped call; the conv-math-3 repeat; a
poisoned workspace; refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import join_ref as jr
from summertts_amd import engine, synth_blob as sb
from test_join_gpu import FADES, JOIN, LENS, LJOIN, LONG, _sentences, _signal, _tiny

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STS_OK, STS_EINVAL = 0, -1
SPAN = int(re.search(r"static constexpr int kJoinSpan = (\d+);", open(os.path.join(ROOT, "summertts_amd", "csrc", "join.hip")).read()).group(1))
LJOIN2 = dict(LJOIN, fade_ms=2.0)


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


# ---- 1. the kernel on caller signals -------------------------------------------------------------------------------------------------------
def _ranges(frames, hop, join):
    """frame ranges of J that begin and end in silence, mid-sentence, exactly on a sentence edge, inside a fade, across several sentences,
    in silence only, and everything"""
    start, total, h = jr.layout(frames, 1, join)
    FJ, hf = int(total), max(1, -(-h // hop))
    out = {(0, FJ), (0, 1), (FJ - 1, FJ)}
    for b, F in enumerate(frames):
        s = int(start[b])
        out |= {(s, s + F), (s + F // 3, s + F // 3 + max(1, F // 3)), (s - 1, s + 1), (s + F - 1, s + F + 1), (s - 2, s + F + 2),
                (s, s + 1), (s + F - 1, s + F), (s + 1, s + 1 + hf), (s + F - hf, s + F), (s + F, s + F + 2), (s - 3, s),
                (s + F // 2, FJ), (0, s + F // 2)}
    return sorted((a, e) for a, e in out if 0 <= a < e <= FJ)


def _range_case(frames, hop, join, seed=0):
    sig = [_signal(int(f) * hop, seed + b) for b, f in enumerate(frames)]
    J, want = jr.join(sig, frames, hop, join)
    silent = 0
    for g0, g1 in _ranges(frames, hop, join):
        y, pcm = engine.join_apply_range(sig, frames, hop, g0, g1 - g0, join)
        assert not np.isnan(y).any(), (hop, list(frames), join, g0, g1)                   # the unwritten-sample sentinel never shows
        bad = np.flatnonzero(y.view(np.uint32) != J[g0 * hop:g1 * hop].view(np.uint32))
        assert y.size == (g1 - g0) * hop and bad.size == 0, (hop, list(frames), join, g0, g1, int(bad[0]) if bad.size else -1)
        assert np.array_equal(pcm, want[g0 * hop:g1 * hop]), (hop, list(frames), join, g0, g1)
        silent += not J[g0 * hop:g1 * hop].any()
    return silent


@pytest.mark.parametrize("hop", [4, 256])
@pytest.mark.parametrize("B", [1, 2, 7])
def test_apply_range_on_every_kind_of_range(hop, B):
    """sentences of one frame, around one span of the kernel and of several spans; gap 0 next to gap 3, a lead and a trail; every fade"""
    S = SPAN // hop
    pool = [S + 1, 1, S - 1, 3, 2 * S + 5, 1, S]
    frames = [pool[b % len(pool)] for b in range(B)]
    gaps = [(0, 3, 0, 1, 3, 0)[b % 6] for b in range(B - 1)]
    silent = 0
    for k, fade in enumerate(FADES):
        silent += _range_case(frames, hop, {"gap_frames": gaps, "lead_frames": 5, "trail_frames": 2, "fade_ms": fade}, seed=k)
    assert silent >= 4                                                                    # ranges that cover only silence
    _range_case(frames, hop, None)


def test_apply_range_over_one_frame_sentences_and_the_scalar_path():
    for hop in (4, 3):
        _range_case([1] * 7, hop, {"gap_frames": [0, 3, 0, 1, 3, 0], "lead_frames": 1, "trail_frames": 1, "fade_ms": 0.0625}, seed=hop)
    for fade in FADES:
        _range_case([1400, 1, 1365, 2], 3, {"gap_frames": [0, 3, 1], "lead_frames": 2, "trail_frames": 1, "fade_ms": fade}, seed=3)
    lib = engine.load_library()
    x = np.zeros(8, np.float32); f = np.asarray([1, 1], np.int32)
    for first, count in ((-1, 1), (0, 0), (1, 2), (2, 1)):                               # outside [0, F_J) or empty
        assert lib.sts_join_apply_range(0, x.ctypes.data, f.ctypes.data, 2, 4, None, first, count, x.ctypes.data, None) == STS_EINVAL
    assert lib.sts_join_apply_range(0, None, f.ctypes.data, 2, 4, None, 0, 1, x.ctypes.data, None) == STS_EINVAL


# ---- 2. the engine: the chunks are the whole joined call --------------------------------------------------------------------------------
def _cat(chunks):
    return np.concatenate([p for _, p in chunks]) if chunks else np.zeros(0, np.int16)


def _check_stream(chunks, whole, FJ, chunk_frames, tag):
    """the concatenation, the offsets as the running sum, one callback per step"""
    assert len(chunks) == -(-FJ // chunk_frames), tag
    pos = 0
    for off, p in chunks:
        assert off == pos, tag
        pos += p.size
    got = _cat(chunks)
    bad = np.flatnonzero(got != whole) if got.size == whole.size else np.zeros(1, int)
    assert got.size == whole.size and bad.size == 0, (tag, got.size, whole.size, int(bad[0]) if bad.size else -1)


def _frames_of(syn, ids, join):
    hop = syn.info.samples_per_frame
    lens = [len(a) for a in ids]
    dur = syn.durations(sum(lens))
    off = np.concatenate([[0], np.cumsum(lens)])
    frames = [max(1, int(dur[off[b]:off[b + 1]].sum())) for b in range(len(lens))]
    return frames, int(jr.layout(frames, hop, join)[1]) // hop


CONFIGS = [(16000, None), (8000, None), (44100, None), (16000, 1.0), (44100, 1.0)]       # (rate, limiter look-ahead in ms)


@pytest.mark.parametrize("rate,look", CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("lens,join", [(LENS, JOIN), (LONG, LJOIN2)], ids=["short", "long"])
@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix"])
def test_chunks_concatenate_to_the_whole_joined_call(kind, lens, join, rate, look):
    cfg, blob = _tiny(kind)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=3 * n + 1) for n in lens]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if look:
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, look)
    whole = syn.infer_joined(ids, join=join)
    frames, FJ = _frames_of(syn, ids, join)
    offsets = syn.join_offsets(len(ids)).tolist()
    halo = syn.stream_halo_frames()
    for chunk in (1, 7, halo, 3 * halo + 1, 100000):
        chunks = syn.infer_joined_stream(ids, chunk, join=join)
        _check_stream(chunks, whole, FJ, chunk, (kind, lens, rate, look, chunk))
        assert syn.stream_total == whole.size and syn.join_offsets(len(ids)).tolist() == offsets
    assert np.array_equal(syn.infer_joined(ids, join=join), whole)
    syn.close()


@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix"])
def test_the_automatic_kernel_choice_agrees_within_one_lsb(kind):
    cfg, blob = _tiny(kind)
    ids = _sentences(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(0)
    whole = syn.infer_joined(ids, join=JOIN)
    frames, FJ = _frames_of(syn, ids, JOIN)
    for chunk in (7, 3 * syn.stream_halo_frames() + 1):
        chunks = syn.infer_joined_stream(ids, chunk, join=JOIN)
        got = _cat(chunks)
        assert len(chunks) == -(-FJ // chunk) and got.size == whole.size
        worst = int(np.abs(got.astype(np.int32) - whole.astype(np.int32)).max())
        print(kind, chunk, "max |stream - whole| =", worst, "LSB")
        assert worst <= 1, (kind, chunk)
    syn.close()


@pytest.mark.parametrize("rate,look", [(16000, None), (44100, 1.0)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix"])
def test_one_sentence_with_an_all_zero_join_is_the_single_stream(kind, rate, look):
    cfg, blob = _tiny(kind)
    a = sb.synthetic_ids(12, cfg.vocab, salt=37)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if look:
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, look)
    for chunk in (1, 7, 100000):
        want, _ = syn.infer_ids_stream(a, chunk)
        for join in ({}, None):
            got = syn.infer_joined_stream([a], chunk, join=join)
            assert len(got) == len(want) and all(np.array_equal(g[1], w) for g, w in zip(got, want)), (kind, rate, chunk)
    syn.close()


def test_a_long_lead_and_a_long_gap_cost_no_decode():
    """a lead of 3 halo + 5 frames and a gap longer than a step between two sentences: the chunks in front of the first sentence are all
    zero, there is one callback per step, and the concatenation is the whole call's.  The silent steps launch no decoder kernel:
    sts_profile.decoder_mfma_launches counts the matrix-core convs of every run_decode of the call, summed over the steps of a stream.
    At the native rate without a limiter the J window of a step is its chunk (Ho = 0), so a lead or a gap that is longer by a multiple
    of the chunk moves every sentence against the chunk grid by whole chunks: the steps that decode anything decode the same windows,
    and only silent steps are added.  The count must then be the same -- and is not if a silent step runs a decode of any kind."""
    cfg, blob = _tiny("hifigan_fix", 9)
    ids = _sentences(cfg, (3, 7, 12))
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    halo = syn.stream_halo_frames()
    lead, gap = 3 * halo + 5, 7 + 2 * halo + 9
    join = {"gap_frames": [gap, 0], "lead_frames": lead, "trail_frames": 0, "fade_ms": 1.0}
    whole = syn.infer_joined(ids, join=join)
    frames, FJ = _frames_of(syn, ids, join)
    chunks = syn.infer_joined_stream(ids, 7, join=join)
    launches = syn.profile()["decoder_mfma_launches"]
    _check_stream(chunks, whole, FJ, 7, "lead")
    lead_steps = lead // 7
    assert lead_steps >= 3 and all(not p.any() for _, p in chunks[:lead_steps])
    assert whole[lead * syn.info.samples_per_frame:].any()
    # the same paragraph with the whole silent steps of the lead taken out, and with three more of them in the gap
    assert launches > 0
    for other in (dict(join, lead_frames=lead % 7), dict(join, gap_frames=[gap + 21, 0]), dict(join, lead_frames=lead + 7 * 40)):
        got = syn.infer_joined_stream(ids, 7, join=other)
        assert len(got) == len(chunks) + (other["lead_frames"] - lead + other["gap_frames"][0] - gap) // 7
        assert syn.profile()["decoder_mfma_launches"] == launches, other
    syn.close()


# ---- 3. speakers and plans per sentence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [16000, 22050])
def test_speakers_mixes_and_plans_per_sentence(rate):
    cfg, blob = _tiny("ms_hifigan_fix", 5)
    lens = (7, 12, 5)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    sid = [0, 2, 1]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    join = {"gap_frames": [4, 0], "lead_frames": 1, "trail_frames": 3, "fade_ms": 1.0}
    db = np.zeros(12, np.float32); db[2] = -float("inf"); db[7] = -6.0
    gains = [None, {"gain_db": db, "ramp_ms": 2.0}, None]
    plans = [{"target_frames": 33}, None, None]
    mixes = [None, {"sid": [0, 2], "weight": [0.25, 0.75]}, None]

    def setup(what):
        if "plan" in what:
            syn.set_duration_plan(lens, plans)
        if "gain" in what:
            syn.set_gain_plan(lens, gains)
        if "mix" in what:
            syn.set_speaker_mix(mixes)

    seen = []
    for what in ((), ("mix",), ("gain",), ("plan",), ("plan", "gain", "mix")):
        setup(what)
        whole = syn.infer_joined(ids, sid, None, join)
        joff, poff, dur = syn.join_offsets(3), syn.phoneme_offsets(sum(lens)), syn.durations(sum(lens))
        frames, FJ = _frames_of(syn, ids, join)
        assert (frames[0] == 33) == ("plan" in what)
        for chunk in (5, 3 * syn.stream_halo_frames() + 1):
            setup(what)
            chunks = syn.infer_joined_stream(ids, chunk, sid, None, join)
            _check_stream(chunks, whole, FJ, chunk, (rate, what, chunk))
            assert np.array_equal(syn.join_offsets(3), joff) and np.array_equal(syn.phoneme_offsets(sum(lens)), poff)
            assert np.array_equal(syn.durations(sum(lens)), dur)
        seen.append(whole.tobytes())
    assert len(set(seen)) == len(seen)                                                    # every setting changed the signal
    other = syn.infer_joined_stream(ids, 5, [0, 0, 0], None, join)                       # the speakers are per sentence
    assert _cat(other).tobytes() != seen[0]
    assert np.array_equal(_cat(syn.infer_joined_stream(ids, 5, sid, None, join)), np.frombuffer(seen[0], np.int16))   # the plans were for one call
    syn.close()


# ---- 4. a stopped call, the conv-math-3 repeat, poison, refusals --------------------------------------------------------------------------
def _fresh_joined(blob, ids, join, mode=6):
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(mode)
    out = syn.infer_joined(ids, join=join)
    syn.close()
    return out


def test_a_callback_can_end_the_call():
    cfg, blob = _tiny("mbb_fix")
    ids = _sentences(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    whole = syn.infer_joined(ids, join=JOIN)
    seen = []
    chunks = syn.infer_joined_stream(ids, 4, join=JOIN, on_chunk=lambda pcm, off, t: seen.append(off) or len(seen) == 3)     # stop at step 2
    assert len(chunks) == 3 and len(seen) == 3
    assert syn.stream_total == sum(p.size for _, p in chunks) == 12 * syn.info.samples_per_frame
    assert np.array_equal(_cat(chunks), whole[:syn.stream_total])
    assert np.array_equal(syn.infer_joined(ids, join=JOIN), _fresh_joined(blob, ids, JOIN))
    syn.close()


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) if a.size else 0


def test_the_split_bf16_repeat_of_a_step_and_of_the_whole_call():
    """STS_DBG_STREAM_RETRY_STEP under conv math 3 (the automatic kernel choice: a pinned variant has no two-term fp16 form).  Raised after
    step 2: the chunks of steps 0 and 1 are those of the two-term fp16 stream, everything from step 2 on is decoded in the split-bf16 form
    and compared with the split-bf16 WHOLE call -- within the 1 LSB the header grants a stream under the automatic choice -- no chunk
    arrives twice and the fallback counter counts once.  Raised at step 0 the whole call is repeated.  Durations are forced: both forms
    then lay out the same J.  The call repeated from step 0 is also the split-bf16 STREAM of the same chunk size bit for bit."""
    cfg, blob = _tiny("hifigan_fix")
    ids = _sentences(cfg)
    total = sum(len(a) for a in ids)
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_conv_math("f16x2")
    plain = syn.infer_joined_stream(ids, 4, join=JOIN)
    dur = syn.durations(total)
    syn.set_conv_math("bf16x3")
    syn.set_forced_durations(dur)
    whole0 = syn.infer_joined(ids, join=JOIN)
    syn.set_forced_durations(dur)
    stream0 = syn.infer_joined_stream(ids, 4, join=JOIN)                                 # the split-bf16 stream of the same chunk size
    syn.set_conv_math("f16x2")
    assert len(plain) > 4 and _cat(plain).size == whole0.size and len(stream0) == len(plain)
    for step, fallbacks in ((2, 1), (0, 2)):
        syn.debug_set("stream_retry_step", step)
        syn.set_forced_durations(dur)
        got = syn.infer_joined_stream(ids, 4, join=JOIN)
        syn.debug_set("stream_retry_step", -1)
        assert syn.profile()["conv_math_fallbacks"] == fallbacks, step                    # (the engine's running count)
        assert [o for o, _ in got] == [o for o, _ in plain] and [p.size for _, p in got] == [p.size for _, p in plain], step
        for i in range(step):
            assert np.array_equal(got[i][1], plain[i][1]), (step, i)
        first = got[step][0]
        worst = _lsb(_cat(got)[first:], whole0[first:])
        print("retry at step", step, ": max |stream - split-bf16 whole call| =", worst, "LSB")
        assert worst <= 1, step
        if step == 0:       # the whole call was repeated in the split-bf16 form: the same launches as the split-bf16 stream, bit for bit
            assert all(np.array_equal(g[1], w[1]) for g, w in zip(got, stream0))
        else:               # (a later step decodes in split-bf16 what the two-term fp16 FLOW produced: no split-bf16 call has that input)
            print("retry at step", step, ": max |stream - split-bf16 stream| =", _lsb(_cat(got)[first:], _cat(stream0)[first:]), "LSB")
        syn.set_conv_math("f16x2")
    syn.close()


@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFFFFFFF, 0x7BFF7BFF], ids=hex)
def test_a_poisoned_workspace_changes_nothing(pattern):
    cfg, blob = _tiny("hifigan_fix", 9)
    ids = _sentences(cfg)
    join = {"gap_frames": [0, 70, 2], "lead_frames": 60, "trail_frames": 9, "fade_ms": 4.0}

    def run(poison):
        syn = engine.Synthesizer(blob)
        if poison:
            syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
        out = [_cat(syn.infer_joined_stream(ids, 9, join=join)).tobytes()]
        assert (syn.profile()["poison_bytes"] > 0) == bool(poison)
        syn.debug_set("stream_direct", 1)          # native rate, no limiter: the join kernel itself stores the chunk into mapped pinned memory
        out.append(_cat(syn.infer_joined_stream(ids, 9, join=join)).tobytes())
        syn.debug_set("stream_direct", 0)
        syn.set_output_rate(24000)
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
        out.append(_cat(syn.infer_joined_stream(ids, 9, join=join)).tobytes())
        syn.debug_set("stream_direct", 1)
        out.append(_cat(syn.infer_joined_stream(ids, 9, join=join)).tobytes())
        syn.debug_set("stream_direct", 0)
        syn.set_output_rate(16000); syn.set_limiter(engine.LIMITER_OFF)
        out.append(syn.infer_joined(ids, join=join).tobytes())                             # and a whole call behind them
        syn.close()
        return out

    want = run(False)
    assert want[0] == want[1] == want[4] and want[2] == want[3]
    assert run(True) == want


def test_refusals_leave_the_engine_as_a_fresh_one():
    cfg, blob = _tiny("mbb_fix")
    ids = _sentences(cfg)
    fresh = _fresh_joined(blob, ids, JOIN)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    p = engine.PreparedBatch(ids, None, None)
    jp, keep = engine._join(p.B, JOIN)
    calls = []
    cb = engine.CHUNK_CB(lambda user, pcm, n, off: calls.append(n) or 0)
    total = C.c_int32(-7)

    def call(B=p.B, ptrs=p.ptrs, n=p.n_p, join=jp, chunk=4, cb=cb):
        return syn.lib.sts_infer_ids_joined_stream(syn.h, B, ptrs, n, p.sid_p, p.ls_p, join, chunk, cb, None, C.byref(total))

    def plain_is_fresh():
        assert not calls and total.value == -7
        assert np.array_equal(syn.infer_joined(ids, join=JOIN), fresh)

    for mode in (engine.LOUD_MEASURE, engine.LOUD_NORMALIZE):
        syn.set_loudness(mode, -20.0, -1.0)
        assert call() == STS_EINVAL
        syn.set_loudness(engine.LOUD_OFF)
        plain_is_fresh()
    syn.set_eq([{"type": engine.EQ_PEAK, "freq_hz": 1000.0, "gain_db": 3.0, "q": 1.0}])
    assert call() == STS_EINVAL
    syn.set_eq([])
    plain_is_fresh()
    bad, keep2 = engine._join(p.B, dict(JOIN, fade_ms=50.5))
    for kw in (dict(chunk=0), dict(chunk=-3), dict(cb=C.cast(None, engine.CHUNK_CB)), dict(join=bad), dict(B=0), dict(ptrs=None), dict(n=None)):
        assert call(**kw) == STS_EINVAL, kw
        plain_is_fresh()
    assert call() == STS_OK and sum(calls) == total.value == fresh.size
    syn.close()
