"""Paragraph join on the MI355X (sts_join_apply, sts_infer_ids_joined, sts_get_join_offsets, sts_pool_submit_joined) against the NumPy
restatement of tests/join_ref.py, bit for bit: the kernel on caller signals across its span, sentence and alignment edges; an engine's
"wave_join" tap and PCM against the restatement applied to the same call's per-sentence "wave" tap; the chain behind the join (resampler,
loudness, limiter) against the existing checkers fed with "wave_join" as ONE utterance; plans, speakers and offsets per sentence; a
poisoned workspace; the pool; refusals.

The resampler is an fp32 FMA chain and tests/resample_ref.py a float64 sum, so the two cannot agree to the bit; the comparison at 8 and
44.1 kHz is the one tests/test_resample_gpu.py (_check_against_checker) makes for a plain utterance, applied to J: the float output within
1e-5 of the checker, the PCM within 1 LSB of the checker's cast and exactly the cast of the float output.  (Measured on an MI355X: 1 of
17184 PCM samples at 8 kHz and 6 of 94727 at 44.1 kHz are 1 LSB off the float64 checker's cast; max |wave_out - checker| 4.1e-08.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gain_ref as gr
import join_ref as jr
import limiter_ref as lref
import loudness_ref as lr
import resample_ref as rr
from summertts_amd import engine, synth_blob as sb
from test_loudness_gpu import _close as loud_close          # the loudness checker's own comparison (lufs 0.01, peak exact, gain 1e-4)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STS_EINVAL = -1
INF, NAN = float("inf"), float("nan")
RESAMPLE_WAVE_TOL = 1e-5        # tests/test_resample_gpu.py _check_against_checker
# samples of J one workgroup of join_kernel owns: read from the kernel file itself
SPAN = int(re.search(r"static constexpr int kJoinSpan = (\d+);", open(os.path.join(ROOT, "summertts_amd", "csrc", "join.hip")).read()).group(1))
FADES = (0.0, 0.0625, 5.0, 50.0)        # h = 0, 1, 80, 800


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _tiny(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    return cfg, sb.make_blob(cfg, seed)


# ---- 1. the kernel on caller signals -------------------------------------------------------------------------------------------------------
def _signal(n, seed):
    x = (0.5 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    x[::53] = np.float32(1.3)            # past 1.0009: the cast wraps, also on a faded edge's inner samples
    x[7::211] = np.float32(-2.7)
    return x


def _apply_case(frames, hop, join, seed=0):
    sig = [_signal(int(f) * hop, seed + b) for b, f in enumerate(frames)]
    y, pcm = engine.join_apply(sig, frames, hop, join)
    J, want = jr.join(sig, frames, hop, join)
    bad = np.flatnonzero(y.view(np.uint32) != J.view(np.uint32))
    assert y.size == J.size and bad.size == 0, (hop, list(frames), join, int(bad[0]) if bad.size else -1)
    assert np.array_equal(pcm, want), (hop, list(frames), join)
    return sig, y, pcm


def test_the_span_constant_is_the_kernel_files():
    assert SPAN == 4096 and SPAN % 256 == 0
    assert [jr.design(f) for f in FADES] == [0, 1, 80, 800]


@pytest.mark.parametrize("hop", [4, 256])
@pytest.mark.parametrize("B", [1, 2, 7])
def test_apply_on_every_span_and_sentence_edge(hop, B):
    """sentences of one frame, of exactly one span of the kernel, one span less a frame and one span plus a frame, three spans and a tail;
    gap 0 next to gap 3; lead only and trail only; every fade, with sentences shorter than 2 h"""
    S = SPAN // hop
    pool = [S, 1, S - 1, S + 1, 3, 3 * S + 5, 1]
    for rot in range(3 if B < 7 else 1):
        frames = [pool[(rot * 2 + b) % len(pool)] for b in range(B)]
        gaps = [(0, 3, 0, 1, 3, 0)[b % 6] for b in range(B - 1)]
        for k, fade in enumerate(FADES):
            for join in ({"gap_frames": gaps, "fade_ms": fade}, {"gap_frames": gaps, "lead_frames": 5, "fade_ms": fade},
                         {"trail_frames": 2, "fade_ms": fade}):
                _apply_case(frames, hop, join, seed=10 * rot + k)
    sig, y, pcm = _apply_case([1, S, 2], hop, None)                 # join == NULL: back to back, bit for bit
    assert y.tobytes() == np.concatenate(sig).tobytes()
    loud = np.concatenate(sig) > 1.0009
    assert loud.any() and (pcm[loud] < 0).all()                     # the cast wrapped around, as the reference's does


def test_apply_takes_the_scalar_path_for_other_hops():
    """samples per frame that are no multiple of 4 (no decoder of the model format has one; the entry accepts them): sample by sample"""
    for hop, frames in ((1, [SPAN, 1, SPAN - 1, SPAN + 1, 3]), (6, [683, 1, 682, 2]), (3, [1, 1, 1])):
        for fade in FADES:
            _apply_case(frames, hop, {"gap_frames": [(0, 3)[b % 2] for b in range(len(frames) - 1)], "lead_frames": 1, "trail_frames": 1,
                                      "fade_ms": fade}, seed=hop)


def test_apply_long_silence_and_refusals():
    hop = 256
    sig, y, pcm = _apply_case([2, 1], hop, {"gap_frames": [40], "lead_frames": 33, "trail_frames": 17, "fade_ms": 1.0})
    assert y.size == (3 + 90) * hop and np.count_nonzero(y) <= 3 * hop          # whole spans of silence, written by the same launch
    lib = engine.load_library()
    x = np.zeros(8, np.float32); f = np.asarray([1, 1], np.int32)
    assert lib.sts_join_apply(0, x.ctypes.data, f.ctypes.data, 0, 4, None, x.ctypes.data, None) == STS_EINVAL
    assert lib.sts_join_apply(0, x.ctypes.data, f.ctypes.data, 2, 0, None, x.ctypes.data, None) == STS_EINVAL
    assert lib.sts_join_apply(0, None, f.ctypes.data, 2, 4, None, x.ctypes.data, None) == STS_EINVAL
    jp, keep = engine._join(2, {"fade_ms": 50.5})
    assert lib.sts_join_apply(0, x.ctypes.data, f.ctypes.data, 2, 4, jp, x.ctypes.data, None) == STS_EINVAL
    f[1] = 0
    assert lib.sts_join_apply(0, x.ctypes.data, f.ctypes.data, 2, 4, None, x.ctypes.data, None) == STS_EINVAL


# ---- 2. the engine, nothing downstream ---------------------------------------------------------------------------------------------------
LENS = (1, 3, 7, 12)
JOIN = {"gap_frames": [0, 3, 1], "lead_frames": 2, "trail_frames": 1, "fade_ms": 5.0}


def _sentences(cfg, lens=LENS):
    return [sb.synthetic_ids(n, cfg.vocab, salt=3 * n + 1) for n in lens]


def _frames(dur, lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    return [max(1, int(dur[off[b]:off[b + 1]].sum())) for b in range(len(lens))]


def _split(wave, frames, hop):
    off = np.concatenate([[0], np.cumsum(frames)]) * hop
    assert wave.size == off[-1]
    return [wave[off[b]:off[b + 1]] for b in range(len(frames))]


def _joined_with_taps(syn, ids, join, sid=None):
    syn.set_record_taps(True)
    pcm = syn.infer_joined(ids, sid, None, join)
    lens = [len(a) for a in ids]
    dur = syn.durations(sum(lens))
    out = pcm, syn.tap("wave")[0], syn.tap("wave_join")[0], dur, _frames(dur, lens)
    syn.set_record_taps(False)
    return out


def _infer_ids_c(syn, ids, sid=0, ls=1.0):
    """sts_infer_ids itself (the class goes through sts_run_batch + sts_copy_pcm_host)"""
    a = np.ascontiguousarray(ids, dtype=np.int32)
    p, n = C.POINTER(C.c_int16)(), C.c_int32()
    rc = syn.lib.sts_infer_ids(syn.h, a.ctypes.data, a.size, sid, ls, C.byref(p), C.byref(n))
    assert rc == 0, syn.lib.sts_last_error()
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    syn.lib.sts_free(p)
    return out


@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix"])
def test_native_rate_is_the_restatement_on_the_calls_own_waves(kind):
    cfg, blob = _tiny(kind)
    ids = _sentences(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    hop = syn.info.samples_per_frame
    members = syn.infer_batch(ids)
    pcm, wave, J, dur, frames = _joined_with_taps(syn, ids, JOIN)
    assert [m.size for m in members] == [f * hop for f in frames]
    want, want_pcm = jr.join(_split(wave, frames, hop), frames, hop, JOIN)
    assert J.tobytes() == want.tobytes() and np.array_equal(pcm, want_pcm), kind
    assert np.array_equal(syn.infer_joined(ids, join=JOIN), pcm), kind                     # without taps: the PCM goes straight to the host
    assert np.array_equal(syn.join_offsets(4), jr.layout(frames, hop, JOIN)[0])
    with pytest.raises(engine.StsError):
        syn.tap("wave_join")                                                               # (the run without taps recorded none)
    # no fade: the members of sts_infer_ids_batch, concatenated with zeros
    nofade = dict(JOIN, fade_ms=0.0)
    start, total, h = jr.layout(frames, hop, nofade)
    cat = np.zeros(total, np.int16)
    for b, m in enumerate(members):
        cat[start[b]:start[b] + m.size] = m
    assert np.array_equal(syn.infer_joined(ids, join=nofade), cat), kind
    assert np.array_equal(syn.infer_joined(ids), np.concatenate(members)), kind           # join == NULL: back to back
    # one sentence, an all-zero join: sts_infer_ids
    for a in ids:
        one = syn.infer_joined([a], join={})
        assert np.array_equal(syn.join_offsets(1), [0])
        assert np.array_equal(one, _infer_ids_c(syn, a)), (kind, len(a))
    # a plain call afterwards is a plain call: per-utterance counts, no join offsets
    assert all(np.array_equal(a, b) for a, b in zip(syn.infer_batch(ids), members))
    with pytest.raises(engine.StsError):
        syn.join_offsets(4)
    syn.close()


# ---- 3. downstream sees one utterance ----------------------------------------------------------------------------------------------------
LONG = (40, 9, 55)
LJOIN = {"gap_frames": [0, 6], "lead_frames": 3, "trail_frames": 2, "fade_ms": 0.0}


@pytest.fixture(scope="module")
def long_model():
    cfg, blob = _tiny("mbb_fix", 7)
    return cfg, blob, [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in LONG]


@pytest.mark.parametrize("rate", [8000, 44100])
def test_the_resampler_reads_the_joined_wave(long_model, rate):
    cfg, blob, ids = long_model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    hop = syn.info.samples_per_frame
    join = dict(LJOIN, fade_ms=2.0)
    syn.set_record_taps(True)
    pcm = syn.infer_joined(ids, join=join)
    wave, J, got = syn.tap("wave")[0], syn.tap("wave_join")[0], syn.tap("wave_out")[0]
    frames = _frames(syn.durations(sum(LONG)), LONG)
    syn.set_record_taps(False)
    assert J.tobytes() == jr.join(_split(wave, frames, hop), frames, hop, join)[0].tobytes()
    want = rr.resample(J, rate)
    err = float(np.abs(got - want).max())
    d = np.abs(pcm.astype(np.int64) - rr.pcm_cast(want).astype(np.int64))
    print(f"rate {rate}: max |wave_out - checker(wave_join)| = {err:.3e}; PCM samples off the checker's cast: {int((d != 0).sum())} of {pcm.size}, max {int(d.max())} LSB")
    assert got.size == pcm.size == rr.out_len(J.size, rate) and err <= RESAMPLE_WAVE_TOL, (rate, err)
    assert d.max() <= 1, (rate, int(d.max()))
    assert np.array_equal(pcm, rr.pcm_cast(got)), rate
    # the taps of the filter reach across the butt join between sentences 0 and 1: with zeros behind sentence 0 the last outputs in front
    # of the join are other numbers, and the engine's are not those
    start = jr.layout(frames, hop, join)[0]
    j1 = rr.out_len(int(start[1]), rate)
    cut = rr.resample(J[:start[1]], rate)
    assert cut.size == j1 and np.abs(got[j1 - 8:j1] - cut[j1 - 8:j1]).max() > 10 * RESAMPLE_WAVE_TOL, rate
    assert np.array_equal(syn.join_offsets(3), [rr.out_len(int(s), rate) for s in start])
    assert np.array_equal(syn.infer_joined(ids, join=join), pcm)                           # without taps
    syn.close()


def test_loudness_measures_and_normalizes_the_paragraph_once(long_model):
    cfg, blob, ids = long_model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    join = dict(LJOIN, fade_ms=3.0)
    plain = syn.infer_joined(ids, join=join)
    syn.set_loudness(engine.LOUD_NORMALIZE, -23.0, -1.0)
    syn.set_record_taps(True)
    pcm = syn.infer_joined(ids, join=join)
    J = syn.tap("wave_join")[0]
    syn.set_record_taps(False)
    res = syn.loudness()
    assert len(res) == 1
    want = lr.loudness(J, 16000, -23.0, -1.0)
    assert np.isfinite(want["lufs"])                                                       # the fixture is long enough to be measured
    loud_close(res[0], want, "joined")
    assert np.array_equal(pcm, lr.normalize(J, res[0]["gain"])) and not np.array_equal(pcm, plain)
    assert np.array_equal(syn.infer_joined(ids, join=join), pcm) and len(syn.loudness()) == 1
    syn.set_loudness(engine.LOUD_MEASURE, -23.0, -1.0)                                     # measuring leaves the PCM alone
    assert np.array_equal(syn.infer_joined(ids, join=join), plain) and len(syn.loudness()) == 1
    assert syn.loudness()[0]["lufs"] == res[0]["lufs"]
    # at another rate the measurement is of the resampled joined wave
    syn.set_loudness(engine.LOUD_NORMALIZE, -23.0, -1.0)
    syn.set_output_rate(22050)
    syn.set_record_taps(True)
    pcm = syn.infer_joined(ids, join=join)
    out = syn.tap("wave_out")[0]
    syn.set_record_taps(False)
    res = syn.loudness()
    assert len(res) == 1 and out.size == pcm.size == rr.out_len(J.size, 22050)
    loud_close(res[0], lr.loudness(out, 22050, -23.0, -1.0), "joined 22050")
    assert np.array_equal(pcm, lr.normalize(out, res[0]["gain"]))
    syn.close()


def test_the_limiter_looks_across_the_joins(long_model):
    cfg, blob, ids = long_model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    hop = syn.info.samples_per_frame
    lim = dict(gain_db=40.0, ceiling_dbfs=-6.0, lookahead_ms=2.0)
    syn.set_limiter(engine.LIMITER_ON, **lim)
    syn.set_record_taps(True)
    pcm = syn.infer_joined(ids, join=LJOIN)                                                # no fade: loud right up to the butt join
    J, ylim = syn.tap("wave_join")[0], syn.tap("wave_lim")[0]
    frames = _frames(syn.durations(sum(LONG)), LONG)
    syn.set_record_taps(False)
    H, c, G = engine.limiter_design(16000, **lim)
    g0 = lref.static_gain(G)
    y, s, S = lref.limit(J, g0, H, c)
    assert ylim.tobytes() == y.tobytes() and np.array_equal(pcm, lref.pcm_cast(y))
    st = syn.limiter()
    assert len(st) == 1
    want = lref.stats(y, s, S, g0, H)
    assert st[0]["gain"] == want["gain"] and st[0]["min_gain"] == want["min_gain"] and st[0]["peak_out"] == want["peak_out"]
    assert st[0]["limited"] == want["limited"] > 0
    # limiting the sentences one by one gives other samples within 2H of the butt join: a per-sentence implementation cannot pass
    start, total, _ = jr.layout(frames, hop, LJOIN)
    sep = np.zeros(total, np.float32)
    for b, f in enumerate(frames):
        sep[start[b]:start[b] + f * hop] = lref.limit(J[start[b]:start[b] + f * hop], g0, H, c)[0]
    a, b = int(start[1]) - 2 * H, int(start[1]) + 2 * H
    differ = np.flatnonzero(y[a:b] != sep[a:b])
    assert differ.size > 0 and not np.array_equal(pcm[a:b], lref.pcm_cast(sep[a:b]))
    assert np.array_equal(syn.infer_joined(ids, join=LJOIN), pcm) and len(syn.limiter()) == 1      # without taps
    syn.close()


# ---- 4. plans, speakers and offsets carry over per sentence --------------------------------------------------------------------------------
def test_plans_speakers_and_offsets_per_sentence():
    cfg, blob = _tiny("ms_hifigan_sdp", 5)
    lens = (7, 12)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    hop = syn.info.samples_per_frame
    join = {"gap_frames": [4], "lead_frames": 1, "trail_frames": 3, "fade_ms": 1.0}
    db = np.zeros(12, np.float32); db[2] = -INF
    gains = [None, {"gain_db": db, "ramp_ms": 2.0}]
    for rate, (P, Q) in ((16000, (1, 1)), (22050, (441, 320))):
        syn.set_output_rate(rate)
        syn.set_duration_plan(lens, [{"target_frames": 40}, None])
        syn.set_gain_plan(lens, gains)
        syn.set_record_taps(True)
        pcm = syn.infer_joined(ids, [0, 1], None, join)
        wave, wg, J = syn.tap("wave")[0], syn.tap("wave_gain")[0], syn.tap("wave_join")[0]
        dur = syn.durations(sum(lens))
        poff, joff = syn.phoneme_offsets(sum(lens)), syn.join_offsets(2)
        syn.set_record_taps(False)
        frames = _frames(dur, lens)
        assert frames[0] == 40
        xs, durs = _split(wave, frames, hop), [dur[:7], dur[7:]]
        gained = [gr.apply(xs[b], durs[b], hop, None if gains[b] is None else gains[b]["gain_db"], 2.0) for b in range(2)]
        assert wg.tobytes() == np.concatenate(gained).tobytes() and gained[0].tobytes() == xs[0].tobytes()
        assert gained[1].tobytes() != xs[1].tobytes()
        want, want_pcm = jr.join(gained, frames, hop, join)
        assert J.tobytes() == want.tobytes(), rate
        if rate == 16000:
            assert np.array_equal(pcm, want_pcm)
        start = jr.layout(frames, hop, join)[0]
        ceil = lambda v: (int(v) * P + Q - 1) // Q
        assert joff.tolist() == [ceil(s) for s in start], rate
        wantp = []
        for b in range(2):
            f = np.concatenate([[0], np.cumsum(durs[b])[:-1]])
            wantp += [ceil(start[b] + int(v) * hop) for v in f]
        assert poff.tolist() == wantp, rate
        assert pcm.size == ceil(J.size)
    syn.set_output_rate(16000)
    # the plans applied to that call only
    nofade = dict(join, fade_ms=0.0)
    pcm = syn.infer_joined(ids, [0, 1], None, nofade)
    alone = syn.infer_batch(ids, [0, 1])
    start = jr.layout([a.size // hop for a in alone], hop, nofade)[0]
    for b in range(2):                                                                     # each sentence with its own speaker
        assert np.array_equal(pcm[start[b]:start[b] + alone[b].size], alone[b]), b
    assert np.array_equal(alone[0], syn.infer_ids(ids[0], 0)) and np.array_equal(alone[1], syn.infer_ids(ids[1], 1))
    other = syn.infer_batch(ids, [0, 0])
    assert np.array_equal(other[0], alone[0]) and not np.array_equal(other[1], alone[1])
    # forced durations carry over too
    forced = np.r_[np.full(7, 2), np.full(12, 1)].astype(np.int32)
    syn.set_forced_durations(forced)
    pcm = syn.infer_joined(ids, [0, 1], None, nofade)
    assert np.array_equal(syn.durations(19), forced) and pcm.size == (14 + 12 + 8) * hop
    assert syn.join_offsets(2).tolist() == [hop, (1 + 14 + 4) * hop]
    syn.close()


# ---- 5. poison ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFFFFFFF, 0x7BFF7BFF], ids=hex)
def test_a_poisoned_workspace_changes_nothing(pattern):
    cfg, blob = _tiny("hifigan_fix", 9)
    ids = _sentences(cfg)
    join = {"gap_frames": [0, 700, 2], "lead_frames": 600, "trail_frames": 9, "fade_ms": 4.0}        # gaps of whole spans

    def run(poison):
        syn = engine.Synthesizer(blob)
        if poison:
            syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
        out = [syn.infer_joined(ids, join=join).tobytes()]
        syn.set_record_taps(True)
        out.append(syn.infer_joined(ids, join=join).tobytes())
        out.append(syn.tap("wave_join").tobytes())
        syn.set_record_taps(False)
        syn.set_output_rate(24000)
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
        syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -1.0)
        out.append(syn.infer_joined(ids, join=join).tobytes())
        out.append(syn.loudness().tobytes() + syn.limiter().tobytes())
        assert (syn.profile()["poison_bytes"] > 0) == bool(poison)
        syn.set_output_rate(16000); syn.set_limiter(engine.LIMITER_OFF); syn.set_loudness(engine.LOUD_OFF)
        out.append(syn.infer_batch(ids)[2].tobytes())                                      # and a plain call behind them
        syn.close()
        return out

    want = run(False)
    assert want[0] == want[1]
    assert run(True) == want


# ---- 6. the pool ---------------------------------------------------------------------------------------------------------------------------
def test_the_pool_runs_a_paragraph_as_one_request():
    cfg, blob = _tiny("hifigan_sdp", 11)
    para = [[sb.synthetic_ids(n, cfg.vocab, salt=n + 20 * k) for n in (5, 11, 3)] for k in range(2)]
    singles = [sb.synthetic_ids(9, cfg.vocab, salt=77), sb.synthetic_ids(14, cfg.vocab, salt=78)]
    joins = [{"gap_frames": [2, 0], "lead_frames": 1, "fade_ms": 3.0}, None]
    syn = engine.Synthesizer(blob)
    want = []
    for k in range(2):
        syn.set_noise(0.4, 0.6, 100 + k)
        want.append(syn.infer_joined(para[k], join=joins[k]))
    syn.set_noise(0.0, 0.0, 0)
    plain = [syn.infer_ids(a) for a in singles]
    syn.close()
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=1)          # a paragraph of 3 sentences: above max_batch
    t = pool.submit_joined(para[0], noise_scale=0.4, noise_scale_w=0.6, seed=100, join=joins[0])
    assert np.array_equal(pool.wait(t), want[0])
    # two paragraphs and two plain requests in flight at once
    tj0 = pool.submit_joined(para[0], noise_scale=0.4, noise_scale_w=0.6, seed=100, join=joins[0])
    tp0 = pool.submit(singles[0])
    tj1 = pool.submit_joined(para[1], noise_scale=0.4, noise_scale_w=0.6, seed=101, join=joins[1])
    tp1 = pool.submit(singles[1])
    assert np.array_equal(pool.wait(tp1), plain[1]) and np.array_equal(pool.wait(tj1), want[1])
    assert np.array_equal(pool.wait(tj0), want[0]) and np.array_equal(pool.wait(tp0), plain[0])
    assert pool.stats() == (5, 5)                                          # one batch and one request per paragraph
    with pytest.raises(engine.StsError):
        pool.submit_joined(para[0], join={"fade_ms": 51.0})
    with pytest.raises(engine.StsError):
        pool.submit_joined(para[0], join={"gap_frames": [0, 100001]})
    t = pool.submit_joined([[0, 1, cfg.vocab]])                            # a bad id fails its own ticket
    with pytest.raises(engine.StsError):
        pool.wait(t)
    assert np.array_equal(pool.wait(pool.submit(singles[0])), plain[0])
    pool.close()
    # the pool's output rate and limiter apply to the joined signal
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=4)
    pool.set_output_rate(8000)
    pool.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
    got = pool.wait(pool.submit_joined(para[1], join=joins[0]))
    pool.close()
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(8000)
    syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
    assert np.array_equal(syn.infer_joined(para[1], join=joins[0]), got)
    syn.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------
def _joined_c(syn, ids, jp):
    """sts_infer_ids_joined itself -> (rc, the output pointer's value, n_out): nothing may be delivered on a failure"""
    p = engine.PreparedBatch(ids)
    out, n = C.POINTER(C.c_int16)(), C.c_int32(-5)
    rc = syn.lib.sts_infer_ids_joined(syn.h, p.B, p.ptrs, p.n_p, p.sid_p, p.ls_p, jp, C.byref(out), C.byref(n))
    return rc, bool(out), n.value


def test_refusals_leave_the_engine_as_a_fresh_one():
    cfg, blob = _tiny("hifigan_fix", 3)
    ids = _sentences(cfg)
    fresh = engine.Synthesizer(blob)
    fresh.set_conv_mode(6)
    want = fresh.infer_ids(ids[3])
    want_j = fresh.infer_joined(ids, join=JOIN)
    fresh.close()
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    for bad in ({"fade_ms": NAN}, {"fade_ms": 50.0001}, {"gap_frames": [0, -1, 0]}, {"gap_frames": [0, 0, 100001]}, {"lead_frames": -1},
                {"trail_frames": 100001}):
        jp, keep = engine._join(4, bad)
        assert _joined_c(syn, ids, jp) == (STS_EINVAL, False, -5), bad
        assert np.array_equal(syn.infer_ids(ids[3]), want), bad
    assert _joined_c(syn, [], None)[0] == STS_EINVAL                                       # B == 0
    # a plan pending for another B: refused, nothing runs, the plan is gone
    for setter in (lambda: syn.set_gain_plan([12], [{"gain_db": [-20.0] * 12}]), lambda: syn.set_duration_plan([12], [{"target_frames": 90}]),
                   lambda: syn.set_gain_plan([1, 3, 7, 11], [None] * 4)):
        setter()
        rc, delivered, n = _joined_c(syn, ids, None)
        assert (rc, delivered, n) == (STS_EINVAL, False, -5) and b"another batch" in syn.lib.sts_last_error()
        assert np.array_equal(syn.infer_ids(ids[3]), want)
    with pytest.raises(engine.StsError):
        syn.join_offsets(4)
    # streaming has no joined form; a stream afterwards is a plain stream
    assert np.array_equal(np.concatenate(syn.infer_ids_stream(ids[3], 4)[0]), want)
    assert np.array_equal(syn.infer_joined(ids, join=JOIN), want_j)
    # a joined call stays off the launch-ahead memo
    assert np.array_equal(syn.infer_ids(ids[3]), want) and syn.profile()["launch_ahead"] == 1
    assert np.array_equal(syn.infer_joined([ids[3]], join={}), want) and syn.profile()["launch_ahead"] == 0
    syn.close()


def test_an_output_longer_than_int32_is_refused_before_the_decoder():
    """lead and 28 gaps of 100000 frames at 256 samples per frame: 742 M native samples, 2.2 G samples at 48 kHz"""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    B = 29
    ids = [sb.synthetic_ids(2 + b % 3, cfg.vocab, salt=b) for b in range(B)]
    join = {"gap_frames": [100000] * (B - 1), "lead_frames": 100000}
    fresh = engine.Synthesizer(blob)
    want = fresh.infer_ids(ids[1])
    fresh.close()
    syn = engine.Synthesizer(blob)
    assert syn.info.samples_per_frame == 256
    syn.set_output_rate(48000)
    jp, keep = engine._join(B, join)
    rc, delivered, n = _joined_c(syn, ids, jp)
    assert (rc, delivered, n) == (STS_EINVAL, False, -5) and b"too long" in syn.lib.sts_last_error()
    assert syn.profile()["ms_decoder"] == 0.0 and syn.profile()["samples"] == 0            # nothing behind the durations ran
    jp, keep = engine._join(B, dict(join, trail_frames=100000, gap_frames=[100000] * 27 + [0]))
    assert _joined_c(syn, ids, jp)[0] == STS_EINVAL
    syn.set_output_rate(16000)
    assert np.array_equal(syn.infer_ids(ids[1]), want)                                     # what a fresh engine returns
    syn.close()
