"""GPU suite (MI355X): no result may depend on stale device memory.

A fresh hipMalloc arena holds whatever the driver hands out -- in practice zero pages -- so a kernel that reads memory no kernel of the
current call wrote (the 64-frame bucket tail of a one-utterance call, a window's halo, a partial tile, a counter that only works from zero)
passes every test that builds a fresh engine.  Here the engine's test hook STS_DBG_POISON fills both workspace arenas after each layout,
and the host-visible outputs before the call, with a pattern:

    0x7FC00000   quiet NaN as fp32
    0xFFFFFFFF   NaN as fp32, -1 as int32 and int16
    0x7BFF7BFF   finite as fp32 (~2.7e36), 65504 in each fp16 half, 31743 as int16

and every call sequence must return, bit for bit, what the same sequence returns on an engine that was never poisoned: PCM, per-utterance
sample counts, durations, loudness results, recorded taps.  Under the default two-term fp16 arithmetic no call may be repeated in the
split-bf16 form (the overflow word must only see values the call computed), except where a model provokes the repeat on purpose.

One further test runs a mixed sequence on one full-size engine WITHOUT the hook: there the memory holds the previous call, the production
form of the same class of bug.

Out of reach of this file: the request pool and sts_multi (their engines are internal and sts_debug_set does not reach them) and the
stand-alone sts_debug_conv* entry points (compared with torch at every position by test_parity_gpu.py).
"""
import dataclasses

import numpy as np
import pytest

from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

PATTERNS = (0x7FC00000, 0xFFFFFFFF, 0x7BFF7BFF)
TAPS = ("x_enc", "z", "wave")


def _s32(p):
    return p - (1 << 32) if p >= (1 << 31) else p


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Rec:
    """Runs calls on one engine and keeps what each returned; on a poisoned engine also checks that the fill happened."""

    def __init__(self, syn, poisoned):
        self.syn, self.poisoned, self.out = syn, poisoned, []

    def _done(self, what, r):
        p = self.syn.profile()
        r["profile"] = p
        r["what"] = what
        if self.poisoned:
            # at least the phoneme-level encoder input and the frame-level latent of the call were filled (both arenas' extents exceed these)
            floor = 4 * self.syn.info.hidden * p["phonemes"] + 4 * self.syn.info.inter_channels * p["frames"]
            assert p["poison_bytes"] >= floor > 0, (what, p["poison_bytes"], floor)
        else:
            assert p["poison_bytes"] == 0, what
        self.out.append(r)

    def run(self, what, ids, sid=None, ls=None, forced=None, taps=False):
        syn = self.syn
        if forced is not None:
            syn.set_forced_durations(forced)
        if taps:
            syn.set_record_taps(True)
        n = syn.run_batch(ids, sid, ls)
        r = {"n": n.copy(), "pcm": syn.pcm_host().copy(), "dur": syn.durations(sum(len(x) for x in ids)), "loud": syn.loudness().tobytes()}
        if taps:
            for t in TAPS:
                r[t] = syn.tap(t)
            syn.set_record_taps(False)
        self._done(what, r)
        return r

    def stream(self, what, ids, chunk, sid=0, ls=1.0):
        chunks, _ = self.syn.infer_ids_stream(ids, chunk, sid, ls)
        self._done(what, {"pcm": np.concatenate(chunks) if chunks else np.zeros(0, np.int16), "sizes": [c.size for c in chunks],
                          "dur": self.syn.durations(len(ids))})

    def bstream(self, what, ids, chunk, sid=None):
        tot = []
        chunks, _ = self.syn.infer_batch_stream(ids, chunk, sid, n_total=tot)
        self._done(what, {"pcm": [np.concatenate(c) if c else np.zeros(0, np.int16) for c in chunks],
                          "sizes": [[x.size for x in c] for c in chunks], "n": tot, "dur": self.syn.durations(sum(len(x) for x in ids))})


def _compare(got, want, label, fallbacks_as_fresh=False):
    assert [r["what"] for r in got] == [r["what"] for r in want]
    for g, w in zip(got, want):
        where = f"{label}: {g['what']}"
        gp, wp = g["profile"], w["profile"]
        if fallbacks_as_fresh:
            assert (gp["conv_math_fallbacks"], gp["conv_math_pinned"]) == (wp["conv_math_fallbacks"], wp["conv_math_pinned"]), where
        else:
            assert wp["conv_math_fallbacks"] == 0 and wp["conv_math_pinned"] == 0, f"{where}: the unpoisoned engine repeated a call"
            assert gp["conv_math_fallbacks"] == 0 and gp["conv_math_pinned"] == 0, \
                f"{where}: split-bf16 repeat under poison (conv_math_fallbacks = {gp['conv_math_fallbacks']})"
        for k in w:
            if k in ("profile", "what"):
                continue
            if isinstance(w[k], list) and w[k] and isinstance(w[k][0], np.ndarray):
                assert len(g[k]) == len(w[k]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(g[k], w[k])), f"{where}: {k} differs"
            elif isinstance(w[k], np.ndarray):
                assert g[k].shape == w[k].shape and np.array_equal(_bits(g[k]), _bits(w[k])), f"{where}: {k} differs"
            else:
                assert g[k] == w[k], f"{where}: {k} differs"


def _check_case(blob, scenario, label, setup=None, fallbacks_as_fresh=False):
    """scenario(rec) on a fresh engine, then on one freshly poisoned engine per pattern: every result equal bit for bit."""
    def one(pattern):
        syn = engine.Synthesizer(blob)
        syn.set_profiling(True)
        if setup:
            setup(syn)
        if pattern:
            syn.debug_set("poison", _s32(pattern))
        rec = Rec(syn, pattern != 0)
        scenario(rec)
        syn.close()
        return rec.out
    want = one(0)
    for pattern in PATTERNS:
        _compare(one(pattern), want, f"{label} / poison {pattern:#010x}", fallbacks_as_fresh)
    return want


def _sid(cfg, k=1):
    return k % cfg.spk_num if cfg.is_ms else 0


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hifigan_sdp", "mbb_fix", "istft_fix", "ms_sdp", "ms_hifigan_sdp"])
def test_single_utterance_calls_do_not_read_stale_memory(kind):
    """One-utterance calls (buffers sized for the 64-frame bucket): frame counts inside a bucket and one that fills it, the launch-ahead
    memo hit, the PCM written into the pinned buffer by the last kernel and downloaded behind it, taps, a one-phoneme utterance."""
    cfg = sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 41)
    s = _sid(cfg)
    a23, a9, a31, a1 = (sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (23, 9, 31, 1))
    a10 = sb.synthetic_ids(10, cfg.vocab, salt=4)

    def scenario(r):
        r.run("23", [a23], [s])
        r.run("9", [a9], [s])
        r.run("23 again (memo hit)", [a23], [s])
        r.run("10, forced to 64 frames", [a10], [s], forced=[7, 6, 7, 6, 7, 6, 7, 6, 7, 5])
        r.syn.debug_set("pcm_direct", 0)
        r.run("23 (download)", [a23], [s])
        r.run("31 (download)", [a31], [s])
        r.syn.debug_set("pcm_direct", 1)
        r.run("1", [a1], [s])
        r.run("31 (taps)", [a31], [s], taps=True)
    want = _check_case(blob, scenario, kind)
    frames = [w["profile"]["frames"] for w in want]
    assert frames[3] == 64 and any(f % 64 for f in frames), frames
    assert want[2]["profile"]["launch_ahead"] == 1


@pytest.mark.parametrize("kind", ["ms_hifigan_sdp", "mbb_fix"])
def test_packed_ragged_batches_do_not_read_stale_memory(kind):
    """Packed batches: ragged lengths with a one-phoneme member, the batch again (launched from the memo), forced durations with zeros and
    one member whose durations are all zero (the reference's one-frame minimum), taps of a batch."""
    cfg = sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 43)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=2 * t) for t in (1, 17, 5, 30, 9)]
    sids = [_sid(cfg, k) for k in range(len(ids))]
    ids3 = [sb.synthetic_ids(t, cfg.vocab, salt=5) for t in (4, 3, 6)]
    forced = [1, 0, 2, 0] + [0, 0, 0] + [3, 1, 0, 2, 0, 1]

    def scenario(r):
        r.run("ragged", ids, sids, [1.0, 1.1, 0.9, 1.0, 1.2])
        r.run("ragged again (memo)", ids, sids, [1.0, 1.1, 0.9, 1.0, 1.2])
        r.run("forced with zeros", ids3, sids[:3], forced=forced)
        r.run("ragged (taps)", ids[1:], sids[1:], taps=True)
    want = _check_case(blob, scenario, kind)
    assert want[1]["profile"]["launch_ahead"] == 1
    assert int(want[2]["n"][1]) == cfg.hop_total          # (all durations zero: one frame)


@pytest.mark.parametrize("kind", ["hifigan_sdp", "ms_sdp"])
def test_streaming_does_not_read_stale_memory(kind):
    """sts_infer_ids_stream at 1-, 7- and 64-frame chunks (windows with halos, a chunk buffer reused step after step) and
    sts_infer_ids_batch_stream (windows of several utterances per step, a per-step table, the packed chunk buffer)."""
    cfg = sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 47)
    s = _sid(cfg)
    a = sb.synthetic_ids(19, cfg.vocab, salt=3)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (12, 1, 25)]
    sids = [_sid(cfg, k) for k in range(3)]

    def scenario(r):
        for chunk in (1, 7, 64):
            r.stream(f"stream {chunk}", a, chunk, s)
        r.bstream("batch stream 7", ids, 7, sids)
        r.bstream("batch stream 64", ids, 64, sids)
        r.syn.debug_set("stream_direct", 1)
        r.bstream("batch stream 5 (direct)", ids, 5, sids)
    _check_case(blob, scenario, kind)


def test_output_rates_do_not_read_stale_memory():
    """Resampled PCM at 8 kHz, 44.1 kHz (coefficient table in global memory) and 48 kHz (table in LDS): one utterance, a batch, a stream, taps."""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 53)
    a = sb.synthetic_ids(21, cfg.vocab, salt=1)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (7, 26, 1)]

    def scenario(r):
        for rate in (8000, 44100, 48000):
            r.syn.set_output_rate(rate)
            r.run(f"{rate}: one", [a])
            r.run(f"{rate}: one again (memo)", [a])
            r.run(f"{rate}: batch", ids)
            r.stream(f"{rate}: stream 7", a, 7)
            r.bstream(f"{rate}: batch stream 9", ids, 9)
            r.run(f"{rate}: taps", [a], taps=True)
        r.syn.set_output_rate(0)
        r.run("native again", [a])
    _check_case(blob, scenario, "output rates")


def test_loudness_does_not_read_stale_memory():
    """Loudness measurement (mode 1) and normalization (mode 2): results per utterance and the PCM, at the native rate and at 44.1 kHz.
    Forced durations stretch the tiny model's utterances past the 400 ms of one gating block for some members, not for others."""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 59)
    a = sb.synthetic_ids(90, cfg.vocab, salt=1)
    lens = (60, 3, 110)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in lens]
    fa, fb = [12] * len(a), [12] * sum(lens)

    def scenario(r):
        for mode in (1, 2):
            r.syn.set_loudness(mode, -20.0, -2.0)
            r.run(f"mode {mode}: one", [a], forced=fa)
            r.run(f"mode {mode}: batch", ids, forced=fb)
            r.run(f"mode {mode}: one, predicted durations", [a])
        r.syn.set_output_rate(44100)
        r.run("mode 2 at 44.1 kHz: batch", ids, forced=fb)
        r.run("mode 2 at 44.1 kHz: one", [a], forced=fa)
    want = _check_case(blob, scenario, "loudness")
    lufs = [np.frombuffer(w["loud"], engine.LOUDNESS_DTYPE)["lufs"] for w in want]
    assert [x.size for x in lufs] == [1, 3, 1, 1, 3, 1, 3, 1]
    assert any(np.isfinite(x).any() for x in lufs), f"no utterance was measured: {lufs}"


def test_sampling_noise_does_not_read_stale_memory():
    """Sampling noise on a model with the stochastic duration predictor (the latent of the predictor and of the prior)."""
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 61)
    a = sb.synthetic_ids(24, cfg.vocab, salt=2)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (11, 1, 20)]

    def scenario(r):
        r.syn.set_noise(0.667, 0.8, 12345)
        r.run("one", [a], [1])
        r.run("one again (memo)", [a], [1])
        r.run("batch", ids, [0, 1, 2])
        r.stream("stream 7", a, 7, 1)
        r.run("taps", [a], [1], taps=True)
    _check_case(blob, scenario, "sampling noise")


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_other_trunk_arithmetics_do_not_read_stale_memory(math):
    """The split-bf16 and exact-fp32 trunk kernels (the default two-term fp16 form runs in every other test of this file)."""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 67)
    a = sb.synthetic_ids(23, cfg.vocab, salt=6)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (13, 1, 29)]

    def scenario(r):
        r.run("one", [a])
        r.run("one again (memo)", [a])
        r.run("batch", ids)
        r.stream("stream 7", a, 7)
        r.run("taps", [a], taps=True)
    _check_case(blob, scenario, math, setup=lambda syn: syn.set_conv_math(math))


@pytest.mark.parametrize("math", ["f16x2", "bf16x3"])
def test_pre_split_stages_do_not_read_stale_memory(math):
    """The pre-split (channel-minor, two-term fp16) ResBlock stages, forced on a small model with 128-channel stages.  The stage entry converts
    and range-checks its input: positions beyond the utterance (the 64-frame bucket tail of a one-utterance call) must not reach the overflow
    word.  (bf16x3: the same model on the staged kernels, as a control.)"""
    cfg = dataclasses.replace(sb.tiny_cfg("hifigan_fix"), up_init=256, res_k=(5, 9), res_d=((1, 2, 4), (3, 1, 5)))
    blob = sb.make_blob(cfg, 31 + 256)
    a41, a9 = sb.synthetic_ids(41, cfg.vocab, salt=2), sb.synthetic_ids(9, cfg.vocab, salt=9)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (17, 1, 33)]

    def setup(syn):
        syn.set_conv_math(math)
        syn.debug_set("h2p", 2)

    def scenario(r):
        r.run("41", [a41])
        r.run("9", [a9])
        r.run("41 again (memo)", [a41])
        r.syn.debug_set("pcm_direct", 0)
        r.run("9 (download)", [a9])
        r.run("batch", ids)
        r.stream("stream 7", a41, 7)
        r.run("41 (taps)", [a41], taps=True)
    _check_case(blob, scenario, f"pre-split {math}", setup=setup)


def test_pre_split_full_size_does_not_read_stale_memory():
    """Full-size HiFi-GAN at 128 phonemes, where the pre-split path engages by itself; then a much shorter and a longer request."""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    a128, a8 = sb.synthetic_ids(128, cfg.vocab), sb.synthetic_ids(8, cfg.vocab, salt=3)
    a200 = sb.synthetic_ids(200, cfg.vocab, salt=1)

    def scenario(r):
        r.run("128", [a128])
        r.run("128 again (memo)", [a128])
        r.run("8", [a8])
        r.run("200", [a200])
    _check_case(blob, scenario, "full-size hifigan_sdp")


def _scaled_conv_pre_blob():
    """test_parity_gpu.py's model whose decoder activations leave fp16's range (conv_pre weights x 3e6)."""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    w = sb._W(5, cfg.stats)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._gen_hdr(w, cfg)
    start = w.n + 6
    assert tuple(blob[w.n:w.n + 3].astype(int)) == (cfg.up_init, cfg.inter, 7)
    big = blob.copy()
    big[start:start + cfg.up_init * 7 * cfg.inter] *= np.float32(3.0e6)
    return cfg, big


def test_split_bf16_repeat_under_poison_counts_as_on_a_fresh_engine():
    """A real overflow: the call is repeated in the split-bf16 form (the repeat lays out and fills the arenas again), twice in a row pins the
    engine, re-arming and streaming repeats again -- the counts are exactly those of the unpoisoned engine, and so are the samples."""
    cfg, big = _scaled_conv_pre_blob()
    ids = sb.synthetic_ids(20, cfg.vocab)

    def scenario(r):
        r.run("forced", [ids], forced=[3] * len(ids))
        r.run("again", [ids])
        r.run("pinned", [ids], forced=[3] * len(ids))
        r.syn.set_conv_math("f16x2")
        r.syn.set_forced_durations([3] * len(ids))
        r.stream("stream 16", ids, 16)
    want = _check_case(big, scenario, "scaled conv_pre", fallbacks_as_fresh=True)
    assert [w["profile"]["conv_math_fallbacks"] for w in want] == [1, 2, 2, 3]


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mixed_history_on_one_engine_equals_fresh_engines():
    """No poison: one f16x2 engine on the full-size HiFi-GAN model (pre-split path engaged) through a mixed sequence, every call equal bit for
    bit to the same call on an engine that served nothing before.  Here the memory holds the previous call, not a pattern: a short call leaves
    its stage-input planes low in the stage buffers, a ~13x longer one then lays its upsampler rows -- bucket tail included -- over them."""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    a128, a97, a8 = sb.synthetic_ids(128, cfg.vocab), sb.synthetic_ids(97, cfg.vocab, salt=4), sb.synthetic_ids(8, cfg.vocab, salt=3)
    batch = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (40, 1, 77, 12)]

    def fresh(call, setup=None):
        syn = engine.Synthesizer(blob)
        syn.set_profiling(True)
        if setup:
            setup(syn)
        rec = Rec(syn, False)
        call(rec)
        syn.close()
        return rec.out[-1]

    # a 200-phoneme request whose frame count is not a multiple of 64
    for salt in range(8):
        a200 = sb.synthetic_ids(200, cfg.vocab, salt=salt)
        w200 = fresh(lambda r: r.run("200", [a200]))
        if w200["profile"]["frames"] % 64:
            break
    assert w200["profile"]["frames"] % 64, "no 200-phoneme request with a partial bucket"

    loud = lambda syn: syn.set_loudness(2, -18.0, -1.0)            # noqa: E731
    rate = lambda syn: syn.set_output_rate(44100)                  # noqa: E731
    steps = [
        ("128", lambda r: r.run("128", [a128]), None),
        ("97", lambda r: r.run("97", [a97]), None),
        ("128 again (memo)", lambda r: r.run("128 again (memo)", [a128]), None),
        ("8", lambda r: r.run("8", [a8]), None),
        ("200", lambda r: r.run("200", [a200]), None),
        ("ragged batch", lambda r: r.run("ragged batch", batch), None),
        ("stream 64", lambda r: r.stream("stream 64", a97, 64), None),
        ("44.1 kHz", lambda r: r.run("44.1 kHz", [a128]), rate),
        ("loudness 2", lambda r: r.run("loudness 2", [a97]), loud),
        ("native", lambda r: r.run("native", [a128]), None),
    ]
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_conv_math("f16x2")
    rec = Rec(syn, False)
    for what, call, setup in steps:
        if what == "loudness 2":
            syn.set_output_rate(0)
        if what == "native":
            syn.set_loudness(0)
        if setup:
            setup(syn)
        call(rec)
        want = w200 if what == "200" else fresh(call, setup)
        _compare([rec.out[-1]], [want], "history")
    assert rec.out[4]["profile"]["frames"] >= 10 * rec.out[3]["profile"]["frames"] > 0      # (the order of the ADVICE: short, then ~13x longer)
    assert rec.out[2]["profile"]["launch_ahead"] == 1
    assert syn.profile()["conv_math_fallbacks"] == 0 and syn.profile()["conv_math_pinned"] == 0
    syn.close()
