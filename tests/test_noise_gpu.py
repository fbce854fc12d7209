"""Sampling noise on the MI355X (sts_set_noise / sts_pool_submit_ex / sts_multi_set_noise): the prior and SDP latents against the
float64 checker of tests/noise_ref.py, zero-noise identity, seeds, batching / pooling / sharding / streaming invariance, the
launch-ahead memo."""
import dataclasses

import numpy as np
import pytest

import noise_ref as nr
from conftest import TAP_MAXABS_TOL, golden_files, load_golden
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

NS, NSW = 0.667, 0.8
SDP_KINDS = ["hifigan_sdp", "ms_hifigan_sdp", "ms_sdp"]


def _tiny(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    return cfg, sb.make_blob(cfg, seed)


def _run(syn, ids, sid=0, ls=1.0):
    pcm = syn.infer_ids(ids, sid, ls)
    return pcm, syn.durations(len(ids))


def test_zero_noise_is_bit_identical_for_every_golden_model():
    seen = set()
    for path in golden_files():
        g, cfg, blob = load_golden(path)[:3]
        if g["kind"].item() in seen:
            continue
        seen.add(g["kind"].item())
        ids, sid = g["ids"], int(g["sid"])
        a, b = engine.Synthesizer(blob), engine.Synthesizer(blob)
        b.set_noise(0.0, 0.0, 987654321)
        assert b.noise() == (0.0, 0.0, 987654321)
        pa, da = _run(a, ids, sid)
        pb, db = _run(b, ids, sid)
        assert np.array_equal(pa, pb) and np.array_equal(da, db), path
        a.set_record_taps(True); b.set_record_taps(True)
        pa, _ = _run(a, ids, sid); pb, _ = _run(b, ids, sid)
        assert np.array_equal(pa, pb), path
        for k in ("m", "logw", "z_p", "z"):
            assert np.array_equal(a.tap(k), b.tap(k)), (path, k)
        a.close(); b.close()
    assert len(seen) >= 5


@pytest.mark.parametrize("math", ["bf16x3", "f32", "f16x2"])
@pytest.mark.parametrize("fused", [1, 0])
def test_prior_sample_matches_the_reference_expression(math, fused):
    cfg = sb.full_cfg("hifigan_sdp") if fused else sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids = sb.synthetic_ids(48, cfg.vocab)
    syn = engine.Synthesizer(blob)
    syn.set_conv_math(math)
    syn.debug_set("flow_fused", fused)
    syn.set_record_taps(True)
    seed = 0xDEADBEEF12345
    syn.set_noise(NS, 0.0, seed)
    syn.infer_ids(ids)
    m, logs, zp, dur = syn.tap("m"), syn.tap("logs"), syn.tap("z_p"), syn.durations(len(ids))
    want, eps = nr.prior(m, logs, dur, NS, seed)
    scale = np.abs(logs[:, np.repeat(np.arange(len(ids)), dur)].astype(np.float64)) * NS    # |logs_expand * ns|
    err = np.abs(zp - want)
    assert (err <= 1e-5 * np.maximum(scale, 1.0)).all(), float(err.max())
    assert np.abs(eps).max() > 1.0          # (real noise, not zeros)
    syn.close()


@pytest.mark.parametrize("kind,full", [("hifigan_sdp", False), ("ms_hifigan_sdp", False), ("ms_sdp", False), ("hifigan_fix", False),
                                       ("ms_hifigan_fix", False), ("hifigan_sdp", True), ("ms_hifigan_sdp", True)])
def test_logs_projection_matches_the_oracle(kind, full):
    """The prior's scale `logs` (the second half of the encoder projection, packed as a conv of its own) against the C oracle's own
    `logs` tap: it is what the noise_scale path multiplies eps by, so it must be the reference's tensor, not the engine's reading of it."""
    cfg = sb.full_cfg(kind) if full else sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 1234)
    T, sid = (9 if full else 17), (2 if cfg.is_ms else 0)
    ids = sb.synthetic_ids(T, cfg.vocab, salt=5)
    o = pyref.PortModel(blob).infer_ids(ids, sid, 1.0, forced_dur=[1] * T, taps=True)
    syn = engine.Synthesizer(blob)
    syn.set_record_taps(True)
    for noise in ((0.0, 0.0, 0), (NS, NSW, 3)):          # the tap is the same tensor whether or not the call samples
        syn.set_noise(*noise)
        syn.infer_ids(ids, sid, 1.0)
        m, logs = syn.tap("m"), syn.tap("logs")
        assert logs.shape == o["logs"].shape == m.shape
        assert np.abs(m - o["m"]).max() <= TAP_MAXABS_TOL
        assert np.abs(logs - o["logs"]).max() <= TAP_MAXABS_TOL, np.abs(logs - o["logs"]).max()
        assert not np.allclose(logs, m)
    syn.close()


def _sdp_case(kind, full):
    cfg = sb.full_cfg(kind) if full else sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 1234)
    return cfg, blob, nr.SdpSection(blob, cfg, 1234)


@pytest.mark.parametrize("nsw", [0.8, 1.0])
@pytest.mark.parametrize("kind,full", [("hifigan_sdp", False), ("ms_hifigan_sdp", False), ("hifigan_sdp", True), ("ms_hifigan_sdp", True)])
def test_sdp_latent_against_the_float64_checker(kind, full, nsw):
    cfg, blob, sec = _sdp_case(kind, full)
    syn = engine.Synthesizer(blob)
    syn.set_record_taps(True)
    T, sid, seed = (40 if full else 17), (1 if cfg.is_ms else 0), 77
    ids = sb.synthetic_ids(T, cfg.vocab, salt=3)
    syn.set_noise(0.0, nsw, seed)
    syn.infer_ids(ids, sid, 1.0)
    x, logw, dur = syn.tap("x_enc"), syn.tap("logw")[0], syn.durations(T)
    r0, r1 = nr.sdp_latent(seed, nsw, T)
    want = nr.sdp_logw(sec, x, r0, r1, sid)
    assert np.abs(logw - want).max() <= 1e-3
    w = np.exp(want)
    clear = np.abs(w - np.round(w)) > 1e-4
    assert np.array_equal(dur[clear], nr.durations(want)[clear])
    # and the noise moved the durations away from the noise-free ones
    syn.set_noise(0.0, 0.0, seed)
    syn.infer_ids(ids, sid, 1.0)
    assert not np.array_equal(syn.tap("logw")[0], logw)
    syn.close()


def test_fix_duration_predictor_ignores_the_latent_scale():
    cfg, blob = _tiny("hifigan_fix")
    ids = sb.synthetic_ids(15, cfg.vocab)
    a, b = engine.Synthesizer(blob), engine.Synthesizer(blob)
    b.set_noise(0.0, 1.0, 5)
    assert np.array_equal(a.infer_ids(ids), b.infer_ids(ids)) and np.array_equal(a.durations(15), b.durations(15))
    a.close(); b.close()


@pytest.mark.parametrize("kind", SDP_KINDS)
def test_seeds_batches_and_repeats(kind):
    cfg, blob = _tiny(kind)
    syn = engine.Synthesizer(blob)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (11, 19, 7, 23)]
    syn.set_noise(NS, NSW, 100)
    one = syn.infer_ids(ids[0])
    assert np.array_equal(one, syn.infer_ids(ids[0]))
    syn.set_noise(NS, NSW, 101)
    other = syn.infer_ids(ids[0])
    assert not (one.size == other.size and np.array_equal(one, other))
    singles = []
    for b in range(len(ids)):
        syn.set_noise(NS, NSW, 100 + b)
        singles.append(syn.infer_ids(ids[b]))
    syn.set_noise(NS, NSW, 100)
    batch = syn.infer_batch(ids)
    for b in range(len(ids)):
        assert np.array_equal(batch[b], singles[b]), b
    syn.close()


def test_pool_packs_noisy_and_noise_free_requests():
    cfg, blob = _tiny("ms_hifigan_sdp")
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (9, 14, 20, 12, 17)]
    reqs = [(0.0, 0.0, 0), (NS, NSW, 5), (NS, 0.0, 9), (0.0, NSW, 2), (1.0, 1.0, 2 ** 63 + 3)]
    syn = engine.Synthesizer(blob)
    want = []
    for i, (ns, nsw, seed) in enumerate(reqs):
        syn.set_noise(ns, nsw, seed)
        want.append(syn.infer_ids(ids[i], i % 3))
    syn.close()
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=8)
    for _ in range(2):
        t = [pool.submit(ids[i], i % 3, 1.0, *reqs[i]) for i in range(len(ids))]
        for i, k in enumerate(t):
            assert np.array_equal(pool.wait(k), want[i]), i
    assert pool.stats()[0] < 2 * len(ids)          # (some requests shared a batch)
    with pytest.raises(engine.StsError):
        pool.submit(ids[0], 0, 1.0, -1.0, 0.0, 0)
    pool.close()


def test_multi_device_equals_the_single_engine_batch():
    cfg, blob = _tiny("hifigan_sdp")
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (9, 30, 14, 22, 5)]
    syn = engine.Synthesizer(blob)
    syn.set_noise(NS, NSW, 40)
    want = syn.infer_batch(ids)
    syn.close()
    md = engine.MultiDevice(blob, [0, 0])
    md.set_noise(NS, NSW, 40)
    got = md.infer_batch(ids)
    for b in range(len(ids)):
        assert np.array_equal(got[b], want[b]), b
    md.close()


def test_stream_chunks_concatenate_to_the_one_pass_pcm():
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids = sb.synthetic_ids(40, cfg.vocab)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_noise(NS, NSW, 11)
    one = syn.infer_ids(ids)
    for chunk in (48, 200):
        chunks, _ = syn.infer_ids_stream(ids, chunk)
        assert np.array_equal(np.concatenate(chunks), one), chunk
    syn.close()


def test_split_bf16_repeat_regenerates_the_same_noise():
    """A call whose decoder activations leave fp16's range (conv_pre scaled up, as in test_parity_gpu.py) is repeated whole in the
    split-bf16 form; the repeat must draw the same noise, so its PCM equals a split-bf16 call with the same noise settings."""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = sb.synthetic_ids(20, cfg.vocab)
    w = sb._W(5, cfg.stats)            # the decoder's input conv follows the text encoder and the generator header (synth_blob.make_blob)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._gen_hdr(w, cfg)
    assert tuple(blob[w.n:w.n + 3].astype(int)) == (cfg.up_init, cfg.inter, 7)
    start = w.n + 6
    big = blob.copy()
    big[start:start + cfg.up_init * 7 * cfg.inter] *= np.float32(3.0e6)
    syn = engine.Synthesizer(big)
    syn.set_profiling(True)
    syn.set_noise(NS, NSW, 8)
    syn.set_conv_math("bf16x3")
    want = syn.infer_ids(ids)
    want_dur = syn.durations(len(ids))
    syn.set_conv_math("f16x2")
    got = syn.infer_ids(ids)
    assert syn.profile()["conv_math_fallbacks"] == 1
    assert np.array_equal(syn.durations(len(ids)), want_dur)
    assert np.array_equal(got, want)
    syn.close()


def test_launch_ahead_memo_keeps_noisy_and_noise_free_requests_apart():
    cfg, blob = _tiny("hifigan_sdp")
    ids = sb.synthetic_ids(21, cfg.vocab)
    ref = engine.Synthesizer(blob)
    ref.debug_set("launch_ahead", 0)
    want = {}
    for key in ((0.0, 1.0, 1), (0.0, 0.0, 0), (0.0, 1.0, 2)):
        ref.set_noise(*key)
        want[key] = (ref.infer_ids(ids), ref.durations(21))
    assert not np.array_equal(want[(0.0, 1.0, 1)][1], want[(0.0, 0.0, 0)][1])
    ref.close()
    syn = engine.Synthesizer(blob)
    for rnd in range(3):            # round 0 fills the memo; later rounds launch ahead from it
        for key in ((0.0, 1.0, 1), (0.0, 0.0, 0), (0.0, 1.0, 2)):
            syn.set_noise(*key)
            pcm = syn.infer_ids(ids)
            assert np.array_equal(pcm, want[key][0]), (rnd, key)
            assert np.array_equal(syn.durations(21), want[key][1]), (rnd, key)
            if rnd:
                assert syn.profile()["launch_ahead"] == 1
    syn.close()


def test_prior_noise_statistics_on_a_long_utterance():
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids = sb.synthetic_ids(200, cfg.vocab)
    syn = engine.Synthesizer(blob)
    syn.set_record_taps(True)
    syn.set_noise(NS, 0.0, 2024)
    syn.infer_ids(ids)
    m, logs, zp, dur = syn.tap("m"), syn.tap("logs"), syn.tap("z_p"), syn.durations(200)
    idx = np.repeat(np.arange(200), dur)
    me, le = m[:, idx].astype(np.float64), logs[:, idx].astype(np.float64)
    ok = np.abs(le) > 1e-3
    e = ((zp - me) / (le * NS))[ok]
    assert e.size > 50000
    assert abs(e.mean()) < 0.02 and abs(e.std() - 1.0) < 0.02, (e.mean(), e.std())
    syn.close()


def test_noise_setter_validation():
    cfg, blob = _tiny("hifigan_sdp")
    syn = engine.Synthesizer(blob)
    syn.set_noise(0.5, 0.25, 3)
    for bad in ((-0.1, 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(engine.StsError):
            syn.set_noise(bad[0], bad[1], 9)
    assert syn.noise() == (0.5, 0.25, 3)
    syn.close()
