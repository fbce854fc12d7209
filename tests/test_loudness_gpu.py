"""Loudness measurement and normalisation on the MI355X (sts_set_loudness, sts_loudness_measure, sts_pool_set_loudness,
sts_multi_set_loudness) against the float64 checker of tests/loudness_ref.py: caller signals, every decoder type at the native and at
resampled rates, the ceiling on the wrap-around fixtures, batches, the launch-ahead and split-bf16 repeats, pool, multi-device, and the
refusal of streaming while the mode is on."""
import numpy as np
import pytest

import loudness_ref as lr
from conftest import golden_files_v2, load_golden_v2
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL, STS_ESTATE = -1, -4
CEIL_PCM = int(np.floor(32737 * 10 ** (-1 / 20))) + 1


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _close(got, want, what, lu=0.01):
    """one sts_loudness entry against the checker's dict"""
    if np.isfinite(want["lufs"]):
        assert abs(float(got["lufs"]) - want["lufs"]) <= lu, (what, float(got["lufs"]), want["lufs"])
    else:
        assert got["lufs"] == -np.inf and got["blocks"] == 0, (what, float(got["lufs"]))
    assert float(got["peak"]) == want["peak"], (what, float(got["peak"]), want["peak"])
    assert abs(float(got["gain"]) / float(want["gain"]) - 1.0) <= 1e-4, (what, float(got["gain"]), float(want["gain"]))


# ---- the utility on caller signals --------------------------------------------------------------------------------------------------
def test_measure_sine_and_noise_batches():
    fs = 48000
    sine = np.sin(2 * np.pi * 997.0 * np.arange(5 * fs) / fs).astype(np.float32)
    r = engine.loudness_measure([sine], fs)[0]
    assert abs(float(r["lufs"]) - (-3.01)) <= 0.01 and float(r["peak"]) == lr.peak(sine)
    rng = np.random.default_rng(7)
    for fs, lens in ((16000, [0, 1, 4 * 1600 - 1, 4 * 1600, 4 * 1600 + 1, 7 * 16000]), (48000, [4 * 4800 + 1, 60 * 48000, 0])):
        sig = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in lens]
        got = engine.loudness_measure(sig, fs, -16.0, -1.0)
        assert got.size == len(lens)
        for b, x in enumerate(sig):
            want = lr.loudness(x, fs, -16.0, -1.0)
            _close(got[b], want, (fs, lens[b]))
            assert got[b]["blocks"] == want["blocks"], (fs, lens[b])


def test_steps_and_impulses_on_chunk_tile_and_subblock_edges():
    """the carry across lanes (32 samples), waves, workgroups (8192 samples) and 100 ms sub-blocks: a loud event, then a quiet sine that
    only measures right if the filter state crossed the edge intact"""
    rng = np.random.default_rng(3)
    for fs in (16000, 22050, 48000):
        S = lr.sub_block(fs)
        sig = []
        for edge in (32, 64 * 32, 8192, 2 * 8192, S, 7 * S, 3 * 8192 + 32):
            n = max(edge + 3 * fs, 5 * S)
            t = np.arange(n)
            x = (1e-3 * np.sin(2 * np.pi * 50.0 * t / fs)).astype(np.float32)
            x[edge:] += np.float32(0.8)                               # a step
            x[edge - 1] += np.float32(0.9)                            # an impulse just before it
            sig.append(x)
            sig.append((0.2 * rng.standard_normal(n)).astype(np.float32) * (t >= edge))
        got = engine.loudness_measure(sig, fs, -23.0, -2.0)
        for b, x in enumerate(sig):
            _close(got[b], lr.loudness(x, fs, -23.0, -2.0), (fs, b))


def test_results_are_bitwise_a_function_of_the_utterance_alone():
    rng = np.random.default_rng(11)
    fs = 24000
    sig = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((50000, 0.3), (8191, 1.0), (123457, 0.01), (3 * fs, 0.5))]
    a = engine.loudness_measure(sig, fs)
    b = engine.loudness_measure(sig, fs)
    assert a.tobytes() == b.tobytes()
    for i, x in enumerate(sig):
        assert engine.loudness_measure([x], fs).tobytes() == a[i:i + 1].tobytes(), i
    assert engine.loudness_measure(sig[::-1], fs)[::-1].tobytes() == a.tobytes()


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
_FINITE = []
FIXTURES = ["full_hifigan_sdp_T128", "real_hifigan_sdp_T96", "real_istft_fix_T96", "real_mbb_fix_T96", "real_ms_hifigan_sdp_T64",
            "loud_hifigan_sdp_T128", "loud_mbb_fix_T96", "full_ms_sdp_T96"]


def _fixture(name):
    g, cfg, blob, utts, stride = load_golden_v2(golden_files_v2(name)[0])
    u, ids, sid, ls, dur, pcm, wave = utts[0]
    return blob, ids, sid, ls, dur


def _signal(syn, rate):
    return syn.tap("wave" if rate in (0, 16000) else "wave_out")[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_measure_mode_leaves_the_pcm_alone_and_matches_the_checker(name):
    blob, ids, sid, ls, dur = _fixture(name)
    syn = engine.Synthesizer(blob)
    for rate in (16000, 8000, 22050, 48000):
        syn.set_output_rate(rate)
        fs = 16000 if rate == 16000 else rate
        syn.set_loudness(engine.LOUD_OFF)
        syn.set_forced_durations(dur)
        p0 = syn.infer_ids(ids, sid, ls)
        assert syn.loudness().size == 0
        syn.set_loudness(engine.LOUD_MEASURE, -16.0, -1.0)
        syn.set_forced_durations(dur)
        p1 = syn.infer_ids(ids, sid, ls)
        assert np.array_equal(p0, p1), (name, rate)
        r1 = syn.loudness()
        syn.set_record_taps(True)
        syn.set_forced_durations(dur)
        assert np.array_equal(syn.infer_ids(ids, sid, ls), p0), (name, rate)
        x = _signal(syn, rate)
        syn.set_record_taps(False)
        assert x.size == p0.size and r1.size == 1
        assert syn.loudness().tobytes() == r1.tobytes(), (name, rate)
        _close(r1[0], lr.loudness(x, fs, -16.0, -1.0), (name, rate))
        _FINITE.append(bool(np.isfinite(r1[0]["lufs"])))
    syn.close()


def test_at_least_one_fixture_was_measured():
    assert len(_FINITE) == 4 * len(FIXTURES) and any(_FINITE)


@pytest.mark.parametrize("name", ["real_hifigan_sdp_T96", "real_mbb_fix_T96", "real_istft_fix_T96", "loud_hifigan_sdp_T128", "full_ms_sdp_T96"])
def test_normalize_mode_is_the_cast_of_the_scaled_wave(name):
    blob, ids, sid, ls, dur = _fixture(name)
    syn = engine.Synthesizer(blob)
    for rate, target in ((16000, -16.0), (48000, -23.0), (22050, -30.0)):
        syn.set_output_rate(rate)
        fs = rate
        syn.set_loudness(engine.LOUD_NORMALIZE, target, -1.0)
        syn.set_record_taps(True)
        syn.set_forced_durations(dur)
        pcm = syn.infer_ids(ids, sid, ls)
        x = _signal(syn, rate)
        r = syn.loudness()[0]
        want = lr.loudness(x, fs, target, -1.0)
        _close(r, want, (name, rate))
        assert np.array_equal(pcm, lr.normalize(x, r["gain"])), (name, rate)
        if np.isfinite(want["lufs"]) and want["gain"] < 10 ** (-1 / 20) / want["peak"] * (1 - 1e-3):
            assert abs(lr.measure(pcm.astype(np.float64) / 32737.0, fs)[0] - target) <= 0.05, (name, rate)
        # the same call without taps (PCM written straight to the host), then again from the launch-ahead memo
        syn.set_record_taps(False)
        for _ in range(2):
            syn.set_forced_durations(dur)
            assert np.array_equal(syn.infer_ids(ids, sid, ls), pcm), (name, rate)
            assert syn.loudness()[0].tobytes() == r.tobytes(), (name, rate)
        assert np.array_equal(syn.infer_ids(ids, sid, ls), syn.infer_ids(ids, sid, ls))
        assert syn.profile()["launch_ahead"] == 1
    syn.close()


@pytest.mark.parametrize("path", golden_files_v2("amp_"), ids=lambda p: p.split("/")[-1])
def test_ceiling_removes_the_wrap_around(path):
    g, cfg, blob, utts, stride = load_golden_v2(path)
    u, ids, sid, ls, dur, pcm_ref, wave_ref = utts[0]
    syn = engine.Synthesizer(blob)
    syn.set_record_taps(True)
    syn.set_forced_durations(dur)
    p0 = syn.infer_ids(ids, sid, ls)
    w0 = syn.tap("wave")[0]
    if "_wrap" in path:      # the reference's cast really wraps here: PCM of the opposite sign where the wave is beyond full scale
        big = np.abs(w0) > 1.01
        assert big.any() and (np.sign(p0[big]) == -np.sign(w0[big])).any()
    syn.set_loudness(engine.LOUD_NORMALIZE, -10.0, -1.0)
    syn.set_forced_durations(dur)
    p2 = syn.infer_ids(ids, sid, ls)
    w2 = syn.tap("wave")[0]
    assert np.array_equal(w0, w2)
    nz = p2 != 0
    assert not (np.sign(p2[nz]) == -np.sign(w2[nz])).any()
    assert np.abs(p2.astype(np.int64)).max() <= CEIL_PCM
    assert np.array_equal(p2, lr.normalize(w2, syn.loudness()[0]["gain"]))
    syn.close()


@pytest.mark.parametrize("path", golden_files_v2("full_batch8_"), ids=lambda p: p.split("/")[-1])
def test_batches_report_every_utterance_in_call_order(path):
    g, cfg, blob, utts, stride = load_golden_v2(path)
    ids = [a[1] for a in utts]; sid = [a[2] for a in utts]; ls = [a[3] for a in utts]; dur = [a[4].astype(np.int32) for a in utts]
    syn = engine.Synthesizer(blob)
    syn.set_loudness(engine.LOUD_NORMALIZE, -18.0, -1.0)
    single, res = [], []
    for b in range(len(ids)):
        syn.set_forced_durations(dur[b])
        single.append(syn.infer_ids(ids[b], sid[b], ls[b]))
        res.append(syn.loudness()[0])
    syn.set_forced_durations(np.concatenate(dur))
    batch = syn.infer_batch(ids, sid, ls)
    rb = syn.loudness()
    assert rb.size == len(ids)
    for b in range(len(ids)):
        if np.isfinite(res[b]["lufs"]):
            assert abs(float(rb[b]["lufs"]) - float(res[b]["lufs"])) <= 1e-3, b
        assert np.abs(batch[b].astype(np.int64) - single[b].astype(np.int64)).max() <= 1, b
    syn.set_forced_durations(np.concatenate(dur))
    n_out = syn.run_batch(ids, sid, ls)
    assert syn.loudness().tobytes() == rb.tobytes()
    assert np.array_equal(syn.pcm_host(), np.concatenate(batch)) and list(n_out) == [p.size for p in batch]
    # a member too short to measure (all-zero forced durations: one frame), beside the others
    k = len(ids) - 1
    short = [d.copy() for d in dur]
    short[k][:] = 0
    syn.set_record_taps(True)
    syn.set_forced_durations(np.concatenate(short))
    out = syn.infer_batch(ids, sid, ls)
    r = syn.loudness()
    x = syn.tap("wave")[0]
    off = sum(p.size for p in out[:k])
    xs = x[off:off + out[k].size]
    want = lr.loudness(xs, 16000, -18.0, -1.0)
    assert r[k]["lufs"] == -np.inf and r[k]["blocks"] == 0
    _close(r[k], want, "short member")
    assert np.array_equal(out[k], lr.normalize(xs, r[k]["gain"]))
    for b in range(k):
        if np.isfinite(rb[b]["lufs"]):
            assert abs(float(r[b]["lufs"]) - float(rb[b]["lufs"])) <= 1e-3, b
    syn.close()


def test_split_bf16_repeat_gives_the_same_results():
    """conv_pre scaled up (as test_parity_gpu.py does): the f16x2 call is repeated in split-bf16, loudness kernels included"""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = sb.synthetic_ids(20, cfg.vocab)
    w = sb._W(5, cfg.stats)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._gen_hdr(w, cfg)
    assert tuple(blob[w.n:w.n + 3].astype(int)) == (cfg.up_init, cfg.inter, 7)
    start = w.n + 6
    big = blob.copy()
    big[start:start + cfg.up_init * 7 * cfg.inter] *= np.float32(3.0e6)
    syn = engine.Synthesizer(big)
    syn.set_profiling(True)
    syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -1.0)
    for rate in (16000, 44100):
        syn.set_output_rate(rate)
        syn.set_conv_math("bf16x3")
        want = syn.infer_ids(ids); rw = syn.loudness()
        before = syn.profile()["conv_math_fallbacks"]
        syn.set_conv_math("f16x2")
        got = syn.infer_ids(ids); rg = syn.loudness()
        assert syn.profile()["conv_math_fallbacks"] == before + 1
        assert np.array_equal(got, want) and rg.tobytes() == rw.tobytes(), rate
    syn.close()


def test_pool_and_multi_device():
    cfg = sb.tiny_cfg("mbb_fix")
    blob = sb.make_blob(cfg, 11)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (40, 33, 5, 61)]
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(24000)
    syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -2.0)
    want = [syn.infer_ids(a) for a in ids]
    syn.close()
    lib = engine.load_library()
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=8)
    pool.set_output_rate(24000)
    assert lib.sts_pool_set_loudness(pool.h, 1, -20.0, -2.0) == STS_EINVAL
    pool.set_loudness(engine.LOUD_NORMALIZE, -20.0, -2.0)
    t = [pool.submit(a) for a in ids]
    assert lib.sts_pool_set_loudness(pool.h, 0, -20.0, -2.0) == STS_ESTATE
    for i, k in enumerate(t):
        got = pool.wait(k)
        assert got.size == want[i].size and np.abs(got.astype(np.int64) - want[i].astype(np.int64)).max() <= 1, i
    pool.close()
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    md.set_output_rate(24000)
    with pytest.raises(engine.StsError):
        md.set_loudness(engine.LOUD_MEASURE)
    md.set_loudness(engine.LOUD_NORMALIZE, -20.0, -2.0)
    got = md.infer_batch(ids)
    for b in range(len(ids)):
        assert got[b].size == want[b].size and np.abs(got[b].astype(np.int64) - want[b].astype(np.int64)).max() <= 1, b
    md.set_loudness(engine.LOUD_OFF, -20.0, -2.0)
    md.close()


def test_streaming_is_refused_while_the_mode_is_on():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids = sb.synthetic_ids(17, cfg.vocab)
    syn = engine.Synthesizer(blob)
    plain, _ = syn.infer_ids_stream(ids, 8)
    for mode in (engine.LOUD_MEASURE, engine.LOUD_NORMALIZE):
        syn.set_loudness(mode)
        with pytest.raises(engine.StsError, match="loudness"):
            syn.infer_ids_stream(ids, 8)
        with pytest.raises(engine.StsError, match="loudness"):
            syn.infer_batch_stream([ids, ids], 8)
        assert syn.loudness().size == 0
        syn.infer_ids(ids)                                   # the engine stays usable
        assert syn.loudness().size == 1
    syn.set_loudness(engine.LOUD_OFF)
    again, _ = syn.infer_ids_stream(ids, 8)
    assert np.array_equal(np.concatenate(again), np.concatenate(plain))
    syn.close()
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=4)
    pool.set_loudness(engine.LOUD_NORMALIZE)
    with pytest.raises(engine.StsError):
        pool.submit_stream(ids, 8, lambda pcm, off: False)
    pool.set_loudness(engine.LOUD_OFF)
    chunks = []
    t = pool.submit_stream(ids, 8, lambda pcm, off: chunks.append(pcm.copy()) and False)
    assert pool.wait(t) == sum(c.size for c in chunks) and np.array_equal(np.concatenate(chunks), np.concatenate(plain))
    pool.close()


def test_invalid_arguments_leave_the_setting_unchanged():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    syn = engine.Synthesizer(blob)
    assert syn.loudness_mode() == (0, -16.0, -1.0)
    syn.set_loudness(engine.LOUD_NORMALIZE, -23.0, -2.0)
    lib = engine.load_library()
    for mode, t, p in ((3, -16.0, -1.0), (-1, -16.0, -1.0), (2, float("nan"), -1.0), (2, -16.0, float("nan")), (2, 0.5, -1.0),
                       (2, -70.5, -1.0), (2, -16.0, 0.1), (2, -16.0, -30.5), (1, float("inf"), -1.0)):
        assert lib.sts_set_loudness(syn.h, mode, t, p) == STS_EINVAL, (mode, t, p)
        assert syn.loudness_mode() == (2, -23.0, -2.0)
    assert lib.sts_loudness_measure(0, None, None, 0, 16000, -16.0, -1.0, None) == STS_EINVAL
    with pytest.raises(engine.StsError):
        engine.loudness_measure([np.zeros(10, np.float32)], 7000)
    with pytest.raises(engine.StsError):
        engine.loudness_measure([np.zeros(10, np.float32)], 16000, 1.0)
    pcm = syn.infer_ids(sb.synthetic_ids(9, cfg.vocab))
    n = lib.sts_get_loudness(syn.h, None, 0)
    assert n == 1
    out = np.zeros(1, engine.LOUDNESS_DTYPE)
    assert lib.sts_get_loudness(syn.h, out.ctypes.data, 0) == STS_EINVAL
    assert pcm.size > 0
    syn.close()
