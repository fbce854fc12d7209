"""Output sample-rate conversion on the MI355X (sts_set_output_rate / sts_pool_set_output_rate / sts_multi_set_output_rate): native-rate
identity, the resampled wave and PCM against the float64 checker of tests/resample_ref.py, batches, streaming, the launch-ahead memo,
sampling noise, the split-bf16 repeat, pool and multi-device."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as rr
from conftest import golden_files, golden_files_v2, load_golden, load_golden_v2
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

RATES = [8000, 22050, 24000, 44100, 48000]
STS_EINVAL, STS_ESTATE = -1, -4


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    """torch's HIP runtime (and the RCCL it ships) initialised before any engine of this process, as in the rest of the suite: the
    device-copy and RCCL-gather tests below use them."""
    import torch
    torch.cuda.init()


def _kinds():
    """one tiny golden fixture per model kind"""
    seen, out = set(), []
    for path in golden_files():
        g, cfg, blob = load_golden(path)
        if g["kind"].item() not in seen:
            seen.add(g["kind"].item())
            out.append((g, cfg, blob))
    assert len(out) >= 5
    return out


def _check_against_checker(syn, ids, sid, rate, what):
    pcm = syn.infer_ids(ids, sid, 1.0)
    wave = syn.tap("wave")[0]
    assert pcm.size == rr.out_len(wave.size, rate), what
    want = rr.resample(wave, rate)
    got = syn.tap("wave_out")[0]
    assert got.size == pcm.size, what
    assert np.abs(got - want).max() <= 1e-5, (what, float(np.abs(got - want).max()))
    d = np.abs(pcm.astype(np.int64) - rr.pcm_cast(want).astype(np.int64))
    assert d.max() <= 1, (what, int(d.max()))
    assert np.array_equal(pcm, rr.pcm_cast(got)), what          # the PCM is the cast of the resampled float, sample for sample


def test_native_rate_is_bit_identical_for_every_golden_model():
    for g, cfg, blob in _kinds():
        ids, sid = g["ids"], int(g["sid"])
        a, b = engine.Synthesizer(blob), engine.Synthesizer(blob)
        for s in (a, b):
            s.set_record_taps(True)
        pa = a.infer_ids(ids, sid); da = a.durations(len(ids)); wa = a.tap("wave")
        for rate in (16000, 0):
            b.set_output_rate(rate)
            assert b.output_rate() == 16000
            pb = b.infer_ids(ids, sid)
            assert np.array_equal(pa, pb) and np.array_equal(da, b.durations(len(ids))) and np.array_equal(wa, b.tap("wave")), g["kind"]
            with pytest.raises(engine.StsError):
                b.tap("wave_out")
        b.set_output_rate(48000)
        assert b.output_rate() == 48000 and b.infer_ids(ids, sid).size == 3 * pa.size
        b.set_output_rate(16000)
        assert np.array_equal(pa, b.infer_ids(ids, sid)) and np.array_equal(wa, b.tap("wave"))
        a.set_record_taps(False); b.set_record_taps(False)          # (no taps: the one-utterance PCM is written straight to the host)
        pb = b.infer_ids(ids, sid)
        assert np.array_equal(a.infer_ids(ids, sid), pb)
        b.set_forced_durations(g["durations"])                      # (the fixture's own durations and length scale: the reference PCM)
        pb = b.infer_ids(ids, sid, float(g["length_scale"]))
        assert pb.size == g["pcm"].size and np.abs(pb.astype(np.int64) - g["pcm"].astype(np.int64)).max() <= 1, g["kind"]
        a.close(); b.close()


def test_resampled_output_against_the_float64_checker():
    for g, cfg, blob in _kinds():
        syn = engine.Synthesizer(blob)
        syn.set_record_taps(True)
        for rate in RATES:
            syn.set_output_rate(rate)
            _check_against_checker(syn, g["ids"], int(g["sid"]), rate, (g["kind"].item(), rate))
        syn.close()


@pytest.mark.parametrize("math", ["bf16x3", "f32", "f16x2"])
def test_resampled_output_under_every_conv_math(math):
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    syn = engine.Synthesizer(blob)
    syn.set_conv_math(math)
    syn.set_record_taps(True)
    syn.set_output_rate(44100)
    _check_against_checker(syn, sb.synthetic_ids(24, cfg.vocab), 0, 44100, math)
    syn.close()


@pytest.mark.parametrize("path", golden_files_v2("real_tiny_"), ids=lambda p: p.split("/")[-1])
def test_end_to_end_against_the_reference_wave(path):
    g, cfg, blob, utts, stride = load_golden_v2(path)
    assert stride == 1
    syn = engine.Synthesizer(blob)
    for u, ids, sid, ls, dur, pcm_ref, wave_ref in utts:
        for rate in (8000, 44100, 48000):
            syn.set_output_rate(rate)
            syn.set_forced_durations(dur)
            pcm = syn.infer_ids(ids, sid, ls)
            want = rr.pcm_cast(rr.resample(wave_ref, rate))
            assert pcm.size == want.size
            assert np.abs(pcm.astype(np.int64) - want.astype(np.int64)).max() <= 1, (path, rate)
    syn.close()


def test_batches_counts_offsets_and_pcm_direct():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    lens = [13, 1, 29, 7]
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    forced = [np.full(n, 2, np.int32) for n in lens]
    forced[1][:] = 0                      # an all-zero forced duration: the utterance still has one frame
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    for rate in (8000, 44100):
        syn.set_output_rate(rate)
        single = []
        for b in range(len(ids)):
            syn.set_forced_durations(forced[b])
            single.append(syn.infer_ids(ids[b]))
        assert single[1].size == rr.out_len(hop, rate)
        syn.set_forced_durations(np.concatenate(forced))
        batch = syn.infer_batch(ids)
        for b in range(len(ids)):
            assert np.array_equal(batch[b], single[b]), (rate, b)
        # run_batch: counts, host copy, zero-copy view, device copy
        syn.set_forced_durations(np.concatenate(forced))
        n_out = syn.run_batch(ids)
        assert list(n_out) == [s.size for s in single]
        flat = np.concatenate(single)
        assert np.array_equal(syn.pcm_host(), flat) and np.array_equal(syn.pcm_host(copy=False), flat)
        import torch
        dst = torch.zeros(flat.size + 8, dtype=torch.int16, device="cuda")
        syn.pcm_to_device_ptr(dst.data_ptr(), dst.numel())
        assert np.array_equal(dst.cpu().numpy()[:flat.size], flat)
        # PCM written straight into the pinned host buffer by the resampler, or downloaded behind it
        for direct in (0, 1):
            syn.debug_set("pcm_direct", direct)
            syn.set_forced_durations(forced[2])
            syn.run_batch([ids[2]])
            assert np.array_equal(syn.pcm_host(), single[2]), (rate, direct)
    syn.close()


@pytest.mark.parametrize("rate", [8000, 44100])
def test_stream_chunks_concatenate_to_the_one_pass_pcm(rate):
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids = sb.synthetic_ids(40, cfg.vocab)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    native_halo = syn.stream_halo_frames()
    syn.set_output_rate(rate)
    assert syn.stream_halo_frames() >= native_halo
    one = syn.infer_ids(ids)
    F = int(syn.durations(len(ids)).sum())
    hop = syn.info.samples_per_frame
    assert one.size == rr.out_len(F * hop, rate)
    for chunk in (1, 7, 64):
        offs = []
        chunks, _ = syn.infer_ids_stream(ids, chunk, on_chunk=lambda pcm, off, t: offs.append((off, pcm.size)) and False)
        assert np.array_equal(np.concatenate(chunks), one), chunk
        pos = 0
        for i, (off, n) in enumerate(offs):
            assert off == pos, (chunk, i)
            f0 = i * chunk
            assert off == rr.out_len(f0 * hop, rate)
            pos += n
        assert pos == one.size
    syn.close()


def test_launch_ahead_memo_follows_the_current_rate():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids = sb.synthetic_ids(21, cfg.vocab)
    ref = engine.Synthesizer(blob)
    ref.debug_set("launch_ahead", 0)
    want = {}
    for rate in (16000, 48000, 8000):
        ref.set_output_rate(rate)
        want[rate] = ref.infer_ids(ids)
    ref.close()
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    aheads = 0
    for it in range(9):
        rate = (16000, 48000, 8000)[it % 3]
        syn.set_output_rate(rate)
        got = syn.infer_ids(ids)
        assert got.size == want[rate].size and np.array_equal(got, want[rate]), (it, rate)
        aheads += syn.profile()["launch_ahead"]
    assert aheads >= 6 and syn.profile()["launch_ahead_misses"] == 0
    syn.close()


def test_sampled_call_equals_the_checker_on_its_own_wave():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    syn = engine.Synthesizer(blob)
    syn.set_noise(0.667, 0.8, 12)
    syn.set_record_taps(True)
    syn.set_output_rate(24000)
    _check_against_checker(syn, sb.synthetic_ids(19, cfg.vocab), 0, 24000, "sampled")
    syn.set_record_taps(False)
    a = syn.infer_ids(sb.synthetic_ids(19, cfg.vocab))
    assert np.array_equal(a, syn.infer_ids(sb.synthetic_ids(19, cfg.vocab)))
    syn.close()


def test_split_bf16_repeat_includes_the_resampler():
    """A call whose decoder activations leave fp16's range (conv_pre scaled up, as in test_parity_gpu.py) is repeated whole in the
    split-bf16 form, resampler included: at 48 kHz its PCM equals the same call pinned to split-bf16."""
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
    syn.set_output_rate(48000)
    syn.set_conv_math("bf16x3")
    want = syn.infer_ids(ids)
    syn.set_conv_math("f16x2")
    got = syn.infer_ids(ids)
    assert syn.profile()["conv_math_fallbacks"] == 1
    assert np.array_equal(got, want)
    syn.close()


def test_loud_fixture_at_48k_is_the_same_under_f16x2_and_bf16x3():
    path = golden_files_v2("loud_hifigan")[0]
    g, cfg, blob, utts, stride = load_golden_v2(path)
    u, ids, sid, ls, dur, pcm_ref, wave_ref = utts[0]
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(48000)
    out = {}
    for math in ("bf16x3", "f16x2"):
        syn.set_conv_math(math)
        syn.set_forced_durations(dur)
        out[math] = syn.infer_ids(ids, sid, ls)
    assert out["f16x2"].size == rr.out_len(pcm_ref.size, 48000)
    assert np.abs(out["f16x2"].astype(np.int64) - out["bf16x3"].astype(np.int64)).max() <= 1
    syn.close()


def test_pool_and_multi_device():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 11)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (9, 33, 5, 21)]
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(22050)
    want = [syn.infer_ids(a) for a in ids]
    syn.close()
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=8)
    pool.set_output_rate(22050)
    t = [pool.submit(a) for a in ids]
    lib = engine.load_library()
    assert lib.sts_pool_set_output_rate(pool.h, 48000) == STS_ESTATE
    for i, k in enumerate(t):
        assert np.array_equal(pool.wait(k), want[i]), i
    assert lib.sts_pool_set_output_rate(pool.h, 47999) == STS_EINVAL
    pool.set_output_rate(16000)
    pool.close()
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    md.set_output_rate(22050)
    got = md.infer_batch(ids)
    for b in range(len(ids)):
        assert np.array_equal(got[b], want[b]), b
    md.close()
    md = engine.MultiDevice(blob, [0], gather="rccl")
    assert md.gather_mode() == "rccl"
    md.set_output_rate(22050)
    got = md.infer_batch(ids)
    for b in range(len(ids)):
        assert got[b].size == want[b].size
        assert np.abs(got[b].astype(np.int64) - want[b].astype(np.int64)).max() <= 1, b     # (a packed batch may pick other tiles)
    md.close()


def test_invalid_rates_leave_the_setting_unchanged():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(24000)
    for bad in (7999, 48001, 47999, -8000):
        assert syn.lib.sts_set_output_rate(syn.h, bad) == STS_EINVAL
        assert syn.output_rate() == 24000
    with pytest.raises(engine.StsError):
        syn.set_output_rate(100000)
    assert syn.output_rate() == 24000
    syn.close()
