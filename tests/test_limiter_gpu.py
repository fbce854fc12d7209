"""The look-ahead peak limiter on the MI355X (sts_set_limiter, sts_limiter_apply, sts_pool_set_limiter, sts_multi_set_limiter) against
the numpy checker of tests/limiter_ref.py, bit for bit: caller signals of every awkward length with peaks on lane, wave, tile and
utterance edges, every decoder type at the native and at resampled rates in both regimes (limiting / untouched), identity at 0 dB / 0 dBFS,
the combination with loudness modes 1 and 2, batches, the launch-ahead and split-bf16 repeats, pool, multi-device, poisoned workspaces,
and the streaming forms (chunks concatenate to the whole-utterance PCM bit for bit under a pinned conv mode)."""
import numpy as np
import pytest

import limiter_ref as lm
import loudness_ref as lr
from conftest import golden_files_v2, load_golden_v2
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL, STS_ESTATE = -1, -4
TILE = 4096


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _check(x, rate, gain_db, ceiling, ms, y, pcm, st, what, g_loud=1.0):
    """one utterance's y / pcm / stats against the checker, every bit; returns the checker's stats"""
    H, c, G = engine.limiter_design(rate, gain_db, ceiling, ms)
    assert H == lm.design_H(rate, ms)
    g0 = lm.static_gain(G, g_loud)
    wy, ws, wS = lm.limit(x, g0, H, c)
    want = lm.stats(wy, ws, wS, g0, H)
    if y is not None:
        assert y.size == wy.size and np.array_equal(y.view(np.uint32), wy.view(np.uint32)), (what, "y")
    if pcm is not None:
        assert np.array_equal(pcm, lm.pcm_cast(wy)), (what, "pcm")
    if st is not None:
        assert np.float32(st["gain"]).tobytes() == np.float32(want["gain"]).tobytes(), (what, "gain", st, want)
        assert np.float32(st["min_gain"]).tobytes() == np.float32(want["min_gain"]).tobytes(), (what, "min_gain", st, want)
        assert np.float32(st["peak_out"]).tobytes() == np.float32(want["peak_out"]).tobytes(), (what, "peak_out", st, want)
        assert int(st["limited"]) == want["limited"], (what, "limited", st, want)
    return want, c


# ---- the utility on caller signals --------------------------------------------------------------------------------------------------
def _noise(rng, n, amp=0.2):
    return (amp * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("rate,ms", [(16000, 5.0), (8000, 0.25), (48000, 10.0), (22050, 3.3)])
def test_apply_lengths_and_planted_peaks(rate, ms):
    H = lm.design_H(rate, ms)
    rng = np.random.default_rng(rate)
    lens = [0, 1, 2 * H, 2 * H + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 517, 0, 5]
    sig = [_noise(rng, n) for n in lens]
    # peaks on lane, wave, tile (4096) and utterance edges of the long signal -- in a full tile a lane owns 16 consecutive outputs and a
    # wave 1024 (a shorter tile: ceil(n / 256) per lane) -- and an over-long run
    big = sig[7]
    for p in (0, 15, 16, 1023, 1024, TILE - 1, TILE, TILE + 1, 2 * TILE - H, 2 * TILE + H, 2 * TILE + 2 * H, big.size - 1):
        big[p] = np.float32(1.5 if p % 2 else -2.5)
    big[2 * TILE + 3 * H + 50:2 * TILE + 3 * H + 50 + 4 * H + 9] = np.float32(1.1)
    sig[5][0] = np.float32(3.0); sig[5][-1] = np.float32(-3.0)
    sig[4][-1] = np.float32(0.95)                         # within 2H of the junction with sig[5]: must not leak across it
    sig[6][:3] = np.float32(4.0)
    sig[1][0] = np.float32(2.0)
    for gain_db, ceiling in ((0.0, -1.0), (6.0, -3.0)):
        y, pcm, st = engine.limiter_apply(sig, rate, gain_db, ceiling, ms)
        lim = []
        for b, x in enumerate(sig):
            want, c = _check(x, rate, gain_db, ceiling, ms, y[b], pcm[b], st[b], (rate, ms, gain_db, lens[b]))
            lim.append(want["limited"])
            if x.size:
                assert np.abs(pcm[b].astype(np.int64)).max() <= lm.ceiling_pcm(c)
        assert lim[7] > 0 and lim[5] > 0 and lim[1] == 1
        # one by one: the neighbours of a packed batch never leak
        for b in (1, 3, 4, 5, 6):
            y1, p1, s1 = engine.limiter_apply([sig[b]], rate, gain_db, ceiling, ms)
            assert y1[0].tobytes() == y[b].tobytes() and p1[0].tobytes() == pcm[b].tobytes() and s1.tobytes() == st[b:b + 1].tobytes(), b
        # reversed order and a repeated call
        yr, pr, sr = engine.limiter_apply(sig[::-1], rate, gain_db, ceiling, ms)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(yr[::-1], y)) and all(a.tobytes() == b.tobytes() for a, b in zip(pr[::-1], pcm))
        assert sr[::-1].tobytes() == st.tobytes()
        y2, p2, s2 = engine.limiter_apply(sig, rate, gain_db, ceiling, ms)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(y2, y)) and s2.tobytes() == st.tobytes()


def test_apply_both_ends_of_every_parameter_range():
    rng = np.random.default_rng(2)
    x = _noise(rng, 2 * TILE + 99, 0.3)
    x[[0, 777, TILE, x.size - 1]] = np.float32(1.2)
    for rate, gain_db, ceiling, ms in ((8000, -40.0, -30.0, 0.25), (48000, 40.0, 0.0, 10.0), (8000, 40.0, -30.0, 10.0), (48000, -40.0, 0.0, 0.25),
                                       (16000, 0.0, 0.0, 5.0), (44100, 12.0, -0.1, 1.0)):
        y, pcm, st = engine.limiter_apply([x, x[:100]], rate, gain_db, ceiling, ms)
        for b, xs in enumerate((x, x[:100])):
            _check(xs, rate, gain_db, ceiling, ms, y[b], pcm[b], st[b], (rate, gain_db, ceiling, ms, b))
    # outputs are optional
    lib = engine.load_library()
    lens = np.asarray([x.size], np.int64)
    st = np.zeros(1, engine.LIMITER_DTYPE)
    assert lib.sts_limiter_apply(0, x.ctypes.data, lens.ctypes.data, 1, 16000, 0.0, -1.0, 5.0, None, None, st.ctypes.data) == 0
    _check(x, 16000, 0.0, -1.0, 5.0, None, None, st[0], "stats only")
    pcm = np.zeros(x.size, np.int16)
    assert lib.sts_limiter_apply(0, x.ctypes.data, lens.ctypes.data, 1, 16000, 0.0, -1.0, 5.0, None, pcm.ctypes.data, None) == 0
    _check(x, 16000, 0.0, -1.0, 5.0, None, pcm, None, "pcm only")


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
def _fixture(name):
    g, cfg, blob, utts, stride = load_golden_v2(golden_files_v2(name)[0])
    u, ids, sid, ls, dur, pcm, wave = utts[0]
    return blob, ids, sid, ls, dur


def _signal(syn, rate):
    return syn.tap("wave" if rate in (0, 16000) else "wave_out")[0]


LIMITING = [("amp_istft_fix_wrap", 0.0), ("amp_mbb_fix_wrap", 0.0), ("amp_ms_sdp_wrap", 0.0), ("real_hifigan_sdp_T96", 12.0),
            ("real_istft_fix_T96", 12.0), ("real_mbb_fix_T96", 12.0), ("real_ms_hifigan_sdp_T64", 12.0)]
UNTOUCHED = [("full_hifigan_sdp_T128", 12.0), ("full_mbb_fix_T96", 12.0)]
RATES = (16000, 8000, 22050, 48000)


def _engine_case(name, gain_db, limiting):
    blob, ids, sid, ls, dur = _fixture(name)
    syn = engine.Synthesizer(blob)
    ceiling, ms = -1.0, 5.0
    for rate in RATES:
        syn.set_output_rate(rate)
        syn.set_limiter(engine.LIMITER_ON, gain_db, ceiling, ms)
        assert syn.limiter_mode() == (1, gain_db, ceiling, ms)
        syn.set_record_taps(True)
        syn.set_forced_durations(dur)
        pcm = syn.infer_ids(ids, sid, ls)
        x = _signal(syn, rate)
        y = syn.tap("wave_lim")[0]
        st = syn.limiter()
        assert st.size == 1 and x.size == pcm.size
        want, c = _check(x, rate, gain_db, ceiling, ms, y, pcm, st[0], (name, rate))
        v = (x * st[0]["gain"]).astype(np.float32)
        if limiting:
            assert st[0]["limited"] > 0 and st[0]["min_gain"] < 1.0, (name, rate, st)
            assert np.abs(v).max() > c, (name, rate)
            assert np.abs(pcm.astype(np.int64)).max() <= lm.ceiling_pcm(c), (name, rate)
            nz = pcm != 0
            assert (np.sign(pcm[nz]) == np.sign(x[nz])).all(), (name, rate)                  # no wrap
        else:
            assert st[0]["limited"] == 0 and st[0]["min_gain"] == np.float32(1.0), (name, rate, st)
            assert np.array_equal(pcm, lm.pcm_cast(v)), (name, rate)
        # the same call without taps (PCM written straight to the host), then again from the launch-ahead memo
        syn.set_record_taps(False)
        for _ in range(2):
            syn.set_forced_durations(dur)
            assert np.array_equal(syn.infer_ids(ids, sid, ls), pcm), (name, rate)
            assert syn.limiter().tobytes() == st.tobytes(), (name, rate)
    syn.close()


@pytest.mark.parametrize("name,gain_db", LIMITING)
def test_engine_limits_the_peaks(name, gain_db):
    _engine_case(name, gain_db, True)


@pytest.mark.parametrize("name,gain_db", UNTOUCHED)
def test_engine_leaves_a_quiet_utterance_untouched(name, gain_db):
    _engine_case(name, gain_db, False)


def test_launch_ahead_repeat_gives_the_same_bits():
    blob, ids, sid, ls, dur = _fixture("real_hifigan_sdp_T96")
    syn = engine.Synthesizer(blob)
    for rate in (16000, 22050):
        syn.set_output_rate(rate)
        syn.set_limiter(engine.LIMITER_ON, 12.0, -1.0, 5.0)
        first = syn.infer_ids(ids, sid, ls)
        st = syn.limiter()
        assert st[0]["limited"] > 0
        again = syn.infer_ids(ids, sid, ls)
        assert syn.profile()["launch_ahead"] == 1
        assert np.array_equal(first, again) and syn.limiter().tobytes() == st.tobytes()
    syn.close()


def test_identity_at_0db_0dbfs_and_off_again():
    blob, ids, sid, ls, dur = _fixture("real_hifigan_sdp_T96")
    fresh = engine.Synthesizer(blob)
    syn = engine.Synthesizer(blob)
    for rate in RATES:
        fresh.set_output_rate(rate); syn.set_output_rate(rate)
        fresh.set_forced_durations(dur)
        p0 = fresh.infer_ids(ids, sid, ls)
        assert fresh.limiter().size == 0
        syn.set_limiter(engine.LIMITER_ON, 0.0, 0.0, 5.0)
        syn.set_record_taps(True)
        syn.set_forced_durations(dur)
        p1 = syn.infer_ids(ids, sid, ls)
        assert np.abs(_signal(syn, rate)).max() < 1.0
        syn.set_record_taps(False)
        st = syn.limiter()
        assert st.size == 1 and st[0]["limited"] == 0 and st[0]["gain"] == np.float32(1.0)
        assert np.array_equal(p0, p1), rate
        syn.set_limiter(engine.LIMITER_OFF, 0.0, 0.0, 5.0)
        syn.set_forced_durations(dur)
        assert np.array_equal(syn.infer_ids(ids, sid, ls), p0), rate
        assert syn.limiter().size == 0 and engine.load_library().sts_get_limiter(syn.h, None, 0) == 0
    fresh.close(); syn.close()


def test_with_loudness_normalization_the_target_is_reached_and_the_ceiling_holds():
    blob, ids, sid, ls, dur = _fixture("loud_hifigan_sdp_T128")
    syn = engine.Synthesizer(blob)
    for rate in (16000, 48000):
        syn.set_output_rate(rate)
        syn.set_record_taps(True)
        syn.set_loudness(engine.LOUD_MEASURE)
        syn.set_forced_durations(dur)
        syn.infer_ids(ids, sid, ls)
        x = _signal(syn, rate)
        m = lr.loudness(x, rate, -16.0, -1.0)
        assert np.isfinite(m["lufs"])
        # a target the peak clamp blocks: the loudness gain alone would put the peak 6 dB above the ceiling
        target = float(np.float32(m["lufs"] + 20.0 * np.log10(10 ** (-1 / 20) / m["peak"]) + 6.0))
        assert -70.0 <= target <= 0.0
        syn.set_loudness(engine.LOUD_NORMALIZE, target, -1.0)
        syn.set_forced_durations(dur)
        p2 = syn.infer_ids(ids, sid, ls)
        r2 = syn.loudness()[0]
        L2 = lr.measure(p2.astype(np.float64) / 32737.0, rate)[0]
        assert abs(L2 - target) > 5.0                                   # mode 2 alone stays under its target
        syn.set_limiter(engine.LIMITER_ON, 0.0, -1.0, 5.0)
        syn.set_forced_durations(dur)
        p3 = syn.infer_ids(ids, sid, ls)
        r3 = syn.loudness()[0]; st = syn.limiter()[0]
        g_L = 10.0 ** ((target - m["lufs"]) / 20.0)
        assert abs(float(r3["gain"]) / g_L - 1.0) <= 1e-4 and float(r3["gain"]) > float(r2["gain"]) * 1.9
        assert np.array_equal(_signal(syn, rate), x)
        want, c = _check(x, rate, 0.0, -1.0, 5.0, syn.tap("wave_lim")[0], p3, st, ("loud+lim", rate), g_loud=r3["gain"])
        assert st["limited"] > 0 and np.abs(p3.astype(np.int64)).max() <= lm.ceiling_pcm(c)
        L3 = lr.measure(p3.astype(np.float64) / 32737.0, rate)[0]
        assert abs(L3 - target) < abs(L2 - target), (rate, L2, L3, target)
        # mode 1 + limiter: the loudness results are those without the limiter (it measures x)
        syn.set_loudness(engine.LOUD_MEASURE, -16.0, -1.0)
        syn.set_forced_durations(dur)
        p4 = syn.infer_ids(ids, sid, ls)
        r4 = syn.loudness()
        _check(x, rate, 0.0, -1.0, 5.0, syn.tap("wave_lim")[0], p4, syn.limiter()[0], ("measure+lim", rate))
        syn.set_limiter(engine.LIMITER_OFF)
        syn.set_forced_durations(dur)
        syn.infer_ids(ids, sid, ls)
        assert syn.loudness().tobytes() == r4.tobytes()
        syn.set_loudness(engine.LOUD_OFF)
        syn.set_record_taps(False)
    syn.close()


@pytest.mark.parametrize("path", golden_files_v2("full_real_batch8_"), ids=lambda p: p.split("/")[-1])
def test_batch_members_equal_the_single_call(path):
    """under a pinned conv mode (the project's contract for bit equality across call forms) member b of a batch IS the single call: PCM
    and the whole stats record, byte for byte"""
    g, cfg, blob, utts, stride = load_golden_v2(path)
    ids = [a[1] for a in utts]; sid = [a[2] for a in utts]; ls = [a[3] for a in utts]; dur = [a[4].astype(np.int32) for a in utts]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    for rate in (16000, 22050):
        syn.set_output_rate(rate)
        syn.set_limiter(engine.LIMITER_ON, 12.0, -1.0, 5.0)
        syn.set_record_taps(True)
        syn.set_forced_durations(np.concatenate(dur))
        batch = syn.infer_batch(ids, sid, ls)
        rb = syn.limiter()
        x = _signal(syn, rate); y = syn.tap("wave_lim")[0]
        syn.set_record_taps(False)
        assert rb.size == len(ids) and (rb["limited"] > 0).any()
        off = 0
        for b in range(len(ids)):
            n = batch[b].size
            _check(x[off:off + n], rate, 12.0, -1.0, 5.0, y[off:off + n], batch[b], rb[b], (rate, b))
            off += n
        for b in range(len(ids)):
            syn.set_forced_durations(dur[b])
            one = syn.infer_ids(ids[b], sid[b], ls[b])
            r1 = syn.limiter()
            assert np.array_equal(one, batch[b]), (rate, b)
            assert r1.tobytes() == rb[b:b + 1].tobytes(), (rate, b, r1, rb[b])
        # run_batch with host PCM, twice (the second from the launch-ahead memo)
        for _ in range(2):
            syn.set_forced_durations(np.concatenate(dur))
            n_out = syn.run_batch(ids, sid, ls)
            assert syn.limiter().tobytes() == rb.tobytes()
            assert np.array_equal(syn.pcm_host(), np.concatenate(batch)) and list(n_out) == [p.size for p in batch]
        a = syn.run_batch(ids, sid, ls); pa = syn.pcm_host().copy(); ra = syn.limiter()
        b2 = syn.run_batch(ids, sid, ls)
        assert np.array_equal(pa, syn.pcm_host()) and ra.tobytes() == syn.limiter().tobytes() and list(a) == list(b2)
    syn.close()


def test_split_bf16_repeat_on_a_model_beyond_fp16_range():
    """a model whose conv_pre is scaled beyond fp16's range (as test_loudness_gpu.py builds it): the f16x2 call is repeated in split-bf16,
    limiter included"""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = sb.synthetic_ids(20, cfg.vocab)
    w = sb._W(5, cfg.stats)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._gen_hdr(w, cfg)
    start = w.n + 6
    big = blob.copy()
    big[start:start + cfg.up_init * 7 * cfg.inter] *= np.float32(3.0e6)
    syn = engine.Synthesizer(big)
    syn.set_limiter(engine.LIMITER_ON, 6.0, -1.0, 5.0)
    for rate in (16000, 44100):
        syn.set_output_rate(rate)
        syn.set_conv_math("bf16x3")
        want = syn.infer_ids(ids); rw = syn.limiter()
        before = syn.profile()["conv_math_fallbacks"]
        syn.set_conv_math("f16x2")
        got = syn.infer_ids(ids); rg = syn.limiter()
        assert syn.profile()["conv_math_fallbacks"] == before + 1
        assert np.array_equal(got, want) and rg.tobytes() == rw.tobytes(), rate
    syn.close()


def _tiny_requests():
    cfg = sb.tiny_cfg("mbb_fix")
    blob = sb.make_blob(cfg, 11)
    return blob, [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (40, 33, 5, 61)]


def _pool_and_multi(blob, ids):
    """what a pool (one request per batch: the single call's shapes, so the single call's kernels) and a two-engine multi-device handle
    return with the limiter on"""
    lib = engine.load_library()
    out = {}
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=1)
    pool.set_output_rate(24000)
    assert lib.sts_pool_set_limiter(pool.h, 2, 20.0, -2.0, 2.5) == STS_EINVAL
    assert lib.sts_pool_set_limiter(pool.h, 1, 20.0, 1.0, 2.5) == STS_EINVAL
    pool.set_limiter(engine.LIMITER_ON, 20.0, -2.0, 2.5)
    t = [pool.submit(a) for a in ids]
    assert lib.sts_pool_set_limiter(pool.h, 0, 20.0, -2.0, 2.5) == STS_ESTATE
    out["pool"] = [pool.wait(k) for k in t]
    chunks = []
    k = pool.submit_stream(ids[0], 8, lambda pcm, off: chunks.append(pcm.copy()) and False)
    assert pool.wait(k) == sum(c.size for c in chunks)
    out["pool_stream"] = np.concatenate(chunks)
    pool.set_limiter(engine.LIMITER_OFF)
    pool.close()
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    md.set_output_rate(24000)
    with pytest.raises(engine.StsError):
        md.set_limiter(engine.LIMITER_ON, 50.0)
    md.set_limiter(engine.LIMITER_ON, 20.0, -2.0, 2.5)
    out["shard"] = md.shard_of([len(a) for a in ids])
    out["multi"] = md.infer_batch(ids)
    md.set_limiter(engine.LIMITER_OFF)
    md.close()
    return out


def test_pool_and_multi_device():
    blob, ids = _tiny_requests()
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(24000)
    syn.set_limiter(engine.LIMITER_ON, 20.0, -2.0, 2.5)
    want = [syn.infer_ids(a) for a in ids]
    got = _pool_and_multi(blob, ids)
    for i in range(len(ids)):
        assert np.array_equal(got["pool"][i], want[i]), i
    # the pool's stream is the single engine's stream (same chunks, same kernels), and within the streaming contract of the whole call
    st = np.concatenate(syn.infer_ids_stream(ids[0], 8)[0])
    assert np.array_equal(got["pool_stream"], st)
    assert st.size == want[0].size and np.abs(st.astype(np.int64) - want[0].astype(np.int64)).max() <= 1
    # each engine of the multi-device handle runs its shard as one batch: the single engine's batch of the same members, bit for bit
    shard = got["shard"]
    for sh in sorted(set(int(v) for v in shard)):
        mem = [b for b in range(len(ids)) if int(shard[b]) == sh]
        ref = syn.infer_batch([ids[b] for b in mem])
        for k, b in enumerate(mem):
            assert np.array_equal(got["multi"][b], ref[k]), (sh, b)
    syn.set_limiter(engine.LIMITER_OFF)
    plain = [syn.infer_ids(a) for a in ids]
    syn.close()
    assert any(not np.array_equal(a, b) for a, b in zip(want, plain))


def test_poisoned_workspace_changes_nothing():
    blob, ids, sid, ls, dur = _fixture("real_mbb_fix_T96")
    cfg = sb.tiny_cfg("hifigan_sdp")
    tiny = sb.make_blob(cfg, 21)
    tids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (17, 9, 30)]

    def scenario(pattern):
        out = []
        for bl, single, batch in ((blob, (ids, sid, ls), None), (tiny, (tids[0], 0, 1.0), tids)):
            syn = engine.Synthesizer(bl)
            if pattern is not None:
                syn.debug_set("poison", pattern)
            for rate, loud in ((16000, 0), (22050, 2), (16000, 1)):
                syn.set_output_rate(rate)
                syn.set_loudness(loud, -14.0, -1.0)
                syn.set_limiter(engine.LIMITER_ON, 14.0, -1.0, 5.0)
                for _ in range(2):
                    out.append(syn.infer_ids(*single).tobytes()); out.append(syn.limiter().tobytes()); out.append(syn.loudness().tobytes())
                if batch:
                    out.append(b"".join(p.tobytes() for p in syn.infer_batch(batch))); out.append(syn.limiter().tobytes())
                    syn.run_batch(batch); out.append(syn.pcm_host().tobytes()); out.append(syn.limiter().tobytes())
                syn.set_record_taps(True)
                out.append(syn.infer_ids(*single).tobytes()); out.append(syn.tap("wave_lim").tobytes())
                syn.set_record_taps(False)
                if loud == 0 and batch:          # the streaming forms (refused under a loudness mode)
                    out.append(np.concatenate(syn.infer_ids_stream(single[0], 7)[0]).tobytes())
                    ch, _ = syn.infer_batch_stream(batch, 5)
                    out.append(b"".join(np.concatenate(c).tobytes() for c in ch))
            if pattern is not None:
                assert syn.profile()["poison_bytes"] > 0
            syn.close()
        return out

    want = scenario(None)
    for pattern in (0x7FC00000, -1, 0x7BFF7BFF):
        assert scenario(pattern) == want, hex(pattern & 0xFFFFFFFF)


# ---- streaming ----------------------------------------------------------------------------------------------------------------------
def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


@pytest.mark.parametrize("rate", [16000, 8000, 22050, 48000])
def test_streams_concatenate_to_the_whole_utterance(rate):
    """pinned conv mode: single and batched streams (B = 1, B = 4 of unequal lengths, one stopped early) at 1 / 7 / 32 frames per chunk are
    the whole-utterance PCM bit for bit, in a regime where the limiter really works"""
    for kind in ("hifigan_sdp", "mbb_fix"):
        cfg = sb.tiny_cfg(kind)
        blob = sb.make_blob(cfg, 1234)
        ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in (23, 9, 31, 14)]
        syn = engine.Synthesizer(blob)
        syn.set_conv_mode(6)
        syn.set_output_rate(rate)
        syn.set_record_taps(True)
        syn.infer_ids(ids[0])
        peak = float(np.abs(_signal(syn, rate)).max())
        syn.set_record_taps(False)
        assert peak > 0
        gain_db = float(np.clip(20.0 * np.log10(0.9 / peak) + 8.0, -40.0, 40.0))     # the peak lands about 8 dB above the ceiling
        syn.set_limiter(engine.LIMITER_ON, gain_db, -1.0, 3.0)
        whole = syn.infer_batch(ids)
        st = syn.limiter()
        assert (st["limited"] > 0).all() and (st["min_gain"] < 1.0).all(), (kind, rate, st)
        assert np.array_equal(syn.infer_ids(ids[0]), whole[0])
        for chunk in (1, 7, 32):
            got, _ = syn.infer_ids_stream(ids[0], chunk)
            assert np.array_equal(_cat(got), whole[0]), (kind, rate, chunk, "single")
            assert syn.limiter().size == 0
            got, _ = syn.infer_batch_stream([ids[2]], chunk)
            assert np.array_equal(_cat(got[0]), whole[2]), (kind, rate, chunk, "B=1")
            tot = []
            got, _ = syn.infer_batch_stream(ids, chunk, n_total=tot)
            for b in range(len(ids)):
                assert np.array_equal(_cat(got[b]), whole[b]) and tot[b] == whole[b].size, (kind, rate, chunk, b)
            stop, _ = syn.infer_batch_stream(ids, chunk, on_chunk=lambda u, pcm, off, t: u == 1)
            assert len(stop[1]) == 1 and np.array_equal(stop[1][0], whole[1][:stop[1][0].size])
            for b in (0, 2, 3):
                assert np.array_equal(_cat(stop[b]), whole[b]), (kind, rate, chunk, b, "one stopped")
        syn.close()


def test_streams_under_the_automatic_conv_choice_stay_within_one_lsb():
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 7)
    ids = sb.synthetic_ids(40, cfg.vocab)
    syn = engine.Synthesizer(blob)
    for rate in (16000, 44100):
        syn.set_output_rate(rate)
        syn.set_limiter(engine.LIMITER_ON, 20.0, -1.0, 5.0)
        whole = syn.infer_ids(ids)
        for chunk in (8, 32):
            got = _cat(syn.infer_ids_stream(ids, chunk)[0])
            assert got.size == whole.size and np.abs(got.astype(np.int64) - whole.astype(np.int64)).max() <= 1, (rate, chunk)
    syn.close()


def test_stream_halo_follows_the_limiter_and_loudness_still_refuses_streams():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids = sb.synthetic_ids(17, cfg.vocab)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    for rate in (16000, 8000, 48000):
        syn.set_output_rate(rate)
        h0 = syn.stream_halo_frames()
        prev = h0
        for ms in (0.25, 2.0, 5.0, 10.0):
            syn.set_limiter(engine.LIMITER_ON, 6.0, -1.0, ms)
            h = syn.stream_halo_frames()
            H = engine.limiter_design(rate, 6.0, -1.0, ms)[0]
            assert h >= prev and h > h0 or ms == 0.25, (rate, ms, h, prev)
            assert (h - h0 + 1) * hop * rate >= 2 * H * 16000, (rate, ms, h, h0)          # the extra frames cover 2H output samples
            prev = h
        assert prev > h0
        syn.set_limiter(engine.LIMITER_OFF)
        assert syn.stream_halo_frames() == h0
    syn.set_output_rate(16000)
    plain, _ = syn.infer_ids_stream(ids, 8)
    syn.set_limiter(engine.LIMITER_ON, 6.0, -1.0, 5.0)
    syn.set_loudness(engine.LOUD_NORMALIZE)
    with pytest.raises(engine.StsError, match="loudness"):
        syn.infer_ids_stream(ids, 8)
    with pytest.raises(engine.StsError, match="loudness"):
        syn.infer_batch_stream([ids, ids], 8)
    syn.infer_ids(ids)                                       # the engine stays usable
    assert syn.limiter().size == 1
    syn.set_loudness(engine.LOUD_OFF)
    syn.set_limiter(engine.LIMITER_OFF)
    again, _ = syn.infer_ids_stream(ids, 8)
    assert np.array_equal(_cat(again), _cat(plain)) and syn.limiter().size == 0
    syn.close()


def test_apply_with_nan_and_inf_samples():
    """a non-finite sample gets gain 0 (its own y is NaN: inf * 0) and pulls its neighbourhood down; peak_out is the peak of the samples
    whose y is a number"""
    rng = np.random.default_rng(9)
    x = _noise(rng, TILE + 300, 0.3)
    x[100] = np.nan; x[TILE - 1] = np.inf; x[TILE + 150] = -np.inf
    y, pcm, st = engine.limiter_apply([x, x[:50]], 16000, 3.0, -1.0, 5.0)
    for b, xs in enumerate((x, x[:50])):
        H, c, G = engine.limiter_design(16000, 3.0, -1.0, 5.0)
        g0 = lm.static_gain(G)
        wy, ws, wS = lm.limit(xs, g0, H, c)
        assert np.array_equal(y[b].view(np.uint32)[np.isfinite(wy)], wy.view(np.uint32)[np.isfinite(wy)]), b
        assert np.array_equal(np.isnan(y[b]), np.isnan(wy)), b
        want = lm.stats(wy, ws, wS, g0, H)
        assert st[b]["min_gain"] == want["min_gain"] and st[b]["limited"] == want["limited"], b
        assert np.float32(st[b]["peak_out"]).tobytes() == np.float32(want["peak_out"]).tobytes(), (b, st[b], want)
        fin = np.isfinite(wy)
        assert np.array_equal(pcm[b][fin], lm.pcm_cast(wy[fin])), b
    assert st[0]["min_gain"] == 0.0 and np.isnan(y[0][[100, TILE - 1, TILE + 150]]).all() and np.isfinite(st[0]["peak_out"])


def test_invalid_arguments_leave_the_setting_unchanged():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    syn = engine.Synthesizer(blob)
    assert syn.limiter_mode()[0] == 0
    syn.set_limiter(engine.LIMITER_ON, 3.0, -2.0, 2.5)
    lib = engine.load_library()
    nan = float("nan")
    for mode, g, c, ms in ((2, 3.0, -2.0, 2.5), (-1, 3.0, -2.0, 2.5), (1, nan, -2.0, 2.5), (1, 3.0, nan, 2.5), (1, 3.0, -2.0, nan),
                           (1, 40.5, -2.0, 2.5), (1, -40.5, -2.0, 2.5), (1, 3.0, 0.5, 2.5), (1, 3.0, -30.5, 2.5), (1, 3.0, -2.0, 0.2),
                           (1, 3.0, -2.0, 10.5), (0, 3.0, -2.0, float("inf"))):
        assert lib.sts_set_limiter(syn.h, mode, g, c, ms) == STS_EINVAL, (mode, g, c, ms)
        assert syn.limiter_mode() == (1, 3.0, -2.0, 2.5)
    pcm = syn.infer_ids(sb.synthetic_ids(9, cfg.vocab))
    assert lib.sts_get_limiter(syn.h, None, 0) == 1
    out = np.zeros(1, engine.LIMITER_DTYPE)
    assert lib.sts_get_limiter(syn.h, out.ctypes.data, 0) == STS_EINVAL
    assert lib.sts_get_limiter(syn.h, out.ctypes.data, 1) == 1 and out[0]["gain"] == lm.static_gain(engine.limiter_design(16000, 3.0, -2.0, 2.5)[2])
    assert pcm.size > 0
    syn.close()
