"""Gain plans on the MI355X (sts_set_gain_plan, sts_gain_plan_apply, sts_pool_submit_gain, sts_multi_set_gain_plan) against the integer
restatement of tests/gain_ref.py, bit for bit: the kernel on caller signals across its tile, window and alignment edges; an engine's
"wave_gain" tap and PCM against the restatement applied to the same call's "wave" tap and durations; the chain behind it (resampler,
loudness, limiter) against the existing checkers fed with "wave_gain"; one utterance in every call form; composition with a duration plan, a
speaker mix and the split-bf16 repeat; lifetime and refusals."""
import ctypes as C

import numpy as np
import pytest

import gain_ref as gr
import loudness_ref as lr
import resample_ref as rr
from conftest import golden_files, load_golden
from summertts_amd import engine, synth_blob as sb
from test_loudness_gpu import _close as loud_close          # the loudness checker's own comparison (lufs 0.01, peak exact, gain 1e-4)

pytestmark = pytest.mark.gpu

STS_EINVAL = -1
INF = float("inf")
TILE = 4096                     # gain_plan.hip GP_TILE
RESAMPLE_WAVE_TOL = 1e-5        # tests/test_resample_gpu.py _check_against_checker: |wave_out - checker| of the resampled float wave


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


def _tiny(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    return cfg, sb.make_blob(cfg, seed)


def _db(n, seed, mute_every=5):
    """per-phoneme gains over the whole valid range, with mutes and a mute right next to +24 dB"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-30.0, 24.0, n).astype(np.float32)
    g[::mute_every] = -INF
    if n > 1:
        g[1::mute_every] = 24.0
    return g


# ---- the kernel on caller signals ---------------------------------------------------------------------------------------------------------
def _signal(n, seed):
    x = (0.5 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    x[::97] = np.float32(0.9)           # (+24 dB takes these past the cast's wrap-around)
    return x


def _apply_case(durs, hop, ramps, seed=0):
    """one launch against the restatement, y and pcm bit for bit; then every member alone against the same member in the batch"""
    B = len(durs)
    sig = [_signal(max(1, int(np.sum(d))) * hop, seed + b) for b, d in enumerate(durs)]
    dbs = [_db(len(d), seed + 10 * b, 3 + b % 3) for b, d in enumerate(durs)]
    out = []
    for r in range(len(ramps)):
        plans = [{"gain_db": dbs[b], "ramp_ms": ramps[(b + r) % len(ramps)]} for b in range(B)]
        y, pcm = engine.gain_plan_apply(sig, durs, plans, hop)
        for b in range(B):
            want = gr.apply(sig[b], durs[b], hop, dbs[b], plans[b]["ramp_ms"])
            assert y[b].tobytes() == want.tobytes(), (hop, r, b, int(np.flatnonzero(y[b] != want)[0]) if (y[b] != want).any() else -1)
            assert np.array_equal(pcm[b], gr.pcm_cast(want)), (hop, r, b)
        out.append((plans, y, pcm))
    plans, y, pcm = out[0]
    for b in range(B):
        ya, pa = engine.gain_plan_apply([sig[b]], [durs[b]], [plans[b]], hop)
        assert ya[0].tobytes() == y[b].tobytes() and np.array_equal(pa[0], pcm[b]), (hop, b)


def test_apply_one_sample_per_frame_on_every_tile_edge():
    """samples_per_frame 1 (the smallest the entry accepts): utterances of 1, 2 and 40 phonemes; signals of exactly one tile, one tile - 1 and
    + 1, and three tiles with a tail; a phoneme longer than a tile whose ramp straddles the tile boundary; forty one-sample phonemes inside
    one window of h = 400, runs of empty phonemes at the start, in the middle and at the end; h = 400, 1 and 0 for every member"""
    z3 = [0, 0, 0]
    durs = [[TILE],                                                            # 1 phoneme, exactly one tile
            [TILE - 96, 95],                                                   # 2 phonemes, one tile - 1
            [1, TILE],                                                         # one tile + 1: the boundary sits on the utterance's first sample
            z3 + [1] * 14 + [0, 0, 0, 0] + [1] * 17 + [0, 0],                  # 40 phonemes, 31 samples: every window holds the whole utterance
            z3 + [TILE - 200] + [1] * 12 + [0] * 5 + [2 * TILE + 333] + [3] * 16 + [0, 0]]     # 40 phonemes, three tiles and a tail
    assert [len(d) for d in durs] == [1, 2, 2, 40, 40]
    _apply_case(durs, 1, [50.0, 0.125, 0.0])


def test_apply_unaligned_members_and_empty_utterances():
    """samples_per_frame 6: members start at odd multiples of 2 samples, so the 4-sample groups meet every alignment; an utterance whose
    durations are all 0 (one frame nobody owns) between two others"""
    rng = np.random.default_rng(3)
    durs = [rng.integers(0, 5, 40).tolist(), [0, 0, 0], [7], rng.integers(0, 300, 9).tolist(), [0], [1, 0, 1]]
    _apply_case(durs, 6, [50.0, 0.125, 0.0], seed=40)
    y, pcm = engine.gain_plan_apply([_signal(6, 1)], [[0, 0, 0]], [{"gain_db": [-INF, -INF, -INF], "ramp_ms": 3.0}], 6)
    assert y[0].tobytes() == _signal(6, 1).tobytes()


def test_apply_at_a_model_hop_and_without_gains():
    rng = np.random.default_rng(4)
    durs = [rng.integers(0, 12, 40).tolist(), [30], rng.integers(1, 4, 2).tolist()]
    _apply_case(durs, 256, [10.0, 50.0], seed=70)
    sig = [_signal(int(np.sum(d)) * 256, 5 + b) for b, d in enumerate(durs)]
    y, pcm = engine.gain_plan_apply(sig, durs, [None, {"ramp_ms": 50.0}, {"gain_db": [0.0, 0.0]}], 256)
    for b in range(3):                                   # no gains, or 0 dB throughout: the signal itself and its plain cast
        assert y[b].tobytes() == sig[b].tobytes() and np.array_equal(pcm[b], gr.pcm_cast(sig[b])), b
    lib = engine.load_library()
    x = np.zeros(8, np.float32); d = np.asarray([1, 1], np.int32); n = np.asarray([2], np.int32)
    arr = (engine.GainPlan * 1)()
    for args in ((0, 4), (1, 0), (65536, 4)):            # B < 1, samples_per_frame < 1, more signals than the grid has rows
        assert lib.sts_gain_plan_apply(0, x.ctypes.data, d.ctypes.data, n.ctypes.data, args[0], args[1], arr, x.ctypes.data, None) == STS_EINVAL
    bad = np.asarray([1, -1], np.int32)
    assert lib.sts_gain_plan_apply(0, x.ctypes.data, bad.ctypes.data, n.ctypes.data, 1, 4, arr, x.ctypes.data, None) == STS_EINVAL
    arr[0].ramp_ms = 51.0
    assert lib.sts_gain_plan_apply(0, x.ctypes.data, d.ctypes.data, n.ctypes.data, 1, 4, arr, x.ctypes.data, None) == STS_EINVAL


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
def _gained(syn, ids, plan, sid=0):
    """one call with a gain plan and taps on -> (pcm, wave, wave_gain, durations)"""
    syn.set_record_taps(True)
    syn.set_gain_plan([len(ids)], [plan])
    pcm = syn.infer_ids(ids, sid)
    out = pcm, syn.tap("wave")[0], syn.tap("wave_gain")[0], syn.durations(len(ids))
    syn.set_record_taps(False)
    return out


@pytest.mark.parametrize("kind", ["hifigan_fix", "mbb_fix", "ms_sdp"])
def test_native_rate_is_the_restatement_on_the_calls_own_wave(kind):
    cfg, blob = _tiny(kind)
    ids = sb.synthetic_ids(23, cfg.vocab, salt=2)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    plain = syn.infer_ids(ids)
    for ramp in (0.0, 5.0, 50.0):
        plan = {"gain_db": _db(len(ids), 9), "ramp_ms": ramp}
        pcm, wave, y, dur = _gained(syn, ids, plan)
        assert np.array_equal(gr.pcm_cast(wave), plain)                          # "wave" stays the un-gained signal
        want = gr.apply(wave, dur, hop, plan["gain_db"], ramp)
        assert y.tobytes() == want.tobytes(), (kind, ramp)
        assert np.array_equal(pcm, gr.pcm_cast(want)) and not np.array_equal(pcm, plain), (kind, ramp)
        syn.set_gain_plan([len(ids)], [plan])                                     # without taps: the gain kernel writes the host PCM itself
        assert np.array_equal(syn.infer_ids(ids), pcm), (kind, ramp)
        syn.debug_set("pcm_direct", 0)
        syn.set_gain_plan([len(ids)], [plan])
        assert np.array_equal(syn.infer_ids(ids), pcm), (kind, ramp)
        syn.debug_set("pcm_direct", 1)
    syn.set_record_taps(True)
    assert np.array_equal(syn.infer_ids(ids), plain) and syn.tap("wave").size == plain.size
    with pytest.raises(engine.StsError):
        syn.tap("wave_gain")                                                      # the tap exists only for a run with a plan
    syn.close()


@pytest.mark.parametrize("path", golden_files(), ids=lambda p: p.split("/")[-1])
def test_a_plan_without_gains_changes_nothing(path):
    """an engine that never set a plan against one given a plan whose gain_db is NULL, plain and with a poisoned workspace"""
    g, cfg, blob = load_golden(path)
    ids, sid, ls = g["ids"], int(g["sid"]), float(g["length_scale"])

    def run(plan, poison):
        syn = engine.Synthesizer(blob)
        if poison:
            syn.debug_set("poison", 0x7FC00000)
        syn.set_record_taps(True)
        if plan:
            syn.set_gain_plan([len(ids)], [{"ramp_ms": 20.0}])
        pcm = syn.infer_ids(ids, sid, ls)
        out = [pcm.tobytes(), syn.durations(len(ids)).tobytes()] + [syn.tap(k).tobytes() for k in ("m", "logw", "z_p", "wave")]
        if plan:
            assert syn.tap("wave_gain").tobytes() == out[-1]
        syn.set_record_taps(False)
        if plan:
            syn.set_gain_plan([len(ids)], [None])
        out.append(syn.infer_ids(ids, sid, ls).tobytes())       # without taps: the PCM goes straight to the host
        syn.close()
        return out

    want = run(False, False)
    assert run(True, False) == want
    assert run(True, True) == want


# ---- the chain behind the envelope ---------------------------------------------------------------------------------------------------------
def test_limiter_loudness_and_resampler_read_the_gained_wave():
    cfg, blob = _tiny("mbb_fix", 7)
    ids = sb.synthetic_ids(60, cfg.vocab, salt=3)
    plan = {"gain_db": _db(len(ids), 21, 7), "ramp_ms": 8.0}
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    # limiter at the native rate: the PCM is the limiter's own entry point on the "wave_gain" tap
    lim = dict(gain_db=6.0, ceiling_dbfs=-3.0, lookahead_ms=2.0)
    syn.set_limiter(engine.LIMITER_ON, **lim)
    pcm, wave, y, dur = _gained(syn, ids, plan)
    assert y.tobytes() == gr.apply(wave, dur, hop, plan["gain_db"], 8.0).tobytes()
    ly, lp, _ = engine.limiter_apply([y], 16000, **lim)
    assert np.array_equal(pcm, lp[0])
    syn.set_record_taps(True); syn.set_gain_plan([len(ids)], [plan]); syn.infer_ids(ids)
    assert syn.tap("wave_lim")[0].tobytes() == ly[0].tobytes()
    syn.set_record_taps(False)
    syn.set_limiter(engine.LIMITER_OFF)
    # loudness mode 2: the existing checker on "wave_gain", its own comparison
    syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -1.0)
    pcm, wave, y, dur = _gained(syn, ids, plan)
    r = syn.loudness()[0]
    loud_close(r, lr.loudness(y, 16000, -20.0, -1.0), "gained")
    assert np.array_equal(pcm, lr.normalize(y, r["gain"]))
    syn.set_loudness(engine.LOUD_OFF)
    # the resampler: "wave_out" against the float64 checker applied to "wave_gain"
    for rate in (8000, 48000):
        syn.set_output_rate(rate)
        syn.set_record_taps(True)
        syn.set_gain_plan([len(ids)], [plan])
        pcm = syn.infer_ids(ids)
        y, got = syn.tap("wave_gain")[0], syn.tap("wave_out")[0]
        assert y.tobytes() == gr.apply(syn.tap("wave")[0], syn.durations(len(ids)), hop, plan["gain_db"], 8.0).tobytes(), rate
        syn.set_record_taps(False)
        want = rr.resample(y, rate)
        err = float(np.abs(got - want).max())
        print(f"rate {rate}: max |wave_out - checker(wave_gain)| = {err:.3e}")
        assert got.size == pcm.size == rr.out_len(y.size, rate) and err <= RESAMPLE_WAVE_TOL, (rate, err)
        assert np.array_equal(pcm, rr.pcm_cast(got)), rate
    syn.close()


# ---- call forms ------------------------------------------------------------------------------------------------------------------------------
def _infer_ids_c(syn, ids, sid=0, ls=1.0):
    """sts_infer_ids itself (the class goes through sts_run_batch + sts_copy_pcm_host)"""
    a = np.ascontiguousarray(ids, dtype=np.int32)
    p, n = C.POINTER(C.c_int16)(), C.c_int32()
    rc = syn.lib.sts_infer_ids(syn.h, a.ctypes.data, a.size, sid, ls, C.byref(p), C.byref(n))
    assert rc == 0, syn.lib.sts_last_error()
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    syn.lib.sts_free(p)
    return out


def _plans3(lens):
    return [{"gain_db": _db(lens[0], 31), "ramp_ms": 20.0}, None, {"gain_db": _db(lens[2], 33, 4), "ramp_ms": 0.0}]


@pytest.mark.parametrize("kind,rate,limiter", [("hifigan_fix", 16000, False), ("mbb_fix", 16000, False), ("mbb_fix", 8000, True)])
def test_one_utterance_gives_the_same_bits_in_every_call_form(kind, rate, limiter):
    """pinned conv mode: sts_infer_ids, a ragged batch of 3 with different plans (one of them absent), sts_run_batch + sts_copy_pcm_host,
    streamed and batch-streamed with a 20 ms ramp (320 native samples: wider than a 5-frame chunk of the HiFi-GAN model, across every chunk
    edge of both)"""
    cfg, blob = _tiny(kind, 11)
    lens = (37, 9, 24)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    plans = _plans3(lens)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if limiter:
        syn.set_limiter(engine.LIMITER_ON, 3.0, -2.0, 1.5)
    halo = syn.stream_halo_frames()
    free = syn.infer_batch(ids)
    alone = []
    for a, p in zip(ids, plans):
        syn.set_gain_plan([len(a)], [p])
        assert syn.stream_halo_frames() == halo                                    # a pending plan does not widen the decode window
        alone.append(_infer_ids_c(syn, a))
    assert np.array_equal(alone[1], free[1]) and not np.array_equal(alone[0], free[0]) and not np.array_equal(alone[2], free[2])
    syn.set_gain_plan(lens, plans)
    batch = syn.infer_batch(ids)                                                   # sts_run_batch + sts_copy_pcm_host
    for b in range(3):
        assert np.array_equal(batch[b], alone[b]), (kind, rate, b)
    assert all(np.array_equal(a, b) for a, b in zip(syn.infer_batch(ids), free))   # consumed: the next batch is plain
    for chunk in (5, 32):
        for b in (0, 2):
            syn.set_gain_plan([lens[b]], [plans[b]])
            assert np.array_equal(_cat(syn.infer_ids_stream(ids[b], chunk)[0]), alone[b]), (kind, rate, chunk, b)
        syn.set_gain_plan(lens, plans)
        got, _ = syn.infer_batch_stream(ids, chunk)
        for b in range(3):
            assert np.array_equal(_cat(got[b]), alone[b]), (kind, rate, chunk, b)
    assert syn.stream_halo_frames() == halo
    syn.close()


def test_pool_and_multi_device_carry_the_plan_per_utterance():
    cfg, blob = _tiny("mbb_fix", 11)
    lens = (40, 33, 5)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    plans = _plans3(lens)
    syn = engine.Synthesizer(blob)
    single = []
    for a, p in zip(ids, plans):
        syn.set_gain_plan([len(a)], [p])
        single.append(syn.infer_ids(a))
    syn.set_gain_plan(lens, plans)
    batch = syn.infer_batch(ids)
    free = syn.infer_batch(ids)
    assert np.array_equal(batch[1], free[1]) and not np.array_equal(batch[0], free[0])
    # one request per batch: the single call's shapes, so the single call, bit for bit; plain submits between them
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=1)
    t = [pool.submit(a, gain=p) if p else pool.submit(a) for a, p in zip(ids, plans)]
    got = [pool.wait(k) for k in t]
    assert all(np.array_equal(g, s) for g, s in zip(got, single))
    with pytest.raises(engine.StsError):
        pool.submit(ids[0], gain={"gain_db": np.full(lens[0], 24.5, np.float32)})
    with pytest.raises(engine.StsError):
        pool.submit(ids[0], gain={"gain_db": np.zeros(lens[0], np.float32), "ramp_ms": 60.0})
    pool.close()
    # requests with and without a plan folded into ONE packed batch: queued while the only worker is inside a long streaming request
    import threading
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=3)
    busy = threading.Event()
    blocker = pool.submit_stream(sb.synthetic_ids(300, cfg.vocab, salt=1), 2, lambda pcm, off: busy.set())
    assert busy.wait(60)
    t = [pool.submit(a, gain=p) if p else pool.submit(a) for a, p in zip(ids, plans)]
    assert pool.wait(blocker) > 0
    got = [pool.wait(k) for k in t]
    assert pool.stats() == (2, 4)
    for b in range(3):
        assert np.array_equal(got[b], batch[b]), b
    pool.close()
    # two engines on one device: each runs its shard as one batch with its members' plans
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    shard = md.shard_of(lens)
    md.set_gain_plan(lens, plans)
    multi = md.infer_batch(ids)
    after = md.infer_batch(ids)                                                         # consumed
    with pytest.raises(engine.StsError):
        md.set_gain_plan(lens, [None, {"gain_db": np.full(lens[1], -97.0, np.float32)}, None])
    md.set_gain_plan(lens[:2], plans[:2])
    with pytest.raises(engine.StsError):
        md.infer_batch(ids)                                                             # set for another batch
    md.close()
    for sh in sorted(set(int(v) for v in shard)):
        mem = [b for b in range(3) if int(shard[b]) == sh]
        syn.set_gain_plan([lens[b] for b in mem], [plans[b] for b in mem])
        ref = syn.infer_batch([ids[b] for b in mem])
        plain = syn.infer_batch([ids[b] for b in mem])
        for k, b in enumerate(mem):
            assert np.array_equal(multi[b], ref[k]) and np.array_equal(after[b], plain[k]), (sh, b)
    syn.close()


# ---- composition ----------------------------------------------------------------------------------------------------------------------------
def test_the_envelope_follows_the_planned_durations_with_a_mix_pending():
    cfg, blob = _tiny("ms_hifigan_sdp", 5)
    ids = sb.synthetic_ids(12, cfg.vocab, salt=4)
    n = len(ids)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    fixed = [-1] * n; fixed[3] = 0; fixed[4] = 25; fixed[5] = 0
    db = np.asarray([0, -6, 6, -INF, -12, 24, 3, -3, -INF, 12, -20, 0], np.float32)
    syn.set_record_taps(True)
    syn.set_duration_plan([n], [{"fixed": fixed, "target_frames": 150}])
    syn.set_speaker_mix([{"sid": [0, 3], "weight": [0.5, 0.5]}])
    syn.set_gain_plan([n], [{"gain_db": db, "ramp_ms": 0.0}])
    pcm = syn.infer_ids(ids, 1)
    wave, y, dur = syn.tap("wave")[0], syn.tap("wave_gain")[0], syn.durations(n)
    off = syn.phoneme_offsets(n)
    syn.set_record_taps(False)
    assert int(dur.sum()) == 150 and dur[4] == 25 and dur[3] == 0 and pcm.size == 150 * hop
    assert y.tobytes() == gr.apply(wave, dur, hop, db, 0.0).tobytes() and np.array_equal(pcm, gr.pcm_cast(y))
    q, _ = gr.design(db, n)
    for i in range(n):                       # with h = 0 every heard phoneme's first sample carries exactly its own gain
        if dur[i] > 0:
            g = np.float32(np.float64(q[i]) / np.float64(gr.ONE))
            assert y[off[i]] == wave[off[i]] * g and y[off[i] + dur[i] * hop - 1] == wave[off[i] + dur[i] * hop - 1] * g, i
    syn.close()


def test_the_split_bf16_repeat_applies_the_plan_once():
    """The f16x2 call is repeated in split-bf16 and the repeat applies the same plan: its PCM equals a bf16x3-pinned run with that plan.
    The fallback is provoked the way every existing test of the repeat provokes it (tests/test_loudness_gpu.py, test_resample_gpu.py,
    test_parity_gpu.py): conv_pre of a synthetic blob scaled up until the trunk's activations leave fp16's range.  The committed
    amplitude-edge goldens (tests/golden/amp_*) cannot serve: they raise the gain of the LAST conv only (conftest.py), behind every conv
    that stages fp16 operands, so a call on them is never repeated."""
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
    plan = {"gain_db": _db(len(ids), 3), "ramp_ms": 12.0}
    syn = engine.Synthesizer(big)
    syn.set_conv_math("bf16x3")
    plain = syn.infer_ids(ids)
    syn.set_gain_plan([len(ids)], [plan])
    want = syn.infer_ids(ids)
    assert not np.array_equal(want, plain)
    before = syn.profile()["conv_math_fallbacks"]
    syn.set_conv_math("f16x2")
    syn.set_gain_plan([len(ids)], [plan])
    got = syn.infer_ids(ids)
    assert syn.profile()["conv_math_fallbacks"] == before + 1
    assert np.array_equal(got, want)
    syn.close()


# ---- lifetime and refusals -------------------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals():
    cfg, blob = _tiny("hifigan_fix", 3)
    ids = sb.synthetic_ids(7, cfg.vocab)
    syn = engine.Synthesizer(blob)
    plain = syn.infer_ids(ids)
    plan = {"gain_db": [0, -6, -INF, 24, 3, -96, 0], "ramp_ms": 4.0}
    syn.set_gain_plan([7], [plan])
    gained = syn.infer_ids(ids)
    assert not np.array_equal(gained, plain) and gained.size == plain.size
    assert np.array_equal(syn.infer_ids(ids), plain)                         # the plan applies once: the second call is plain
    # an invalid plan at the set call leaves an earlier pending plan in force
    syn.set_gain_plan([7], [plan])
    nan = float("nan")
    for bad in ({"gain_db": [0, nan, 0, 0, 0, 0, 0]}, {"gain_db": [24.01] + [0] * 6}, {"gain_db": [-96.01] + [0] * 6}, {"gain_db": [INF] + [0] * 6},
                {"gain_db": [0] * 7, "ramp_ms": -1.0}, {"gain_db": [0] * 7, "ramp_ms": 50.01}, {"ramp_ms": nan}):
        with pytest.raises(engine.StsError):
            syn.set_gain_plan([7], [bad])
    with pytest.raises(engine.StsError):
        syn.set_gain_plan([0], [{}])
    lib = engine.load_library()
    n = np.asarray([7], np.int32)
    arr = (engine.GainPlan * 1)()
    assert lib.sts_set_gain_plan(syn.h, -1, n.ctypes.data, arr) == STS_EINVAL and lib.sts_set_gain_plan(syn.h, 1, None, arr) == STS_EINVAL
    assert np.array_equal(syn.infer_ids(ids), gained)
    # a plan for another batch: refused, nothing runs, the plan is gone
    for n_set, call in (([8], lambda: syn.infer_ids(ids)), ([7, 7], lambda: syn.infer_ids(ids)), ([7], lambda: syn.infer_batch([ids, ids])),
                        ([7], lambda: syn.infer_ids_stream(sb.synthetic_ids(6, cfg.vocab), 4)), ([7, 3], lambda: syn.infer_batch_stream([ids, ids], 4))):
        syn.set_gain_plan(n_set, [{"gain_db": [-20.0] * n_set[0]}] + [None] * (len(n_set) - 1))
        with pytest.raises(engine.StsError, match="another batch"):
            call()
        assert np.array_equal(syn.infer_ids(ids), plain)
    # a failed run consumes the plan as well; B == 0 / plans == NULL drop it
    syn.set_gain_plan([7], [plan])
    with pytest.raises(engine.StsError):
        syn.infer_ids([0, 1, 2, 3, 4, 5, cfg.vocab])
    assert np.array_equal(syn.infer_ids(ids), plain)
    syn.set_gain_plan([7], [plan]); syn.set_gain_plan(None)
    assert np.array_equal(syn.infer_ids(ids), plain)
    # a run with a gain plan neither reads nor feeds the launch-ahead memo
    assert np.array_equal(syn.infer_ids(ids), plain) and syn.profile()["launch_ahead"] == 1
    syn.set_gain_plan([7], [plan])
    assert np.array_equal(syn.infer_ids(ids), gained) and syn.profile()["launch_ahead"] == 0
    assert np.array_equal(syn.infer_ids(ids), plain) and syn.profile()["launch_ahead"] == 1
    syn.close()
