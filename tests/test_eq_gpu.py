"""Parametric equaliser on the MI355X (sts_eq_apply, sts_set_eq, sts_pool_set_eq, sts_multi_set_eq) against tests/eq_ref.py: the kernels on
caller signals at every chunk, tile and alignment edge; an engine's "wave_eq" tap against the definition applied to the same call's input
tap, for every non-streaming call form and rate; loudness and the limiter behind it through their own checkers; plans, the launch-ahead
memo, a poisoned workspace, refusals.

Tolerances (include/summertts_hip.h sts_set_eq): y within 2^-24 |ref| + 2^-26 max |ref| of the sequential float64 definition, sample by
sample; the PCM within 1 LSB of the cast of float32(ref), at most 1e-3 of an utterance's samples (utterances of 4096 and more) differing.
The cast compares modulo 2^16: a sample on the cast's wrap boundary may land on either side."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eq_ref
import limiter_ref as lref
import loudness_ref as lr
from summertts_amd import engine, synth_blob as sb
from test_loudness_gpu import _close as loud_close          # the loudness checker's own comparison (lufs 0.01, peak exact, gain 1e-4)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STS_EINVAL = -1
_SRC = open(os.path.join(ROOT, "summertts_amd", "csrc", "eq.hip")).read()
THREADS, R = (int(v) for v in re.search(r"constexpr int EQ_THREADS = (\d+), EQ_R = (\d+), EQ_TILE = EQ_THREADS \* EQ_R;", _SRC).groups())
T = THREADS * R

P, LS, HS, HP, LP = eq_ref.PEAK, eq_ref.LOWSHELF, eq_ref.HIGHSHELF, eq_ref.HIGHPASS, eq_ref.LOWPASS
# valid at 8, 16 and 48 kHz; every type between them
BANDS4 = [(HP, 100.0, 0.0, 0.707), (P, 1000.0, 6.0, 2.0), (LS, 300.0, -6.0, 0.7), (P, 3000.0, -9.0, 4.0)]
BANDS4B = [(LP, 3400.0, 0.0, 0.707), (HS, 2000.0, 9.0, 0.9), (P, 250.0, 12.0, 8.0), (HP, 60.0, 0.0, 1.2)]
BANDS1 = [(P, 1000.0, 6.0, 2.0)]


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def test_the_tile_constants_are_the_kernel_files():
    assert (THREADS, R, T) == (eq_ref.THREADS, eq_ref.R, eq_ref.TILE) == (256, 32, 8192)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def _wrapped(a, b):
    return (np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64) + 32768) % 65536 - 32768


def _check(y, pcm, x, rate, bands, what):
    """one utterance: the kernel's y (and pcm, or None) against the definition on x"""
    ref = eq_ref.apply(x, eq_ref.design(rate, bands))
    assert y.size == ref.size == x.size, what
    if ref.size == 0:
        return
    peak = np.abs(ref).max()
    err = np.abs(y.astype(np.float64) - ref)
    tol = 2.0 ** -24 * np.abs(ref) + 2.0 ** -26 * peak
    worst = float((err - 2.0 ** -24 * np.abs(ref)).max() / peak) if peak > 0 else 0.0
    print(f"{what}: N {ref.size} max (|y - ref| - 2^-24 |ref|) / peak = {worst:.3e} (cap 2^-26 = {2.0 ** -26:.3e})")
    assert not np.isnan(y).any() and (err <= tol).all(), (what, int(np.argmax(err - tol)), float((err - tol).max()))
    if pcm is not None:
        assert np.array_equal(pcm, eq_ref.pcm_cast(y)), what                       # the kernel's cast is the cast of its own y
        d = np.abs(_wrapped(pcm, eq_ref.pcm_cast(ref.astype(np.float32))))
        print(f"{what}: PCM samples off the cast of float32(ref): {int((d != 0).sum())} of {d.size}, max {int(d.max())} LSB")
        assert d.max() <= 1, (what, int(d.max()))
        if d.size >= 4096:
            assert (d != 0).mean() <= 1e-3, (what, float((d != 0).mean()))


def _noise(n, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _apply_case(lengths, rate, bands, seed=0, amp=0.3):
    sig = [_noise(n, seed + 17 * b, amp) for b, n in enumerate(lengths)]
    y, pcm = engine.eq_apply(sig, rate, bands)
    for b, x in enumerate(sig):
        _check(y[b], pcm[b], x, rate, bands, f"rate {rate} S {len(bands)} lengths {list(lengths)} utterance {b}")
    return sig, y, pcm


# ---- 1. the kernels on caller signals ---------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 5)


@pytest.mark.parametrize("bands", [BANDS1, BANDS4], ids=["1band", "4bands"])
def test_apply_on_every_chunk_and_tile_edge(bands):
    for k, n in enumerate(LENGTHS):
        _apply_case([n], 16000, bands, seed=k)


@pytest.mark.parametrize("which", range(3))
def test_apply_the_three_filter_sets_at_their_rates(which):
    """the 4-band set at 48 kHz, the q fs / f0 = 6400 corner at 16 kHz, the telephone band at 8 kHz"""
    rate, bands = eq_ref.FILTER_SETS[which]
    _apply_case([2 * T + 5], rate, bands, seed=which)
    _apply_case([T + 1, 1, 2 * T - 3], rate, bands, seed=10 + which)


@pytest.mark.parametrize("bands", [BANDS1, BANDS4B, [(LS, 200.0, -12.0, 0.5), (HS, 5000.0, 6.0, 1.0)], [(LP, 3000.0, 0.0, 1.0), (HP, 300.0, 0.0, 0.7), (P, 50.0, 3.0, 1.0)]],
                         ids=["1", "4", "2", "3"])
def test_apply_a_batch_whose_utterances_start_unaligned(bands):
    """B = 3 with (T + 1, 1, 2T - 3): no utterance after the first starts on a 16-byte boundary; 1 to 4 sections; an empty utterance"""
    _apply_case([T + 1, 1, 2 * T - 3], 16000, bands, seed=3)
    _apply_case([5, 0, R + 2, 3], 16000, bands, seed=4)


def test_apply_a_signal_that_wraps_the_cast():
    x = _noise(T + 77, 5)
    x[::53] = np.float32(1.3)
    x[7::211] = np.float32(-2.7)
    bands = [(P, 1000.0, 6.0, 1.0)]
    y, pcm = engine.eq_apply([x], 16000, bands)
    _check(y[0], pcm[0], x, 16000, bands, "wrapping")
    over = np.abs(y[0]) * 32737.0 > 32767.0
    assert over.sum() > 100
    v = np.trunc(y[0].astype(np.float32) * np.float32(32737.0)).astype(np.int64)
    assert np.array_equal(pcm[0].astype(np.int64), (v + 32768) % 65536 - 32768) and (np.sign(pcm[0][over]) != np.sign(y[0][over])).any()


def test_no_leakage_across_utterances_bit_for_bit():
    x = _noise(T + 1, 6)
    big = (1e6 * np.random.default_rng(7).standard_normal(2 * T - 3)).astype(np.float32)
    for bands in (BANDS1, BANDS4, eq_ref.FILTER_SETS[1][1]):
        y1, p1 = engine.eq_apply([x], 16000, bands)
        y2, p2 = engine.eq_apply([x, big], 16000, bands)
        y3, p3 = engine.eq_apply([big, x], 16000, bands)
        assert y1[0].tobytes() == y2[0].tobytes() == y3[1].tobytes() and p1[0].tobytes() == p2[0].tobytes() == p3[1].tobytes()
        assert np.isfinite(y2[1]).all() and y2[1].tobytes() == y3[0].tobytes()


def test_a_sine_at_the_peak_gains_six_decibels():
    n = np.arange(16000)
    x = (0.25 * np.sin(2.0 * np.pi * 1000.0 * n / 16000.0)).astype(np.float32)
    y, _ = engine.eq_apply([x], 16000, [(P, 1000.0, 6.0, 2.0)])
    ratio = np.sqrt(np.mean(y[0][8000:].astype(np.float64) ** 2)) / np.sqrt(np.mean(x[8000:].astype(np.float64) ** 2))
    assert abs(ratio - 10.0 ** (6.0 / 20.0)) <= 1e-4, ratio


def test_a_high_pass_removes_a_constant():
    x = np.full(16000, 0.5, np.float32)
    y, pcm = engine.eq_apply([x], 16000, [(HP, 80.0, 0.0, 0.707)])
    assert np.abs(y[0][:10]).max() > 0.3 and np.abs(y[0][-1000:]).max() < 1e-6 and not pcm[0][-1000:].any()


def test_each_output_is_optional_and_no_sentinel_survives():
    lengths = [T + 1, 1, 2 * T - 3]
    sig = [_noise(n, 8 + b, amp=0.05) for b, n in enumerate(lengths)]
    y, pcm = engine.eq_apply(sig, 16000, BANDS4)
    for b in range(3):
        assert not np.isnan(y[b]).any() and (np.abs(pcm[b].astype(np.int32)) < 0x7FFF).all()
    y_only, p_none = engine.eq_apply(sig, 16000, BANDS4, want_pcm=False)
    y_none, p_only = engine.eq_apply(sig, 16000, BANDS4, want_y=False)
    for b in range(3):
        assert y_only[b].tobytes() == y[b].tobytes() and p_only[b].tobytes() == pcm[b].tobytes()
        assert (p_none[b] == 0x7FFF).all() and np.isnan(y_none[b]).all()           # the caller's buffers, untouched
    lib = engine.load_library()
    lens = np.asarray(lengths, np.int64)
    x = np.concatenate(sig)
    n, arr = engine._eq_bands(BANDS4)
    assert lib.sts_eq_apply(0, x.ctypes.data, lens.ctypes.data, 3, 16000, n, arr, None, None) == 0
    assert lib.sts_eq_apply(0, None, lens.ctypes.data, 3, 16000, n, arr, None, None) == STS_EINVAL
    assert lib.sts_eq_apply(0, x.ctypes.data, lens.ctypes.data, 3, 8000, *engine._eq_bands([(P, 3700.0, 0.0, 1.0)]), None, None) == STS_EINVAL


# ---- 2. the engine ----------------------------------------------------------------------------------------------------------------------
LONG = (40, 9, 55)


def _tiny(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    return cfg, sb.make_blob(cfg, seed)


@pytest.fixture(scope="module")
def model():
    cfg, blob = _tiny("mbb_fix", 7)
    return cfg, blob, [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in LONG]


def _infer_ids_c(syn, ids, sid=0, ls=1.0):
    """sts_infer_ids itself (the class goes through sts_run_batch + sts_copy_pcm_host)"""
    a = np.ascontiguousarray(ids, dtype=np.int32)
    p, n = C.POINTER(C.c_int16)(), C.c_int32()
    rc = syn.lib.sts_infer_ids(syn.h, a.ctypes.data, a.size, sid, ls, C.byref(p), C.byref(n))
    assert rc == 0, syn.lib.sts_last_error()
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    syn.lib.sts_free(p)
    return out


def _split(flat, counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert flat.size == off[-1], (flat.size, int(off[-1]))
    return [flat[off[b]:off[b + 1]] for b in range(len(counts))]


def _engine_case(syn, call, rate, bands, in_tap, what, downstream=False):
    """call() -> list of per-utterance PCM; checks "wave_eq" against the definition on the call's own input tap, utterance by utterance"""
    syn.set_record_taps(True)
    pcm = call()
    x, y = syn.tap(in_tap)[0], syn.tap("wave_eq")[0]
    syn.set_record_taps(False)
    counts = [p.size for p in pcm]
    xs, ys = _split(x, counts), _split(y, counts)
    for b in range(len(pcm)):
        _check(ys[b], None, xs[b], rate, bands, f"{what} utterance {b}")
        if not downstream:
            assert np.array_equal(pcm[b], eq_ref.pcm_cast(ys[b])), (what, b)
    again = call()                                                                  # without taps
    assert all(np.array_equal(a, b) for a, b in zip(again, pcm)), what
    return pcm, xs, ys


@pytest.mark.parametrize("rate", [16000, 8000, 48000])
def test_every_whole_utterance_form_filters_its_own_input(model, rate):
    cfg, blob, ids = model
    bands = BANDS4
    in_tap = "wave" if rate == 16000 else "wave_out"
    plain = engine.Synthesizer(blob)
    plain.set_conv_mode(6)
    plain.set_output_rate(rate)
    want_plain = plain.infer_batch(ids)
    plain.close()
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    syn.set_eq(bands)
    got = syn.get_eq()
    assert [b[0] for b in got] == [b[0] for b in bands] and np.allclose([b[1:] for b in got], [b[1:] for b in bands], rtol=1e-6)
    one, _, _ = _engine_case(syn, lambda: [_infer_ids_c(syn, ids[2])], rate, bands, in_tap, f"infer_ids {rate}")
    assert one[0].size == want_plain[2].size and not np.array_equal(one[0], want_plain[2])
    batch, _, _ = _engine_case(syn, lambda: syn.infer_batch(ids), rate, bands, in_tap, f"batch {rate}")
    assert [p.size for p in batch] == [p.size for p in want_plain]
    assert np.array_equal(batch[2], one[0])                                         # the same utterance alone and third in a pack

    def run_then_copy():
        n_out = syn.run_batch(ids)
        return _split(syn.pcm_host(), n_out)
    rb, _, _ = _engine_case(syn, run_then_copy, rate, bands, in_tap, f"run_batch {rate}")
    assert all(np.array_equal(a, b) for a, b in zip(rb, batch))
    join = {"gap_frames": [0, 6], "lead_frames": 3, "trail_frames": 2, "fade_ms": 2.0}
    _engine_case(syn, lambda: [syn.infer_joined(ids, join=join)], rate, bands, "wave_join" if rate == 16000 else "wave_out", f"joined {rate}")
    # the pool: one setting for every request (its engines choose their conv kernels themselves, as a default engine does)
    ref = engine.Synthesizer(blob)
    ref.set_output_rate(rate)
    want_off = [ref.infer_ids(a) for a in ids]
    ref.set_eq(bands)
    want_on = [ref.infer_ids(a) for a in ids]
    ref.close()
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=1)
    pool.set_output_rate(rate)
    pool.set_eq(bands)
    tickets = [pool.submit(a) for a in ids]
    for b, t in enumerate(tickets):
        assert np.array_equal(pool.wait(t), want_on[b]), (rate, b)
    with pytest.raises(engine.StsError):
        pool.submit_stream(ids[0], 4, lambda *a: False)
    with pytest.raises(engine.StsError):
        pool.set_eq([(P, 10.0, 0.0, 1.0)])
    assert np.array_equal(pool.wait(pool.submit(ids[1])), want_on[1])               # a refused set changed nothing
    pool.set_eq(None)
    assert np.array_equal(pool.wait(pool.submit(ids[1])), want_off[1])
    pool.close()
    # 0 bands afterwards: the PCM of an engine that never had an EQ, bit for bit
    syn.set_eq([])
    assert syn.get_eq() == []
    assert all(np.array_equal(a, b) for a, b in zip(syn.infer_batch(ids), want_plain))
    syn.close()


def test_one_band_and_the_launch_ahead_memo(model):
    cfg, blob, ids = model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_eq(BANDS1)
    first = syn.infer_ids(ids[0])
    second = syn.infer_ids(ids[0])
    assert syn.profile()["launch_ahead"] == 1 and np.array_equal(first, second)
    got, _, _ = _engine_case(syn, lambda: [syn.infer_ids(ids[0])], 16000, BANDS1, "wave", "one band")
    assert np.array_equal(got[0], first)
    b1 = syn.infer_batch(ids)
    b2 = syn.infer_batch(ids)                                                       # a batch launched from the memo
    assert all(np.array_equal(a, b) for a, b in zip(b1, b2)) and np.array_equal(b1[0], first)
    syn.close()


def test_loudness_and_the_limiter_read_the_equalised_signal(model):
    cfg, blob, ids = model
    rate = 16000
    cut = [(LS, 1000.0, -12.0, 0.7)]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_loudness(engine.LOUD_MEASURE, -23.0, -1.0)
    syn.infer_batch(ids)
    flat = syn.loudness().copy()
    syn.set_eq(cut)
    # mode 1: measures the EQ's output, the EQ writes the PCM
    pcm, xs, ys = _engine_case(syn, lambda: syn.infer_batch(ids), rate, cut, "wave", "loudness 1")
    res = syn.loudness()
    assert len(res) == 3
    for b in range(3):
        want = lr.loudness(ys[b], rate, -23.0, -1.0)
        loud_close(res[b], want, f"measure {b}")
        if np.isfinite(want["lufs"]):
            assert abs(float(res[b]["lufs"]) - float(flat[b]["lufs"])) > 0.1, (b, res[b], flat[b])   # the stage really is in front
    assert any(np.isfinite(float(r["lufs"])) for r in res)
    # mode 2: one gain per utterance on the EQ's output
    syn.set_loudness(engine.LOUD_NORMALIZE, -23.0, -1.0)
    pcm, xs, ys = _engine_case(syn, lambda: syn.infer_batch(ids), rate, cut, "wave", "loudness 2", downstream=True)
    res = syn.loudness()
    for b in range(3):
        loud_close(res[b], lr.loudness(ys[b], rate, -23.0, -1.0), f"normalize {b}")
        assert np.array_equal(pcm[b], lr.normalize(ys[b], res[b]["gain"])), b
    # the limiter alone, at another rate: limits the EQ's output of the resampled wave
    syn.set_loudness(engine.LOUD_OFF)
    syn.set_output_rate(48000)
    lim = dict(gain_db=30.0, ceiling_dbfs=-6.0, lookahead_ms=2.0)
    syn.set_limiter(engine.LIMITER_ON, **lim)
    syn.set_record_taps(True)
    pcm = syn.infer_batch(ids)
    x, y, ylim = syn.tap("wave_out")[0], syn.tap("wave_eq")[0], syn.tap("wave_lim")[0]
    syn.set_record_taps(False)
    counts = [p.size for p in pcm]
    H, c, G = engine.limiter_design(48000, **lim)
    g0 = lref.static_gain(G)
    st = syn.limiter()
    for b, (xb, yb, lb) in enumerate(zip(_split(x, counts), _split(y, counts), _split(ylim, counts))):
        _check(yb, None, xb, 48000, cut, f"limiter {b}")
        want, s, S = lref.limit(yb, g0, H, c)
        assert lb.tobytes() == want.tobytes() and np.array_equal(pcm[b], lref.pcm_cast(want)), b
        assert st[b]["limited"] == lref.stats(want, s, S, g0, H)["limited"]
    assert st[2]["limited"] > 0
    # both behind it
    syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -1.0)
    syn.set_record_taps(True)
    pcm = syn.infer_batch(ids)
    y, ylim = syn.tap("wave_eq")[0], syn.tap("wave_lim")[0]
    syn.set_record_taps(False)
    res = syn.loudness()
    for b, (yb, lb) in enumerate(zip(_split(y, counts), _split(ylim, counts))):
        loud_close(res[b], dict(lr.loudness(yb, 48000, -20.0, -1.0), gain=res[b]["gain"]), f"both {b}")
        want = lref.limit(yb, lref.static_gain(G, res[b]["gain"]), H, c)[0]
        assert lb.tobytes() == want.tobytes() and np.array_equal(pcm[b], lref.pcm_cast(want)), b
    syn.close()


def test_composition_with_a_gain_plan_and_a_duration_plan():
    cfg, blob = _tiny("ms_hifigan_sdp", 5)
    lens = (7, 12)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    hop = syn.info.samples_per_frame
    syn.set_eq(BANDS4B)
    db = np.zeros(12, np.float32); db[2] = -np.inf; db[5] = 6.0
    for rate, in_tap in ((16000, "wave_gain"), (8000, "wave_out")):
        syn.set_output_rate(rate)
        syn.set_duration_plan(lens, [{"target_frames": 40}, None])
        syn.set_gain_plan(lens, [None, {"gain_db": db, "ramp_ms": 2.0}])
        syn.set_record_taps(True)
        pcm = syn.infer_batch(ids, [0, 1])
        x, y = syn.tap(in_tap)[0], syn.tap("wave_eq")[0]
        dur = syn.durations(sum(lens))
        syn.set_record_taps(False)
        assert int(dur[:7].sum()) == 40
        counts = [p.size for p in pcm]
        if rate == 16000:
            assert counts == [40 * hop, max(1, int(dur[7:].sum())) * hop]
        for b, (xb, yb) in enumerate(zip(_split(x, counts), _split(y, counts))):
            _check(yb, None, xb, rate, BANDS4B, f"plans {rate} utterance {b}")
            assert np.array_equal(pcm[b], eq_ref.pcm_cast(yb)), (rate, b)
    # the plans applied to that call only; the EQ persists
    syn.set_output_rate(16000)
    _engine_case(syn, lambda: syn.infer_batch(ids, [0, 1]), 16000, BANDS4B, "wave", "after the plans")
    syn.close()


@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFFFFFFF, 0x7BFF7BFF], ids=hex)
def test_a_poisoned_workspace_changes_nothing(model, pattern):
    cfg, blob, ids = model

    def run(poison):
        syn = engine.Synthesizer(blob)
        if poison:
            syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
        syn.set_eq(BANDS4)
        out = [b"".join(p.tobytes() for p in syn.infer_batch(ids))]
        syn.set_record_taps(True)
        out.append(b"".join(p.tobytes() for p in syn.infer_batch(ids)))
        out.append(syn.tap("wave_eq").tobytes())
        syn.set_record_taps(False)
        out.append(syn.infer_ids(ids[1]).tobytes())
        out.append(syn.infer_joined(ids, join={"gap_frames": [3, 0], "fade_ms": 1.0}).tobytes())
        syn.set_output_rate(24000)
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
        syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -1.0)
        out.append(b"".join(p.tobytes() for p in syn.infer_batch(ids)))
        out.append(syn.loudness().tobytes() + syn.limiter().tobytes())
        assert (syn.profile()["poison_bytes"] > 0) == bool(poison)
        syn.set_output_rate(16000); syn.set_limiter(engine.LIMITER_OFF); syn.set_loudness(engine.LOUD_OFF); syn.set_eq(None)
        out.append(syn.infer_batch(ids)[2].tobytes())                                      # and a plain call behind them
        syn.close()
        return out

    want = run(False)
    assert want[0] == want[1]
    assert run(True) == want


def test_refusals(model):
    cfg, blob, ids = model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    want = syn.infer_ids(ids[1])
    want_stream = np.concatenate(syn.infer_ids_stream(ids[1], 4)[0])
    syn.set_eq(BANDS4)
    eqd = syn.infer_ids(ids[1])
    assert not np.array_equal(eqd, want)
    # an invalid set changes nothing
    for bad in ([(P, 10.0, 0.0, 1.0)], [(P, 1000.0, 25.0, 1.0)], [(P, 1000.0, 0.0, 0.05)], [(0, 1000.0, 0.0, 1.0)], [(6, 1000.0, 0.0, 1.0)],
                [(P, float("nan"), 0.0, 1.0)], [(HP, 1000.0, float("inf"), 1.0)], [(P, 20.0, 0.0, 8.0 + 1e-3)], [(P, 7300.0, 0.0, 1.0)],
                [(P, 1000.0, 0.0, 1.0)] * 5, BANDS4[:3] + [(P, 19.0, 0.0, 1.0)]):
        with pytest.raises(engine.StsError):
            syn.set_eq(bad)
        assert [b[0] for b in syn.get_eq()] == [b[0] for b in BANDS4], bad
    assert np.array_equal(syn.infer_ids(ids[1]), eqd)
    # streaming is refused while bands are set, with the reason, and works again afterwards
    with pytest.raises(engine.StsError, match="finite halo"):
        syn.infer_ids_stream(ids[1], 4)
    with pytest.raises(engine.StsError, match="equaliser"):
        syn.infer_batch_stream(ids, 4)
    assert np.array_equal(syn.infer_ids(ids[1]), eqd)
    syn.set_eq([])
    assert np.array_equal(np.concatenate(syn.infer_ids_stream(ids[1], 4)[0]), want_stream)
    chunks, _ = syn.infer_batch_stream(ids, 4)
    assert np.array_equal(np.concatenate(chunks[1]), want_stream)
    # a band that fits 16 kHz and not 8 kHz (0.45 x 8000 = 3600): accepted now, refused by the run after the rate changed
    syn.set_eq([(P, 3700.0, 3.0, 1.0)])
    ok16 = syn.infer_ids(ids[1])
    syn.set_output_rate(8000)
    with pytest.raises(engine.StsError, match="output rate"):
        syn.infer_ids(ids[1])
    assert syn.profile()["samples"] == 0                                            # nothing was enqueued
    with pytest.raises(engine.StsError):
        syn.infer_batch(ids)
    with pytest.raises(engine.StsError):
        syn.set_eq([(P, 3700.0, 3.0, 1.0)])                                         # and a set at this rate refuses it as well
    syn.set_output_rate(16000)
    assert np.array_equal(syn.infer_ids(ids[1]), ok16)
    syn.set_eq(None)
    assert np.array_equal(syn.infer_ids(ids[1]), want)
    syn.close()


def test_multi_set_eq_reaches_every_engine(model):
    cfg, blob, ids = model
    lens = [len(a) for a in ids]
    syn = engine.Synthesizer(blob)
    plain = syn.infer_batch(ids)
    # two engines on one device: each runs its shard as one batch
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    shard = md.shard_of(lens)
    md.set_eq(BANDS4)
    multi = md.infer_batch(ids)
    with pytest.raises(engine.StsError):
        md.set_eq([(P, 10.0, 0.0, 1.0)])
    still = md.infer_batch(ids)                                                     # persists; a refused set changed nothing
    md.set_eq(None)
    off = md.infer_batch(ids)
    md.close()
    syn.set_eq(BANDS4)
    for sh in sorted(set(int(v) for v in shard)):
        mem = [b for b in range(3) if int(shard[b]) == sh]
        ref = syn.infer_batch([ids[b] for b in mem])
        for k, b in enumerate(mem):
            assert np.array_equal(multi[b], ref[k]) and np.array_equal(still[b], ref[k]) and np.array_equal(off[b], plain[b]), (sh, b)
            assert not np.array_equal(multi[b], plain[b])
    syn.close()
