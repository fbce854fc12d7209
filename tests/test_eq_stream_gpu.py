"""The equaliser in a stream on the MI355X (sts_set_eq_streaming, sts_eq_apply_chunked; DESIGN.md 9j "streamed").

1. The stream-mode kernels on caller signals against the whole-call kernels (sts_eq_apply) on the same input: y and PCM bit for bit for
   every step list that crosses a chunk or a tile edge, with the window widened by `back` on either side, every step's WHOLE window
   (the re-presented part included) against the whole call's slice; and y against tests/eq_stream_ref.py, the float64 restatement.
2. The engine: the concatenated chunks of every streaming form against the corresponding whole call, bit for bit with the conv mode
   pinned, on an utterance longer than two tiles.

Nothing here has a tolerance: the stream evaluates the recurrence in the whole call's order, so every comparison is of bytes.  (Streams
do not report limiter statistics -- sts_get_limiter is empty after one -- so the limiter cases compare the PCM.)"""
import ctypes as C

import numpy as np
import pytest

import eq_ref
import eq_stream_ref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

R, T = eq_ref.R, eq_ref.TILE
P, LS, HS, HP, LP = eq_ref.PEAK, eq_ref.LOWSHELF, eq_ref.HIGHSHELF, eq_ref.HIGHPASS, eq_ref.LOWPASS
BANDS4 = [(HP, 100.0, 0.0, 0.707), (P, 1000.0, 6.0, 2.0), (LS, 300.0, -6.0, 0.7), (P, 3000.0, -9.0, 4.0)]     # valid at 8, 16 and 48 kHz
BANDS1 = [(P, 1000.0, 6.0, 2.0)]
BACKS = (0, 7, 1920)


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _noise(n, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _step_lists(N):
    return {"every sample of the first 70": list(range(0, 71)),
            "chunk and tile edges": [0] + [c for c in (R - 1, R, R + 1, 2 * R + 5, T - 1, T, T + 1, 2 * T + 5)],
            "one step": [0],
            "steps of 1000": list(range(0, max(N, 1), 1000))}


_whole_cache = {}


def _whole(sig, rate, bands):
    """sts_eq_apply on the same signals, computed once per input"""
    key = (tuple(s.tobytes() for s in sig), rate, tuple(bands))
    if key not in _whole_cache:
        _whole_cache[key] = engine.eq_apply(sig, rate, bands)
    return _whole_cache[key]


def _chunked_case(sig, rate, bands, bounds, back, what):
    """-> (y, pcm): the chunked call's outputs, checked bit for bit against the whole call, window by window"""
    wy, wp = _whole(sig, rate, bands)
    y, pcm, wins = engine.eq_apply_chunked(sig, rate, bands, bounds, back)
    for b in range(len(sig)):
        assert y[b].tobytes() == wy[b].tobytes(), (what, b, "y")
        assert pcm[b].tobytes() == wp[b].tobytes(), (what, b, "pcm")
        assert not np.isnan(y[b]).any()
    for k, row in enumerate(wins):
        for b, w in enumerate(row):
            if w is None:
                assert sig[b].size <= bounds[k], (what, k, b)
                continue
            a0, v = w
            assert v.tobytes() == wy[b][a0:a0 + v.size].tobytes(), (what, "window", k, b, a0, v.size)
    return y, pcm


# ---- 1. the kernels on caller signals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back", BACKS)
@pytest.mark.parametrize("N", [2 * T + 5, 3 * T + 5])
def test_chunked_equals_the_whole_call_at_every_edge(N, back):
    """N = 3T + 5: the single step runs over more than two tiles"""
    x = _noise(N, N)
    for name, bounds in _step_lists(N).items():
        for bands in (BANDS1, BANDS4):
            _chunked_case([x], 16000, bands, bounds, back, f"N {N} back {back} {name} S {len(bands)}")


@pytest.mark.parametrize("which", range(3))
def test_chunked_the_three_filter_sets_and_the_float64_restatement(which):
    """every section count of each set; y of the kernels against tests/eq_stream_ref.py within the whole call's own bound"""
    rate, bands = eq_ref.FILTER_SETS[which]
    N = 2 * T + 5
    x = _noise(N, 40 + which)
    for S in range(1, len(bands) + 1):
        for name, bounds in _step_lists(N).items():
            y, _ = _chunked_case([x], rate, bands[:S], bounds, 7, f"set {which} S {S} {name}")
        ref, _ = eq_stream_ref.chunked(x, eq_ref.design(rate, bands[:S]), [0, 1000, T + 3], 7)
        err = np.abs(y[0].astype(np.float64) - ref)
        # (the header's bound of the kernels against the definition; here both sides evaluate one order and differ by the float32
        # rounding and the fused multiply-adds only)
        assert (err <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -26 * np.abs(ref).max()).all(), (which, S, float(err.max()))


@pytest.mark.parametrize("N", [1, 2, R, T])
def test_chunked_short_signals(N):
    x = _noise(N, 100 + N)
    for back in BACKS:
        for bounds in ([0], [0, 1], list(range(0, N, 7)), [0, N - 1] if N > 1 else [0], [0, N + 5]):
            _chunked_case([x], 16000, BANDS4, bounds, back, f"N {N} back {back} bounds {bounds[:4]}")


@pytest.mark.parametrize("back", BACKS)
def test_chunked_batch_state_is_per_utterance(back):
    """B = 3 with (T + 1, 1, 2T - 3) and 1000-sample steps: utterance 1 leaves after step 0, no later utterance starts aligned; utterance 0
    next to a neighbour at amplitude 1e6 equals its B = 1 result bit for bit"""
    lengths = (T + 1, 1, 2 * T - 3)
    sig = [_noise(n, 7 + b) for b, n in enumerate(lengths)]
    bounds = list(range(0, 2 * T, 1000))
    y, pcm = _chunked_case(sig, 16000, BANDS4, bounds, back, f"batch back {back}")
    alone_y, alone_p = _chunked_case(sig[:1], 16000, BANDS4, bounds, back, "alone")
    big = (1e6 * np.random.default_rng(9).standard_normal(2 * T - 3)).astype(np.float32)
    y2, p2, _ = engine.eq_apply_chunked([sig[0], sig[1], big], 16000, BANDS4, bounds, back)
    assert y2[0].tobytes() == alone_y[0].tobytes() == y[0].tobytes() and p2[0].tobytes() == alone_p[0].tobytes()
    assert np.isfinite(y2[2]).all()
    y3, p3, _ = engine.eq_apply_chunked([big, sig[0]], 16000, BANDS4, bounds, back)
    assert y3[1].tobytes() == alone_y[0].tobytes() and p3[1].tobytes() == alone_p[0].tobytes()


def test_chunked_a_signal_that_wraps_the_cast():
    x = _noise(T + 77, 5)
    x[::53] = np.float32(1.3)
    x[7::211] = np.float32(-2.7)
    bands = [(P, 1000.0, 6.0, 1.0)]
    y, pcm = _chunked_case([x], 16000, bands, list(range(0, T + 77, 1000)), 7, "wrapping")
    over = np.abs(y[0]) * 32737.0 > 32767.0
    assert over.sum() > 100 and (np.sign(pcm[0][over]) != np.sign(y[0][over])).any()


def test_chunked_sentinels_and_refusals():
    """behind every output: the binding's buffers start as NaN / 0x7FFF and hold one more element than the kernels may write"""
    lengths = [T + 1, 1, 2 * T - 3]
    sig = [_noise(n, 8 + b, amp=0.05) for b, n in enumerate(lengths)]
    lib = engine.load_library()
    lens = np.asarray(lengths, np.int64)
    total = int(lens.sum())
    x = np.concatenate(sig)
    n, arr = engine._eq_bands(BANDS4)
    bnd = np.asarray([0, 1000, T + 5], np.int64)
    back = 7
    wtotal = sum(min(N, c1 + back) - max(0, c0 - back) for c0, c1 in ((0, 1000), (1000, T + 5), (T + 5, 1 << 40)) for N in lengths if N > c0)
    y = np.full(total + 8, np.nan, np.float32)
    pcm = np.full(total + 8, 0x7FFF, np.int16)
    wy = np.full(wtotal + 8, np.nan, np.float32)
    woff = np.full(9, -2, np.int64)
    args = lambda **k: (0, x.ctypes.data, lens.ctypes.data, 3, 16000, n, arr, k.get("bounds", bnd.ctypes.data), k.get("steps", 3), k.get("back", back),
                        y.ctypes.data, pcm.ctypes.data, wy.ctypes.data, k.get("cap", wtotal), woff.ctypes.data)
    assert lib.sts_eq_apply_chunked(*args()) == 0, lib.sts_last_error()
    assert not np.isnan(y[:total]).any() and np.isnan(y[total:]).all()
    assert (np.abs(pcm[:total].astype(np.int32)) < 0x7FFF).all() and (pcm[total:] == 0x7FFF).all()
    assert not np.isnan(wy[:wtotal]).any() and np.isnan(wy[wtotal:]).all()
    assert woff[0] == 0 and woff[1] == 1000 + back and list(woff[[4, 6, 7]]) == [-1, -1, -1] and (woff[[0, 1, 2, 3, 5, 8]] >= 0).all()
    wy_all, wp_all = engine.eq_apply(sig, 16000, BANDS4)
    assert y[:total].tobytes() == np.concatenate(wy_all).tobytes() and pcm[:total].tobytes() == np.concatenate(wp_all).tobytes()
    # each output is optional
    assert lib.sts_eq_apply_chunked(0, x.ctypes.data, lens.ctypes.data, 3, 16000, n, arr, bnd.ctypes.data, 3, back, None, None, None, 0, None) == 0
    STS_EINVAL = -1
    assert lib.sts_eq_apply_chunked(*args(cap=wtotal - 1)) == STS_EINVAL
    assert lib.sts_eq_apply_chunked(*args(back=2049)) == STS_EINVAL and lib.sts_eq_apply_chunked(*args(back=-1)) == STS_EINVAL
    assert lib.sts_eq_apply_chunked(*args(steps=0)) == STS_EINVAL
    for bad in ([1, 5, 9], [0, 5, 5], [0, 9, 5]):
        b = np.asarray(bad, np.int64)
        assert lib.sts_eq_apply_chunked(*args(bounds=b.ctypes.data)) == STS_EINVAL, bad


# ---- 2. the engine ----------------------------------------------------------------------------------------------------------------------
LONG = (40, 9, 55)


@pytest.fixture(scope="module")
def model():
    cfg = sb.tiny_cfg("mbb_fix")
    blob = sb.make_blob(cfg, 7)
    return cfg, blob, [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in LONG]


def _syn(blob, rate=16000, bands=BANDS4, streaming=True, lim=False):
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    syn.set_eq(bands)
    syn.set_eq_streaming(streaming)
    if lim:
        syn.set_limiter(engine.LIMITER_ON, 20.0, -3.0, 5.0)        # (5 ms: the widest look-ahead the tests of the limiter use)
    return syn


def _cat(chunks):
    return np.concatenate(chunks) if len(chunks) else np.zeros(0, np.int16)


def _stream(syn, ids, chunk):
    offs = []
    chunks, _ = syn.infer_ids_stream(ids, chunk, on_chunk=lambda pcm, off, t: offs.append((off, pcm.size)) and False)
    pos = 0
    for off, n in offs:
        assert off == pos
        pos += n
    return _cat(chunks)


@pytest.mark.parametrize("lim", [False, True], ids=["cast", "limiter"])
@pytest.mark.parametrize("rate", [16000, 8000, 48000])
def test_a_streamed_utterance_is_the_whole_call_for_every_chunk_size(model, rate, lim):
    cfg, blob, ids = model
    syn = _syn(blob, rate, lim=lim)
    whole = syn.infer_ids(ids[2])
    assert whole.size * 16000 // rate > 2 * T, whole.size             # more than two tiles at 16 kHz: the carry crosses tile boundaries
    if rate == 48000:
        assert whole.size > 6 * T
    halo = syn.stream_halo_frames()
    syn.set_eq_streaming(False)
    assert syn.stream_halo_frames() == halo                         # the switch does not change the halo
    syn.set_eq_streaming(True)
    plain = engine.Synthesizer(blob)
    plain.set_conv_mode(6)
    plain.set_output_rate(rate)
    if lim:
        plain.set_limiter(engine.LIMITER_ON, 20.0, -3.0, 5.0)
    assert plain.stream_halo_frames() == halo
    assert not np.array_equal(plain.infer_ids(ids[2]), whole)        # the EQ really is in the chain
    plain.close()
    for chunk in (1, 4, 7, 100000):
        got = _stream(syn, ids[2], chunk)
        assert got.size == whole.size, (rate, lim, chunk, got.size, whole.size)
        d = np.abs(got.astype(np.int64) - whole.astype(np.int64))
        print(f"rate {rate} limiter {lim} chunk {chunk}: {int((d != 0).sum())} of {d.size} samples differ, max {int(d.max())}")
        assert np.array_equal(got, whole), (rate, lim, chunk, int(np.argmax(d != 0)))
    assert len(syn.limiter()) == 0                                   # (streams report no limiter statistics)
    syn.close()


def test_a_gain_plan_and_a_duration_plan_in_front_of_the_streamed_eq(model):
    cfg, blob, ids = model
    n = len(ids[2])
    db = np.zeros(n, np.float32); db[3] = -np.inf; db[20] = 6.0; db[40] = -9.0
    for rate in (16000, 8000):
        syn = _syn(blob, rate)

        def plans():
            syn.set_duration_plan([n], [{"target_frames": 300}])
            syn.set_gain_plan([n], [{"gain_db": db, "ramp_ms": 2.0}])
        plans()
        whole = syn.infer_ids(ids[2])
        assert whole.size * 16000 // rate == 300 * syn.info.samples_per_frame > 2 * T
        for chunk in (1, 7, 100000):
            plans()
            assert np.array_equal(_stream(syn, ids[2], chunk), whole), (rate, chunk)
        unplanned = syn.infer_ids(ids[2])
        assert unplanned.size != whole.size and np.array_equal(_stream(syn, ids[2], 4), unplanned)      # the plans applied to their call only
        syn.close()


@pytest.mark.parametrize("rate,lim", [(16000, False), (48000, True)])
def test_a_batched_stream_and_a_stopped_utterance(model, rate, lim):
    cfg, blob, ids = model
    syn = _syn(blob, rate, lim=lim)
    want = syn.infer_batch(ids)
    for chunk in (4, 7):
        chunks, _ = syn.infer_batch_stream(ids, chunk)
        for b in range(3):
            assert np.array_equal(_cat(chunks[b]), want[b]), (rate, chunk, b)
    # utterance 0 stopped by its callback at chunk 2: windows shift, the others' state does not
    seen = [0, 0, 0]

    def on_chunk(u, pcm, off, t):
        seen[u] += 1
        return u == 0 and seen[0] == 3
    got, _ = syn.infer_batch_stream(ids, 4, on_chunk=on_chunk)
    assert len(got[0]) == 3 and np.array_equal(_cat(got[0]), want[0][:_cat(got[0]).size])
    for b in (1, 2):
        assert np.array_equal(_cat(got[b]), want[b]), b
    syn.close()


@pytest.mark.parametrize("rate,lim", [(16000, False), (8000, True), (48000, False)])
def test_a_joined_stream_with_silence_only_steps(model, rate, lim):
    cfg, blob, ids = model
    join = {"gap_frames": [30, 12], "lead_frames": 9, "trail_frames": 11, "fade_ms": 2.0}
    syn = _syn(blob, rate, lim=lim)
    want = syn.infer_joined(ids, join=join)
    assert want.size * 16000 // rate > 2 * T
    for chunk in (4, 7, 100000):                                     # (4 and 7 < the gaps: some steps hold silence only)
        got = syn.infer_joined_stream(ids, chunk, join=join)
        pos = 0
        for off, pcm in got:
            assert off == pos
            pos += pcm.size
        assert np.array_equal(_cat([p for _, p in got]), want), (rate, lim, chunk)
    syn.close()


def test_the_pool_streams_with_the_switch_on(model):
    cfg, blob, ids = model
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=4)
    pool.set_eq(BANDS4)
    with pytest.raises(engine.StsError, match="finite halo"):
        pool.submit_stream(ids[0], 4, lambda *a: False)
    pool.set_eq_streaming(True)
    want = [pool.wait(pool.submit(a)) for a in ids]
    chunks = [[] for _ in ids]
    tickets = [pool.submit_stream(a, 8, (lambda b: lambda pcm, off: chunks[b].append(pcm.copy()) and False)(b)) for b, a in enumerate(ids)]
    for b, t in enumerate(tickets):
        assert pool.wait(t) == sum(c.size for c in chunks[b]) == want[b].size, b
        d = np.abs(_cat(chunks[b]).astype(np.int64) - want[b].astype(np.int64))
        print(f"pool request {b}: {int((d != 0).sum())} of {d.size} samples differ from submit, max {int(d.max())}")
        assert np.array_equal(_cat(chunks[b]), want[b]), b
    pool.set_eq_streaming(False)
    with pytest.raises(engine.StsError, match="equaliser"):
        pool.submit_stream(ids[0], 4, lambda *a: False)
    pool.close()


def test_a_step_decoded_twice_starts_from_the_same_state(model):
    """STS_DBG_STREAM_RETRY_STEP under conv math 3 (the conv mode pinned: the repeat computes what the first attempt did)"""
    cfg, blob, ids = model
    for rate, lim in ((16000, False), (48000, True)):
        syn = _syn(blob, rate, lim=lim)
        syn.set_conv_math("f16x2")
        whole = syn.infer_ids(ids[2])
        dur = syn.durations(len(ids[2]))
        steps = (int(dur.sum()) + 6) // 7
        assert steps > 3
        for k in (1, steps - 1):
            syn.set_conv_math("f16x2")                               # (two repeats in a row would pin the engine to split-bf16)
            before = syn.profile()["conv_math_fallbacks"]
            syn.debug_set("stream_retry_step", k)
            got = _stream(syn, ids[2], 7)
            syn.debug_set("stream_retry_step", -1)
            assert syn.profile()["conv_math_fallbacks"] == before + 1, k
            assert np.array_equal(got, whole), (rate, lim, k)
        syn.set_conv_math("f16x2")
        before = syn.profile()["conv_math_fallbacks"]
        syn.debug_set("stream_retry_step", 1)
        chunks, _ = syn.infer_batch_stream(ids, 7)
        syn.debug_set("stream_retry_step", -1)
        assert syn.profile()["conv_math_fallbacks"] == before + 1
        syn.set_conv_math("f16x2")
        want = syn.infer_batch(ids)
        for b in range(3):
            assert np.array_equal(_cat(chunks[b]), want[b]), (rate, b)
        syn.close()


@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFFFFFFF], ids=hex)
def test_a_poisoned_workspace_changes_nothing(model, pattern):
    cfg, blob, ids = model
    join = {"gap_frames": [9, 0], "fade_ms": 1.0}

    def run(poison):
        syn = _syn(blob)
        if poison:
            syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
        out = [_stream(syn, ids[2], 7).tobytes()]
        out.append(b"".join(_cat(c).tobytes() for c in syn.infer_batch_stream(ids, 4)[0]))
        out.append(_cat([p for _, p in syn.infer_joined_stream(ids, 7, join=join)]).tobytes())
        syn.set_output_rate(48000)
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
        out.append(_stream(syn, ids[0], 4).tobytes())
        assert (syn.profile()["poison_bytes"] > 0) == bool(poison)
        syn.close()
        return out

    assert run(True) == run(False)


def test_switch_off_no_bands_loudness_and_no_state_survives(model):
    cfg, blob, ids = model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    assert syn.get_eq_streaming() is False
    plain_whole = syn.infer_ids(ids[1])
    plain_stream = _stream(syn, ids[1], 4)
    plain_batch = [_cat(c) for c in syn.infer_batch_stream(ids, 4)[0]]
    # switch on with 0 bands: the plain stream
    syn.set_eq_streaming(True)
    assert syn.get_eq_streaming() is True
    assert np.array_equal(_stream(syn, ids[1], 4), plain_stream)
    assert all(np.array_equal(_cat(c), p) for c, p in zip(syn.infer_batch_stream(ids, 4)[0], plain_batch))
    # switch off with bands: today's refusals, with their words
    syn.set_eq(BANDS4)
    syn.set_eq_streaming(False)
    eqd = syn.infer_ids(ids[1])
    with pytest.raises(engine.StsError, match="finite halo"):
        syn.infer_ids_stream(ids[1], 4)
    with pytest.raises(engine.StsError, match="equaliser"):
        syn.infer_batch_stream(ids, 4)
    with pytest.raises(engine.StsError, match="equaliser"):
        syn.infer_joined_stream(ids, 4)
    # loudness mode 1 or 2 with the switch on: still refused
    syn.set_eq_streaming(True)
    for mode in (engine.LOUD_MEASURE, engine.LOUD_NORMALIZE):
        syn.set_loudness(mode, -23.0, -1.0)
        with pytest.raises(engine.StsError, match="loudness"):
            syn.infer_ids_stream(ids[1], 4)
    syn.set_loudness(engine.LOUD_OFF)
    # a streamed EQ call, then a whole call, a plain stream, and the streamed call again: nothing survives a call
    first = _stream(syn, ids[1], 4)
    assert np.array_equal(first, eqd)
    assert np.array_equal(syn.infer_ids(ids[1]), eqd)
    assert np.array_equal(_stream(syn, ids[2], 7), syn.infer_ids(ids[2]))
    assert np.array_equal(_stream(syn, ids[1], 4), first)
    syn.set_eq(None)
    assert np.array_equal(_stream(syn, ids[1], 4), plain_stream) and np.array_equal(syn.infer_ids(ids[1]), plain_whole)
    syn.close()
