"""Loudness in a stream on the MI355X (sts_set_loudness_streaming, sts_loudness_measure_chunked; DESIGN.md 9d "streamed").

1. The stream-mode kernels on caller signals against the whole-call kernels (sts_loudness_measure) on the same input: the results bit
   for bit for every step list that crosses a chunk, a tile or a sub-block edge, with the window widened by `back` on either side, and
   every step's partial result against the whole call on the signal cut behind that step; the whole call against tests/loudness_ref.py
   within the bounds of tests/test_loudness_gpu.py.
2. The engine: sts_get_loudness after every streaming form against the corresponding whole call, and every chunk against the same
   stream under mode 0, with the conv mode pinned, on an utterance longer than two tiles.
3. The switches.

Every comparison of the stream against the whole call is of bytes."""
import numpy as np
import pytest

import loudness_ref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

R, T = 32, 8192
BACKS = (0, 7, 1920)
STS_EINVAL = -1
P, LS, HS, HP, LP = 1, 2, 3, 4, 5
BANDS4 = [(HP, 100.0, 0.0, 0.707), (P, 1000.0, 6.0, 2.0), (LS, 300.0, -6.0, 0.7), (P, 3000.0, -9.0, 4.0)]     # (tests/test_eq_stream_gpu.py's)


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _close(got, ref):
    """the bounds of tests/test_loudness_gpu.py: L within 0.01 LU, peak exact, gain within 1e-4 relative, blocks equal"""
    if np.isfinite(ref["lufs"]):
        assert abs(float(got["lufs"]) - ref["lufs"]) <= 0.01, (got, ref)
    else:
        assert np.isneginf(got["lufs"]), (got, ref)
    assert float(got["peak"]) == ref["peak"], (got, ref)
    assert abs(float(got["gain"]) - float(ref["gain"])) <= 1e-4 * float(ref["gain"]), (got, ref)
    assert int(got["blocks"]) == ref["blocks"], (got, ref)


def _signal(N):
    """noise at amplitude 0.3 with a middle third 50 dB down and a stretch of digital silence: both gates act"""
    x = (0.3 * np.random.default_rng(N).standard_normal(N)).astype(np.float32)
    x[N // 3:2 * N // 3] *= np.float32(0.003)
    x[2 * N // 3:2 * N // 3 + N // 6] = 0
    return x


def _step_lists(N, S):
    return {"every sample of the first 70": list(range(0, 71)),
            "chunk and tile edges": [0, R - 1, R, R + 1, 2 * R + 5, T - 1, T, T + 1, 2 * T + 5],
            "sub-block edges": [0, S - 1, S, S + 1, 4 * S],
            "one step": [0],
            "steps of 1000": list(range(0, max(N, 1), 1000))}


# ---- 1. the kernels on caller signals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,rate", [(3 * T + 5, 16000), (3 * T + 5, 8000), (7 * T + 5, 48000)])
def test_chunked_equals_the_whole_call_and_every_partial_the_cut_signal(N, rate):
    x = _signal(N)
    S = loudness_ref.sub_block(rate)
    whole = engine.loudness_measure([x], rate)
    _close(whole[0], loudness_ref.loudness(x, rate))
    assert 0 < int(whole[0]["blocks"]) < N // S - 3                   # (both gates act)
    for name, bounds in _step_lists(N, S).items():
        cuts = [min(N, b) for b in bounds[1:]] + [N]
        want_partial = engine.loudness_measure([x[:c] for c in cuts], rate)      # the whole call on every cut, one launch set
        for back in BACKS:
            out, partial = engine.loudness_measure_chunked([x], rate, bounds, back)
            assert out.tobytes() == whole.tobytes(), (name, back, out, whole)
            assert partial.shape == (len(bounds), 1)
            for k in range(len(bounds)):
                assert partial[k].tobytes() == want_partial[k:k + 1].tobytes(), (name, back, k, partial[k], want_partial[k])
        out, none = engine.loudness_measure_chunked([x], rate, bounds, 7, want_partial=False)
        assert none is None and out.tobytes() == whole.tobytes(), name


def test_short_signals_and_the_unmeasured_ones():
    rate = 16000
    S = loudness_ref.sub_block(rate)
    lens = [0, 1, 2, R, T, 4 * S - 1, 4 * S, 4 * S + 1]
    sig = [(0.3 * np.random.default_rng(100 + n).standard_normal(n)).astype(np.float32) for n in lens]
    whole = engine.loudness_measure(sig, rate)
    for n, w, s in zip(lens, whole, sig):
        _close(w, loudness_ref.loudness(s, rate))
        if n < 4 * S:
            assert np.isneginf(w["lufs"]) and w["blocks"] == 0, n
        else:
            assert np.isfinite(w["lufs"]) and w["blocks"] > 0, n
    for bounds in ([0], [0, 1, 2, R], sorted([0, R - 1, T - 1, T, 4 * S - 1, 4 * S]), list(range(0, 71))):
        for back in (0, 7):
            out, partial = engine.loudness_measure_chunked(sig, rate, bounds, back)
            assert out.tobytes() == whole.tobytes(), (bounds, back)
            assert partial[-1].tobytes() == whole.tobytes()
            cuts = bounds[1:]
            want = engine.loudness_measure([s[:c] for c in cuts for s in sig], rate).reshape(len(cuts), len(sig)) if cuts else None
            for k in range(len(cuts)):
                assert partial[k].tobytes() == want[k].tobytes(), (bounds, back, k)


def test_an_utterance_measures_itself_whatever_its_neighbours():
    rate = 16000
    lens = (T + 1, 1, 2 * T - 3)
    sig = [(0.3 * np.random.default_rng(7 + i).standard_normal(n)).astype(np.float32) for i, n in enumerate(lens)]
    bounds, back = [0, 31, 4000, T, T + 5000], 7
    three, p3 = engine.loudness_measure_chunked(sig, rate, bounds, back)
    assert three.tobytes() == engine.loudness_measure(sig, rate).tobytes()
    alone, pa = engine.loudness_measure_chunked([sig[0]], rate, bounds, back)
    assert alone.tobytes() == three[:1].tobytes() and pa.tobytes() == p3[:, :1].tobytes()
    big = (1e6 * np.random.default_rng(99).standard_normal(2 * T - 3)).astype(np.float32)
    loud, pl = engine.loudness_measure_chunked([sig[0], big], rate, bounds, back)
    assert loud[:1].tobytes() == alone.tobytes() and pl[:, :1].tobytes() == pa.tobytes()
    rev, pr = engine.loudness_measure_chunked(sig[::-1], rate, bounds, back)
    assert rev[::-1].tobytes() == three.tobytes() and pr[:, ::-1].tobytes() == p3.tobytes()


def test_chunked_entry_refuses_malformed_step_lists():
    lib = engine.load_library()
    x = _signal(1000)
    lens = np.asarray([1000], np.int64)
    out = np.zeros(1, engine.LOUDNESS_DTYPE)

    def call(bounds, back=0, nb=None, rate=16000):
        b = np.asarray(bounds, np.int64)
        return lib.sts_loudness_measure_chunked(0, x.ctypes.data, lens.ctypes.data, 1, rate, -16.0, -1.0, b.ctypes.data,
                                                len(bounds) if nb is None else nb, back, out.ctypes.data, None)
    assert call([0, 100, 500]) == 0, lib.sts_last_error()
    assert out.tobytes() == engine.loudness_measure([x], 16000).tobytes()
    for bad in ([1, 5], [0, 5, 5], [0, 9, 5]):
        assert call(bad) == STS_EINVAL, bad
    assert call([0], nb=0) == STS_EINVAL and call([0], back=-1) == STS_EINVAL and call([0], back=2049) == STS_EINVAL
    assert call([0], rate=50000) == STS_EINVAL


# ---- 2. the engine ----------------------------------------------------------------------------------------------------------------------
LONG = (40, 9, 55)
TARGET, CEILING = -23.0, -2.0


@pytest.fixture(scope="module")
def model():
    cfg = sb.tiny_cfg("mbb_fix")
    blob = sb.make_blob(cfg, 7)
    return cfg, blob, [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in LONG]


def _syn(blob, rate=16000, lim=False, mode=engine.LOUD_MEASURE, streaming=True, bands=None):
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if bands:
        syn.set_eq(bands)
        syn.set_eq_streaming(True)
    syn.set_loudness(mode, TARGET, CEILING)
    syn.set_loudness_streaming(streaming)
    if lim:
        syn.set_limiter(engine.LIMITER_ON, 20.0, -3.0, 5.0)
    return syn


def _cat(chunks):
    return np.concatenate(chunks) if len(chunks) else np.zeros(0, np.int16)


def _same_chunks(got, want):
    return len(got) == len(want) and all(a.size == b.size and np.array_equal(a, b) for a, b in zip(got, want))


def _streams_equal_the_whole_call(syn, plain, ids, chunks_of=(1, 4, 7, 100000)):
    """-> the whole call's entry.  loudness() after each stream is the whole call's in bytes; each chunk is the mode-0 stream's"""
    whole_pcm = syn.infer_ids(ids)
    want = syn.loudness()
    assert len(want) == 1
    assert np.array_equal(plain.infer_ids(ids), whole_pcm) and len(plain.loudness()) == 0
    for chunk in chunks_of:
        got, _ = syn.infer_ids_stream(ids, chunk)
        res = syn.loudness()
        print(f"chunk {chunk}: stream {res} whole {want}")
        assert res.tobytes() == want.tobytes(), (chunk, res, want)
        ref, _ = plain.infer_ids_stream(ids, chunk)
        assert _same_chunks(got, ref), chunk
        assert np.array_equal(_cat(got), whole_pcm), chunk
    return want[0]


@pytest.mark.parametrize("lim", [False, True], ids=["cast", "limiter"])
@pytest.mark.parametrize("rate", [16000, 8000, 48000])
def test_a_streamed_utterance_measures_as_the_whole_call_for_every_chunk_size(model, rate, lim):
    cfg, blob, ids = model
    syn, plain = _syn(blob, rate, lim), _syn(blob, rate, lim, mode=engine.LOUD_OFF)
    w = _streams_equal_the_whole_call(syn, plain, ids[2])
    n = syn.infer_ids(ids[2]).size
    assert n * 16000 // rate > 2 * T                                  # more than two tiles at 16 kHz: the carry crosses tile boundaries
    assert np.isfinite(w["lufs"]) and w["blocks"] > 0
    if lim:                                                           # (under the limiter the reported gain is g_L, as in a whole call)
        assert abs(float(w["gain"]) - 10.0 ** ((TARGET - float(w["lufs"])) / 20.0)) <= 1e-4 * float(w["gain"])
    syn.close(); plain.close()


def test_the_three_utterances_cover_measured_unmeasured_and_tile_crossings(model):
    cfg, blob, ids = model
    syn = _syn(blob)
    pcm = syn.infer_batch(ids)
    res = syn.loudness()
    assert [p.size for p in pcm] == [12736, 3392, 17536]
    assert np.isfinite(res[0]["lufs"]) and res[0]["blocks"] > 0 and np.isfinite(res[2]["lufs"]) and res[2]["blocks"] > 0
    assert np.isneginf(res[1]["lufs"]) and res[1]["blocks"] == 0
    syn.close()


@pytest.mark.parametrize("rate,lim", [(16000, False), (48000, True)])
def test_loudness_reads_the_streamed_eq(model, rate, lim):
    cfg, blob, ids = model
    syn, plain = _syn(blob, rate, lim, bands=BANDS4), _syn(blob, rate, lim, mode=engine.LOUD_OFF, bands=BANDS4)
    w = _streams_equal_the_whole_call(syn, plain, ids[2], chunks_of=(1, 7, 100000))
    no_eq = _syn(blob, rate, lim)
    no_eq.infer_ids_stream(ids[2], 7)
    assert np.isfinite(w["lufs"]) and float(no_eq.loudness()[0]["lufs"]) != float(w["lufs"])
    syn.close(); plain.close(); no_eq.close()


def test_a_gain_plan_that_mutes_and_ducks(model):
    """the phonemes whose frames lie in the middle 60 % of the utterance are muted (more than six 100 ms sub-blocks of digital silence:
    at least two 400 ms blocks fall to the absolute gate), the three behind them ducked by 30 dB, the second one raised by 6 dB"""
    cfg, blob, ids = model
    n = len(ids[2])
    probe = _syn(blob)
    probe.infer_ids(ids[2])
    edges = np.concatenate([[0], np.cumsum(probe.durations(n))]).astype(np.float64)
    probe.close()
    mid = (edges[:-1] >= 0.25 * edges[-1]) & (edges[1:] <= 0.85 * edges[-1])
    last = int(np.flatnonzero(mid)[-1])
    assert mid.sum() > 10 and last + 4 < n
    db = np.zeros(n, np.float32); db[mid] = -np.inf; db[last + 1:last + 4] = -30.0; db[1] = 6.0
    for rate in (16000, 8000):
        syn, plain = _syn(blob, rate), _syn(blob, rate, mode=engine.LOUD_OFF)
        syn.set_gain_plan([n], [{"gain_db": db, "ramp_ms": 2.0}])
        whole_pcm = syn.infer_ids(ids[2])
        want = syn.loudness()
        S = loudness_ref.sub_block(rate)
        assert 0 < int(want[0]["blocks"]) < whole_pcm.size // S - 3, want   # the gates drop blocks
        for chunk in (1, 7, 100000):
            syn.set_gain_plan([n], [{"gain_db": db, "ramp_ms": 2.0}])
            got, _ = syn.infer_ids_stream(ids[2], chunk)
            assert syn.loudness().tobytes() == want.tobytes(), (rate, chunk, syn.loudness(), want)
            plain.set_gain_plan([n], [{"gain_db": db, "ramp_ms": 2.0}])
            assert _same_chunks(got, plain.infer_ids_stream(ids[2], chunk)[0]) and np.array_equal(_cat(got), whole_pcm)
        syn.close(); plain.close()


@pytest.mark.parametrize("rate,bands,tap", [(16000, None, "wave"), (48000, None, "wave_out"), (16000, BANDS4, "wave_eq")])
def test_a_batched_stream_and_a_stopped_utterance(model, rate, bands, tap):
    cfg, blob, ids = model
    syn, plain = _syn(blob, rate, bands=bands), _syn(blob, rate, mode=engine.LOUD_OFF, bands=bands)
    syn.set_record_taps(True)
    want_pcm = syn.infer_batch(ids)
    signal = syn.tap(tap)[0]
    syn.set_record_taps(False)
    want = syn.loudness()
    assert len(want) == 3 and syn.infer_batch(ids)[0].size == want_pcm[0].size and syn.loudness().tobytes() == want.tobytes()
    assert engine.loudness_measure([signal[:want_pcm[0].size]], rate, TARGET, CEILING).tobytes() == want[:1].tobytes()
    for chunk in (4, 7):
        chunks, _ = syn.infer_batch_stream(ids, chunk)
        assert syn.loudness().tobytes() == want.tobytes(), (chunk, syn.loudness(), want)
        ref, _ = plain.infer_batch_stream(ids, chunk)
        for b in range(3):
            assert _same_chunks(chunks[b], ref[b]) and np.array_equal(_cat(chunks[b]), want_pcm[b]), (chunk, b)
    # utterance 0 stopped by its callback at chunk 2: its entry measures what was delivered, the others are unaffected
    seen = [0, 0, 0]

    def on_chunk(u, pcm, off, t):
        seen[u] += 1
        return u == 0 and seen[0] == 3
    total = []
    got, _ = syn.infer_batch_stream(ids, 4, on_chunk=on_chunk, n_total=total)
    res = syn.loudness()
    delivered = _cat(got[0]).size
    assert len(got[0]) == 3 and delivered == total[0] and 0 < delivered < want_pcm[0].size
    cut = engine.loudness_measure([signal[:delivered]], rate, TARGET, CEILING)
    assert res[:1].tobytes() == cut.tobytes(), (res[0], cut[0])
    assert res[1:].tobytes() == want[1:].tobytes()
    syn.close(); plain.close()


@pytest.mark.parametrize("rate,lim,bands", [(16000, False, None), (8000, True, None), (48000, False, BANDS4)])
def test_a_joined_stream_with_silence_only_steps(model, rate, lim, bands):
    cfg, blob, ids = model
    join = {"gap_frames": [30, 12], "lead_frames": 9, "trail_frames": 11, "fade_ms": 2.0}
    syn, plain = _syn(blob, rate, lim, bands=bands), _syn(blob, rate, lim, mode=engine.LOUD_OFF, bands=bands)
    want_pcm = syn.infer_joined(ids, join=join)
    want = syn.loudness()
    assert len(want) == 1 and np.isfinite(want[0]["lufs"]) and want_pcm.size * 16000 // rate > 2 * T
    for chunk in (4, 7, 100000):                                     # (4 and 7 < the gaps: some steps hold silence only)
        got = syn.infer_joined_stream(ids, chunk, join=join)
        assert syn.loudness().tobytes() == want.tobytes(), (rate, lim, chunk, syn.loudness(), want)
        ref = plain.infer_joined_stream(ids, chunk, join=join)
        assert [o for o, _ in got] == [o for o, _ in ref] and _same_chunks([p for _, p in got], [p for _, p in ref])
        assert np.array_equal(_cat([p for _, p in got]), want_pcm)
    syn.close(); plain.close()


def test_a_step_decoded_twice_starts_from_the_same_state(model):
    """STS_DBG_STREAM_RETRY_STEP under conv math 3 (the conv mode pinned: the repeat computes what the first attempt did)"""
    cfg, blob, ids = model
    for rate, lim in ((16000, False), (48000, True)):
        syn = _syn(blob, rate, lim)
        syn.set_conv_math("f16x2")
        whole = syn.infer_ids(ids[2])
        want = syn.loudness()
        steps = (int(syn.durations(len(ids[2])).sum()) + 6) // 7
        assert steps > 3
        for k in (1, steps - 1):
            syn.set_conv_math("f16x2")                               # (two repeats in a row would pin the engine to split-bf16)
            before = syn.profile()["conv_math_fallbacks"]
            syn.debug_set("stream_retry_step", k)
            got, _ = syn.infer_ids_stream(ids[2], 7)
            syn.debug_set("stream_retry_step", -1)
            assert syn.profile()["conv_math_fallbacks"] == before + 1, k
            assert np.array_equal(_cat(got), whole) and syn.loudness().tobytes() == want.tobytes(), (rate, lim, k)
        syn.set_conv_math("f16x2")
        wantb_pcm = syn.infer_batch(ids)
        wantb = syn.loudness()
        before = syn.profile()["conv_math_fallbacks"]
        syn.debug_set("stream_retry_step", 1)
        chunks, _ = syn.infer_batch_stream(ids, 7)
        syn.debug_set("stream_retry_step", -1)
        assert syn.profile()["conv_math_fallbacks"] == before + 1
        assert syn.loudness().tobytes() == wantb.tobytes()
        for b in range(3):
            assert np.array_equal(_cat(chunks[b]), wantb_pcm[b]), (rate, b)
        syn.close()


@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFFFFFFF], ids=hex)
def test_a_poisoned_workspace_changes_nothing(model, pattern):
    cfg, blob, ids = model
    join = {"gap_frames": [9, 0], "fade_ms": 1.0}

    def run(poison):
        syn = _syn(blob)
        if poison:
            syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
        out = [_cat(syn.infer_ids_stream(ids[2], 7)[0]).tobytes(), syn.loudness().tobytes()]
        out.append(b"".join(_cat(c).tobytes() for c in syn.infer_batch_stream(ids, 4)[0]))
        out.append(syn.loudness().tobytes())
        out.append(_cat([p for _, p in syn.infer_joined_stream(ids, 7, join=join)]).tobytes())
        out.append(syn.loudness().tobytes())
        syn.set_output_rate(48000)
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
        out.append(_cat(syn.infer_ids_stream(ids[0], 4)[0]).tobytes())
        out.append(syn.loudness().tobytes())
        assert (syn.profile()["poison_bytes"] > 0) == bool(poison)
        syn.close()
        return out

    a, b = run(True), run(False)
    assert a == b
    assert all(len(r) > 0 for r in a[1::2])


# ---- 3. the switches --------------------------------------------------------------------------------------------------------------------
def test_switch_off_refuses_with_todays_words(model):
    """(passes without the feature too: the refusal is the behaviour every earlier build has)"""
    cfg, blob, ids = model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    for mode in (engine.LOUD_MEASURE, engine.LOUD_NORMALIZE):
        syn.set_loudness(mode, TARGET, CEILING)
        for call in (lambda: syn.infer_ids_stream(ids[1], 4), lambda: syn.infer_batch_stream(ids, 4), lambda: syn.infer_joined_stream(ids, 4)):
            with pytest.raises(engine.StsError, match=r"streaming is not available while loudness measurement or normalization is on "
                                                      r"\(sts_set_loudness mode 0 first\): normalizing needs the whole utterance before its "
                                                      r"first sample leaves$"):
                call()
            assert len(syn.loudness()) == 0
        assert syn.infer_ids(ids[1]).size == 3392 and len(syn.loudness()) == 1      # the engine is usable afterwards
    syn.close()


def test_switch_on_mode_2_mode_0_the_halo_and_no_state_survives(model):
    cfg, blob, ids = model
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    assert syn.loudness_streaming() is False
    halo = syn.stream_halo_frames()
    plain_stream, _ = syn.infer_ids_stream(ids[1], 4)
    plain_whole = syn.infer_ids(ids[0])
    syn.set_loudness_streaming(True)
    assert syn.loudness_streaming() is True and syn.stream_halo_frames() == halo
    # mode 0: the plain stream, nothing measured
    got, _ = syn.infer_ids_stream(ids[1], 4)
    assert _same_chunks(got, plain_stream) and len(syn.loudness()) == 0
    # mode 2: refused with the reason and the remedy
    syn.set_loudness(engine.LOUD_NORMALIZE, TARGET, CEILING)
    for call in (lambda: syn.infer_ids_stream(ids[1], 4), lambda: syn.infer_batch_stream(ids, 4), lambda: syn.infer_joined_stream(ids, 4)):
        with pytest.raises(engine.StsError, match=r"gain needs the integrated loudness of the whole utterance.*measure in a stream.*limiter"):
            call()
        assert len(syn.loudness()) == 0
    normalized = syn.infer_ids(ids[0])                                # (whole calls: the switch has no effect)
    assert len(syn.loudness()) == 1 and np.isfinite(syn.loudness()[0]["lufs"]) and not np.array_equal(normalized, plain_whole)
    # mode 1: runs, the halo unchanged; stream A, then B, equals B alone
    syn.set_loudness(engine.LOUD_MEASURE, TARGET, CEILING)
    assert syn.stream_halo_frames() == halo
    syn.infer_ids_stream(ids[2], 7)
    a = syn.loudness()
    syn.infer_ids_stream(ids[0], 4)
    b_after_a = syn.loudness()
    fresh = _syn(blob)
    fresh.infer_ids_stream(ids[0], 4)
    assert b_after_a.tobytes() == fresh.loudness().tobytes() and a.tobytes() != b_after_a.tobytes()
    syn.infer_ids(ids[0])
    assert syn.loudness().tobytes() == b_after_a.tobytes()
    # switched off again: refused, the count back to 0
    syn.set_loudness_streaming(False)
    with pytest.raises(engine.StsError, match="streaming is not available while loudness"):
        syn.infer_ids_stream(ids[0], 4)
    assert len(syn.loudness()) == 0 and syn.loudness_streaming() is False
    syn.close(); fresh.close()
