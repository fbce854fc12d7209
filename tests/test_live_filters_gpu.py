"""Per-slot filter state on the MI355X: an open stream (sts_stream_open / _open_ex) with the streamed EQ (sts_set_eq_streaming) and with
loudness measurement (mode 1, sts_set_loudness_streaming).  Every slot's chunks against that utterance's own sts_infer_ids_stream chunks
under the same settings, chunk by chunk, bit for bit with the kernel variant pinned; every retired slot's sts_stream_get_loudness entry
against sts_get_loudness after that utterance's own closed stream, byte for byte; slots and tile ranges reused under poison; the repeat of
a step; the states; the pool.  Nothing here has a tolerance but the pool's leg, whose engines choose their kernels themselves."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import golden_files, load_golden
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL, STS_ESTATE = -1, -4
INF = float("inf")
TILE = 8192
LENS = [9, 31, 5, 17, 1, 24, 60]           # (the lengths of tests/test_live_plans_gpu.py, and a long one: _long_scale stretches it over two tile edges)
LS = [1.0, 0.8, 1.2, 1.0, 0.6, 0.9, 1.0]
LONG, SHORT = 6, 4
CAPACITY = 8192          # (frames of 8 samples: the long utterance at 8 kHz alone has more than 4096)
PHONEMES = 256
# admissions at step counts 0, 1, 3 and 4: both parities of the state slots
SCHEDULE = ((0, LONG), "step", (2,), "step", "step", (3, 4, 5), "step", (1,))
HP, PK, LSH = engine.EQ_HIGHPASS, engine.EQ_PEAK, engine.EQ_LOWSHELF
BANDS4 = [(HP, 100.0, 0.0, 0.707), (PK, 1000.0, 6.0, 2.0), (LSH, 300.0, -6.0, 0.7), (PK, 3000.0, -9.0, 4.0)]      # valid at 8, 16 and 22.05 kHz
TARGET, CEILING = -23.0, -2.0
LEGS = {"native": (16000, False), "22050+limiter": (22050, True), "8000": (8000, False)}

def _kind_files():
    """one tiny golden model per kind: {kind: its first fixture} (the names alone: nothing is built when the tests are collected)"""
    first = {}
    for path in golden_files():
        first.setdefault(str(np.load(path)["kind"]), path)
    return first


KIND_FILES = _kind_files()
KINDS = sorted(KIND_FILES)
_models = {}


def _model(kind):
    if kind not in _models:
        _, cfg, blob = load_golden(KIND_FILES[kind])
        _models[kind] = (cfg, blob)
    return _models[kind]


def test_there_is_a_model_of_every_kind():
    assert len(KINDS) >= 5 and any(_model(k)[0].is_ms for k in KINDS)


def _batch(cfg):
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate(LENS)]
    nspk = max(int(cfg.spk_num), 1)
    sids = [(3 * u + 1) % nspk for u in range(len(LENS))] if cfg.is_ms else [0] * len(LENS)
    return ids, sids, list(LS)


def _syn(blob, rate=16000, lim=False, eq=True, loud=False):
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if lim:
        syn.set_limiter(engine.LIMITER_ON, 12.0, -1.0, 5.0)
    if eq:
        syn.set_eq(BANDS4)
        syn.set_eq_streaming(True)
    if loud:
        syn.set_loudness(engine.LOUD_MEASURE, TARGET, CEILING)
        syn.set_loudness_streaming(True)
    return syn


def _long_scale(syn, ids, sid, rate):
    """the length scale at which the long utterance's output crosses two tile edges at `rate` with a margin"""
    n = syn.infer_ids(ids, sid, 1.0).size
    return max(1.0, 1.25 * (2 * TILE + 512) / n)


def _short_scale(syn, ids, sid, rate):
    """the length scale at which the one-phoneme utterance has at most 3 frames: shorter than a chunk of 4 (its duration is the ceiling
    of w * scale, and w is at most its frame count at scale 1)"""
    frames = syn.infer_ids(ids, sid, 1.0).size * 16000 // rate // int(syn.info.samples_per_frame)
    return min(1.0, 2.5 / max(frames, 1))


def _scales(syn, ids, sids, ls, rate):
    ls[LONG] = _long_scale(syn, ids[LONG], sids[LONG], rate)
    ls[SHORT] = _short_scale(syn, ids[SHORT], sids[SHORT], rate)


def _cat(chunks):
    return np.concatenate([p for _, p in chunks]) if chunks else np.zeros(0, np.int16)


def _same_chunks(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(got, want))


def _set_tables(syn, n, tabs):
    if not tabs:
        return
    if tabs.get("mix") and any(m is not None for m in tabs["mix"]):
        syn.set_speaker_mix(tabs["mix"])
    if tabs.get("gain") and any(g is not None for g in tabs["gain"]):
        syn.set_gain_plan(n, tabs["gain"])
    if tabs.get("forced") is not None:
        syn.set_forced_durations(np.concatenate(tabs["forced"]))


def _pick(tabs, us):
    return {k: [v[u] for u in us] for k, v in tabs.items()} if tabs else None


def _single(syn, ids, sid, ls, chunk, tabs=None, stop_after=0, loud=False):
    """one utterance's own stream as [(sample_offset, pcm)] -- stopped by its callback behind chunk `stop_after` (0: never) -- and, with
    `loud`, what sts_get_loudness reports after it"""
    _set_tables(syn, [len(ids)], tabs)
    out = []

    def on_chunk(pcm, off, t):
        out.append((off, pcm))
        return len(out) == stop_after
    syn.infer_ids_stream(ids, chunk, sid, ls, on_chunk=on_chunk)
    if not loud:
        return out
    res = syn.loudness()
    assert len(res) == 1
    return out, res.tobytes()


def _run(syn, ids, sids, ls, schedule=SCHEDULE, tabs=None, stop=None, loud=False):
    """drives an open stream through `schedule`, then steps until it is empty.  stop: {utterance: chunks after which its callback stops
    it}.  With `loud`: behind every step the reported slots are exactly those that retired in it, ascending, and sts_get_loudness returns
    the same entries.  -> chunks per utterance, total samples per utterance, the result's bytes per utterance"""
    got = [[] for _ in ids]
    total, utt_of, res_of = {}, {}, {}
    stop = stop or {}

    def step():
        before = {s for s in utt_of if utt_of[s] is not None}

        def on_chunk(s, pcm, off):
            u = utt_of[s]
            got[u].append((off, pcm))
            return len(got[u]) == stop.get(u, 0)
        chunks, live = syn.stream_step(on_chunk)
        retired = sorted(s for s, pcm, off in chunks if off + pcm.size == total[utt_of[s]] or len(got[utt_of[s]]) == stop.get(utt_of[s], 0))
        assert {s for s, _, _ in chunks} == before and live == len(before) - len(retired)
        if loud:
            slots, res = syn.stream_loudness()
            assert list(slots) == retired, (list(slots), retired)
            assert syn.loudness().tobytes() == res.tobytes()
            for s, r in zip(slots, res):
                res_of[utt_of[int(s)]] = r.tobytes()
        for s in retired:
            utt_of[s] = None
        return live
    for op in schedule:
        if op == "step":
            step()
            continue
        _set_tables(syn, [len(ids[u]) for u in op], _pick(tabs, op))
        r = syn.stream_admit([ids[u] for u in op], [sids[u] for u in op], [ls[u] for u in op])
        assert r is not None, op
        for u, s, t in zip(op, *r):
            assert utt_of.get(s) is None
            utt_of[s] = u
            total[u] = t
    for _ in range(100000):
        if step() == 0:
            break
    assert syn.stream_info()["live"] == 0
    return got, total, res_of


def _assert_shapes(total, chunk, hop, rate):
    """the tile carry and the sub-chunk utterance are really exercised"""
    assert total[LONG] > 2 * TILE, total                                    # crosses two EQ / loudness tile edges
    assert min(total.values()) < -(-chunk * hop * rate // 16000), total     # one utterance is shorter than a chunk


# ---- 1. the EQ ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [4, 8])
@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("kind", KINDS)
def test_eq_each_slot_equals_its_single_stream(kind, leg, chunk):
    rate, lim = LEGS[leg]
    cfg, blob = _model(kind)
    ids, sids, ls = _batch(cfg)
    syn = _syn(blob, rate, lim)
    hop = int(syn.info.samples_per_frame)
    _scales(syn, ids, sids, ls, rate)
    want = [_single(syn, ids[b], sids[b], ls[b], chunk) for b in range(len(ids))]
    if chunk == 4:          # the EQ really is in the chain
        plain = _syn(blob, rate, lim, eq=False)
        assert not np.array_equal(_cat(_single(plain, ids[0], sids[0], ls[0], chunk)), _cat(want[0]))
        plain.close()
    syn.stream_open(chunk, len(ids), CAPACITY)
    got, total, _ = _run(syn, ids, sids, ls)
    syn.stream_close()
    _assert_shapes(total, chunk, hop, rate)
    for b in range(len(ids)):
        assert _same_chunks(got[b], want[b]), (kind, leg, chunk, b)
        assert total[b] == _cat(want[b]).size, (kind, leg, chunk, b)
    syn.close()


# ---- 2. loudness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [4, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_loudness_results_per_retired_slot(kind, chunk):
    cfg, blob = _model(kind)
    ids, sids, ls = _batch(cfg)
    syn = _syn(blob, eq=False, loud=True)
    hop = int(syn.info.samples_per_frame)
    _scales(syn, ids, sids, ls, 16000)
    want = [_single(syn, ids[b], sids[b], ls[b], chunk, loud=True) for b in range(len(ids))]
    # the plain open stream's chunks
    plain = _syn(blob, eq=False)
    plain.stream_open(chunk, len(ids), CAPACITY)
    ref, _, _ = _run(plain, ids, sids, ls)
    plain.stream_close()
    plain.close()
    syn.stream_open(chunk, len(ids), CAPACITY)
    got, total, res = _run(syn, ids, sids, ls, loud=True)
    _assert_shapes(total, chunk, hop, 16000)
    assert sorted(res) == list(range(len(ids)))
    for b in range(len(ids)):
        assert _same_chunks(got[b], ref[b]) and _same_chunks(got[b], want[b][0]), (kind, chunk, b)
        assert res[b] == want[b][1], (kind, chunk, b, np.frombuffer(res[b], engine.LOUDNESS_DTYPE), np.frombuffer(want[b][1], engine.LOUDNESS_DTYPE))
    assert np.isfinite(np.frombuffer(res[LONG], engine.LOUDNESS_DTYPE)["lufs"][0]), kind     # (longer than 400 ms: measured)
    # the long utterance and a short one stopped by their callbacks behind their second chunk: what a closed stream stopped there
    # reports; the others are unaffected
    stop = {LONG: 2, 1: 2}
    syn.stream_close()
    cut = {u: _single(syn, ids[u], sids[u], ls[u], chunk, stop_after=2, loud=True) for u in stop}
    syn.stream_open(chunk, len(ids), CAPACITY)
    got, total, res = _run(syn, ids, sids, ls, stop=stop, loud=True)
    syn.stream_close()
    for b in range(len(ids)):
        w = cut[b] if b in stop else want[b]
        assert _same_chunks(got[b], w[0]) and res[b] == w[1], (kind, chunk, b)
    assert all(len(got[u]) == 2 for u in stop) and res[LONG] != want[LONG][1], kind
    syn.close()


# ---- 3. both at once, planned ---------------------------------------------------------------------------------------------------------
def _ms_model():
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    return cfg, sb.make_blob(cfg, 21)


def _tables(cfg, sids):
    nspk = int(cfg.spk_num)
    gain, mix = [None] * len(LENS), [None] * len(LENS)
    gain[0] = {"gain_db": [0, 0, -INF, -INF, 0, 6, 6, 0, -12], "ramp_ms": 5.0}
    gain[3] = {"gain_db": [0] * 3 + [6] * 5 + [0] * 2 + [-12] * 4 + [-INF] + [0] * 2, "ramp_ms": 50.0}
    gain[LONG] = {"gain_db": [0.0] * 20 + [-9.0] * 20 + [3.0] * 20, "ramp_ms": 10.0}
    mix[0] = {"sid": [0, nspk - 1], "weight": [0.6, 0.3]}
    mix[1] = {"sid": [1 % nspk, 2 % nspk], "weight": [1.5, -0.5]}
    return {"gain": gain, "mix": mix}


@pytest.mark.parametrize("leg", ["native", "22050+limiter"])
def test_eq_and_loudness_with_a_gain_plan_and_a_speaker_mix(leg):
    rate, lim = LEGS[leg]
    cfg, blob = _ms_model()
    ids, sids, ls = _batch(cfg)
    tabs = _tables(cfg, sids)
    syn = _syn(blob, rate, lim, loud=True)
    _scales(syn, ids, sids, ls, rate)
    chunk = 8
    want = [_single(syn, ids[b], sids[b], ls[b], chunk, _pick(tabs, [b]), loud=True) for b in range(len(ids))]
    bare = _single(syn, ids[0], sids[0], ls[0], chunk, loud=True)
    assert not np.array_equal(_cat(bare[0]), _cat(want[0][0])) and bare[1] != want[0][1]        # the tables are in the chain, in front of both stages
    syn.stream_open(chunk, len(ids), CAPACITY, PHONEMES)
    got, total, res = _run(syn, ids, sids, ls, tabs=tabs, loud=True)
    syn.stream_close()
    assert total[LONG] > 2 * TILE
    for b in range(len(ids)):
        assert _same_chunks(got[b], want[b][0]) and res[b] == want[b][1], (leg, b)
    syn.close()


# ---- 4. slot reuse under poison ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0x7BFF7BFF], ids=hex)
def test_slots_and_tiles_reused_under_poison(pattern):
    """max_live = 2: every later utterance takes a slot, a state and tiles that another retired from -- the long one's among them -- and
    gives the chunks and the result of a fresh stream"""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = _syn(blob, 22050, True, loud=True)
    _scales(syn, ids, sids, ls, 22050)
    chunk = 4
    want = [_single(syn, ids[b], sids[b], ls[b], chunk, loud=True) for b in range(len(ids))]
    syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
    syn.stream_open(chunk, 2, CAPACITY)
    got, res, utt_of = [[] for _ in ids], {}, {}
    # the long one and the shortest; the short one's slot and tile go to the next, twice; then two into what the long one left; then one more
    for op in ((LONG, SHORT), (2,), (0,), (1, 3), (5,)):
        while syn.stream_info()["free_slots"] < len(op):
            _step_into(syn, got, res, utt_of)
        r = syn.stream_admit([ids[u] for u in op], [sids[u] for u in op], [ls[u] for u in op])
        assert r is not None, op
        utt_of.update(zip(r[0], op))
    while syn.stream_info()["live"]:
        _step_into(syn, got, res, utt_of)
    syn.stream_close()
    syn.debug_set("poison", 0)
    for b in range(len(ids)):
        assert _same_chunks(got[b], want[b][0]) and res[b] == want[b][1], b
    syn.close()


def _step_into(syn, got, res, utt_of):
    chunks, _ = syn.stream_step()
    for s, pcm, off in chunks:
        got[utt_of[s]].append((off, pcm))
    slots, r = syn.stream_loudness()
    for s, e in zip(slots, r):
        res[utt_of[int(s)]] = e.tobytes()


# ---- 5. the repeat of a step ----------------------------------------------------------------------------------------------------------
def test_a_step_decoded_twice_starts_from_the_same_state():
    """STS_DBG_STREAM_RETRY_STEP under conv math 3, both stages on: step 2 -- a step with carried state, in which a slot retires -- is
    decoded twice; chunks and results are those of the stream without the repeat (the conv mode pinned: both forms compute the same)"""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = _syn(blob, loud=True)
    syn.set_profiling(True)
    syn.set_conv_math("f16x2")
    _scales(syn, ids, sids, ls, 16000)
    chunk = 4
    runs = []
    for k in (-1, 2, 5):
        syn.set_conv_math("f16x2")
        syn.stream_open(chunk, len(ids), CAPACITY)
        before = syn.profile()["conv_math_fallbacks"]
        syn.debug_set("stream_retry_step", k)
        runs.append(_run(syn, ids, sids, ls, loud=True))
        syn.debug_set("stream_retry_step", -1)
        assert syn.profile()["conv_math_fallbacks"] == before + (k >= 0), k
        syn.stream_close()
    for got, total, res in runs[1:]:
        for b in range(len(ids)):
            assert _same_chunks(got[b], runs[0][0][b]) and res[b] == runs[0][2][b], b
    syn.close()


# ---- 6. states ------------------------------------------------------------------------------------------------------------------------
def test_refusals_setters_and_the_result_entry():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    ids = sb.synthetic_ids(9, cfg.vocab)
    syn = engine.Synthesizer(blob)
    lib = syn.lib
    syn.set_conv_mode(6)
    opens = (lambda: lib.sts_stream_open(syn.h, 8, 2, 1000), lambda: lib.sts_stream_open_ex(syn.h, 8, 2, 1000, 64))
    # no stream: the result entry answers STS_ESTATE
    assert lib.sts_stream_get_loudness(syn.h, None, None, 0) == STS_ESTATE
    # the refusals that stay: bands or mode 1 without their stream modes, mode 2 always, taps, a pending table
    syn.set_eq(BANDS4)
    assert [o() for o in opens] == [STS_EINVAL] * 2 and b"equaliser" in lib.sts_last_error()
    syn.set_eq(None)
    syn.set_eq_streaming(True)
    syn.set_loudness(engine.LOUD_MEASURE, TARGET, CEILING)
    assert [o() for o in opens] == [STS_EINVAL] * 2 and b"loudness" in lib.sts_last_error()
    syn.set_loudness_streaming(True)
    syn.set_loudness(engine.LOUD_NORMALIZE, TARGET, CEILING)
    assert [o() for o in opens] == [STS_EINVAL] * 2 and b"loudness" in lib.sts_last_error()
    syn.set_loudness(engine.LOUD_MEASURE, TARGET, CEILING)
    syn.set_eq(BANDS4)
    syn.set_record_taps(True)
    assert [o() for o in opens] == [STS_EINVAL] * 2 and b"taps" in lib.sts_last_error()
    syn.set_record_taps(False)
    syn.set_gain_plan([len(ids)], [{"gain_db": [0.0] * len(ids)}])
    assert [o() for o in opens] == [STS_EINVAL] * 2
    syn.set_gain_plan(None)
    assert not syn.stream_info()["open"]
    # open paragraphs keep their refusals
    assert lib.sts_para_open(syn.h, 8, 4, 1000, 0, 0.0) == STS_EINVAL
    want, want_res = _single(syn, ids, 0, 1.0, 8, loud=True)
    # both stages on: it opens, and the four setters are facts that open fixed
    syn.stream_open(8, 2, 1000)
    n, arr = engine._eq_bands(BANDS4)
    assert lib.sts_set_eq(syn.h, n, arr) == STS_ESTATE and lib.sts_set_eq(syn.h, 0, None) == STS_ESTATE
    assert lib.sts_set_eq_streaming(syn.h, 0) == STS_ESTATE and lib.sts_set_eq_streaming(syn.h, 1) == STS_ESTATE
    assert lib.sts_set_loudness(syn.h, 0, TARGET, CEILING) == STS_ESTATE
    assert lib.sts_set_loudness_streaming(syn.h, 0) == STS_ESTATE and lib.sts_set_loudness_streaming(syn.h, 1) == STS_ESTATE
    assert lib.sts_stream_get_loudness(syn.h, None, None, 0) == 0                     # nothing has retired
    r = syn.stream_admit([ids])
    assert r is not None
    got = []
    while True:
        chunks, live = syn.stream_step()
        got += [(off, pcm) for _, pcm, off in chunks]
        if live == 0:
            break
        assert lib.sts_stream_get_loudness(syn.h, None, None, 0) == 0 and len(syn.loudness()) == 0      # a step that retired nothing
    assert _same_chunks(got, want)
    # capacity 0: the count alone, nothing is written; capacity 1 of 1: the entry
    slot, out = np.full(1, -7, np.int32), np.zeros(1, engine.LOUDNESS_DTYPE)
    assert lib.sts_stream_get_loudness(syn.h, slot.ctypes.data, out.ctypes.data, 0) == 1 and slot[0] == -7 and out.tobytes() == bytes(16)
    assert lib.sts_stream_get_loudness(syn.h, slot.ctypes.data, out.ctypes.data, 1) == 1 and slot[0] == r[0][0] and out.tobytes() == want_res
    assert lib.sts_stream_get_loudness(syn.h, None, out.ctypes.data, 5) == 1
    # a step of the empty stream changes nothing of it
    assert syn.stream_step() == ([], 0) and lib.sts_stream_get_loudness(syn.h, None, None, 0) == 1
    syn.stream_close()
    assert lib.sts_stream_get_loudness(syn.h, None, None, 0) == STS_ESTATE
    # the closed paths are what they were
    assert _same_chunks(_single(syn, ids, 0, 1.0, 8), want)
    syn.close()


def test_results_begin_and_end_with_their_stream():
    """a stream that retired slots is closed and another opened -- at once, behind a closed measuring call, and with loudness off: the
    new stream reports nothing until a step of its own retires a slot, and a stream that does not measure never reports"""
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=t) for t in (9, 5, 7)]
    syn = _syn(blob, eq=False, loud=True)
    lib = syn.lib
    slot, out = np.full(8, -7, np.int32), np.zeros(8, engine.LOUDNESS_DTYPE)

    def count():
        slot[:] = -7
        n = lib.sts_stream_get_loudness(syn.h, slot.ctypes.data, out.ctypes.data, 8)
        assert (slot[max(n, 0):] == -7).all()
        return n

    def three_retire_together():
        syn.stream_open(100000, 3, 1000)
        assert count() == 0 and len(syn.loudness()) == 0
        assert syn.stream_admit(ids) is not None and count() == 0
        chunks, live = syn.stream_step()
        assert live == 0 and count() == 3 and list(slot[:3]) == [0, 1, 2] and len(syn.loudness()) == 3
        syn.stream_close()
        assert len(syn.loudness()) == 0 and lib.sts_stream_get_loudness(syn.h, None, None, 0) == STS_ESTATE
    three_retire_together()
    three_retire_together()                                  # reopened at once
    syn.infer_ids(ids[0])                                    # a closed measuring call in between: one result, no slots
    assert len(syn.loudness()) == 1
    syn.stream_open(8, 3, 1000)
    assert count() == 0 and len(syn.loudness()) == 0
    syn.stream_close()
    three_retire_together()
    syn.infer_ids_stream(ids[1], 8)                          # ... and a closed measuring stream
    assert len(syn.loudness()) == 1
    three_retire_together()
    # loudness off: the stream never reports, whatever the one before it left
    syn.set_loudness(engine.LOUD_OFF)
    syn.stream_open(100000, 3, 1000)
    assert count() == 0
    assert syn.stream_admit(ids) is not None
    chunks, live = syn.stream_step()
    assert live == 0 and len(chunks) == 3 and count() == 0 and len(syn.loudness()) == 0
    syn.stream_close()
    syn.close()


def test_no_room_in_the_tile_pool_leaves_the_stream_unchanged():
    """A planned stream with forced durations (exact frame counts), 96 frames of 256 samples = 3 + max_live 4 = 7 tiles.  A5 B6 C5 D6 take
    tiles 0 1 2 3; A is stopped; E40 takes tiles 4 5 (tile 0 alone is too small); C is stopped: tiles 0, 2 and 6 are free, 34 frames in
    one range and a slot are free -- and F32, 8192 samples, needs two tiles side by side.  Frames and slots alone would take it."""
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    syn = _syn(blob, eq=False, loud=True)
    hop = int(syn.info.samples_per_frame)
    assert TILE % hop == 0
    k = 256 // hop if hop <= 256 else 0
    assert k >= 1
    frames = {"A": 5 * k, "B": 6 * k, "C": 5 * k, "D": 6 * k, "E": 40 * k, "F": 32 * k}
    ids = {u: sb.synthetic_ids(3, cfg.vocab, salt=i) for i, u in enumerate(frames)}
    dur = {u: np.array([f - 2, 1, 1], np.int32) for u, f in frames.items()}
    chunk = 2 * k

    def admit(us):
        syn.set_forced_durations(np.concatenate([dur[u] for u in us]))
        return syn.stream_admit([ids[u] for u in us])
    want = {}
    for u in ("B", "E", "F"):
        want[u] = _single(syn, ids[u], 0, 1.0, chunk, {"forced": [dur[u]]}, loud=True)
        assert _cat(want[u][0]).size == frames[u] * hop
    syn.stream_open(chunk, 4, 96 * k, 64)
    r = admit("ABCD")
    assert r is not None and r[0] == [0, 1, 2, 3]
    slot = dict(zip("ABCD", r[0]))
    got = {u: [] for u in frames}
    name = {s: u for u, s in slot.items()}

    def step(stop=None):
        chunks, live = syn.stream_step(lambda s, pcm, off: name[s] == stop)
        for s, pcm, off in chunks:
            got[name[s]].append((off, pcm))
        return live
    assert step("A") == 3 and list(syn.stream_loudness()[0]) == [slot["A"]]
    r = admit("E")
    assert r is not None and r[0] == [slot["A"]]
    name[r[0][0]] = "E"
    assert step("C") == 3
    info = syn.stream_info()
    assert info["free_slots"] == 1 and info["free_frames"] == (96 - 6 - 6 - 40) * k
    assert admit("F") is None                                    # no room now: the tiles
    assert syn.stream_info() == info
    assert list(syn.stream_loudness()[0]) == [slot["C"]]         # (a refused admission leaves the last step's results too)
    while step():
        pass
    assert _same_chunks(got["B"], want["B"][0]) and _same_chunks(got["E"], want["E"][0])
    r = admit("F")                                               # the empty pools take it
    assert r is not None
    name = {r[0][0]: "F"}
    while step():
        pass
    assert _same_chunks(got["F"], want["F"][0]) and syn.stream_loudness()[1].tobytes() == want["F"][1]
    syn.stream_close()
    syn.close()


# ---- 7. the pool ------------------------------------------------------------------------------------------------------------------------
def test_pool_admits_a_late_request_with_the_eq_set():
    """one engine, a group of 4 streaming requests with the EQ set; a late request is submitted after the group's second step has
    delivered and joins the running stream.  The pool's engines choose their kernels themselves: the terms of include/summertts_hip.h for
    that are 1 LSB of the PCM against the single stream (the decoder's float outputs differ far below a rounding step, and behind the
    EQ the PCM still differs by a rounding step at most).  With eq_streaming off the submit is refused, as before."""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    late = sb.synthetic_ids(9, cfg.vocab, salt=77)
    syn = engine.Synthesizer(blob)
    syn.set_eq(BANDS4)
    syn.set_eq_streaming(True)
    want_late = _single(syn, late, 0, 1.0, 6)
    want = [_single(syn, ids[b], sids[b], ls[b], 6) for b in (1, 3, 5, 0)]
    syn.close()
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=8)
    pool.set_eq(BANDS4)
    pool.set_stream_admission(True)
    with pytest.raises(engine.StsError, match="finite halo"):
        pool.submit_stream(late, 6, lambda *a: False)
    pool.set_eq_streaming(True)
    three, queued, second = threading.Event(), threading.Event(), threading.Event()
    got = {k: [] for k in ("late", 0, 1, 2, 3)}
    events = []

    def on(k):
        def cb(pcm, off):
            events.append(k)
            got[k].append((off, pcm.copy()))
            if k == 0 and len(got[0]) == 1:
                assert three.wait(30.0)
            if k == 0 and len(got[0]) == 3:
                second.set()
                assert queued.wait(30.0)
            return False
        return cb
    tickets = [pool.submit_stream(ids[b], 6, on(i), sid=sids[b], length_scale=ls[b]) for i, b in enumerate((1, 3, 5, 0))]
    three.set()
    if not second.wait(60.0):
        queued.set()
        pytest.fail("the group's second step never delivered")
    tl = pool.submit_stream(late, 6, on("late"))
    queued.set()
    assert pool.wait(tl) == _cat(want_late).size
    for t, w in zip(tickets, want):
        assert pool.wait(t) == _cat(w).size
    groups, mid = pool.stream_stats()
    assert groups >= 1 and mid >= 1 and events.index("late") < max(i for i, e in enumerate(events) if e == 0)
    for k, w in [("late", want_late)] + list(enumerate(want)):
        assert [o for o, _ in got[k]] == [o for o, _ in w] and [p.size for _, p in got[k]] == [p.size for _, p in w], k
        d = np.abs(_cat(got[k]).astype(np.int64) - _cat(w).astype(np.int64))
        print(f"pool request {k}: {int((d != 0).sum())} of {d.size} samples differ from the single stream, max {int(d.max())}")
        assert int(d.max()) <= 1, k
    pool.set_eq_streaming(False)
    with pytest.raises(engine.StsError, match="equaliser"):
        pool.submit_stream(late, 6, lambda *a: False)
    pool.close()
