"""Planned open streams on the MI355X (sts_stream_open_ex, sts_pool_submit_stream_ex): utterances admitted with a duration plan, forced
durations, a speaker mix and a gain plan between the steps of a running stream, each against its own single stream with the same table --
chunk by chunk, bit for bit with the kernel variant pinned; slots and phoneme ranges reused under poison; room over phonemes; the tables'
lifetime and the states that stay refused; the split-bf16 repeat of an admission; captions; the adoption kernel against numpy; the pool."""
import threading

import numpy as np
import pytest

from conftest import golden_files, load_golden
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL, STS_ESTATE = -1, -4
INF = float("inf")
LENS = [9, 31, 5, 17, 1, 24]
LS = [1.0, 0.8, 1.2, 1.0, 1.1, 0.9]
CAPACITY = 4096
PHONEMES = 256
SCHEDULE = ((0, 1), "step", "step", (2,), "step", (3, 4, 5))

_kinds_cache = []


def _kinds():
    """one tiny golden model per kind (multi-speaker HiFi-GAN with its decoder conditioning among them)"""
    if not _kinds_cache:
        seen = set()
        for path in golden_files():
            g, cfg, blob = load_golden(path)
            if g["kind"].item() not in seen:
                seen.add(g["kind"].item())
                _kinds_cache.append((g["kind"].item(), cfg, blob))
        assert len(_kinds_cache) >= 5
    return _kinds_cache


def _batch(cfg, lens=LENS):
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate(lens)]
    nspk = max(int(cfg.spk_num), 1)
    sids = [(3 * u + 1) % nspk for u in range(len(lens))] if cfg.is_ms else [0] * len(lens)
    return ids, sids, LS[:len(lens)]


def _cat(chunks):
    return np.concatenate([p for _, p in chunks]) if chunks else np.zeros(0, np.int16)


def _same_chunks(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(got, want))


def _lsb(a, b):
    assert a.size == b.size, (a.size, b.size)
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()) if a.size else 0


def _set_tables(syn, n, tabs):
    """tabs: {"plan" | "mix" | "gain": one entry or None per utterance, "forced": packed durations}; a kind whose entries are all None is
    not set at all"""
    if tabs.get("plan") and any(p is not None for p in tabs["plan"]):
        syn.set_duration_plan(n, tabs["plan"])
    if tabs.get("mix") and any(m is not None for m in tabs["mix"]):
        syn.set_speaker_mix(tabs["mix"])
    if tabs.get("gain") and any(g is not None for g in tabs["gain"]):
        syn.set_gain_plan(n, tabs["gain"])
    if tabs.get("forced") is not None:
        syn.set_forced_durations(tabs["forced"])


def _pick(tabs, us, ids):
    """the tables of the utterances `us` out of per-utterance lists"""
    out = {k: [tabs[k][u] for u in us] for k in ("plan", "mix", "gain") if tabs.get(k)}
    if tabs.get("forced"):
        out["forced"] = np.concatenate([tabs["forced"][u] for u in us]) if all(tabs["forced"][u] is not None for u in us) else None
    return out


def _single(syn, ids, sid, ls, chunk, tabs=None):
    """the chunks of one utterance's own stream, its tables set just before it, as [(sample_offset, pcm)]"""
    if tabs:
        _set_tables(syn, [len(ids)], tabs)
    out = []
    syn.infer_ids_stream(ids, chunk, sid, ls, on_chunk=lambda pcm, off, t: out.append((off, pcm)) and False)
    return out


def _singles(syn, ids, sids, ls, chunk, tabs):
    return [_single(syn, ids[b], sids[b], ls[b], chunk, _pick(tabs, [b], ids)) for b in range(len(ids))]


def _run(syn, ids, sids, ls, tabs, schedule=SCHEDULE):
    """drives an open stream through `schedule`, the tables of every admission set right before it, then steps until it is empty"""
    got = [[] for _ in ids]
    total, utt_of = {}, {}

    def step():
        chunks, live = syn.stream_step()
        for s, pcm, off in chunks:
            got[utt_of[s]].append((off, pcm))
        return live
    for op in schedule:
        if op == "step":
            step()
            continue
        _set_tables(syn, [len(ids[u]) for u in op], _pick(tabs, op, ids))
        r = syn.stream_admit([ids[u] for u in op], [sids[u] for u in op], [ls[u] for u in op])
        assert r is not None, op
        for u, s, t in zip(op, *r):
            utt_of[s] = u
            total[u] = t
    for _ in range(100000):
        if step() == 0:
            break
    assert syn.stream_info()["live"] == 0
    return got, total


def _gains():
    """a mute, a +6 dB span and a -12 dB span; ramps of 5, 50 (h = 400 samples: wider than a frame) and 0 ms; on utterances 0, 3 and the
    1-phoneme utterance 4"""
    g = [None] * len(LENS)
    g[0] = {"gain_db": [0, 0, -INF, -INF, 0, 6, 6, 0, -12], "ramp_ms": 5.0}
    g[3] = {"gain_db": [0] * 3 + [6] * 5 + [0] * 2 + [-12] * 4 + [-INF] + [0] * 2, "ramp_ms": 50.0}
    g[4] = {"gain_db": [-12.0], "ramp_ms": 0.0}
    return g


def _mixes(cfg, sids):
    """two table terms plus a caller vector, an extrapolation with a negative weight, k = 1 with weight 1 (the plain sid), empty entries"""
    nspk, gin = int(cfg.spk_num), int(cfg.gin)
    vec = (0.1 * np.random.default_rng(5).standard_normal(gin)).astype(np.float32)
    m = [None] * len(LENS)
    m[0] = {"sid": [0, nspk - 1], "weight": [0.6, 0.3], "vector": vec, "vector_weight": 0.5}
    m[1] = {"sid": [1 % nspk, 2 % nspk], "weight": [1.5, -0.5]}
    m[2] = {"sid": [sids[2]], "weight": [1.0]}
    m[4] = {"sid": [], "weight": []}
    return m


def _plans():
    """a rate span, a `fixed` break, a target length"""
    p = [None] * len(LENS)
    p[0] = {"rate": [1.0] * 3 + [1.6] * 4 + [1.0] * 2}
    p[1] = {"fixed": [-1] * 10 + [12] + [-1] * 20}
    p[3] = {"target_frames": 61}
    return p


def _forced():
    return [np.array([(3 * u + i) % 4 + (1 if i == 0 else 0) for i in range(t)], np.int32) for u, t in enumerate(LENS)]


def _chunk_of(name, halo):
    return {"1": 1, "7": 7, "3halo+1": 3 * halo + 1}[name]


@pytest.mark.parametrize("chunk_name", ["1", "7", "3halo+1"])
@pytest.mark.parametrize("table", ["gain", "mix", "plan", "forced"])
def test_each_table_alone_equals_the_single_stream(table, chunk_name):
    for kind, cfg, blob in _kinds():
        if table == "mix" and not cfg.is_ms:
            continue
        ids, sids, ls = _batch(cfg)
        tabs = {"gain": {"gain": _gains()}, "mix": {"mix": _mixes(cfg, sids)} if cfg.is_ms else None, "plan": {"plan": _plans()},
                "forced": {"forced": _forced()}}[table]
        syn = engine.Synthesizer(blob)
        chunk = _chunk_of(chunk_name, syn.stream_halo_frames())
        syn.set_conv_mode(6)
        hop = int(syn.info.samples_per_frame)
        want = _singles(syn, ids, sids, ls, chunk, tabs)
        plain = _singles(syn, ids, sids, ls, chunk, {})
        syn.stream_open(chunk, len(ids), CAPACITY, PHONEMES)
        assert syn.stream_tables_info() == {"planned": True, "capacity_phonemes": PHONEMES, "free_phonemes": PHONEMES}
        got, total = _run(syn, ids, sids, ls, tabs)
        assert syn.stream_tables_info()["free_phonemes"] == PHONEMES
        syn.stream_close()
        for b in range(len(ids)):
            assert _same_chunks(got[b], want[b]), (kind, table, chunk, b)
            assert total[b] == _cat(want[b]).size, (kind, table, chunk, b)
        if table == "gain":          # a slot without a plan, stepped next to slots with one: its unplanned stream, bit for bit
            for b in (1, 2, 5):
                assert _same_chunks(got[b], plain[b]), (kind, chunk, b)
            for b in (0, 3, 4):
                assert not np.array_equal(_cat(got[b]), _cat(plain[b])), (kind, chunk, b)
        if table == "mix":           # k = 1, weight = 1 is the plain sid; the blends are not
            assert _same_chunks(got[2], plain[2]) and _same_chunks(got[4], plain[4]), kind
            assert not np.array_equal(_cat(got[0]), _cat(plain[0])) and not np.array_equal(_cat(got[1]), _cat(plain[1])), kind
        if table == "plan":
            assert total[3] == 61 * hop and total[3] != _cat(plain[3]).size, kind
            assert total[0] != _cat(plain[0]).size or not np.array_equal(_cat(got[0]), _cat(plain[0])), kind
        if table == "forced":
            assert [total[b] for b in range(len(ids))] == [max(int(d.sum()), 1) * hop for d in _forced()], kind
        syn.close()


def _all_tables(cfg, sids):
    return {"gain": _gains(), "mix": _mixes(cfg, sids), "plan": _plans()}


def test_all_three_tables_at_22050_with_the_limiter():
    """the gain stage sits in front of the resampler's and the limiter's halos"""
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    tabs = _all_tables(cfg, sids)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(22050)
    syn.set_limiter(engine.LIMITER_ON, 12.0, -1.0, 1.0)
    hop = int(syn.info.samples_per_frame)
    want = _singles(syn, ids, sids, ls, 6, tabs)
    syn.stream_open(6, len(ids), CAPACITY, PHONEMES)
    got, total = _run(syn, ids, sids, ls, tabs)
    syn.stream_close()
    for b in range(len(ids)):
        assert _same_chunks(got[b], want[b]), b
        assert total[b] == _cat(want[b]).size, b
    assert total[3] == -(-61 * hop * 22050 // 16000)
    syn.close()


def test_automatic_kernel_choice_is_within_one_lsb():
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    tabs = _all_tables(cfg, sids)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    want = _singles(syn, ids, sids, ls, 7, tabs)
    syn.set_conv_mode(0)
    syn.stream_open(7, len(ids), CAPACITY, PHONEMES)
    got, total = _run(syn, ids, sids, ls, tabs)
    syn.stream_close()
    for b in range(len(ids)):
        assert total[b] == _cat(want[b]).size and _lsb(_cat(got[b]), _cat(want[b])) <= 1, b
    syn.close()


@pytest.mark.parametrize("pattern", [0x7FC00000, 0x7BFF7BFF])
def test_stale_tables_under_poison(pattern):
    """max_live = 2 and a phoneme pool of one utterance's plan: the slot and the phoneme range a gain-planned, mixed utterance frees are
    taken by a plain one and by a differently planned one; each equals its own single stream"""
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    nspk = int(cfg.spk_num)
    A, Cp, D, E = 0, 2, 3, 5
    tabs = {"gain": [None] * 6, "mix": [None] * 6}
    tabs["gain"][A] = {"gain_db": [-INF, 6, 6, 0, -12, -12, 0, 3, -INF], "ramp_ms": 50.0}
    tabs["mix"][A] = {"sid": [0, nspk - 1], "weight": [0.5, 0.5]}
    tabs["gain"][D] = {"gain_db": [3.0] * 8 + [-20.0] * 9, "ramp_ms": 2.0}
    tabs["gain"][E] = {"gain_db": [-6.0] * 24, "ramp_ms": 0.0}
    tabs["mix"][E] = {"sid": [1 % nspk], "weight": [-1.0]}
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    chunk = 5
    want = _singles(syn, ids, sids, ls, chunk, tabs)
    syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
    syn.stream_open(chunk, 2, CAPACITY, 24)
    got = [[] for _ in ids]
    for op in ((A,), (Cp, D), (E,)):          # A alone; then the plain one into A's slot, the planned one over A's phonemes; then E over both
        _set_tables(syn, [len(ids[u]) for u in op], _pick(tabs, op, ids))
        r = syn.stream_admit([ids[u] for u in op], [sids[u] for u in op], [ls[u] for u in op])
        assert r is not None and r[0] == list(range(len(op))), op
        assert syn.stream_tables_info()["free_phonemes"] == 24 - sum(len(ids[u]) for u in op if tabs["gain"][u])
        utt_of = dict(zip(r[0], op))
        while True:
            chunks, live = syn.stream_step()
            for s, pcm, off in chunks:
                got[utt_of[s]].append((off, pcm))
            if live == 0:
                break
        assert syn.stream_tables_info()["free_phonemes"] == 24
    syn.stream_close()
    syn.debug_set("poison", 0)
    for b in (A, Cp, D, E):
        assert _same_chunks(got[b], want[b]), b
    syn.close()


def test_room_over_phonemes_and_consumption():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    X, P0, P1 = 2, 0, 3
    gain = [None] * 6
    gain[X] = {"gain_db": [-6.0] * LENS[X], "ramp_ms": 1.0}
    gain[P0] = _gains()[0]
    gain[P1] = _gains()[3]
    tabs = {"gain": gain}
    cap = LENS[X] + LENS[P0] + LENS[P1] - 1          # one short of the pair's needs while X lives
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    chunk = 4
    want = _singles(syn, ids, sids, ls, chunk, tabs)
    plain = _singles(syn, ids, sids, ls, chunk, {})
    syn.stream_open(chunk, 3, CAPACITY, cap)
    _set_tables(syn, [LENS[X]], _pick(tabs, [X], ids))
    rx = syn.stream_admit([ids[X]], [sids[X]], [ls[X]])
    assert rx is not None
    info, tinfo = syn.stream_info(), syn.stream_tables_info()
    assert tinfo == {"planned": True, "capacity_phonemes": cap, "free_phonemes": cap - LENS[X]}
    pair = [P0, P1]
    args = ([ids[u] for u in pair], [sids[u] for u in pair], [ls[u] for u in pair])
    _set_tables(syn, [LENS[u] for u in pair], _pick(tabs, pair, ids))
    assert syn.stream_admit(*args) is None                                   # slots and frames suffice: the phonemes do not
    assert syn.stream_info() == info and syn.stream_tables_info() == tinfo
    # the refused admission consumed the plans: the same pair, nothing set again, runs unplanned
    r = syn.stream_admit(*args)
    assert r is not None and syn.stream_tables_info() == tinfo
    utt_of = {rx[0][0]: X, r[0][0]: P0, r[0][1]: P1}
    got = {u: [] for u in (X, P0, P1)}

    def drain():
        while True:
            chunks, live = syn.stream_step()
            for s, pcm, off in chunks:
                got[utt_of[s]].append((off, pcm))
            if live == 0:
                return
    drain()
    assert _same_chunks(got[X], want[X]) and _same_chunks(got[P0], plain[P0]) and _same_chunks(got[P1], plain[P1])
    # X has retired: with the plans set again the pair fits, and runs planned
    assert syn.stream_tables_info()["free_phonemes"] == cap
    _set_tables(syn, [LENS[u] for u in pair], _pick(tabs, pair, ids))
    r = syn.stream_admit(*args)
    assert r is not None and syn.stream_tables_info()["free_phonemes"] == cap - LENS[P0] - LENS[P1]
    utt_of = {r[0][0]: P0, r[0][1]: P1}
    got = {u: [] for u in (X, P0, P1)}
    drain()
    assert _same_chunks(got[P0], want[P0]) and _same_chunks(got[P1], want[P1])
    syn.stream_close()
    syn.close()


def test_wrong_shape_and_states():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    ids = sb.synthetic_ids(9, cfg.vocab)
    other = sb.synthetic_ids(5, cfg.vocab, salt=4)
    syn = engine.Synthesizer(blob)
    lib = syn.lib
    syn.set_conv_mode(6)
    gplan = {"gain_db": [0, 0, -INF, -INF, 0, 6, 6, 0, -12], "ramp_ms": 5.0}
    plain = _single(syn, ids, 0, 1.0, 8)
    gained = _single(syn, ids, 0, 1.0, 8, {"gain": [gplan]})
    assert not np.array_equal(_cat(plain), _cat(gained))
    # refused at open, as sts_stream_open refuses: an equaliser, loudness, a pending plan; bad capacities
    syn.set_eq([(engine.EQ_PEAK, 1000.0, 3.0, 1.0)])
    assert lib.sts_stream_open_ex(syn.h, 8, 2, 1000, 64) == STS_EINVAL
    syn.set_eq(None)
    syn.set_loudness(engine.LOUD_MEASURE)
    assert lib.sts_stream_open_ex(syn.h, 8, 2, 1000, 64) == STS_EINVAL
    syn.set_loudness(engine.LOUD_OFF)
    syn.set_gain_plan([len(ids)], [gplan])
    assert lib.sts_stream_open_ex(syn.h, 8, 2, 1000, 64) == STS_EINVAL
    syn.set_gain_plan(None)
    for cap_p in (-1, (1 << 24) + 1):
        assert lib.sts_stream_open_ex(syn.h, 8, 2, 1000, cap_p) == STS_EINVAL, cap_p
    assert not syn.stream_info()["open"]
    # capacity_phonemes == 0 is sts_stream_open: the four setters stay refused
    assert lib.sts_stream_open_ex(syn.h, 8, 2, 1000, 0) == 0
    assert syn.stream_tables_info() == {"planned": False, "capacity_phonemes": 0, "free_phonemes": 0}
    d = np.ones(len(ids), np.int32)
    for call in (lambda: syn.set_gain_plan([len(ids)], [gplan]), lambda: syn.set_duration_plan([len(ids)], [{"target_frames": 30}]),
                 lambda: syn.set_speaker_mix([None]), lambda: syn.set_forced_durations(d)):
        with pytest.raises(engine.StsError, match="sts error -4"):
            call()
    syn.stream_close()
    # a planned stream: the four work, everything else open fixed stays refused
    syn.stream_open(8, 2, 1000, 64)
    assert lib.sts_set_output_rate(syn.h, 44100) == STS_ESTATE and lib.sts_set_conv_mode(syn.h, 6) == STS_ESTATE
    assert lib.sts_set_limiter(syn.h, 1, 0.0, -1.0, 5.0) == STS_ESTATE and lib.sts_set_record_taps(syn.h, 1) == STS_ESTATE
    with pytest.raises(engine.StsError, match="sts error -4"):
        syn.infer_ids(ids)
    # a gain plan for B = 2, an admission of 1: STS_EINVAL, nothing admitted, the plan dropped
    syn.set_gain_plan([len(ids), len(other)], [gplan, None])
    with pytest.raises(engine.StsError, match="sts error -1"):
        syn.stream_admit([ids])
    assert syn.stream_info() == {"open": True, "live": 0, "free_slots": 2, "free_frames": 1000, "steps": 0}
    assert syn.stream_tables_info()["free_phonemes"] == 64
    # ... and a plan for other phoneme counts
    syn.set_gain_plan([len(other)], [{"gain_db": [0.0] * len(other)}])
    with pytest.raises(engine.StsError, match="sts error -1"):
        syn.stream_admit([ids])
    # a duration plan together with forced durations: STS_EINVAL, both dropped
    syn.set_duration_plan([len(ids)], [{"target_frames": 30}])
    syn.set_forced_durations(d)
    with pytest.raises(engine.StsError, match="sts error -1"):
        syn.stream_admit([ids])
    # the stream still works, and none of the dropped tables applies
    r = syn.stream_admit([ids])
    assert r is not None and r[1] == [_cat(plain).size]
    got = []
    while True:
        chunks, live = syn.stream_step()
        got += [(off, pcm) for _, pcm, off in chunks]
        if live == 0:
            break
    assert _same_chunks(got, plain)
    syn.stream_close()
    assert np.array_equal(_cat(_single(syn, ids, 0, 1.0, 8)), _cat(plain))
    syn.close()


def test_the_split_bf16_repeat_of_an_admission_applies_its_plan():
    """STS_DBG_STREAM_RETRY_STEP = -2 under conv math 3: the overflow word counts as raised in the admission, which is repeated in form 0
    with the same tables -- the utterance's length is the planned one and its PCM within 1 LSB of the bf16x3 single stream with that plan.
    (The hook then names step 0, so that the steps decode in form 0 too, as the reference does.)"""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = sb.synthetic_ids(20, cfg.vocab)
    tabs = {"plan": [{"target_frames": 77}], "gain": [{"gain_db": [0.0] * 8 + [-9.0] * 6 + [-INF] * 2 + [6.0] * 4, "ramp_ms": 10.0}]}
    forced = {"forced": np.array([(i % 3) + 1 for i in range(20)], np.int32), "gain": tabs["gain"]}
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    hop = int(syn.info.samples_per_frame)
    syn.set_conv_math("bf16x3")
    want = _cat(_single(syn, ids, 0, 1.0, 8, tabs))
    want_f = _cat(_single(syn, ids, 0, 1.0, 8, forced))
    assert want.size == 77 * hop and want_f.size == int(forced["forced"].sum()) * hop
    syn.set_conv_math("f16x2")
    for t, w in ((tabs, want), (forced, want_f)):          # (forced durations are consumed by the duration stage: the repeat gets them again)
        syn.stream_open(8, 2, CAPACITY, PHONEMES)
        syn.debug_set("stream_retry_step", -2)
        before = syn.profile()["conv_math_fallbacks"]
        _set_tables(syn, [len(ids)], t)
        r = syn.stream_admit([ids])
        assert r is not None and r[1] == [w.size]
        assert syn.profile()["conv_math_fallbacks"] == before + 1
        syn.debug_set("stream_retry_step", 0)
        got = []
        while True:
            chunks, live = syn.stream_step()
            got += [pcm for _, pcm, _ in chunks]
            if live == 0:
                break
        syn.debug_set("stream_retry_step", -1)
        syn.stream_close()
        assert _lsb(np.concatenate(got), w) <= 1
    syn.close()


def test_captions_after_a_planned_admission():
    cfg = sb.tiny_cfg("mbb_fix")
    blob = sb.make_blob(cfg, 5)
    ids, sids, ls = _batch(cfg, LENS[:3])
    plans = [{"rate": [1.0] * 3 + [1.6] * 4 + [1.0] * 2}, {"target_frames": 90}, None]
    syn = engine.Synthesizer(blob)
    syn.set_output_rate(22050)
    want_d, want_o = [], []
    for b in range(3):
        _single(syn, ids[b], sids[b], ls[b], 8, {"plan": [plans[b]]})
        want_d.append(syn.durations(LENS[b]))
        want_o.append(syn.phoneme_offsets(LENS[b]))
    syn.stream_open(8, 3, CAPACITY, PHONEMES)
    _set_tables(syn, LENS[:3], {"plan": plans})
    assert syn.stream_admit(ids, sids, ls) is not None
    T = sum(LENS[:3])
    assert np.array_equal(syn.durations(T), np.concatenate(want_d)) and np.array_equal(syn.phoneme_offsets(T), np.concatenate(want_o))
    syn.stream_close()
    # ... and a plain admission into an unplanned stream reports its own
    syn.stream_open(8, 3, CAPACITY)
    assert syn.stream_admit([ids[2]], [sids[2]], [ls[2]]) is not None
    assert np.array_equal(syn.durations(LENS[2]), want_d[2]) and np.array_equal(syn.phoneme_offsets(LENS[2]), want_o[2])
    syn.stream_close()
    syn.close()


@pytest.mark.parametrize("B", [1, 7])
def test_debug_adopt_tables_against_numpy(B):
    """gin not a multiple of 4; phoneme counts 1, 3, 64, 257; unaligned source and destination offsets; a newcomer that carries no
    phonemes and one without a slot; the three destinations come back unchanged outside the ranges"""
    rng = np.random.default_rng(B)
    gin, max_live, cap = 13, 9, 700
    ns = [257] if B == 1 else [1, 3, 0, 64, 257, 5, 2]
    slot = [4] if B == 1 else [8, 0, 3, 5, 1, -1, 7]
    src_off, s = [], 1
    for i, n in enumerate(ns):
        src_off.append(s)
        s += n + (i % 3) + 1
    n_src = s + 5
    dst_off, d = [0] * B, 3                    # the pool's ranges in another order than the table's, at offsets of every alignment
    for i in rng.permutation(B):
        dst_off[i] = d
        d += ns[i] + (i % 2)
    assert d <= cap
    g = rng.standard_normal((gin, B)).astype(np.float32)
    gpool = rng.standard_normal((gin, max_live)).astype(np.float32)
    cum = rng.integers(0, 1 << 20, n_src).astype(np.int32)
    q = rng.integers(0, 1 << 24, n_src).astype(np.int32)
    pool = rng.integers(-9, 9, (2, cap + 1)).astype(np.int32)
    words = rng.integers(-9, 9, (3, max_live)).astype(np.int32)
    h = [int(v) for v in rng.integers(0, 401, B)]
    wg, wp, ww = gpool.copy(), pool.copy(), words.copy()
    for b in range(B):
        if slot[b] < 0:
            continue
        wg[:, slot[b]] = g[:, b]
        if ns[b] > 0:
            wp[0, dst_off[b]:dst_off[b] + ns[b]] = cum[src_off[b]:src_off[b] + ns[b]]
            wp[1, dst_off[b]:dst_off[b] + ns[b]] = q[src_off[b]:src_off[b] + ns[b]]
            ww[:, slot[b]] = (dst_off[b], ns[b], h[b])
        else:
            ww[:, slot[b]] = (cap, 1, 0)
    got_g, got_p, got_w = engine.debug_adopt_tables(g, gpool, cum, q, pool, words, slot, src_off, ns, dst_off, h)
    assert np.array_equal(got_g.view(np.uint32), wg.view(np.uint32)) and np.array_equal(got_p, wp) and np.array_equal(got_w, ww)
    # no conditioning vectors (a single-speaker model): the phonemes and the words alone
    _, got_p, got_w = engine.debug_adopt_tables(None, None, cum, q, pool, words, slot, src_off, ns, dst_off, h)
    assert np.array_equal(got_p, wp) and np.array_equal(got_w, ww)
    # refusals (tests/test_live_tables_cpu.py has the rest)
    with pytest.raises(engine.StsError):
        engine.debug_adopt_tables(g, gpool, cum, q, pool, words, slot, src_off, ns, [cap - 1] * B, h)
    if B > 1:
        with pytest.raises(engine.StsError):
            engine.debug_adopt_tables(g, gpool, cum, q, pool, words, slot, src_off, ns, [dst_off[4]] * B, h)


@pytest.mark.parametrize("admission", [True, False])
def test_pool_admits_a_planned_request_midstream(admission):
    """one engine, a group of 4 plain streaming requests; the planned request (all three tables) is submitted after the group's second
    step has delivered.  With admission on it joins the running stream; with it off it runs as a closed group behind it.  Either way its
    samples are within 1 LSB of an engine's single stream with the same tables, and its length is the planned one."""
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    nspk = int(cfg.spk_num)
    late = sb.synthetic_ids(9, cfg.vocab, salt=77)
    plan = {"target_frames": 45}
    mix = {"sid": [0, nspk - 1], "weight": [0.7, 0.3]}
    gain = _gains()[0]
    syn = engine.Synthesizer(blob)
    hop = int(syn.info.samples_per_frame)
    want_late = _cat(_single(syn, late, 1, 1.0, 6, {"plan": [plan], "mix": [mix], "gain": [gain]}))
    want = [_cat(_single(syn, ids[b], sids[b], ls[b], 6)) for b in (1, 3, 5, 0)]
    syn.close()
    assert want_late.size == 45 * hop
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=8)
    if admission:
        pool.set_stream_admission(True)
    three, queued, second = threading.Event(), threading.Event(), threading.Event()
    got = {k: [] for k in ("late", 0, 1, 2, 3)}
    events = []

    def on(k):
        def cb(pcm, off):
            events.append(k)
            got[k].append(pcm)
            if k == 0 and len(got[0]) == 1:          # (its worker waits here until the other three are queued: they join at the next step)
                assert three.wait(30.0)
            if k == 0 and len(got[0]) == 3:          # the longest member's third chunk: the group of 4 has stepped twice
                second.set()
                assert queued.wait(30.0)
            return False
        return cb
    tickets = [pool.submit_stream(ids[b], 6, on(i), sid=sids[b], length_scale=ls[b]) for i, b in enumerate((1, 3, 5, 0))]
    three.set()
    if not second.wait(60.0):
        queued.set()
        pytest.fail("the group's second step never delivered")
    tl = pool.submit_stream(late, 6, on("late"), sid=1, plan=plan, mix=mix, gain=gain)
    queued.set()
    assert pool.wait(tl) == want_late.size
    for t, w in zip(tickets, want):
        assert pool.wait(t) == w.size
    groups, mid = pool.stream_stats()
    first_late = events.index("late")
    last_group = max(i for i, e in enumerate(events) if e == 0)
    if admission:
        assert mid >= 1 and first_late < last_group
    else:
        assert mid == 0 and groups == 0 and first_late > last_group
    assert _lsb(np.concatenate(got["late"]), want_late) <= 1
    for i, w in enumerate(want):
        assert _lsb(np.concatenate(got[i]), w) <= 1, i
    # all three NULL is sts_pool_submit_stream
    lib, arr = pool.lib, np.ascontiguousarray(late, np.int32)

    def raw(ex):
        out = []

        def _cb(user, pcm, ns, off):
            out.append(np.ctypeslib.as_array(pcm, shape=(ns,)).copy())
            return 0
        cb = engine.CHUNK_CB(_cb)
        head = (pool.h, arr.ctypes.data, arr.size, 1, 1.0, 0.0, 0.0, 0, 6, cb, None)
        t = int(lib.sts_pool_submit_stream_ex(*head, None, None, None) if ex else lib.sts_pool_submit_stream(*head))
        assert t > 0
        pool._streams[t] = cb
        assert pool.wait(t) > 0
        return np.concatenate(out)
    assert np.array_equal(raw(True), raw(False))
    pool.close()
