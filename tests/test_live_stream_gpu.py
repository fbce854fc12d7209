"""Open streams on the MI355X (sts_stream_open / admit / step / close, sts_pool_set_stream_admission): utterances admitted between the
steps of a running stream against each one's own single stream -- chunk by chunk, bit for bit with the kernel variant pinned -- at every
output rate, with the limiter, with slots and pool columns reused, with a stopped slot, with per-utterance noise, through the split-bf16
repeat of a step; the states that are refused; the adoption kernel against numpy; and the pool admitting a late request into a running
group."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import golden_files, load_golden
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL, STS_ESTATE = -1, -4
LENS = [9, 31, 5, 17, 1, 24]
LS = [1.0, 0.8, 1.2, 1.0, 1.1, 0.9]
CAPACITY = 4096
# admit {0, 1}; two steps; admit {2}; one step; admit {3, 4, 5}; steps until empty
SCHEDULE = ((0, 1), "step", "step", (2,), "step", (3, 4, 5))

_kinds_cache = []
_ref_cache = {}


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


def _single(syn, ids, sid, ls, chunk):
    """the chunks of one utterance's own stream as [(sample_offset, pcm)]"""
    out = []
    syn.infer_ids_stream(ids, chunk, sid, ls, on_chunk=lambda pcm, off, t: out.append((off, pcm)) and False)
    return out


def _same_chunks(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(got, want))


def _lsb(a, b):
    assert a.size == b.size, (a.size, b.size)
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()) if a.size else 0


def _run(syn, ids, sids, ls, schedule=SCHEDULE, noise=None, stop=None, steps_seen=None):
    """drives an open stream through `schedule` (tuples admit those utterances, "step" steps once), then steps until it is empty.  Returns
    (per-utterance [(sample_offset, pcm)], per-utterance totals from the admission).  stop: utterances whose first chunk's callback stops them"""
    got = [[] for _ in ids]
    total = {}
    utt_of = {}

    def step():
        chunks, live = syn.stream_step(on_chunk=lambda s, pcm, off: stop is not None and utt_of[s] in stop)
        if steps_seen is not None:
            steps_seen.append([(utt_of[s], off, pcm.size) for s, pcm, off in chunks])
        for s, pcm, off in chunks:
            got[utt_of[s]].append((off, pcm))
        return live
    for op in schedule:
        if op == "step":
            step()
            continue
        r = syn.stream_admit([ids[u] for u in op], [sids[u] for u in op], [ls[u] for u in op], noise=None if noise is None else [noise[u] for u in op])
        assert r is not None, op
        for u, s, t in zip(op, *r):
            utt_of[s] = u
            total[u] = t
    for _ in range(100000):
        if step() == 0:
            break
    assert syn.stream_info()["live"] == 0
    return got, total


def _chunk_of(name, halo):
    return {"1": 1, "7": 7, "halo": halo, "3halo+1": 3 * halo + 1}[name]


@pytest.mark.parametrize("chunk_name", ["1", "7", "halo", "3halo+1"])
def test_staggered_admission_equals_the_single_stream(chunk_name):
    for kind, cfg, blob in _kinds():
        ids, sids, ls = _batch(cfg)
        syn = engine.Synthesizer(blob)
        chunk = _chunk_of(chunk_name, syn.stream_halo_frames())
        syn.set_conv_mode(6)
        want = [_single(syn, ids[b], sids[b], ls[b], chunk) for b in range(len(ids))]
        syn.stream_open(chunk, len(ids), CAPACITY)
        got, total = _run(syn, ids, sids, ls)
        syn.stream_close()
        for b in range(len(ids)):
            assert _same_chunks(got[b], want[b]), (kind, chunk, b)
            assert total[b] == _cat(want[b]).size, (kind, chunk, b)
        if chunk_name in ("7", "3halo+1"):
            # automatic kernel choice: within 1 LSB of the pinned result and of the oracle
            if kind not in _ref_cache:
                port = pyref.PortModel(blob)
                _ref_cache[kind] = [port.infer_ids(ids[b], sids[b], ls[b])["pcm"] for b in range(len(ids))]
            syn.set_conv_mode(0)
            syn.stream_open(chunk, len(ids), CAPACITY)
            auto, _ = _run(syn, ids, sids, ls)
            syn.stream_close()
            for b in range(len(ids)):
                assert _lsb(_cat(auto[b]), _cat(want[b])) <= 1, (kind, chunk, b)
                assert _lsb(_cat(auto[b]), _ref_cache[kind][b]) <= 1, (kind, chunk, b, "oracle")
        syn.close()


@pytest.mark.parametrize("kind", ["hifigan_sdp", "mbb_fix"])
@pytest.mark.parametrize("rate", [8000, 44100, 48000])
@pytest.mark.parametrize("lim", [False, True])
def test_resampler_and_limiter(kind, rate, lim):
    cfg = sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if lim:
        syn.set_limiter(engine.LIMITER_ON, 20.0, -1.0, 1.0)
    want = [_single(syn, ids[b], sids[b], ls[b], 6) for b in range(len(ids))]
    syn.stream_open(6, len(ids), CAPACITY)
    got, total = _run(syn, ids, sids, ls)
    syn.stream_close()
    for b in range(len(ids)):
        assert _same_chunks(got[b], want[b]), b
        assert total[b] == _cat(want[b]).size, b
    syn.close()


def _frames(syn, ids, sids, ls):
    syn.infer_batch(ids, sids, ls)
    dur = syn.durations(sum(len(x) for x in ids))
    toff = np.concatenate([[0], np.cumsum([len(x) for x in ids])])
    return [int(dur[toff[b]:toff[b + 1]].sum()) for b in range(len(ids))]


@pytest.mark.parametrize("pattern", [0, 0x7FC00000, 0x7BFF7BFF])
def test_reuse_and_room(pattern):
    """max_live = 2 and a pool of exactly the two first utterances' frames: the third is refused while both live, and is admitted into the
    shorter one's slot and columns once that has retired"""
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    F = _frames(syn, ids, sids, ls)
    order = sorted(range(len(ids)), key=lambda b: (F[b], b))
    c, s, a = order[0], order[1], order[-1]          # the third (no longer than the short one), the short one, the long one
    assert 0 < F[c] <= F[s] < F[a]
    chunk = 4
    assert -(-F[a] // chunk) > -(-F[s] // chunk) + 1           # the long one is still live after the short one has retired
    want = {b: _single(syn, ids[b], sids[b], ls[b], chunk) for b in (a, s, c)}
    if pattern:
        syn.debug_set("poison", pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
    syn.stream_open(chunk, 2, F[a] + F[s])
    r = syn.stream_admit([ids[a], ids[s]], [sids[a], sids[s]], [ls[a], ls[s]])
    assert r is not None and sorted(r[0]) == [0, 1] and r[1] == [_cat(want[a]).size, _cat(want[s]).size]
    utt_of = {r[0][0]: a, r[0][1]: s}
    info = syn.stream_info()
    assert info == {"open": True, "live": 2, "free_slots": 0, "free_frames": 0, "steps": 0}
    assert syn.stream_admit([ids[c]], [sids[c]], [ls[c]]) is None and syn.stream_info() == info        # no slot
    got = {b: [] for b in (a, s, c)}

    def step():
        chunks, live = syn.stream_step()
        for slot, pcm, off in chunks:
            got[utt_of[slot]].append((off, pcm))
        return live
    while step() == 2:
        pass
    info = syn.stream_info()
    assert info["live"] == 1 and info["free_slots"] == 1 and info["free_frames"] == F[s]
    r3 = syn.stream_admit([ids[c]], [sids[c]], [ls[c]])
    assert r3 is not None and r3[0] == [r[0][1]] and r3[1] == [_cat(want[c]).size]       # the freed slot (and, the pool being full, its columns)
    utt_of[r3[0][0]] = c
    assert syn.stream_info()["free_frames"] == F[s] - F[c]
    while step() > 0:
        pass
    info = syn.stream_info()
    assert info["live"] == 0 and info["free_slots"] == 2 and info["free_frames"] == F[a] + F[s]
    syn.stream_close()
    assert syn.stream_info() == {"open": False, "live": 0, "free_slots": 0, "free_frames": 0, "steps": 0}
    for b in (a, s, c):
        assert _same_chunks(got[b], want[b]), b
    syn.close()


def test_stop_and_close():
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    before = syn.infer_ids(ids[1], sids[1], ls[1])
    want = [_single(syn, ids[b], sids[b], ls[b], 4) for b in range(len(ids))]
    syn.stream_open(4, len(ids), CAPACITY)
    got, _ = _run(syn, ids, sids, ls, stop={1, 3})
    for b in range(len(ids)):
        if b in (1, 3):          # stopped by its first chunk's callback: that chunk alone, and its slot has retired
            assert len(got[b]) == 1 and _same_chunks(got[b], want[b][:1]), b
        else:
            assert _same_chunks(got[b], want[b]), b
    # close with live slots: nothing more is delivered, and the engine is what it was
    assert syn.stream_admit([ids[1], ids[5]], [sids[1], sids[5]], [ls[1], ls[5]]) is not None
    chunks, live = syn.stream_step()
    assert live == 2 and len(chunks) == 2
    syn.stream_close()
    assert not syn.stream_info()["open"]
    assert np.array_equal(syn.infer_ids(ids[1], sids[1], ls[1]), before)
    syn.close()


def test_noise_per_utterance_and_seed_plus_b():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    noise = [(0.667, 0.8, 1000 + 17 * u) if u % 2 == 0 else (0.3, 0.0, 5 + u) for u in range(len(ids))]
    want = []
    for b in range(len(ids)):
        syn.set_noise(*noise[b])
        want.append(_single(syn, ids[b], sids[b], ls[b], 9))
    syn.set_noise(0.0, 0.0, 0)
    syn.stream_open(9, len(ids), CAPACITY)
    got, _ = _run(syn, ids, sids, ls, noise=noise)
    for b in range(len(ids)):
        assert _same_chunks(got[b], want[b]), b
    # NULL: the engine's setting, utterance b of each ADMISSION with seed + b
    s = 77
    syn.set_noise(0.667, 0.8, s)
    got, _ = _run(syn, ids, sids, ls)
    syn.stream_close()
    pos = {}
    for op in SCHEDULE:
        if op != "step":
            pos.update({u: i for i, u in enumerate(op)})
    for b in range(len(ids)):
        syn.set_noise(0.667, 0.8, s + pos[b])
        assert _same_chunks(got[b], _single(syn, ids[b], sids[b], ls[b], 9)), b
    syn.close()


def test_retry_of_a_step_in_split_bf16():
    """STS_DBG_STREAM_RETRY_STEP = 1 under conv math 3: the overflow word counts as raised behind step 1 -- step 0's chunks are the two-term
    fp16 ones, step 1 and every later one are decoded in split-bf16 (admissions after it too), no chunk arrives twice, and
    conv_math_fallbacks rises by one.  Forced durations are not available to an open stream: both maths must agree on the frame counts,
    which the test checks before it compares."""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate((20, 7, 13))]
    sids, ls = [0, 0, 0], [1.0, 1.0, 1.0]
    schedule = ((0, 1), "step", "step", (2,))
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_conv_math("f16x2")
    syn.stream_open(8, 3, CAPACITY)
    plain, tot_plain = _run(syn, ids, sids, ls, schedule)
    syn.stream_close()
    syn.set_conv_math("bf16x3")
    syn.stream_open(8, 3, CAPACITY)
    bf3, tot_bf3 = _run(syn, ids, sids, ls, schedule)
    syn.stream_close()
    assert tot_plain == tot_bf3, "the two arithmetics disagree on a frame count: choose other utterances"
    syn.set_conv_math("f16x2")
    before = syn.profile()["conv_math_fallbacks"]
    syn.debug_set("stream_retry_step", 1)
    syn.stream_open(8, 3, CAPACITY)
    steps = []
    got, tot = _run(syn, ids, sids, ls, schedule, steps_seen=steps)
    assert syn.profile()["conv_math_fallbacks"] == before + 1
    syn.stream_close()
    syn.debug_set("stream_retry_step", -1)
    assert tot == tot_plain
    for b in range(len(ids)):
        assert len(got[b]) == len(plain[b]) == len(bf3[b]), b
        assert [o for o, _ in got[b]] == list(np.cumsum([0] + [p.size for _, p in got[b]])[:-1]), b       # every chunk once, in order
    for u, off, n in steps[0]:
        assert off == 0 and np.array_equal(got[u][0][1], plain[u][0][1]), u          # step 0 is unchanged
    for b in range(len(ids)):
        first = 1 if b in (0, 1) else 0          # utterance 2 arrives behind step 1: all of it in split-bf16
        for i in range(first, len(got[b])):
            assert _lsb(got[b][i][1], bf3[b][i][1]) <= 1, (b, i)
    syn.close()


def test_states_and_arguments():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    ids = sb.synthetic_ids(9, cfg.vocab)
    syn = engine.Synthesizer(blob)
    lib = syn.lib
    # refused at open: an equaliser, loudness, a pending gain plan
    syn.set_eq([(engine.EQ_PEAK, 1000.0, 3.0, 1.0)])
    assert lib.sts_stream_open(syn.h, 8, 2, 1000) == STS_EINVAL
    syn.set_eq(None)
    syn.set_loudness(engine.LOUD_MEASURE)
    assert lib.sts_stream_open(syn.h, 8, 2, 1000) == STS_EINVAL
    syn.set_loudness(engine.LOUD_OFF)
    syn.set_gain_plan([len(ids)], [{"gain_db": [0.0] * len(ids)}])
    assert lib.sts_stream_open(syn.h, 8, 2, 1000) == STS_EINVAL
    syn.set_gain_plan(None)
    # bad arguments
    for args in ((0, 2, 1000), (8, 0, 1000), (8, 1025, 1000), (8, 2, 0), (8, 2, 1 << 40)):
        assert lib.sts_stream_open(syn.h, *args) == STS_EINVAL, args
    # nothing is open
    assert lib.sts_stream_close(syn.h) == STS_ESTATE
    assert lib.sts_stream_step(syn.h, engine.BATCH_CHUNK_CB(lambda *a: 0), None, None) == STS_ESTATE
    with pytest.raises(engine.StsError):
        syn.stream_admit([ids])
    whole = syn.infer_ids(ids)
    syn.stream_open(8, 2, 1000)
    assert lib.sts_stream_open(syn.h, 8, 2, 1000) == STS_ESTATE
    assert lib.sts_set_output_rate(syn.h, 44100) == STS_ESTATE
    assert lib.sts_set_conv_mode(syn.h, 6) == STS_ESTATE and lib.sts_set_conv_math(syn.h, 0) == STS_ESTATE
    assert lib.sts_set_limiter(syn.h, 1, 0.0, -1.0, 5.0) == STS_ESTATE and lib.sts_set_record_taps(syn.h, 1) == STS_ESTATE
    with pytest.raises(engine.StsError, match="sts error -4"):
        syn.infer_ids(ids)
    with pytest.raises(engine.StsError, match="sts error -4"):
        syn.infer_ids_stream(ids, 8)
    with pytest.raises(engine.StsError, match="sts error -4"):
        syn.infer_batch_stream([ids], 8)
    one = np.zeros(1, np.int32)
    a = np.ascontiguousarray(ids, np.int32)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    n = np.array([a.size], np.int32)
    assert lib.sts_stream_admit(syn.h, 0, ptrs, n.ctypes.data, None, None, None, None, None, one.ctypes.data) == STS_EINVAL
    assert lib.sts_stream_admit(syn.h, 1, None, n.ctypes.data, None, None, None, None, None, one.ctypes.data) == STS_EINVAL
    assert lib.sts_stream_admit(syn.h, 1, ptrs, n.ctypes.data, None, None, None, None, None, None) == STS_EINVAL
    assert lib.sts_stream_admit(syn.h, 3, ptrs, n.ctypes.data, None, None, None, None, None, one.ctypes.data) == STS_EINVAL      # > max_live
    assert lib.sts_stream_step(syn.h, engine.BATCH_CHUNK_CB(), None, None) == STS_EINVAL
    bad = a.copy()
    bad[2] = cfg.vocab + 5
    badp = (C.c_void_p * 1)(bad.ctypes.data)
    assert lib.sts_stream_admit(syn.h, 1, badp, n.ctypes.data, None, None, None, None, None, one.ctypes.data) == STS_EINVAL
    assert syn.stream_info() == {"open": True, "live": 0, "free_slots": 2, "free_frames": 1000, "steps": 0}
    # a step of an empty stream does nothing; the stream still works after the refusals
    assert syn.stream_step() == ([], 0) and syn.stream_info()["steps"] == 0
    got, _ = _run(syn, [ids], [0], [1.0], schedule=((0,),))
    assert _lsb(_cat(got[0]), whole) <= 1
    syn.stream_close()
    # a free slot but not the frames: refused once the frame counts are known, nothing changes, and a later admission that fits runs
    F = _frames(syn, [ids], [0], [1.0])[0]
    syn.stream_open(8, 2, 2 * F - 1)
    assert syn.stream_admit([ids, ids]) is None
    assert syn.stream_info() == {"open": True, "live": 0, "free_slots": 2, "free_frames": 2 * F - 1, "steps": 0}
    got, total = _run(syn, [ids], [0], [1.0], schedule=((0,),))
    assert _lsb(_cat(got[0]), whole) <= 1 and total[0] == whole.size
    syn.stream_close()
    assert np.array_equal(syn.infer_ids(ids), whole)
    syn.close()


@pytest.mark.parametrize("C_", [1, 3, 192])
def test_debug_adopt_z_against_numpy(C_):
    """segments of every length class (below / at / above a quad and a wave), source and destination offsets co-aligned and not, leading
    dimensions that are whole quads and not; the destination comes back with every element outside the ranges unchanged"""
    rng = np.random.default_rng(C_)
    lens = [1, 3, 4, 63, 64, 65, 257, 700]
    for ld_src, ld_dst, shift in ((1500, 2000, 0), (1500, 2000, 1), (1501, 2000, 0), (1500, 1999, 2), (1500, 2000, 4)):
        src = rng.standard_normal((C_, ld_src)).astype(np.float32)
        dst = rng.standard_normal((C_, ld_dst)).astype(np.float32)
        so, do = [], []
        s = d = 0
        for i, n in enumerate(lens):
            s += i % 3                   # source offsets of every alignment
            d = d + ((s - d) % 4) + shift if shift != 4 else d + 4 * (i % 2) + ((s - d) % 4)
            so.append(s); do.append(d)
            s += n; d += n
        assert s <= ld_src and d <= ld_dst
        if shift == 0:
            assert all((a - b) % 4 == 0 for a, b in zip(so, do))
        if shift in (1, 2):
            assert all((a - b) % 4 != 0 for a, b in zip(so, do))
        want = dst.copy()
        for a, b, n in zip(so, do, lens):
            want[:, b:b + n] = src[:, a:a + n]
        perm = rng.permutation(len(lens))          # (the table's order is not the columns')
        got = engine.debug_adopt_z(src, dst, [so[i] for i in perm], [do[i] for i in perm], [lens[i] for i in perm])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ld_src, ld_dst, shift)
    # a length of 0 moves nothing
    src = rng.standard_normal((C_, 8)).astype(np.float32)
    dst = rng.standard_normal((C_, 8)).astype(np.float32)
    assert np.array_equal(engine.debug_adopt_z(src, dst, [3], [2], [0]), dst)


@pytest.mark.parametrize("admission", [True, False])
def test_pool_admits_a_late_request_into_the_running_group(admission):
    """one engine, max_batch 4: request A's first chunk blocks its worker until B (same chunk size) is queued.  With admission on, B joins
    the running stream -- its first chunk arrives before A's last -- with it off B waits for A's group to drain.  Both PCMs either way."""
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 11)
    ids_a = sb.synthetic_ids(33, cfg.vocab, salt=33)
    ids_b = sb.synthetic_ids(9, cfg.vocab, salt=9)
    syn = engine.Synthesizer(blob)
    want_a = _cat(_single(syn, ids_a, 0, 1.0, 6))
    want_b = _cat(_single(syn, ids_b, 0, 1.0, 6))
    whole_a, whole_b = syn.infer_ids(ids_a), syn.infer_ids(ids_b)
    syn.close()
    assert want_a.size == whole_a.size and want_b.size == whole_b.size
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=4)
    assert not pool.stream_admission()
    if admission:
        pool.set_stream_admission(True)
    assert pool.stream_admission() == admission
    queued, started = threading.Event(), threading.Event()
    events = []          # ("a" | "b", sample offset, samples) in arrival order (one worker thread)
    got = {"a": [], "b": []}

    def on_a(pcm, off):
        events.append(("a", off, pcm.size))
        got["a"].append((off, pcm))
        if off == 0:
            started.set()
            assert queued.wait(30.0)
        return False

    def on_b(pcm, off):
        events.append(("b", off, pcm.size))
        got["b"].append((off, pcm))
        return False
    ta = pool.submit_stream(ids_a, 6, on_a)
    assert started.wait(60.0) and events[0][0] == "a"          # A's first chunk has arrived: its worker is inside the callback
    if admission:
        assert engine.load_library().sts_pool_set_stream_admission(pool.h, 0) == STS_ESTATE      # requests are outstanding
    tb = pool.submit_stream(ids_b, 6, on_b)
    queued.set()
    assert pool.wait(ta) == want_a.size and pool.wait(tb) == want_b.size
    first_b = next(i for i, e in enumerate(events) if e[0] == "b")
    last_a = max(i for i, e in enumerate(events) if e[0] == "a")
    groups, mid = pool.stream_stats()
    if admission:
        assert mid >= 1 and groups == 1 and first_b < last_a
    else:
        assert mid == 0 and groups == 0 and first_b > last_a
    for k, want, whole in (("a", want_a, whole_a), ("b", want_b, whole_b)):
        pcm = _cat(got[k])
        assert [o for o, _ in got[k]] == list(np.cumsum([0] + [p.size for _, p in got[k]])[:-1]), k
        assert _lsb(pcm, want) <= 1 and _lsb(pcm, whole) <= 1, k
    pool.close()
