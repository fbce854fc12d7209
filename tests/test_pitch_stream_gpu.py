"""A stream through the pitch warp on the MI355X.  The range form of the warp kernel alone (sts_pitch_apply_range against sts_pitch_apply,
bytes equal for y and PCM): [0, N') cut at every output-tile edge and +-1 around it, into single outputs across a phoneme boundary, at
ranges that step over empty phonemes, as one range, with an empty range included -- every range given exactly the input span it reads,
NaN on both sides of it; several members in one launch; a window one sample short.  Then the engine (sts_set_pitch_streaming): the
concatenated chunks of sts_infer_ids_stream / sts_infer_ids_batch_stream equal the whole call with the same plan bit for bit."""
import numpy as np
import pytest

import pitch_ref as pr
import pitch_stream_ref as ps
from summertts_amd import engine
from summertts_amd import synth_blob as sb
from test_pitch_plan_gpu import _cents, _signal

pytestmark = pytest.mark.gpu

TILE = 256                      # pitch_plan.hip PP_TILE
PAD = 5                         # NaN samples on either side of every window in the caller's buffer


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------------------
def _ranges_against_the_whole(durs, plans, hop, edges, seed):
    """every utterance b cut at edges[b]: one launch of all the ranges against the whole-utterance kernel's samples"""
    sig = [_signal(max(1, int(np.sum(d))) * hop, seed + b) for b, d in enumerate(durs)]
    whole_y, whole_pcm = engine.pitch_apply(sig, durs, plans, hop)
    utts = [ps.Utt(d, p, hop) for d, p in zip(durs, plans)]
    buf, wins, want = [], [], []
    at = 0
    for b, u in enumerate(utts):
        assert whole_y[b].size == u.Nw
        for (u0, xlen, y0, y1) in ps.cut_ranges(u, edges[b]) + [(0, 0, u.Nw // 2, u.Nw // 2)]:      # (... and an empty range)
            buf += [np.full(PAD, np.nan, np.float32), sig[b][u0:u0 + xlen], np.full(PAD, np.nan, np.float32)]
            wins.append((b, at + PAD, u0, xlen, y0, y1))
            want.append((whole_y[b][y0:y1], whole_pcm[b][y0:y1]))
            at += xlen + 2 * PAD
    y, pcm = engine.pitch_apply_range(np.concatenate(buf), durs, plans, hop, wins)
    assert len(y) == len(wins)
    for i, (w, (wy, wp)) in enumerate(zip(wins, want)):
        assert not np.isnan(y[i]).any(), (hop, w)
        assert y[i].tobytes() == wy.tobytes() and pcm[i].tobytes() == wp.tobytes(), (hop, w)
    return sig, utts, wins


def _tile_edges(n):
    return [t + k for t in range(TILE, n, TILE) for k in (-1, 0, 1)]


MIXED_D = [0, 0, 70] + [1] * 9 + [0, 0, 0, 40, 1, 20, 0, 300, 0, 0, 0, 300]
MIXED_C = [600, -600, 600] + [600] * 9 + [0, 1, -1, -600, 0, -1, 600, 37, 600, -600, 0, -600]


@pytest.mark.parametrize("hop", [1, 6, 256])
def test_ranges_equal_the_whole_utterance_kernel(hop):
    d = MIXED_D if hop < 256 else [2, 0, 1, 3, 0, 0, 2]
    c = MIXED_C if hop < 256 else [600, 600, -600, 1, 0, -1, -600]
    u = ps.Utt(d, c, hop)
    assert u.Nw > 3 * TILE
    bound = [v for v in u.o[1:-1]]                               # the phoneme boundaries, those of empty phonemes included
    single = [bound[3] + k for k in range(-3, 4)] + [bound[-2] + k for k in range(-2, 3)]        # single outputs across a boundary
    over = [o for o, n in zip(u.o[1:], np.diff(u.o)) if n == 0]                                   # ranges that end where empty phonemes sit
    plain_d = [5, 0, 600 // hop + 1]
    durs, plans = [d, plain_d, d, [0, 0, 0]], [c, None, [0] * len(d), [600, -600, 1]]            # a copied member among planned ones
    up = ps.Utt(plain_d, None, hop)
    edges = [_tile_edges(u.Nw) + single + over, _tile_edges(up.Nw) + [1, 2], [], []]               # (no edges: the whole signal as one range)
    _ranges_against_the_whole(durs, plans, hop, edges, 7)


def test_a_window_one_sample_short_is_refused():
    hop = 6
    d, c = [20, 0, 15, 1, 30], [600, 0, -600, 600, 37]
    u = ps.Utt(d, c, hop)
    x = _signal(u.N, 3)
    mid0, mid1 = u.Nw // 3, 2 * u.Nw // 3
    c0, c1 = ps.staged(u, mid0, mid1)
    assert 0 < c0 and c1 < u.N
    whole_y, _ = engine.pitch_apply([x], [d], [c], hop)
    y, _ = engine.pitch_apply_range(x[c0:c1], [d], [c], hop, [(0, 0, c0, c1 - c0, mid0, mid1)])
    assert y[0].tobytes() == whole_y[0][mid0:mid1].tobytes()
    for (u0, u1) in ((c0 + 1, c1), (c0, c1 - 1)):
        with pytest.raises(engine.StsError, match="cover"):
            engine.pitch_apply_range(x[u0:u1], [d], [c], hop, [(0, 0, u0, u1 - u0, mid0, mid1)])
    for bad in ((1, 0, c0, c1 - c0, mid0, mid1), (0, 1, c0, c1 - c0, mid0, mid1), (0, 0, c0, c1 - c0, mid0, u.Nw + 1),
                (0, 0, c0, c1 - c0, mid1, mid0), (0, 0, u.N - 3, 4, mid0, mid0)):
        with pytest.raises(engine.StsError):
            engine.pitch_apply_range(x[c0:c1], [d], [c], hop, [bad])
    p = ps.Utt(d, None, hop)                                       # a member without a plan reads its own samples alone
    y, _ = engine.pitch_apply_range(x[10:20], [d], [None], hop, [(0, 0, 10, 10, 10, 20)])
    assert y[0].tobytes() == x[10:20].tobytes() and p.Nw == u.N
    with pytest.raises(engine.StsError, match="cover"):
        engine.pitch_apply_range(x[10:20], [d], [None], hop, [(0, 0, 10, 10, 10, 21)])


# ---- the engine -------------------------------------------------------------------------------------------------------------------------------
LENS = (19, 5, 11)


def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


def _engine(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    syn = engine.Synthesizer(sb.make_blob(cfg, seed))
    syn.set_conv_mode(6)            # pinned, as tests/test_batch_stream_gpu.py pins it: a window's kernel variant must not depend on its length
    syn.set_pitch_streaming(True)
    ids = [sb.synthetic_ids(k, cfg.vocab, salt=k) for k in LENS]
    plans = [_cents(LENS[0], 31), None, _cents(LENS[2], 33)]
    return cfg, syn, ids, plans


def _stream_one(syn, ids, cents, chunk, sid=0, before=None, on_chunk=None):
    """one utterance -> (chunks, [(first output, count)])"""
    offs = []
    if before:
        before()
    syn.set_pitch_plan([len(ids)], [cents])

    def cb(pcm, off, t):
        offs.append((off, pcm.size))
        return bool(on_chunk and on_chunk(len(offs) - 1))
    chunks, _ = syn.infer_ids_stream(ids, chunk, sid, on_chunk=cb)
    return chunks, offs


def _stream_batch(syn, ids, plans, chunk, sids=None, before=None, stop=None):
    offs = [[] for _ in ids]
    if before:
        before()
    syn.set_pitch_plan([len(a) for a in ids], plans)

    def cb(u, pcm, off, t):
        offs[u].append((off, pcm.size))
        return stop is not None and u == stop
    tot = []
    chunks, _ = syn.infer_batch_stream(ids, chunk, sids, on_chunk=cb, n_total=tot)
    return chunks, offs, tot


def _whole_one(syn, ids, cents, sid=0, before=None):
    if before:
        before()
    syn.set_pitch_plan([len(ids)], [cents])
    return syn.infer_ids(ids, sid)


def _whole_batch(syn, ids, plans, sids=None, before=None):
    if before:
        before()
    syn.set_pitch_plan([len(a) for a in ids], plans)
    return syn.infer_batch(ids, sids)


def _grid(syn, dur, cents, chunk):
    """the restatement's chunks of one utterance from the durations the run reported: [(first output, count)], empty ones dropped"""
    hop = syn.info.samples_per_frame
    rate = syn.output_rate()
    import math
    g = math.gcd(rate, 16000)
    P, Q = rate // g, 16000 // g
    u = ps.Utt(dur, cents, hop)
    return [c for c in ps.chunks(u, chunk, P, Q) if c[1] > 0]


@pytest.mark.parametrize("kind,rate,lim", [("hifigan_sdp", 16000, False), ("hifigan_sdp", 16000, True), ("mbb_fix", 8000, False),
                                           ("mbb_fix", 22050, True), ("hifigan_sdp", 48000, False), ("ms_hifigan_sdp", 22050, False)])
def test_chunks_equal_the_whole_call(kind, rate, lim):
    """B = 1 and B = 3 (different lengths, one member without a plan), chunks of 1, 3 and 4 frames and one larger than every utterance"""
    cfg, syn, ids, plans = _engine(kind)
    sids = [1, 0, 2] if cfg.is_ms else None
    syn.set_output_rate(rate)
    if lim:
        syn.set_limiter(engine.LIMITER_ON, 6.0, -3.0, 1.0)
    whole = _whole_batch(syn, ids, plans, sids)
    dur = syn.durations(sum(LENS))
    offsets = syn.phoneme_offsets(sum(LENS))
    plain = syn.infer_batch(ids, sids)
    assert whole[0].size != plain[0].size and np.array_equal(whole[1], plain[1])
    alone = _whole_one(syn, ids[0], plans[0], sids[0] if sids else 0)
    assert np.array_equal(alone, whole[0])
    halo_plain = syn.stream_halo_frames()
    syn.set_pitch_plan([LENS[0]], [plans[0]])
    assert syn.stream_halo_frames() > halo_plain                   # the larger halo while a plan is pending
    syn.set_pitch_plan(None)
    assert syn.stream_halo_frames() == halo_plain
    cuts = np.concatenate([[0], np.cumsum(LENS)])
    for chunk in (1, 3, 4, 100000):
        got, offs = _stream_one(syn, ids[0], plans[0], chunk, sids[0] if sids else 0)
        assert np.array_equal(_cat(got), alone), (kind, rate, chunk)
        assert offs == _grid(syn, dur[:LENS[0]], plans[0], chunk), (kind, rate, chunk)
        chunks, offs, tot = _stream_batch(syn, ids, plans, chunk, sids)
        assert np.array_equal(syn.phoneme_offsets(sum(LENS)), offsets)
        for b in range(3):
            assert np.array_equal(_cat(chunks[b]), whole[b]), (kind, rate, chunk, b)
            assert offs[b] == _grid(syn, dur[cuts[b]:cuts[b + 1]], plans[b], chunk), (kind, rate, chunk, b)
            assert tot[b] == whole[b].size
    # the plan is consumed: the next stream is the plain one, with the switch on or off
    on = _cat(syn.infer_ids_stream(ids[0], 4, sids[0] if sids else 0)[0])
    syn.set_pitch_streaming(False)
    off = _cat(syn.infer_ids_stream(ids[0], 4, sids[0] if sids else 0)[0])
    assert np.array_equal(on, off) and np.array_equal(on, plain[0])
    syn.close()


def test_composition_with_the_other_tables_and_noise():
    """a gain plan, duration-plan rates, a speaker mix and seeded noise, all at once, at 22.05 kHz under the limiter"""
    cfg, syn, ids, plans = _engine("ms_hifigan_sdp", 5)
    sids = [1, 0, 2]
    syn.set_output_rate(22050)
    syn.set_limiter(engine.LIMITER_ON, 3.0, -2.0, 1.5)
    syn.set_noise(0.667, 0.8, 77)
    db = [np.linspace(-12, 6, k).astype(np.float32) for k in LENS]
    rates = [np.linspace(0.7, 1.6, k).astype(np.float32) for k in LENS]

    def before():
        syn.set_gain_plan(LENS, [{"gain_db": db[0], "ramp_ms": 2.0}, None, {"gain_db": db[2], "ramp_ms": 0.5}])
        syn.set_duration_plan(LENS, [{"rate": r} for r in rates])
        syn.set_speaker_mix([{"sid": [0, 3], "weight": [0.5, 0.5]}, None, None])
    whole = _whole_batch(syn, ids, plans, sids, before)
    bare = _whole_batch(syn, ids, plans, sids)
    assert not np.array_equal(whole[0], bare[0])
    for chunk in (3, 100000):
        chunks, _, _ = _stream_batch(syn, ids, plans, chunk, sids, before)
        for b in range(3):
            assert np.array_equal(_cat(chunks[b]), whole[b]), (chunk, b)
    syn.close()


def test_a_callback_stop_ends_that_utterance_only():
    cfg, syn, ids, plans = _engine("hifigan_sdp")
    full, _, _ = _stream_batch(syn, ids, plans, 4)
    got, _, tot = _stream_batch(syn, ids, plans, 4, stop=0)
    assert len(got[0]) == 1 and np.array_equal(got[0][0], full[0][0]) and tot[0] == got[0][0].size
    for b in (1, 2):
        assert np.array_equal(_cat(got[b]), _cat(full[b])), b
    syn.close()


def test_the_split_bf16_repeat_of_a_later_step():
    """STS_DBG_STREAM_RETRY_STEP as tests/test_batch_stream_gpu.py uses it: step 0 leaves in the two-term fp16 form, the later steps are
    decoded (and warped) again in split-bf16 -- no chunk leaves twice, chunk 0 is the fp16 form's bit for bit, and the later ones are
    the split-bf16 stream's within 1 LSB (that stream ran its front and flow in split-bf16 too: the tolerance of the test this follows)"""
    cfg, syn, ids, plans = _engine("hifigan_sdp")
    syn.set_conv_math("f16x2")
    plain, offs = _stream_one(syn, ids[0], plans[0], 4)
    dur = syn.durations(LENS[0])
    assert len(plain) > 2
    syn.set_conv_math("bf16x3")
    bf3, _ = _stream_one(syn, ids[0], plans[0], 4, before=lambda: syn.set_forced_durations(dur))
    syn.set_conv_math("f16x2")
    before = syn.profile()["conv_math_fallbacks"]
    syn.debug_set("stream_retry_step", 1)
    got, goffs = _stream_one(syn, ids[0], plans[0], 4, before=lambda: syn.set_forced_durations(dur))
    syn.debug_set("stream_retry_step", -1)
    assert syn.profile()["conv_math_fallbacks"] == before + 1
    assert goffs == offs and len(got) == len(plain)
    assert np.array_equal(got[0], plain[0])
    for i in range(1, len(got)):
        assert got[i].size == bf3[i].size and int(np.abs(got[i].astype(np.int64) - bf3[i].astype(np.int64)).max()) <= 1, i
    syn.close()


def test_a_poisoned_workspace_changes_nothing():
    def run(poison):
        cfg, syn, ids, plans = _engine("mbb_fix", 9)
        if poison:
            syn.debug_set("poison", 0x7FC00000)
        syn.set_output_rate(44100)
        syn.set_limiter(engine.LIMITER_ON, 3.0, -2.0, 1.5)
        out = []
        for chunk in (3, 100000):
            chunks, offs, tot = _stream_batch(syn, ids, plans, chunk)
            out += [_cat(c).tobytes() for c in chunks] + [offs, tot, syn.phoneme_offsets(sum(LENS)).tobytes()]
        syn.set_output_rate(16000)
        syn.set_limiter(engine.LIMITER_OFF)
        out += [_cat(_stream_one(syn, ids[0], plans[0], 3)[0]).tobytes()]
        assert (syn.profile()["poison_bytes"] > 0) == bool(poison)
        syn.close()
        return out
    assert run(True) == run(False)


def test_refusals():
    cfg, syn, ids, plans = _engine("hifigan_fix", 3)
    a, cents = ids[0], plans[0]
    n = [len(a)]
    plain = syn.infer_ids(a)
    shifted = _whole_one(syn, a, cents)

    def refused(call, what):
        base = syn.infer_ids(a)                                     # (under the settings of the moment)
        syn.set_pitch_plan(n, [cents])
        with pytest.raises(engine.StsError):
            call()
        assert np.array_equal(syn.infer_ids(a), base), what       # nothing is open, and the plan is gone
    # the switch off: streams refuse as they did
    syn.set_pitch_streaming(False)
    refused(lambda: syn.infer_ids_stream(a, 4), "switch off")
    refused(lambda: syn.infer_batch_stream([a], 4), "switch off, batch")
    syn.set_pitch_streaming(True)
    assert np.array_equal(_cat(_stream_one(syn, a, cents, 4)[0]), shifted)
    # the streamed EQ, streamed loudness and the taps
    syn.set_eq([(engine.EQ_PEAK, 1000.0, 3.0, 1.0)]); syn.set_eq_streaming(True)
    refused(lambda: syn.infer_ids_stream(a, 4), "streamed EQ")
    syn.set_eq(None); syn.set_eq_streaming(False)
    syn.set_loudness(engine.LOUD_MEASURE); syn.set_loudness_streaming(True)
    refused(lambda: syn.infer_ids_stream(a, 4), "streamed loudness")
    syn.set_loudness(engine.LOUD_OFF); syn.set_loudness_streaming(False)
    syn.set_record_taps(True)
    refused(lambda: syn.infer_batch_stream([a], 4), "taps")
    syn.set_record_taps(False)
    # the other streaming forms and the joined runs
    for k, call in enumerate([lambda: syn.infer_joined([a]), lambda: syn.infer_joined_stream([a], 4), lambda: syn.stream_open(4, 2, 4096),
                              lambda: syn.stream_open(4, 2, 4096, 64), lambda: syn.para_open(4, 2, 4096)]):
        refused(call, k)
    syn.stream_open(4, 2, 4096, 64)
    syn.set_pitch_plan(n, [cents])
    with pytest.raises(engine.StsError):
        syn.stream_admit([a])
    with pytest.raises(engine.StsError):
        syn.set_pitch_streaming(False)                              # (the switch is fixed while a stream is open)
    syn.stream_close()
    assert np.array_equal(syn.infer_ids(a), plain)
    assert np.array_equal(_cat(_stream_one(syn, a, cents, 3)[0]), shifted)
    syn.close()


@pytest.mark.parametrize("rate", [16000, 48000])
def test_chunks_stored_into_host_memory(rate):
    """STS_DBG_STREAM_DIRECT: the step's writer -- the warp itself at the native rate -- stores the chunks into mapped pinned memory"""
    cfg, syn, ids, plans = _engine("hifigan_sdp", 7)
    syn.set_output_rate(rate)
    whole = _whole_batch(syn, ids, plans)
    syn.debug_set("stream_direct", 1)
    for chunk in (2, syn.stream_halo_frames()):
        chunks, _, _ = _stream_batch(syn, ids, plans, chunk)
        for b in range(3):
            assert np.array_equal(_cat(chunks[b]), whole[b]), (rate, chunk, b)
        assert np.array_equal(_cat(_stream_one(syn, ids[2], plans[2], chunk)[0]), whole[2]), (rate, chunk)
    syn.close()
