"""Batched streaming on the MI355X (sts_infer_ids_batch_stream, sts_pool_submit_stream): each utterance's chunks against its own single
stream, the packed batch and the oracle for every decoder family; the chunk geometry and delivery order; B = 1; per-utterance stop;
output rates; sampling noise; the full-size golden batches; the split-bf16 repeat (whole call and later step); the pool; the rejections."""
import ctypes as C
import threading

import numpy as np
import pytest

import resample_ref as rr
from conftest import golden_files, golden_files_v2, load_golden, load_golden_v2
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL, STS_ESTATE = -1, -4
LENS = [9, 31, 5, 17, 1, 24]
LS = [1.0, 0.8, 1.2, 1.0, 1.1, 0.9]


def _kinds():
    """one tiny golden model per kind (multi-speaker HiFi-GAN with its decoder conditioning among them)"""
    seen, out = set(), []
    for path in golden_files():
        g, cfg, blob = load_golden(path)
        if g["kind"].item() not in seen:
            seen.add(g["kind"].item())
            out.append((g["kind"].item(), cfg, blob))
    assert len(out) >= 5
    return out


def _batch(cfg, lens=LENS):
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate(lens)]
    nspk = max(int(cfg.spk_num), 1)
    sids = [(3 * u + 1) % nspk for u in range(len(lens))] if cfg.is_ms else [0] * len(lens)
    return ids, sids, LS[:len(lens)]


def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


def _streams(syn, ids, sids, ls, chunk):
    return [_cat(syn.infer_ids_stream(ids[b], chunk, sids[b], ls[b])[0]) for b in range(len(ids))]


def _lsb(a, b):
    assert a.size == b.size, (a.size, b.size)
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()) if a.size else 0


def test_equal_to_single_stream_and_batch_pinned_and_auto():
    for kind, cfg, blob in _kinds():
        ids, sids, ls = _batch(cfg)
        syn = engine.Synthesizer(blob)
        halo = syn.stream_halo_frames()
        syn.set_conv_mode(6)
        batch = syn.infer_batch(ids, sids, ls)
        single = _streams(syn, ids, sids, ls, 7)
        for b in range(len(ids)):
            assert np.array_equal(single[b], batch[b]), (kind, b)
        for chunk in (1, 7, halo, 3 * halo + 1, 100000):
            tot = []
            chunks, _ = syn.infer_batch_stream(ids, chunk, sids, ls, n_total=tot)
            for b in range(len(ids)):
                got = _cat(chunks[b])
                assert np.array_equal(got, batch[b]), (kind, chunk, b)
                assert tot[b] == batch[b].size, (kind, chunk, b)
        # automatic kernel choice: within 1 LSB of the pinned results and of the oracle
        syn.set_conv_mode(0)
        port = pyref.PortModel(blob)
        for chunk in (7, 3 * halo + 1):
            chunks, _ = syn.infer_batch_stream(ids, chunk, sids, ls)
            for b in range(len(ids)):
                got = _cat(chunks[b])
                assert _lsb(got, batch[b]) <= 1, (kind, chunk, b)
                o = port.infer_ids(ids[b], sids[b], ls[b])
                assert _lsb(got, o["pcm"]) <= 1, (kind, chunk, b, "oracle")
        syn.close()


def _geometry_check(syn, ids, sids, ls, chunk, rate):
    hop = syn.info.samples_per_frame
    one = syn.infer_batch(ids, sids, ls)
    dur = syn.durations(sum(len(x) for x in ids))
    toff = np.concatenate([[0], np.cumsum([len(x) for x in ids])])
    F = [int(dur[toff[b]:toff[b + 1]].sum()) for b in range(len(ids))]
    seen = []
    tot = []
    chunks, _ = syn.infer_batch_stream(ids, chunk, sids, ls, on_chunk=lambda u, pcm, off, t: seen.append((u, off, pcm.size)) and False,
                                       n_total=tot)
    pos = [0] * len(ids)
    k_of = [0] * len(ids)
    order = []
    for u, off, n in seen:
        k = k_of[u]
        assert off == pos[u], (u, k)
        assert off == (rr.out_len(k * chunk * hop, rate) if rate != 16000 else k * chunk * hop), (u, k)
        order.append((k, u))
        pos[u] += n; k_of[u] += 1
    assert order == sorted(order), "chunks must arrive step by step, ascending utterance within a step"
    for b in range(len(ids)):
        assert k_of[b] == -(-F[b] // chunk), b               # short utterances stop appearing once they are done
        native = F[b] * hop
        assert one[b].size == (rr.out_len(native, rate) if rate != 16000 else native)
        assert pos[b] == tot[b] == one[b].size, b
        assert np.array_equal(_cat(chunks[b]), one[b]), b


def test_geometry_order_and_totals():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    for chunk in (3, 16):
        _geometry_check(syn, ids, sids, ls, chunk, 16000)
    syn.set_output_rate(44100)
    _geometry_check(syn, ids, sids, ls, 5, 44100)
    syn.close()


def test_single_utterance_is_the_single_stream_under_auto():
    for kind in ("hifigan_sdp", "mbb_fix"):
        cfg = sb.full_cfg(kind)
        blob = sb.make_blob(cfg, 7)
        ids = sb.synthetic_ids(40, cfg.vocab)
        syn = engine.Synthesizer(blob)
        for chunk in (8, 33):
            want, _ = syn.infer_ids_stream(ids, chunk)
            got, _ = syn.infer_batch_stream([ids], chunk)
            assert len(got[0]) == len(want) and all(np.array_equal(a, b) for a, b in zip(got[0], want)), (kind, chunk)
        syn.close()


def _offsets_run(offs):
    pos = 0
    for off, n in offs:
        assert off == pos, (off, pos)
        pos += n


_ONE_UTT = [(k, r, lim, None) for k in ("ms_hifigan_sdp", "mbb_fix") for r, lim in ((44100, False), (16000, True), (44100, True))] + \
           [("ms_hifigan_sdp", 16000, False, "direct"), ("ms_hifigan_sdp", 16000, False, "retry")]


@pytest.mark.parametrize("kind,rate,lim,extra", _ONE_UTT, ids=lambda v: str(v))
def test_one_utterance_is_the_one_window_step(kind, rate, lim, extra):
    """sts_infer_ids_stream is the B = 1 case of the step loop: with the conv mode pinned its chunks are the one-pass PCM bit for bit and
    every sample_offset is the running sum, for chunks below / at / above the halo, at another rate, with the limiter (1 ms look-ahead),
    and with both.  (The native rate without a limiter is tests/test_parity_gpu.py::test_streaming_equals_one_pass for these kinds; here
    only its two remaining forms: the chunks stored into host memory by the pack kernel, and the later-step split-bf16 repeat.)"""
    cfg = sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 99)
    ids = sb.synthetic_ids(13, cfg.vocab, salt=5)
    sid = 1 if cfg.is_ms else 0
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    if lim:
        syn.set_limiter(engine.LIMITER_ON, 20.0, -1.0, 1.0)

    def stream(chunk):
        offs = []
        chunks, _ = syn.infer_ids_stream(ids, chunk, sid, on_chunk=lambda pcm, off, t: offs.append((off, pcm.size)) and False)
        _offsets_run(offs)
        return chunks

    if extra == "retry":
        # the overflow word counts as raised after step 1: step 0 left in the two-term fp16 form, step 1 and the later ones are decoded in
        # split-bf16 (tolerance and forced durations as in test_split_bf16_repeat_whole_call_and_later_step)
        syn.set_conv_math("f16x2")
        plain = stream(1)
        dur = syn.durations(len(ids))
        assert len(plain) > 2
        syn.set_conv_math("bf16x3")
        syn.set_forced_durations(dur)
        bf3 = stream(1)
        syn.set_conv_math("f16x2")
        before = syn.profile()["conv_math_fallbacks"]
        syn.debug_set("stream_retry_step", 1)
        syn.set_forced_durations(dur)
        got = stream(1)
        syn.debug_set("stream_retry_step", -1)
        assert syn.profile()["conv_math_fallbacks"] == before + 1
        assert len(got) == len(plain) == len(bf3)
        assert np.array_equal(got[0], plain[0])
        for i in range(1, len(got)):
            assert _lsb(got[i], bf3[i]) <= 1, i
    else:
        whole = syn.infer_ids(ids, sid)
        assert whole.size > 0
        if extra == "direct":
            syn.debug_set("stream_direct", 1)
        for chunk in (1, 7, syn.stream_halo_frames(), 100000):
            assert np.array_equal(_cat(stream(chunk)), whole), chunk
    syn.close()


def test_stop_one_utterance():
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 21)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    full, _ = syn.infer_batch_stream(ids, 4, sids, ls)
    got, _ = syn.infer_batch_stream(ids, 4, sids, ls, on_chunk=lambda u, pcm, off, t: u == 1)
    assert len(got[1]) == 1 and np.array_equal(got[1][0], full[1][0])
    for b in range(len(ids)):
        if b != 1:
            assert np.array_equal(_cat(got[b]), _cat(full[b])), b
    syn.close()


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_output_rates(rate):
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    native = [x.size for x in syn.infer_batch(ids, sids, ls)]
    syn.set_output_rate(rate)
    single = _streams(syn, ids, sids, ls, 6)
    for chunk in (1, 6, 23):
        chunks, _ = syn.infer_batch_stream(ids, chunk, sids, ls)
        for b in range(len(ids)):
            got = _cat(chunks[b])
            assert got.size == rr.out_len(native[b], rate), (chunk, b)
            assert np.array_equal(got, single[b]), (chunk, b)
    syn.close()


def test_noise_uses_seed_plus_utterance():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    ids, sids, ls = _batch(cfg)
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    s = 77
    syn.set_noise(0.667, 0.8, s)
    chunks, _ = syn.infer_batch_stream(ids, 9, sids, ls)
    for b in range(len(ids)):
        syn.set_noise(0.667, 0.8, s + b)
        want = _cat(syn.infer_ids_stream(ids[b], 9, sids[b], ls[b])[0])
        assert np.array_equal(_cat(chunks[b]), want), b
    syn.close()


@pytest.mark.parametrize("path", golden_files_v2("full_batch8_") + golden_files_v2("full_batch32_ms_hifigan_sdp"),
                         ids=lambda p: p.split("/")[-1])
def test_full_size_golden_batches(path):
    g, cfg, blob, utts, stride = load_golden_v2(path)
    lens = [int(t) for t in g["batch_lens"]]
    sids = [int(v) for v in g["batch_sids"]]
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate(lens)]
    syn = engine.Synthesizer(blob)
    chunks, _ = syn.infer_batch_stream(ids, 32, sids, [1.0] * len(ids))
    dur = syn.durations(sum(lens))
    toff = np.concatenate([[0], np.cumsum(lens)])
    for u, ids_u, sid_u, ls_u, dur_u, pcm_u, wave_u in utts:
        assert np.array_equal(ids_u, ids[u]) and sid_u == sids[u]
        assert (dur[toff[u]:toff[u + 1]] == dur_u).all(), u
        assert _lsb(_cat(chunks[u]), pcm_u) <= 1, u
    syn.close()


def _loud_blob():
    """the full HiFi-GAN blob with its decoder input conv scaled up (tests/test_resample_gpu.py): f16x2 must repeat in split-bf16"""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    w = sb._W(5, cfg.stats)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._gen_hdr(w, cfg)
    assert tuple(blob[w.n:w.n + 3].astype(int)) == (cfg.up_init, cfg.inter, 7)
    start = w.n + 6
    big = blob.copy()
    big[start:start + cfg.up_init * 7 * cfg.inter] *= np.float32(3.0e6)
    return cfg, big


def _once_each(chunks, offs):
    for b in range(len(chunks)):
        pos = 0
        for off, n in offs[b]:
            assert off == pos, b
            pos += n


def test_split_bf16_repeat_whole_call_and_later_step():
    cfg, big = _loud_blob()
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate((20, 7, 13))]
    syn = engine.Synthesizer(big)
    syn.set_profiling(True)
    syn.set_conv_math("bf16x3")
    want, _ = syn.infer_batch_stream(ids, 16)
    syn.set_conv_math("f16x2")
    offs = [[] for _ in ids]
    got, _ = syn.infer_batch_stream(ids, 16, on_chunk=lambda u, pcm, off, t: offs[u].append((off, pcm.size)) and False)
    assert syn.profile()["conv_math_fallbacks"] == 1
    _once_each(got, offs)
    for b in range(len(ids)):
        assert len(got[b]) == len(want[b]) and np.array_equal(_cat(got[b]), _cat(want[b])), b
    syn.close()

    # a later step (the hook: the overflow word counts as raised after step k) is decoded again in split-bf16, and so is every step
    # after it; the steps before it are the plain f16x2 ones.  Forced durations: the two maths then share every frame count.
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate((20, 7, 13))]
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_conv_math("f16x2")
    plain, _ = syn.infer_batch_stream(ids, 8)
    dur = syn.durations(sum(len(x) for x in ids))
    syn.set_conv_math("bf16x3")
    syn.set_forced_durations(dur)
    bf3, _ = syn.infer_batch_stream(ids, 8)
    k = 2
    syn.set_conv_math("f16x2")
    syn.debug_set("stream_retry_step", k)
    syn.set_forced_durations(dur)
    offs = [[] for _ in ids]
    got, _ = syn.infer_batch_stream(ids, 8, on_chunk=lambda u, pcm, off, t: offs[u].append((off, pcm.size)) and False)
    assert syn.profile()["conv_math_fallbacks"] == 1
    _once_each(got, offs)
    for b in range(len(ids)):
        assert len(got[b]) == len(plain[b]) == len(bf3[b]), b
        for i in range(len(got[b])):
            if i < k:
                assert np.array_equal(got[b][i], plain[b][i]), (b, i)
            else:
                assert _lsb(got[b][i], bf3[b][i]) <= 1, (b, i)
    syn.debug_set("stream_retry_step", 0)        # step 0: nothing has left yet, the whole call is repeated
    syn.set_conv_math("f16x2")
    got0, _ = syn.infer_batch_stream(ids, 8)
    assert syn.profile()["conv_math_fallbacks"] == 2          # (the engine's running count: this call adds one)
    for b in range(len(ids)):
        assert len(got0[b]) == len(bf3[b]) and _lsb(_cat(got0[b]), _cat(bf3[b])) <= 1, b
    syn.close()


def test_pool_streaming_requests():
    cfg = sb.tiny_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 11)
    lens = [9, 33, 5, 21, 14, 27, 3, 18, 11]
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    syn = engine.Synthesizer(blob)
    want = [_cat(syn.infer_ids_stream(a, 6)[0]) for a in ids]
    whole = [syn.infer_ids(a) for a in ids[:3]]
    syn.close()
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=8)
    got = [[] for _ in ids]
    tickets = {}
    lock = threading.Lock()

    def client(part):
        for i in part:
            t = pool.submit_stream(ids[i], 6, lambda pcm, off, i=i: got[i].append((off, pcm)) and False)
            with lock:
                tickets[i] = t
    th = [threading.Thread(target=client, args=(list(range(j, len(ids), 3)),)) for j in range(3)]
    wt = [pool.submit(a) for a in ids[:3]]
    for t in th:
        t.start()
    for t in th:
        t.join()
    lib = engine.load_library()
    for i, t in tickets.items():
        n = pool.wait(t)
        pcm = _cat([p for _, p in got[i]])
        assert n == pcm.size == want[i].size, i
        assert [o for o, _ in got[i]] == list(np.cumsum([0] + [p.size for _, p in got[i]])[:-1]), i
        assert _lsb(pcm, want[i]) <= 1, i
    for i, t in enumerate(wt):
        assert np.array_equal(pool.wait(t), whole[i]), i
    b, r = pool.stats()
    assert r == len(ids) + 3 and b < r
    # a bad phoneme id fails only its own ticket; the output rate cannot change while a stream is outstanding
    got2 = [[] for _ in range(3)]
    bad = np.array(ids[1]).copy()
    bad[2] = cfg.vocab + 5
    t2 = [pool.submit_stream(x, 6, lambda pcm, off, i=i: got2[i].append(pcm) and False) for i, x in enumerate((ids[0], bad, ids[2]))]
    assert lib.sts_pool_set_output_rate(pool.h, 48000) == STS_ESTATE
    assert pool.wait(t2[0]) == want[0].size
    with pytest.raises(engine.StsError):
        pool.wait(t2[1])
    assert pool.wait(t2[2]) == want[2].size
    assert _lsb(_cat(got2[0]), want[0]) <= 1 and _lsb(_cat(got2[2]), want[2]) <= 1
    pool.close()


def test_invalid_arguments():
    cfg = sb.tiny_cfg("hifigan_fix")
    blob = sb.make_blob(cfg, 3)
    syn = engine.Synthesizer(blob)
    lib = syn.lib
    a = np.ascontiguousarray(sb.synthetic_ids(9, cfg.vocab), np.int32)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    n = np.array([a.size], np.int32)
    calls = []
    cb = engine.BATCH_CHUNK_CB(lambda u, utt, pcm, ns, off: calls.append(utt) or 0)
    assert lib.sts_infer_ids_batch_stream(syn.h, 1, ptrs, n.ctypes.data, None, None, 0, cb, None, None) == STS_EINVAL
    assert lib.sts_infer_ids_batch_stream(syn.h, 0, ptrs, n.ctypes.data, None, None, 8, cb, None, None) == STS_EINVAL
    assert lib.sts_infer_ids_batch_stream(syn.h, 1, ptrs, n.ctypes.data, None, None, 8, engine.BATCH_CHUNK_CB(), None, None) == STS_EINVAL
    assert lib.sts_infer_ids_batch_stream(syn.h, 1, None, n.ctypes.data, None, None, 8, cb, None, None) == STS_EINVAL
    assert not calls
    assert lib.sts_infer_ids_batch_stream(syn.h, 1, ptrs, n.ctypes.data, None, None, 8, cb, None, None) == 0 and calls
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=4)
    assert lib.sts_pool_submit_stream(pool.h, a.ctypes.data, a.size, 0, 1.0, 0.0, 0.0, 0, 0, engine.CHUNK_CB(lambda *x: 0), None) == STS_EINVAL
    assert lib.sts_pool_submit_stream(pool.h, a.ctypes.data, a.size, 0, 1.0, 0.0, 0.0, 0, 8, engine.CHUNK_CB(), None) == STS_EINVAL
    pool.close()
    syn.close()
