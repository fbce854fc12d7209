"""Speaker blending on the MI355X (sts_set_speaker_mix, sts_speaker_blend, sts_get_speaker_embedding, sts_pool_submit_mix,
sts_multi_set_speaker_mix), bit for bit against tests/speaker_ref.py.

The yardstick: blob B is blob A with ``speaker_ref.blend`` of the mixes under test appended to its speaker table, so an engine on blob B
with the plain sid = speaker_num + j launches what an engine on blob A launches with mix j -- only the way g is produced differs.  PCM,
durations and the taps must be the same bits in every call form; these comparisons take no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

import speaker_ref as sr
from conftest import assert_pcm_close, assert_wave_close
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL = -1
KINDS = ("ms_hifigan_sdp", "ms_hifigan_fix")
TAPS = ("m", "logw", "z_p", "z", "wave")
LENS = (5, 13, 21)                  # a batch: the shortest first, so that in a batched stream it leaves steps before the others


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


class Case:
    """one model: blob A, the mixes under test, blob B with their blends as speakers spk .. spk + 2, and the utterances"""

    def __init__(self, kind):
        self.kind = kind
        self.cfg = cfg = sb.tiny_cfg(kind)
        self.blob_a = sb.make_blob(cfg, 1234)
        self.spk, self.gin = cfg.spk_num, cfg.gin
        _, self.table = sr.blob_tail(self.blob_a, self.spk, self.gin)
        rng = np.random.default_rng(len(kind))
        v = rng.standard_normal(self.gin).astype(np.float32)
        self.mixes = [{"sid": [0, self.spk - 1], "weight": [0.6, 0.4]},                                              # a two-term blend
                      {"sid": [1, 2], "weight": [1.5, -0.5], "vector": v, "vector_weight": 0.25},                   # an extrapolation + a vector
                      {"vector": (0.5 * rng.standard_normal(self.gin)).astype(np.float32)}]                        # a caller's own embedding
        self.cols = sr.blend_batch(self.table, self.mixes)
        self.blob_b = sr.blob_with_extra_speakers(self.blob_a, self.spk, self.gin, self.cols)
        self.ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in LENS]
        # the batch of the call forms: no mix, the two-term blend, the extrapolation -- the mixed utterances last
        self.batch_mix = [None, self.mixes[0], self.mixes[1]]
        self.sid_a = [1, 2, 0]                              # (a mixed utterance's own sid is not used)
        self.sid_b = [1, self.spk, self.spk + 1]


@pytest.fixture(scope="module", params=KINDS)
def case(request):
    return Case(request.param)


@pytest.fixture(scope="module")
def engines(case):
    a, b = engine.Synthesizer(case.blob_a), engine.Synthesizer(case.blob_b)
    assert a.get_speaker_num() == case.spk and b.get_speaker_num() == case.spk + 3
    yield a, b
    a.close(); b.close()


def _snap(syn, n_phonemes, taps=TAPS):
    return [syn.durations(n_phonemes).tobytes()] + [syn.tap(k).tobytes() for k in taps]


# ---- 1: the kernel on caller tables ------------------------------------------------------------------------------------------------------
def _kernel_mixes(rng, spk, gin, B):
    """B entries cycling through K = 0 with a vector, 1, 2 and 16, alone and with a vector term, repeated rows, zero and negative weights,
    sums that are not 1, a pair that cancels exactly -- and empty entries, which take the row of the sid list"""
    out = []
    for b in range(B):
        kind = b % 10
        vec = rng.standard_normal(gin).astype(np.float32)
        k = (0, 1, 2, 16, 1, 2, 16, 2, 0, 0)[kind]
        sid = rng.integers(0, spk, k)
        w = rng.uniform(-2.0, 2.0, k).astype(np.float32)
        m = {"sid": sid, "weight": w}
        if kind == 1:
            w[0] = 1.0                                      # one-hot
        if kind == 2:
            w[1] = 0.0
        if kind == 7:
            sid[1] = sid[0]; w[1] = -w[0]                   # the same row twice, cancelling to exactly zero
        if kind in (0, 4, 5, 6):
            m.update(vector=vec, vector_weight=float(rng.uniform(-2.0, 2.0)) if kind != 0 else 1.0)
        out.append(None if kind >= 8 else m)
    return out


@pytest.mark.parametrize("gin", [1, 16, 255, 256])
@pytest.mark.parametrize("spk", [1, 3, 174])
def test_kernel_equals_the_reference_bit_for_bit(spk, gin):
    rng = np.random.default_rng(1000 * spk + gin)
    table = rng.standard_normal((gin, spk)).astype(np.float32)
    for B in (1, 3, 65):
        mixes = _kernel_mixes(rng, spk, gin, B) if B > 1 else [_kernel_mixes(rng, spk, gin, 10)[3]]
        sid = rng.integers(-1, spk + 1, B).astype(np.int32)                  # (outside the table -> row 0, as a plain call)
        got = engine.speaker_blend(table, mixes, sid)
        want = sr.blend_batch(table, mixes, sid)
        assert got.dtype == np.float32 and got.shape == (B, gin)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (spk, gin, B)
        mag = np.abs(want[want != 0])
        assert mag.size == 0 or mag.min() >= np.finfo(np.float32).tiny        # zero or normal: denormals are outside the contract
    one_hot = [{"sid": [s], "weight": [1.0]} for s in range(spk)]
    assert np.array_equal(engine.speaker_blend(table, one_hot), table.T)
    assert np.array_equal(engine.speaker_blend(table, [None] * spk, np.arange(spk)), table.T)     # all empty: the gather
    assert np.array_equal(engine.speaker_blend(table, [{"vector": table[:, 0]}]), table[:, :1].T)


def test_kernel_entry_refuses_what_the_check_refuses():
    lib = engine.load_library()
    table = np.ones((4, 3), np.float32); out = np.zeros((2, 4), np.float32)
    for m in ({"sid": [3], "weight": [1.0]}, {"sid": [0], "weight": [float("nan")]}, {"vector": [0.0, float("inf"), 0.0, 0.0]}):
        with pytest.raises(engine.StsError, match="speaker mix"):
            engine.speaker_blend(table, [None, m])
    arr, keep = engine._speaker_mixes([None, None])
    args = (C.cast(arr, C.c_void_p), out.ctypes.data)
    assert lib.sts_speaker_blend(0, table.ctypes.data, 3, 4, 0, None, *args) == STS_EINVAL
    assert lib.sts_speaker_blend(0, None, 3, 4, 2, None, *args) == STS_EINVAL
    assert lib.sts_speaker_blend(0, table.ctypes.data, 0, 4, 2, None, *args) == STS_EINVAL
    assert lib.sts_speaker_blend(0, table.ctypes.data, 3, 4, 2, None, C.cast(arr, C.c_void_p), None) == STS_EINVAL
    assert lib.sts_speaker_blend(0, table.ctypes.data, 3, 4, 2, None, None, out.ctypes.data) == 0 and (out == 1).all()


# ---- 2: a one-hot mix is the plain sid ---------------------------------------------------------------------------------------------------
def test_one_hot_equals_the_plain_sid(case, engines):
    syn, _ = engines
    ids, n = case.ids, sum(LENS)
    sid = [case.spk - 1, 0, 1]
    hot = [{"sid": [s], "weight": [1.0]} for s in sid]
    syn.set_record_taps(True)
    plain = syn.infer_ids(ids[2], sid[0]); plain_s = _snap(syn, LENS[2])
    syn.set_speaker_mix(hot[:1])
    assert np.array_equal(syn.infer_ids(ids[2], 0), plain) and _snap(syn, LENS[2]) == plain_s
    plain = syn.infer_batch(ids, sid); plain_s = _snap(syn, n)
    syn.set_speaker_mix(hot)
    got = syn.infer_batch(ids, [0, 0, 0])
    assert all(np.array_equal(a, b) for a, b in zip(got, plain)) and _snap(syn, n) == plain_s
    syn.set_record_taps(False)
    plain = _cat(syn.infer_ids_stream(ids[2], 4, sid[0])[0])
    syn.set_speaker_mix(hot[:1])
    assert np.array_equal(_cat(syn.infer_ids_stream(ids[2], 4, 0)[0]), plain)


# ---- 3: blob-B equality in every call form -----------------------------------------------------------------------------------------------
def _c_infer_ids(syn, ids, sid):
    """sts_infer_ids itself (Synthesizer.infer_ids goes through sts_run_batch)"""
    a = np.ascontiguousarray(ids, np.int32)
    p, n = C.POINTER(C.c_int16)(), C.c_int32()
    engine._check(syn.lib, syn.lib.sts_infer_ids(syn.h, a.ctypes.data, a.size, int(sid), 1.0, C.byref(p), C.byref(n)))
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    syn.lib.sts_free(p)
    return out


def _c_infer_ids_batch(syn, ids, sid):
    """sts_infer_ids_batch itself"""
    B = len(ids)
    arrs = [np.ascontiguousarray(x, np.int32) for x in ids]
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in arrs])
    n = np.asarray([a.size for a in arrs], np.int32); s = np.ascontiguousarray(sid, np.int32)
    pcm = (C.POINTER(C.c_int16) * B)(); n_out = np.zeros(B, np.int32)
    f = syn.lib.sts_infer_ids_batch
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    engine._check(syn.lib, f(syn.h, B, ptrs, n.ctypes.data, s.ctypes.data, None, pcm, n_out.ctypes.data))
    out = [np.ctypeslib.as_array(pcm[b], shape=(int(n_out[b]),)).copy() for b in range(B)]
    for b in range(B):
        syn.lib.sts_free(pcm[b])
    return out


def test_blob_b_single_utterance(case, engines):
    a, b = engines
    ids = case.ids[2]
    for syn in (a, b):
        syn.set_record_taps(True)
    for j, m in enumerate(case.mixes):
        a.set_speaker_mix([m])
        got = _c_infer_ids(a, ids, 1); got_s = _snap(a, len(ids))
        want = _c_infer_ids(b, ids, case.spk + j); want_s = _snap(b, len(ids))
        assert np.array_equal(got, want) and got_s == want_s, (case.kind, j)
        assert not np.array_equal(got, _c_infer_ids(a, ids, 1))               # (and the mix is audible: sid 1 alone is another voice)
    for syn in (a, b):
        syn.set_record_taps(False)
    # the embedding the engine reports for the extra speakers of blob B is the reference's blend
    for j in range(3):
        assert np.array_equal(b.speaker_embedding(case.spk + j).view(np.uint32), case.cols[j].view(np.uint32))


def test_blob_b_batches(case, engines):
    a, b = engines
    n = sum(LENS)
    for syn in (a, b):
        syn.set_record_taps(True)
    a.set_speaker_mix(case.batch_mix)
    got = _c_infer_ids_batch(a, case.ids, case.sid_a); got_s = _snap(a, n)
    want = _c_infer_ids_batch(b, case.ids, case.sid_b); want_s = _snap(b, n)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and got_s == want_s
    a.set_speaker_mix(case.batch_mix)
    n_out = a.run_batch(case.ids, case.sid_a); got = a.pcm_host(); got_s = _snap(a, n)          # sts_run_batch
    assert np.array_equal(n_out, b.run_batch(case.ids, case.sid_b)) and np.array_equal(got, b.pcm_host()) and got_s == _snap(b, n)
    for syn in (a, b):
        syn.set_record_taps(False)
    a.set_speaker_mix(case.batch_mix)                       # without taps: launch-ahead is allowed, and a mixed run must not take it
    got = a.infer_batch(case.ids, case.sid_a)
    assert a.profile()["launch_ahead"] == 0
    assert all(np.array_equal(x, y) for x, y in zip(got, want))


def test_blob_b_streams(case, engines):
    a, b = engines
    ids = case.ids[2]
    for syn in (a, b):
        syn.set_record_taps(True)
    for j, m in enumerate(case.mixes[:2]):
        a.set_speaker_mix([m])
        got = _cat(a.infer_ids_stream(ids, 4, 1)[0]); got_s = _snap(a, len(ids), TAPS[:4])
        want = _cat(b.infer_ids_stream(ids, 4, case.spk + j)[0])
        assert np.array_equal(got, want) and got_s == _snap(b, len(ids), TAPS[:4]), (case.kind, j)
    # batched: the plain, shortest utterance is first and leaves the steps first, so the mixed ones' window index drops below their
    # utterance index
    want_chunks, _ = b.infer_batch_stream(case.ids, 4, case.sid_b); want_s = _snap(b, sum(LENS), TAPS[:4])
    want = [_cat(c) for c in want_chunks]
    steps = [len(c) for c in want_chunks]
    assert steps[0] < min(steps[1], steps[2]), steps        # (the premise: utterance 0 finishes steps before the others)
    a.set_speaker_mix(case.batch_mix)
    got_chunks, _ = a.infer_batch_stream(case.ids, 4, case.sid_a)
    assert [len(c) for c in got_chunks] == steps and _snap(a, sum(LENS), TAPS[:4]) == want_s
    for u in range(3):
        assert np.array_equal(_cat(got_chunks[u]), want[u]), (case.kind, u)
    for syn in (a, b):
        syn.set_record_taps(False)
    # the whole-call repeat of the two-term fp16 arithmetic applies the mix again
    before = a.profile()["conv_math_fallbacks"]
    a.debug_set("stream_retry_step", 0); b.debug_set("stream_retry_step", 0)
    a.set_speaker_mix(case.batch_mix)
    got_chunks, _ = a.infer_batch_stream(case.ids, 4, case.sid_a)
    ref_chunks, _ = b.infer_batch_stream(case.ids, 4, case.sid_b)
    a.debug_set("stream_retry_step", -1); b.debug_set("stream_retry_step", -1)
    assert a.profile()["conv_math_fallbacks"] == before + 1
    for u in range(3):
        assert np.array_equal(_cat(got_chunks[u]), _cat(ref_chunks[u])), (case.kind, u)
    a.set_conv_math("f16x2"); b.set_conv_math("f16x2")      # (re-arm the default form: one repeat does not pin, but leave no count behind)


def test_blob_b_pool_and_multi_device(case, engines):
    a, b = engines
    want = b.infer_batch(case.ids, case.sid_b)
    # mixed and plain requests folded into ONE packed batch: queued while the only worker is inside a long streaming request
    pool = engine.Pool(case.blob_a, device=0, n_engines=1, max_batch=3)
    busy = threading.Event()
    blocker = pool.submit_stream(sb.synthetic_ids(200, case.cfg.vocab, salt=1), 2, lambda pcm, off: busy.set())
    assert busy.wait(60)
    t = [pool.submit(x, sid=s, mix=m) for x, s, m in zip(case.ids, case.sid_a, case.batch_mix)]
    assert pool.wait(blocker) > 0
    got = [pool.wait(k) for k in t]
    assert pool.stats() == (2, 4)
    for u in range(3):
        assert np.array_equal(got[u], want[u]), (case.kind, u)
    with pytest.raises(engine.StsError, match="speaker mix"):
        pool.submit(case.ids[0], mix={"sid": [case.spk], "weight": [1.0]})
    pool.close()
    # two engines on one device: mixes[b] follows utterance b into its shard
    md = engine.MultiDevice(case.blob_a, [0, 0], gather="download")
    shard = md.shard_of(LENS)
    md.set_speaker_mix(case.batch_mix)
    multi = md.infer_batch(case.ids, case.sid_a)
    after = md.infer_batch(case.ids, case.sid_a)            # consumed: the plain sids
    md.set_speaker_mix(case.batch_mix[:2])
    with pytest.raises(engine.StsError, match="another batch"):
        md.infer_batch(case.ids, case.sid_a)
    with pytest.raises(engine.StsError, match="speaker mix"):
        md.set_speaker_mix([None, {"sid": [0], "weight": [17.0]}, None])
    md.close()
    assert len(set(int(v) for v in shard)) == 2
    for sh in sorted(set(int(v) for v in shard)):
        mem = [u for u in range(3) if int(shard[u]) == sh]
        ref = b.infer_batch([case.ids[u] for u in mem], [case.sid_b[u] for u in mem])
        plain = a.infer_batch([case.ids[u] for u in mem], [case.sid_a[u] for u in mem])
        for k, u in enumerate(mem):
            assert np.array_equal(multi[u], ref[k]) and np.array_equal(after[u], plain[k]), (case.kind, sh, u)


def test_cli_mix_flag(case, engines, tmp_path):
    """tools/cli/tts_ids --mix sid:weight,... against blob B's extra speaker (the flag is what this test is about: one child process)"""
    import os
    import subprocess
    from conftest import ROOT
    _, b = engines
    exe = tmp_path / "tts_ids"
    subprocess.run(["g++", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "cli", "tts_ids.cpp"),
                    "-L", os.path.dirname(engine.LIB_PATH), "-lsummertts_hip", "-Wl,-rpath," + os.path.dirname(engine.LIB_PATH),
                    "-o", str(exe)], check=True)
    ids = case.ids[1]
    (tmp_path / "m.bin").write_bytes(case.blob_a.tobytes())
    (tmp_path / "ids.txt").write_text(" ".join(str(int(i)) for i in ids) + "\n")
    out = tmp_path / "o.wav"
    r = subprocess.run([str(exe), "--mix", "0:0.6,%d:0.4" % (case.spk - 1), str(tmp_path / "ids.txt"), str(tmp_path / "m.bin"), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.frombuffer(out.read_bytes()[44:], np.int16), _c_infer_ids(b, ids, case.spk))
    r = subprocess.run([str(exe), "--mix", "%d:1" % case.spk, str(tmp_path / "ids.txt"), str(tmp_path / "m.bin"), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "speaker mix" in r.stdout


# ---- 4: the oracle -----------------------------------------------------------------------------------------------------------------------
def test_mixed_pcm_against_the_oracle_on_blob_b(case, engines):
    from oracle import pyref
    a, _ = engines
    ids = case.ids[2]
    port = pyref.PortModel(case.blob_b)
    a.set_record_taps(True)
    a.set_speaker_mix([case.mixes[1]])
    pcm = a.infer_ids(ids, 0)
    wave = a.tap("wave")[0]
    a.set_record_taps(False)
    o = port.infer_ids(ids, case.spk + 1, 1.0, forced_dur=a.durations(len(ids)))
    assert_pcm_close(pcm, o["pcm"], case.kind)
    assert_wave_close(wave, o["wave"], case.kind)


# ---- 5: lifetime -------------------------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals(case, engines):
    syn, b = engines
    ids = case.ids[1]
    plain = syn.infer_ids(ids, 2)
    mixed = b.infer_ids(ids, case.spk)
    syn.set_speaker_mix([case.mixes[0]])
    assert np.array_equal(syn.infer_ids(ids, 2), mixed)
    assert np.array_equal(syn.infer_ids(ids, 2), plain)                     # the call after a mixed call is the plain-sid result
    # B mismatch: refused, nothing runs, the mix is gone, the engine works
    for n_set, call in ((2, lambda: syn.infer_ids(ids, 2)), (1, lambda: syn.infer_batch([ids, ids], [2, 2])),
                        (2, lambda: syn.infer_ids_stream(ids, 4, 2)), (1, lambda: syn.infer_batch_stream([ids, ids], 4, [2, 2]))):
        syn.set_speaker_mix([case.mixes[0]] * n_set)
        with pytest.raises(engine.StsError, match="another batch"):
            call()
        assert np.array_equal(syn.infer_ids(ids, 2), plain)
    # a failed run consumes the mix; dropping a mix; a refused set call leaves a pending mix alone
    syn.set_speaker_mix([case.mixes[0]])
    with pytest.raises(engine.StsError):
        syn.infer_ids(list(ids[:-1]) + [case.cfg.vocab], 2)
    assert np.array_equal(syn.infer_ids(ids, 2), plain)
    syn.set_speaker_mix([case.mixes[0]]); syn.set_speaker_mix(None)
    assert np.array_equal(syn.infer_ids(ids, 2), plain)
    syn.set_speaker_mix([case.mixes[0]])
    for bad in ({"sid": [case.spk], "weight": [1.0]}, {"sid": [0], "weight": [float("nan")]}, {"sid": [0], "weight": [16.5]},
                {"vector": np.full(case.gin, np.inf, np.float32)}, {"vector": np.zeros(case.gin, np.float32), "vector_weight": float("inf")}):
        with pytest.raises(engine.StsError, match="speaker mix"):
            syn.set_speaker_mix([bad])
    assert syn.lib.sts_set_speaker_mix(syn.h, -1, None) == 0                # (mixes == NULL drops, whatever B)
    syn.set_speaker_mix([case.mixes[0]])
    arr = (engine.SpeakerMix * 1)()
    assert syn.lib.sts_set_speaker_mix(syn.h, -1, C.cast(arr, C.c_void_p)) == STS_EINVAL
    assert np.array_equal(syn.infer_ids(ids, 2), mixed)
    # an entry that is empty is the plain sid, in a batch that also blends
    syn.set_speaker_mix([{}, case.mixes[0]])
    got = syn.infer_batch([ids, ids], [2, 0])
    ref = b.infer_batch([ids, ids], [2, case.spk])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # sts_get_speaker_embedding: the blob's column; a bad sid or a short capacity is refused
    for s in range(case.spk):
        assert np.array_equal(syn.speaker_embedding(s).view(np.uint32), case.table[:, s].view(np.uint32))
    out = np.zeros(case.gin, np.float32)
    f = syn.lib.sts_get_speaker_embedding
    assert f(syn.h, case.spk, out.ctypes.data, case.gin) == STS_EINVAL and f(syn.h, -1, out.ctypes.data, case.gin) == STS_EINVAL
    assert f(syn.h, 0, out.ctypes.data, case.gin - 1) == STS_EINVAL and f(syn.h, 0, None, case.gin) == STS_EINVAL
    assert f(syn.h, 0, out.ctypes.data, case.gin) == 0 and np.array_equal(out, case.table[:, 0])


def test_a_single_speaker_engine_refuses_a_mix():
    cfg = sb.tiny_cfg("hifigan_fix")
    ids = sb.synthetic_ids(7, cfg.vocab)
    syn = engine.Synthesizer(sb.make_blob(cfg, 3))
    plain = syn.infer_ids(ids)
    for m in ({"sid": [0], "weight": [1.0]}, {"vector": [1.0]}):
        with pytest.raises(engine.StsError, match="single-speaker"):
            syn.set_speaker_mix([m])
    out = np.zeros(16, np.float32)
    assert syn.lib.sts_get_speaker_embedding(syn.h, 0, out.ctypes.data, 16) == STS_EINVAL
    syn.set_speaker_mix([None])                              # an empty entry is no mix
    assert np.array_equal(syn.infer_ids(ids), plain) and np.array_equal(syn.infer_ids(ids), plain)
    syn.close()


# ---- 6: combinations ---------------------------------------------------------------------------------------------------------------------
def test_mix_with_a_duration_plan_noise_and_forced_durations(case, engines):
    a, b = engines
    ids = case.ids[2]
    hop = a.info.samples_per_frame
    plan = {"target_frames": 4 * len(ids) + 3}
    a.set_speaker_mix([case.mixes[1]]); a.set_duration_plan([len(ids)], [plan])
    got = a.infer_ids(ids, 0); got_d = a.durations(len(ids))
    b.set_duration_plan([len(ids)], [plan])
    assert np.array_equal(got, b.infer_ids(ids, case.spk + 1)) and np.array_equal(got_d, b.durations(len(ids)))
    assert got.size == plan["target_frames"] * hop
    for syn in (a, b):
        syn.set_noise(0.667, 0.8, 99)
    a.set_speaker_mix(case.batch_mix)
    got = a.infer_batch(case.ids, case.sid_a)
    want = b.infer_batch(case.ids, case.sid_b)
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    for syn in (a, b):
        syn.set_noise(0.0, 0.0, 0)
    assert not np.array_equal(want[1], b.infer_batch(case.ids, case.sid_b)[1])        # (the noise was on)
    forced = np.full(len(ids), 3, np.int32)
    a.set_speaker_mix([case.mixes[0]]); a.set_forced_durations(forced); b.set_forced_durations(forced)
    got = a.infer_ids(ids, 0)
    assert np.array_equal(got, b.infer_ids(ids, case.spk)) and got.size == 3 * len(ids) * hop


def test_a_mixed_batch_under_poison(case, engines):
    a, b = engines
    want = b.infer_batch(case.ids, case.sid_b)
    a.debug_set("poison", 0x7FC00000)
    a.set_speaker_mix(case.batch_mix)
    got = a.infer_batch(case.ids, case.sid_a)
    poisoned = a.profile()["poison_bytes"]
    a.set_speaker_mix(case.batch_mix)
    chunks, _ = a.infer_batch_stream(case.ids, 4, case.sid_a)
    a.debug_set("poison", 0)
    assert poisoned > 0
    for u in range(3):
        assert np.array_equal(got[u], want[u]) and np.array_equal(_cat(chunks[u]), want[u]), (case.kind, u)


def test_the_memo_never_sees_a_mixed_run(case):
    syn = engine.Synthesizer(case.blob_a)
    ids = case.ids[2]
    first = syn.infer_ids(ids, 1)
    misses = syn.profile()["launch_ahead_misses"]
    assert np.array_equal(syn.infer_ids(ids, 1), first) and syn.profile()["launch_ahead"] == 1
    # a mix whose frame count differs from sid 1's would leave a wrong count under sid 1's key if it fed the memo
    for m in case.mixes:
        syn.set_speaker_mix([m])
        syn.infer_ids(ids, 1)
        assert syn.profile()["launch_ahead"] == 0
        again = syn.infer_ids(ids, 1)
        p = syn.profile()
        assert np.array_equal(again, first) and p["launch_ahead"] == 1 and p["launch_ahead_misses"] == misses
    b_first = syn.infer_batch(case.ids, case.sid_a); syn.infer_batch(case.ids, case.sid_a)
    assert syn.profile()["launch_ahead"] == 1
    syn.set_speaker_mix(case.batch_mix)
    syn.infer_batch(case.ids, case.sid_a)
    assert syn.profile()["launch_ahead"] == 0
    after = syn.infer_batch(case.ids, case.sid_a)
    p = syn.profile()
    assert all(np.array_equal(x, y) for x, y in zip(after, b_first)) and p["launch_ahead"] == 1 and p["launch_ahead_misses"] == misses
    syn.close()
