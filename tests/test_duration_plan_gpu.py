"""Duration plans on the MI355X (sts_set_duration_plan, sts_duration_plan_apply, sts_get_phoneme_offsets, sts_pool_submit_plan,
sts_multi_set_duration_plan) against the integer checker of tests/duration_ref.py, bit for bit: the kernel on caller weights across the wave,
the 256-thread loop and tail boundaries; an engine with an empty plan against one that never set a plan; per-phoneme rate, fixed pauses and
fit-to-length through both duration predictors; waveform parity with the oracle run on the planned durations; one utterance alone, in a
ragged batch, through a pool, through two engines and streamed; the launch-ahead memo; phoneme offsets at three output rates; every refusal."""
import numpy as np
import pytest

import duration_ref as dr
from conftest import TAP_MAXABS_TOL, assert_pcm_close, golden_files, load_golden
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

STS_EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


# ---- the kernel on caller weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1, 65, 300), (257,)], ids=str)
def test_apply_equals_the_reference_bit_for_bit(lens):
    """ragged batches across the wave (64), the 256-thread loop and a non-multiple tail; every adversarial weight set; without a target,
    at the minimum, at sum ceil(w) and at three times that; with and without fixed entries"""
    sets = [dr.weight_sets(n, 7 * n + 1) for n in lens]
    for name in sets[0]:
        ws = [s[name] for s in sets]
        for with_fixed in (False, True):
            fixed = [[(-1 if i % 3 else i % 5) for i in range(n)] for n in lens] if with_fixed else None
            per_utt = []
            for b, n in enumerate(lens):
                fx = fixed[b] if fixed else [-1] * n
                free = [ws[b][i] for i in range(n) if fx[i] < 0]
                sfix = sum(v for v in fx if v >= 0)
                per_utt.append([0] + (dr.targets(free, len(free), sfix) if free else [sfix]))
            for j in range(4):
                tg = [t[min(j, len(t) - 1)] for t in per_utt]
                if j == 3:
                    tg = [t if b % 2 else 0 for b, t in enumerate(tg)] if len(lens) > 1 else tg    # targets and none in one launch
                got = engine.duration_plan_apply(ws, fixed, tg)
                for b in range(len(lens)):
                    want = dr.fit(ws[b], fixed[b] if fixed else None, tg[b])
                    assert np.array_equal(got[b], want), (name, with_fixed, tg, b)
    # the members do not see each other, and target_frames / fixed may be absent altogether
    ws = [s["random"] for s in sets]
    alone = [engine.duration_plan_apply([w], None, [3 * w.size + 1])[0] for w in ws]
    both = engine.duration_plan_apply(ws, None, [3 * w.size + 1 for w in ws])
    assert all(np.array_equal(a, b) for a, b in zip(alone, both))
    plain = engine.duration_plan_apply(ws)
    assert all(np.array_equal(p, dr.fit(w)) for p, w in zip(plain, ws))


def test_apply_one_utterance_of_7000_weights():
    rng = np.random.default_rng(70)
    w = np.exp(rng.normal(0.5, 1.0, 7000)).astype(np.float32)
    w[rng.integers(0, 7000, 50)] = 0.0
    fixed = np.full(7000, -1, np.int32); fixed[::97] = 12
    for fx, target in ((None, 7000), (None, 7000 + 6999), (None, 31 * 7000 + 5), (fixed, 40000), (None, 1 << 20)):
        got = engine.duration_plan_apply([w], None if fx is None else [fx], [target])[0]
        assert np.array_equal(got, dr.fit(w, fx, target)), target
        assert int(got.sum()) == target
    eq = engine.duration_plan_apply([np.full(7000, 1.5, np.float32)], None, [7000 + 4321])[0]
    assert eq.tolist() == [2] * 4321 + [1] * (7000 - 4321)                 # ties go by index across every 256-thread pass


def test_apply_refuses_what_the_set_call_refuses():
    lib = engine.load_library()
    w = np.ones(6, np.float32); lens = np.asarray([2, 4], np.int32); out = np.zeros(6, np.int32)
    for fixed, tg in ((None, [1, 4]), ([0, 0, -1, -1, -1, -1], [1, 4]), ([-1, -1, 5, -1, -1, -1], [2, 7]), (None, [2, -4]), ([-3] + [-1] * 5, [0, 0])):
        f = None if fixed is None else np.asarray(fixed, np.int32)
        t = np.asarray(tg, np.int32)
        assert lib.sts_duration_plan_apply(0, w.ctypes.data, None if f is None else f.ctypes.data, lens.ctypes.data, 2, t.ctypes.data,
                                           out.ctypes.data) == STS_EINVAL, (fixed, tg)
    bad = np.asarray([2, 0], np.int32)
    assert lib.sts_duration_plan_apply(0, w.ctypes.data, None, bad.ctypes.data, 2, None, out.ctypes.data) == STS_EINVAL
    assert lib.sts_duration_plan_apply(0, w.ctypes.data, None, lens.ctypes.data, 0, None, out.ctypes.data) == STS_EINVAL


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
def _tiny(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    return cfg, sb.make_blob(cfg, seed)


def _planned(syn, ids, plan, sid=0, ls=1.0, taps=True):
    """one planned call -> (pcm, durations, dur_w tap or None)"""
    syn.set_record_taps(taps)
    syn.set_duration_plan([len(ids)], [plan])
    pcm = syn.infer_ids(ids, sid, ls)
    dur = syn.durations(len(ids))
    w = syn.tap("dur_w")[0] if taps else None
    syn.set_record_taps(False)
    return pcm, dur, w


@pytest.mark.parametrize("path", golden_files(), ids=lambda p: p.split("/")[-1])
def test_an_empty_plan_changes_nothing(path):
    """an engine that never set a plan against one given a plan whose fields are all NULL / 0, plain and with a poisoned workspace"""
    g, cfg, blob = load_golden(path)
    ids, sid, ls = g["ids"], int(g["sid"]), float(g["length_scale"])

    def run(plan, poison):
        syn = engine.Synthesizer(blob)
        if poison:
            syn.debug_set("poison", 0x7FC00000)
        syn.set_record_taps(True)
        if plan:
            syn.set_duration_plan([len(ids)], [{}])
        pcm = syn.infer_ids(ids, sid, ls)
        out = [pcm.tobytes(), syn.durations(len(ids)).tobytes()] + [syn.tap(k).tobytes() for k in ("m", "logw", "z_p")]
        has_w = True
        try:
            syn.tap("dur_w")
        except engine.StsError:
            has_w = False
        assert has_w == plan                                # the tap exists only for a run with a plan
        syn.set_record_taps(False)
        if plan:
            syn.set_duration_plan([len(ids)], [None])
        out.append(syn.infer_ids(ids, sid, ls).tobytes())   # without taps: the PCM goes straight to the host
        syn.close()
        return out

    want = run(False, False)
    assert (np.frombuffer(want[1], np.int32) == g["durations"]).all()
    assert run(True, False) == want
    assert run(True, True) == want


@pytest.mark.parametrize("kind", ["hifigan_sdp", "mbb_fix"])
def test_rate(kind):
    cfg, blob = _tiny(kind)
    ids = sb.synthetic_ids(70, cfg.vocab, salt=2)
    syn = engine.Synthesizer(blob)
    plain_pcm = syn.infer_ids(ids, 0, 1.1)
    plain_dur = syn.durations(len(ids))
    _, d0, w0 = _planned(syn, ids, {}, ls=1.1)
    assert np.array_equal(d0, plain_dur) and np.array_equal(d0, dr.fit(w0))
    rng = np.random.default_rng(3)
    rate = np.exp(rng.uniform(np.log(1 / 64), np.log(64), len(ids))).astype(np.float32)
    rate[:4] = (np.float32(1 / 64), np.float32(64), np.float32(1), np.float32(0.5))
    pcm, d, w = _planned(syn, ids, {"rate": rate}, ls=1.1)
    assert np.array_equal(w.view(np.uint32), (w0 * rate).astype(np.float32).view(np.uint32))
    assert np.array_equal(d, dr.fit(w)) and pcm.size == int(d.sum()) * syn.info.samples_per_frame
    assert not np.array_equal(d, plain_dur)
    pcm1, d1, w1 = _planned(syn, ids, {"rate": np.ones(len(ids), np.float32)}, ls=1.1)
    assert np.array_equal(d1, plain_dur) and np.array_equal(w1.view(np.uint32), w0.view(np.uint32)) and np.array_equal(pcm1, plain_pcm)
    syn.close()


@pytest.mark.parametrize("T", [1, 3, 64, 300])
@pytest.mark.parametrize("kind", ["hifigan_sdp", "mbb_fix"])
def test_fit_to_length(kind, T):
    cfg, blob = _tiny(kind)
    ids = sb.synthetic_ids(T, cfg.vocab, salt=T)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    syn.infer_ids(ids)
    natural = int(syn.durations(T).sum())
    for target in sorted({T, max(T, natural // 2), natural + 37, 2 * natural + T}):
        pcm, d, w = _planned(syn, ids, {"target_frames": target})
        assert int(d.sum()) == target and pcm.size == target * hop and syn.profile()["frames"] == target, (kind, T, target)
        assert np.array_equal(d, dr.fit(w, None, target)) and (d >= 1).all(), (kind, T, target)
    # fixed pauses inside a target, with a rate on top
    fixed = np.full(T, -1, np.int32); fixed[::4] = 5
    if T > 1:
        fixed[1] = 0
    n_free = int((fixed < 0).sum()); sfix = int(fixed[fixed >= 0].sum())
    target = sfix + (3 * n_free + 2 if n_free else 0)
    rate = np.linspace(0.5, 2.0, T).astype(np.float32)
    pcm, d, w = _planned(syn, ids, {"fixed": fixed, "target_frames": target, "rate": rate})
    assert np.array_equal(d, dr.fit(w, fixed, target)) and (d[fixed >= 0] == fixed[fixed >= 0]).all() and pcm.size == target * hop
    pcm, d, w = _planned(syn, ids, {"fixed": fixed})                       # pauses alone: the others keep their prediction
    assert np.array_equal(d, dr.fit(w, fixed, 0)) and pcm.size == max(int(d.sum()), 1) * hop
    # with sampling noise on: the plan sees the sampled logw
    syn.set_noise(0.667, 0.8, 99)
    target = natural + 11
    pcm, d, w = _planned(syn, ids, {"target_frames": target})
    assert int(d.sum()) == target and pcm.size == target * hop and np.array_equal(d, dr.fit(w, None, target))
    pcm2, d2, _ = _planned(syn, ids, {"target_frames": target}, taps=False)
    assert np.array_equal(pcm2, pcm) and np.array_equal(d2, d)
    syn.close()


@pytest.mark.parametrize("kind", ["hifigan_sdp", "ms_hifigan_sdp", "mbb_fix"])
def test_waveform_parity_with_the_oracle_on_the_planned_durations(kind):
    from oracle import pyref
    cfg, blob = _tiny(kind, 4321)
    ids = sb.synthetic_ids(29, cfg.vocab, salt=3)
    sid = 1 if cfg.is_ms else 0
    port = pyref.PortModel(blob)
    syn = engine.Synthesizer(blob)
    fixed = np.full(len(ids), -1, np.int32); fixed[[4, 17]] = (6, 0)
    rate = np.where(np.arange(len(ids)) < 10, 1.5, 0.8).astype(np.float32)
    free_run = port.infer_ids(ids, sid, 1.1)
    for plan in ({"rate": rate}, {"fixed": fixed, "target_frames": int(free_run["durations"].sum()) + 23}, {"target_frames": 2 * len(ids)}):
        syn.set_record_taps(True)
        syn.set_duration_plan([len(ids)], [plan])
        pcm = syn.infer_ids(ids, sid, 1.1)
        d = syn.durations(len(ids))
        o = port.infer_ids(ids, sid, 1.1, forced_dur=d, taps=True)
        assert_pcm_close(pcm, o["pcm"], f"{kind} {sorted(plan)}")
        for k in ("m", "z_p", "z"):
            assert np.abs(syn.tap(k) - o[k]).max() <= TAP_MAXABS_TOL, (kind, k)
        assert np.abs(syn.tap("wave")[0] - o["wave"]).max() <= TAP_MAXABS_TOL, kind
        syn.set_record_taps(False)
    syn.close()


def _plans3(lens):
    """a ragged batch of three: only the middle utterance has a plan"""
    n = lens[1]
    fixed = np.full(n, -1, np.int32); fixed[n // 2] = 7
    rate = np.linspace(0.7, 1.6, n).astype(np.float32)
    return [None, {"rate": rate, "fixed": fixed, "target_frames": 4 * n + 9}, None]


@pytest.mark.parametrize("kind", ["hifigan_sdp", "mbb_fix"])
def test_a_planned_utterance_does_not_depend_on_its_companions(kind):
    cfg, blob = _tiny(kind, 11)
    lens = (9, 31, 17)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    plans = _plans3(lens)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    syn.set_conv_mode(6)                                   # the project's contract for bit equality across call forms
    free = [syn.infer_ids(a) for a in ids]
    syn.set_duration_plan([lens[1]], [plans[1]])
    alone = syn.infer_ids(ids[1])
    alone_dur = syn.durations(lens[1])
    assert alone.size == plans[1]["target_frames"] * hop
    syn.set_duration_plan(lens, plans)
    batch = syn.infer_batch(ids)
    dur = syn.durations(sum(lens))
    assert np.array_equal(batch[1], alone) and np.array_equal(dur[lens[0]:lens[0] + lens[1]], alone_dur)
    assert np.array_equal(batch[0], free[0]) and np.array_equal(batch[2], free[2])
    assert all(np.array_equal(a, b) for a, b in zip(syn.infer_batch(ids), free))          # consumed: the next batch is unplanned
    # streamed: the chunks concatenate to the one-pass PCM
    for chunk in (5, 32):
        syn.set_duration_plan([lens[1]], [plans[1]])
        assert np.array_equal(_cat(syn.infer_ids_stream(ids[1], chunk)[0]), alone), (kind, chunk)
        syn.set_duration_plan(lens, plans)
        got, _ = syn.infer_batch_stream(ids, chunk)
        for b in range(3):
            assert np.array_equal(_cat(got[b]), batch[b]), (kind, chunk, b)
    syn.close()


def test_pool_and_multi_device_carry_the_plan_per_utterance():
    cfg, blob = _tiny("mbb_fix", 11)
    lens = (40, 33, 5)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    plans = _plans3(lens)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    single = []
    for a, p in zip(ids, plans):
        if p:
            syn.set_duration_plan([len(a)], [p])
        single.append(syn.infer_ids(a))
    syn.set_duration_plan(lens, plans)
    batch = syn.infer_batch(ids)
    assert single[1].size == batch[1].size == plans[1]["target_frames"] * hop
    # one request per batch: the single call's shapes, so the single call, bit for bit
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=1)
    t = [pool.submit(a, plan=p) for a, p in zip(ids, plans)]
    got = [pool.wait(k) for k in t]
    assert all(np.array_equal(g, s) for g, s in zip(got, single))
    with pytest.raises(engine.StsError):
        pool.submit(ids[0], plan={"target_frames": 3})                                  # fewer frames than phonemes
    with pytest.raises(engine.StsError):
        pool.submit(ids[0], plan={"rate": np.full(lens[0], 65.0, np.float32)})
    pool.close()
    # planned and unplanned requests folded into ONE packed batch: they are queued while the only worker is inside a long streaming request
    # (streaming and whole-utterance requests never share a batch), whose first chunk tells this thread that the worker is busy
    import threading
    pool = engine.Pool(blob, device=0, n_engines=1, max_batch=3)
    busy = threading.Event()
    blocker = pool.submit_stream(sb.synthetic_ids(300, cfg.vocab, salt=1), 2, lambda pcm, off: busy.set())
    assert busy.wait(60)
    t = [pool.submit(a, plan=p) for a, p in zip(ids, plans)]
    assert pool.wait(blocker) > 0
    got = [pool.wait(k) for k in t]
    assert pool.stats() == (2, 4)
    for b in range(3):
        assert np.array_equal(got[b], batch[b]), b                                      # the same packed batch as the engine's own
    pool.close()
    # two engines on one device: each runs its shard as one batch with its members' plans
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    shard = md.shard_of(lens)
    md.set_duration_plan(lens, plans)
    multi = md.infer_batch(ids)
    free = md.infer_batch(ids)                                                          # consumed
    with pytest.raises(engine.StsError):
        md.set_duration_plan(lens, [None, {"target_frames": 1}, None])
    md.set_duration_plan(lens[:2], plans[:2])
    with pytest.raises(engine.StsError):
        md.infer_batch(ids)                                                             # set for another batch
    md.close()
    assert multi[1].size == plans[1]["target_frames"] * hop and free[1].size != multi[1].size
    for sh in sorted(set(int(v) for v in shard)):
        mem = [b for b in range(3) if int(shard[b]) == sh]
        syn.set_duration_plan([lens[b] for b in mem], [plans[b] for b in mem])
        ref = syn.infer_batch([ids[b] for b in mem])
        for k, b in enumerate(mem):
            assert np.array_equal(multi[b], ref[k]), (sh, b)
    syn.close()


def test_the_memo_never_sees_a_planned_run():
    cfg, blob = _tiny("hifigan_sdp", 21)
    ids = sb.synthetic_ids(30, cfg.vocab, salt=5)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    first = syn.infer_ids(ids)
    natural = first.size // hop
    misses = syn.profile()["launch_ahead_misses"]
    for target in (natural + 200, natural + 70):
        syn.set_duration_plan([len(ids)], [{"target_frames": target}])
        assert syn.infer_ids(ids).size == target * hop
        assert syn.profile()["launch_ahead"] == 0
        again = syn.infer_ids(ids)                          # the plan is consumed; this one runs ahead, from the count the unplanned call left
        p = syn.profile()
        assert np.array_equal(again, first) and p["launch_ahead"] == 1 and p["launch_ahead_misses"] == misses, target
    # batches: the same through the per-utterance memo
    b_ids = [ids, sb.synthetic_ids(12, cfg.vocab, salt=6)]
    b_first = syn.infer_batch(b_ids); syn.infer_batch(b_ids)
    assert syn.profile()["launch_ahead"] == 1
    syn.set_duration_plan([30, 12], [None, {"target_frames": 100}])
    planned = syn.infer_batch(b_ids)
    assert planned[1].size == 100 * hop and planned[0].size == b_first[0].size and syn.profile()["launch_ahead"] == 0
    after = syn.infer_batch(b_ids)
    p = syn.profile()
    assert all(np.array_equal(a, b) for a, b in zip(after, b_first)) and p["launch_ahead"] == 1 and p["launch_ahead_misses"] == misses
    # the whole-call repeat of a batched stream under the two-term fp16 arithmetic applies the plan again
    syn.set_conv_math("f16x2")
    before = syn.profile()["conv_math_fallbacks"]
    syn.debug_set("stream_retry_step", 0)
    syn.set_duration_plan([30, 12], [{"target_frames": 64}, {"target_frames": 100}])
    tot = []
    syn.infer_batch_stream(b_ids, 16, n_total=tot)
    syn.debug_set("stream_retry_step", -1)
    assert tot == [64 * hop, 100 * hop] and syn.profile()["conv_math_fallbacks"] == before + 1
    tot = []
    syn.infer_batch_stream(b_ids, 16, n_total=tot)
    assert tot == [b_first[0].size, b_first[1].size]
    syn.close()


def test_phoneme_offsets():
    cfg, blob = _tiny("mbb_fix", 5)
    lens = (13, 4, 21)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in lens]
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    for rate in (16000, 8000, 44100):
        syn.set_output_rate(rate)
        P, Q = (1, 1) if rate == 16000 else engine.resample_table(16000, rate)[:2]
        pcm = syn.infer_ids(ids[0])
        d = syn.durations(lens[0])
        off = syn.phoneme_offsets(lens[0])
        want = np.ceil(np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.float64) * hop * P / Q).astype(np.int64)
        assert np.array_equal(off, want) and np.array_equal(off, dr.offsets(d, lens[:1], hop, P, Q)), rate
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= pcm.size
        syn.set_duration_plan(lens, [None, {"target_frames": 9}, {"rate": np.full(lens[2], 2.0, np.float32)}])
        batch = syn.infer_batch(ids)
        d = syn.durations(sum(lens))
        off = syn.phoneme_offsets(sum(lens))
        assert np.array_equal(off, dr.offsets(d, lens, hop, P, Q)), rate
        assert [int(off[o]) for o in (0, lens[0], lens[0] + lens[1])] == [0, 0, 0]
        chunks, _ = syn.infer_ids_stream(ids[2], 8)                          # after a streaming call too
        assert np.array_equal(syn.phoneme_offsets(lens[2]), dr.offsets(syn.durations(lens[2]), lens[2:], hop, P, Q))
    lib = engine.load_library()
    small = np.zeros(3, np.int64)
    assert lib.sts_get_phoneme_offsets(syn.h, small.ctypes.data, 3) < 0 and lib.sts_get_phoneme_offsets(syn.h, None, 100) < 0
    syn.close()


def test_every_refusal_leaves_the_engine_usable():
    cfg, blob = _tiny("hifigan_fix", 3)
    ids = sb.synthetic_ids(7, cfg.vocab)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    plain = syn.infer_ids(ids)
    nan, inf = float("nan"), float("inf")
    ok_fixed = [-1, 2, -1, -1, 0, -1, -1]
    bad = [{"rate": [1, 1, nan, 1, 1, 1, 1]}, {"rate": [1, inf, 1, 1, 1, 1, 1]}, {"rate": [1 / 65, 1, 1, 1, 1, 1, 1]}, {"rate": [1, 1, 1, 1, 1, 1, 64.5]},
           {"rate": [0, 1, 1, 1, 1, 1, 1]}, {"rate": [-1, 1, 1, 1, 1, 1, 1]}, {"fixed": [-2] + ok_fixed[1:]}, {"fixed": [100001] + ok_fixed[1:]},
           {"target_frames": -1}, {"target_frames": (1 << 20) + 1}, {"target_frames": 6},
           {"fixed": ok_fixed, "target_frames": 6}, {"fixed": [1] * 7, "target_frames": 8}, {"fixed": [1] * 7, "target_frames": 6}]
    syn.set_duration_plan([7], [{"target_frames": 20}])                     # a pending plan survives every refused set call
    for p in bad:
        with pytest.raises(engine.StsError):
            syn.set_duration_plan([7], [p])
    with pytest.raises(engine.StsError):
        syn.set_duration_plan([0], [{}])
    lib = engine.load_library()
    n = np.asarray([7], np.int32)
    arr = (engine.DurPlan * 1)()
    assert lib.sts_set_duration_plan(syn.h, -1, n.ctypes.data, arr) == STS_EINVAL and lib.sts_set_duration_plan(syn.h, 1, None, arr) == STS_EINVAL
    assert syn.infer_ids(ids).size == 20 * hop
    # the limits themselves are valid
    syn.set_duration_plan([7], [{"rate": [1 / 64, 64, 1, 1, 1, 1, 1], "fixed": [100000, 0, -1, -1, -1, -1, -1], "target_frames": 100005}])
    assert syn.infer_ids(ids).size == 100005 * hop
    syn.set_duration_plan([7], [{"fixed": [1] * 7, "target_frames": 7}])
    assert syn.infer_ids(ids).size == 7 * hop
    # a plan for another batch: refused, nothing runs, the plan is gone
    for n_set, call in (([8], lambda: syn.infer_ids(ids)), ([7, 7], lambda: syn.infer_ids(ids)), ([7], lambda: syn.infer_batch([ids, ids])),
                        ([7], lambda: syn.infer_ids_stream(sb.synthetic_ids(6, cfg.vocab), 4)), ([7, 3], lambda: syn.infer_batch_stream([ids, ids], 4))):
        syn.set_duration_plan(n_set, [{"target_frames": 50}] + [None] * (len(n_set) - 1))
        with pytest.raises(engine.StsError, match="another batch"):
            call()
        assert np.array_equal(syn.infer_ids(ids), plain)
    # a failed run consumes the plan as well
    syn.set_duration_plan([7], [{"target_frames": 50}])
    with pytest.raises(engine.StsError):
        syn.infer_ids([0, 1, 2, 3, 4, 5, cfg.vocab])
    assert np.array_equal(syn.infer_ids(ids), plain)
    # dropping a plan; a plan together with forced durations
    syn.set_duration_plan([7], [{"target_frames": 50}]); syn.set_duration_plan(None)
    assert np.array_equal(syn.infer_ids(ids), plain)
    syn.set_duration_plan([7], [{"target_frames": 50}]); syn.set_forced_durations([3] * 7)
    with pytest.raises(engine.StsError, match="both"):
        syn.infer_ids(ids)
    assert np.array_equal(syn.infer_ids(ids), plain)                         # both are gone
    syn.close()
