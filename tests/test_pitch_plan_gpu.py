"""The pitch plan's warp kernel on the MI355X (sts_pitch_apply) against the float64 restatement of tests/pitch_ref.py: hop 1, 6 and 256;
warped lengths of exactly one output tile, one less, one more, and three tiles with a tail; a phoneme boundary on a tile boundary; cents
+-600, +-1 and 0; a member without a plan between two planned ones; long members next to short ones; each member alone against the batch.
|y - ref| <= 2^-23 |ref| + 2^-40 S_j (DESIGN.md 9l has the derivation; the worst observed err / tol is printed)."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as pr
from summertts_amd import engine

pytestmark = pytest.mark.gpu

STS_EINVAL = -1
TILE = 256                      # pitch_plan.hip PP_TILE


def _signal(n, seed):
    t = np.arange(n)
    rng = np.random.default_rng(seed)
    return np.clip(0.3 * np.sin(2 * np.pi * 0.031 * t + seed) + 0.1 * rng.standard_normal(n), -0.7, 0.7).astype(np.float32)


def _fit(d, cents, hop, target):
    """d, cents + one more phoneme so that the warped length is exactly `target`"""
    for c in [0, 600, -600, 1, -1] + list(range(-599, 600)):       # (hop > 1: the length moves in steps of about hop / ratio, so the cents are searched too)
        for dl in range(0, 3 * target // hop + 3):
            dd, cc = list(d) + [dl], list(cents) + [c]
            if pr.warped_length(dd, pr.design(cc)[1], hop) == target:
                return dd, cc
    raise AssertionError((hop, target))


def _check(sig, durs, plans, hop, worst):
    """one launch against the restatement; -> (y, pcm, reference results per member)"""
    B = len(durs)
    y, pcm = engine.pitch_apply(sig, durs, plans, hop)
    refs = []
    for b in range(B):
        ry, S, y64 = pr.apply(sig[b], durs[b], hop, plans[b])
        refs.append((ry, S))
        want_len = sig[b].size if plans[b] is None else pr.warped_length(durs[b], pr.design(plans[b])[1], hop)
        assert y[b].size == want_len == ry.size and pcm[b].size == want_len, (hop, b, y[b].size, want_len)
        assert np.array_equal(pcm[b], pr.pcm_cast(y[b])), (hop, b)                   # the cast of the kernel's own y, bit for bit
        if plans[b] is None:
            assert y[b].tobytes() == sig[b].tobytes(), (hop, b)
            continue
        assert np.isfinite(y[b]).all()
        ref = ry.astype(np.float64)
        tol = pr.tolerance(ref, S)
        err = np.abs(y[b].astype(np.float64) - ref)
        ratio = float((err / np.maximum(tol, 1e-300)).max())
        worst.append(ratio)
        assert (err <= tol).all(), (hop, b, int(np.argmax(err / np.maximum(tol, 1e-300))), ratio)
        # PCM: within 1 LSB of the cast of ref, and different only where ref 32737 lies within tol 32737 of an integer
        want = pr.pcm_cast(ry)
        diff = pcm[b].astype(np.int64) - want.astype(np.int64)
        assert np.abs(diff).max() <= 1, (hop, b)
        v = ref * 32737.0
        near = np.abs(v - np.round(v)) <= tol * 32737.0
        assert not (diff != 0)[~near].any() and int((diff != 0).sum()) <= int(near.sum()), (hop, b)
    print(f"hop {hop}: worst err / tol over {len(worst)} planned members so far: {max(worst):.3g}")
    return y, pcm, refs


def _alone(sig, durs, plans, hop, y, pcm):
    for b in range(len(durs)):
        ya, pa = engine.pitch_apply([sig[b]], [durs[b]], [plans[b]], hop)
        assert ya[0].tobytes() == y[b].tobytes() and np.array_equal(pa[0], pcm[b]), (hop, b)


WORST = []


def test_one_sample_per_frame_on_every_tile_edge():
    """hop 1: warped lengths TILE, TILE - 1, TILE + 1 and 3 TILE + 77 out of mixed cents with one-sample phonemes that are stepped over and
    runs of empty ones; a phoneme boundary on the tile boundary (the first phoneme emits exactly TILE outputs, at 0 and at -600 cents); a
    member without a plan between planned ones; members alone"""
    hop = 1
    pre_d, pre_c = [0, 0, 70] + [1] * 9 + [0, 0, 0, 40, 1, 20, 0], [600, -600, 600] + [600] * 9 + [0, 1, -1, -600, 0, -1, 600]
    cases = [_fit(pre_d, pre_c, hop, t) for t in (TILE, TILE - 1, TILE + 1, 3 * TILE + 77)]
    for (d, c), t in zip(cases, (TILE, TILE - 1, TILE + 1, 3 * TILE + 77)):
        assert pr.warped_length(d, pr.design(c)[1], hop) == t
    cases.append(([TILE, 50, 0, 30], [0, 600, 0, -600]))                           # boundary on the tile boundary, no residue
    for c in (600, -600):                                                          # ... and with a residue carried across it
        first = next(dl for dl in range(TILE // 2, 2 * TILE) if pr.warped_length([dl], pr.design([c])[1], hop) == TILE)
        assert pr.layout([first], pr.design([c])[1], hop)[1][1] > 0
        cases.append(([first, 33, 1, 1, 0, 21], [c, 600, 600, 600, 0, -c]))
    durs = [c[0] for c in cases]
    plans = [c[1] for c in cases]
    durs.insert(3, [5, 0, 600]); plans.insert(3, None)                            # copied, between planned members
    sig = [_signal(max(1, int(np.sum(d))) * hop, 3 + b) for b, d in enumerate(durs)]
    y, pcm, _ = _check(sig, durs, plans, hop, WORST)
    _alone(sig, durs, plans, hop, y, pcm)


def test_hop_6_long_members_next_to_short_ones():
    """hop 6: one-frame and empty utterances (shorter than the filter's reach: every tap outside reads 0, never the neighbour's samples,
    which are large) next to members of several tiles; all durations 0; exact tile lengths where the search finds them"""
    hop = 6
    rng = np.random.default_rng(11)
    long_d = rng.integers(0, 60, 12).tolist()
    long_c = [600, -600, 1, -1, 0, 37, -600, 600, 0, 0, -333, 599]
    fit_d, fit_c = _fit([20, 0, 0, 15, 1], [600, 0, 0, -600, 600], hop, 2 * TILE)
    durs = [long_d, [1], [0, 0, 0], fit_d, [0, 1, 0], [400, 0, 175]]
    plans = [long_c, [600], [600, -600, 1], fit_c, [0, -600, 0], None]
    sig = [_signal(max(1, int(np.sum(d))) * hop, 20 + b) for b, d in enumerate(durs)]
    sig[0] = (sig[0] * 1.3).astype(np.float32)                                     # the neighbours of the short members are loud
    y, pcm, _ = _check(sig, durs, plans, hop, WORST)
    assert y[2].size == hop and y[1].size == pr.warped_length([1], pr.design([600])[1], hop)
    _alone(sig, durs, plans, hop, y, pcm)


def test_a_model_hop_and_the_entrys_refusals():
    hop = 256
    durs = [[2, 0, 1, 3, 0], [4], [1, 1], [0, 0], [3, 2]]
    plans = [[600, 600, -600, 1, 0], [0], None, [600, 0], [-1, -600]]
    sig = [_signal(max(1, int(np.sum(d))) * hop, 40 + b) for b, d in enumerate(durs)]
    y, pcm, _ = _check(sig, durs, plans, hop, WORST)
    assert y[1].size == 4 * hop and y[3].size == hop                               # all cents 0 keeps the length; all durations 0: one frame
    _alone(sig, durs, plans, hop, y, pcm)
    lib = engine.load_library()
    x = np.zeros(8, np.float32); d = np.asarray([1, 1], np.int32); n = np.asarray([2], np.int32)
    cents = np.asarray([0, 0], np.int32)
    arr = (engine.PitchPlan * 1)()
    arr[0].cents = cents.ctypes.data
    out = np.zeros(8, np.float32); ln = np.zeros(1, np.int64)

    def call(B, spf, dd=d, cap=8):
        return lib.sts_pitch_apply(0, x.ctypes.data, dd.ctypes.data, n.ctypes.data, B, spf, arr, ln.ctypes.data, out.ctypes.data, None, cap)
    assert call(1, 4) == 0 and ln[0] == 8
    for B, spf in ((0, 4), (1, 0), (65536, 4), (1, (1 << 20) + 1)):
        assert call(B, spf) == STS_EINVAL
    assert call(1, 4, np.asarray([1, -1], np.int32)) == STS_EINVAL
    ln[0] = 0
    assert call(1, 4, cap=7) == STS_EINVAL and ln[0] == 8                          # too small: the lengths are still reported
    cents[1] = 601
    assert call(1, 4) == STS_EINVAL


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
import loudness_ref as lr          # noqa: E402
import resample_ref as rr          # noqa: E402
from summertts_amd import synth_blob as sb                  # noqa: E402
from test_loudness_gpu import _close as loud_close          # noqa: E402  (the loudness checker's own comparison)

RESAMPLE_WAVE_TOL = 1e-5        # tests/test_resample_gpu.py: |wave_out - checker| of the resampled float wave


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _tiny(kind, seed=1234):
    cfg = sb.tiny_cfg(kind)
    return cfg, sb.make_blob(cfg, seed)


def _cents(n, seed):
    """per-phoneme cents over the whole range: both limits, +-1, 0 and random values"""
    c = np.random.default_rng(seed).integers(-600, 601, n).astype(np.int32)
    c[::5] = 600; c[1::5] = -600
    if n > 4:
        c[2], c[3], c[4] = 1, -1, 0
    return c


def _pitched(syn, ids, cents, sid=0, before=None):
    """one call with a pitch plan and taps on -> (pcm, wave, wave_pitch, durations, offsets); before(): further setters of the call"""
    syn.set_record_taps(True)
    if before:
        before()
    syn.set_pitch_plan([len(ids)], [cents])
    pcm = syn.infer_ids(ids, sid)
    out = pcm, syn.tap("wave")[0], syn.tap("wave_pitch")[0], syn.durations(len(ids)), syn.phoneme_offsets(len(ids))
    syn.set_record_taps(False)
    return out


def _against_ref(x, dur, hop, cents, y, what):
    """the engine's warped signal against the restatement applied to x; -> the restatement's o"""
    ry, S, y64 = pr.apply(x, dur, hop, cents)
    assert y.size == ry.size, (what, y.size, ry.size)
    ref = ry.astype(np.float64)
    tol = pr.tolerance(ref, S)
    err = np.abs(y.astype(np.float64) - ref)
    print(f"{what}: worst err / tol {float((err / np.maximum(tol, 1e-300)).max()):.3g}")
    assert (err <= tol).all(), what
    return pr.rows(dur, pr.design(cents)[1], hop)[0] if int(np.sum(dur)) > 0 else [0] * (len(dur) + 1)


@pytest.mark.parametrize("kind", ["hifigan_sdp", "mbb_fix"])
def test_native_rate_is_the_restatement_on_the_calls_own_wave(kind):
    cfg, blob = _tiny(kind)
    ids = sb.synthetic_ids(23, cfg.vocab, salt=2)
    n = len(ids)
    cents = _cents(n, 5)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    plain = syn.infer_ids(ids)
    plain_dur = syn.durations(n)
    pcm, wave, y, dur, off = _pitched(syn, ids, cents)
    o = _against_ref(wave, dur, hop, cents, y, kind)
    assert np.array_equal(pcm, pr.pcm_cast(y)) and pcm.size == o[-1]
    assert np.array_equal(off, np.asarray(o[:-1], np.int64))
    # the durations are those of a run with the duration plan rate = ratio
    syn.set_duration_plan([n], [{"rate": pr.design(cents)[0]}])
    stretched = syn.infer_ids(ids)
    assert np.array_equal(syn.durations(n), dur) and stretched.size == int(dur.sum()) * hop and not np.array_equal(dur, plain_dur)
    # without taps: the warp kernel writes the host PCM itself; and through a download
    syn.set_pitch_plan([n], [cents])
    assert np.array_equal(syn.infer_ids(ids), pcm)
    syn.debug_set("pcm_direct", 0)
    syn.set_pitch_plan([n], [cents])
    assert np.array_equal(syn.infer_ids(ids), pcm)
    syn.debug_set("pcm_direct", 1)
    # all cents 0: the durations and the length of a plain call, filtered all the same
    pcm0, wave0, y0, dur0, off0 = _pitched(syn, ids, np.zeros(n, np.int32))
    assert np.array_equal(dur0, plain_dur) and pcm0.size == plain.size and np.array_equal(pr.pcm_cast(wave0), plain)
    _against_ref(wave0, dur0, hop, np.zeros(n, np.int32), y0, kind + " 0 cents")
    assert np.array_equal(off0, np.concatenate([[0], np.cumsum(dur0)[:-1]]) * hop)
    # the next plain call is the one before, and has no "wave_pitch"
    syn.set_record_taps(True)
    assert np.array_equal(syn.infer_ids(ids), plain)
    with pytest.raises(engine.StsError):
        syn.tap("wave_pitch")
    syn.set_record_taps(False)
    assert np.array_equal(syn.infer_ids(ids), plain) and syn.profile()["launch_ahead"] == 1
    syn.set_pitch_plan([n], [cents])
    assert np.array_equal(syn.infer_ids(ids), pcm) and syn.profile()["launch_ahead"] == 0      # never launched ahead, never in the memo
    assert np.array_equal(syn.infer_ids(ids), plain) and syn.profile()["launch_ahead"] == 1
    syn.close()


def test_counts_offsets_and_the_chain_behind_the_warp():
    """8000, 44100 and 48000 Hz: counts ceil(N' P / Q), offsets ceil(o_i P / Q), "wave_out" against the resampler's checker fed "wave_pitch";
    then the limiter and loudness against their checkers fed the same signal"""
    cfg, blob = _tiny("mbb_fix", 7)
    ids = sb.synthetic_ids(40, cfg.vocab, salt=3)
    n = len(ids)
    cents = _cents(n, 8)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    for rate in (8000, 44100, 48000):
        syn.set_output_rate(rate)
        pcm, wave, y, dur, off = _pitched(syn, ids, cents)
        syn.set_record_taps(True); syn.set_pitch_plan([n], [cents]); syn.infer_ids(ids)
        got = syn.tap("wave_out")[0]
        syn.set_record_taps(False)
        o = _against_ref(wave, dur, hop, cents, y, f"rate {rate}")
        want = rr.resample(y, rate)
        err = float(np.abs(got - want).max())
        print(f"rate {rate}: max |wave_out - checker(wave_pitch)| = {err:.3e}")
        assert got.size == pcm.size == rr.out_len(y.size, rate) and err <= RESAMPLE_WAVE_TOL, (rate, err)
        assert np.array_equal(pcm, rr.pcm_cast(got)), rate
        assert np.array_equal(off, np.asarray([rr.out_len(v, rate) for v in o[:-1]], np.int64)), rate
    syn.set_output_rate(16000)
    lim = dict(gain_db=6.0, ceiling_dbfs=-3.0, lookahead_ms=2.0)
    syn.set_limiter(engine.LIMITER_ON, **lim)
    pcm, wave, y, dur, off = _pitched(syn, ids, cents)
    _against_ref(wave, dur, hop, cents, y, "limiter")
    ly, lp, _ = engine.limiter_apply([y], 16000, **lim)
    assert np.array_equal(pcm, lp[0])
    syn.set_limiter(engine.LIMITER_OFF)
    syn.set_loudness(engine.LOUD_NORMALIZE, -20.0, -1.0)
    pcm, wave, y, dur, off = _pitched(syn, ids, cents)
    r = syn.loudness()[0]
    loud_close(r, lr.loudness(y, 16000, -20.0, -1.0), "warped")
    assert np.array_equal(pcm, lr.normalize(y, r["gain"]))
    syn.set_loudness(engine.LOUD_OFF)
    syn.close()


def test_composition_with_a_gain_plan_a_mix_and_forced_durations():
    cfg, blob = _tiny("ms_hifigan_sdp", 5)
    ids = sb.synthetic_ids(12, cfg.vocab, salt=4)
    n = len(ids)
    cents = _cents(n, 2)
    syn = engine.Synthesizer(blob)
    hop = syn.info.samples_per_frame
    db = np.asarray([0, -6, 6, -float("inf"), -12, 12, 3, -3, -6, 6, -20, 0], np.float32)

    def before():
        syn.set_speaker_mix([{"sid": [0, 3], "weight": [0.5, 0.5]}])
        syn.set_gain_plan([n], [{"gain_db": db, "ramp_ms": 2.0}])
    pcm, wave, y, dur, off = _pitched(syn, ids, cents, sid=1, before=before)
    syn.set_record_taps(True); before(); syn.set_pitch_plan([n], [cents]); syn.infer_ids(ids, 1)
    gained = syn.tap("wave_gain")[0]
    syn.set_record_taps(False)
    import gain_ref as gr
    assert gained.tobytes() == gr.apply(wave, dur, hop, db, 2.0).tobytes()        # "wave_gain" stays the gained, unwarped signal
    o = _against_ref(gained, dur, hop, cents, y, "gain + mix")
    assert np.array_equal(pcm, pr.pcm_cast(y)) and pcm.size == o[-1]
    # forced durations are used as given
    forced = [3, 0, 5, 1, 0, 0, 7, 2, 1, 4, 0, 6]
    pcm, wave, y, dur, off = _pitched(syn, ids, cents, before=lambda: syn.set_forced_durations(forced))
    assert dur.tolist() == forced
    o = _against_ref(wave, dur, hop, cents, y, "forced")
    assert np.array_equal(pcm, pr.pcm_cast(y)) and np.array_equal(off, np.asarray(o[:-1], np.int64))
    # a duration plan's rates are multiplied by the ratios; a fixed phoneme takes 0 cents only; target_frames admits no cents
    rate = np.linspace(0.7, 1.6, n).astype(np.float32)
    fixed = [-1] * n; fixed[3] = 4
    c2 = cents.copy(); c2[3] = 0
    pcm, wave, y, dur, off = _pitched(syn, ids, c2, before=lambda: syn.set_duration_plan([n], [{"rate": rate, "fixed": fixed}]))
    syn.set_duration_plan([n], [{"rate": rate * pr.design(c2)[0], "fixed": fixed}])
    syn.infer_ids(ids)
    assert np.array_equal(syn.durations(n), dur) and dur[3] == 4
    _against_ref(wave, dur, hop, c2, y, "duration plan")
    plain = syn.infer_ids(ids)
    c3 = c2.copy(); c3[3] = 5
    for plan, c in (({"fixed": fixed}, c3), ({"target_frames": 90}, c2)):
        syn.set_duration_plan([n], [plan]); syn.set_pitch_plan([n], [c])
        with pytest.raises(engine.StsError):
            syn.infer_ids(ids)
        assert np.array_equal(syn.infer_ids(ids), plain)                          # both plans are gone
    syn.set_duration_plan([n], [{"target_frames": 90}]); syn.set_pitch_plan([n], [np.zeros(n, np.int32)])
    assert syn.infer_ids(ids).size == 90 * hop                                     # all cents 0 go with a fitted length
    syn.close()


def _infer_ids_c(syn, ids, sid=0, ls=1.0):
    """sts_infer_ids itself (the class goes through sts_run_batch + sts_copy_pcm_host)"""
    a = np.ascontiguousarray(ids, dtype=np.int32)
    p, n = C.POINTER(C.c_int16)(), C.c_int32()
    rc = syn.lib.sts_infer_ids(syn.h, a.ctypes.data, a.size, sid, ls, C.byref(p), C.byref(n))
    assert rc == 0, syn.lib.sts_last_error()
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    syn.lib.sts_free(p)
    return out


@pytest.mark.parametrize("kind,rate", [("hifigan_sdp", 16000), ("mbb_fix", 44100)])
def test_one_utterance_gives_the_same_bits_in_every_call_form(kind, rate):
    """pinned conv mode (as the gain plan's call-form test): sts_infer_ids, a ragged batch of 3 with plans on two members, the member
    without one bit-identical to a batch without any plan; pool and multi-device"""
    cfg, blob = _tiny(kind, 11)
    lens = (37, 9, 24)
    ids = [sb.synthetic_ids(k, cfg.vocab, salt=k) for k in lens]
    plans = [_cents(lens[0], 31), None, _cents(lens[2], 33)]
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(rate)
    free = syn.infer_batch(ids)
    alone = []
    for a, p in zip(ids, plans):
        syn.set_pitch_plan([len(a)], [p])
        alone.append(_infer_ids_c(syn, a))
    assert np.array_equal(alone[1], free[1]) and alone[0].size != free[0].size
    syn.set_pitch_plan(lens, plans)
    batch = syn.infer_batch(ids)                                                   # sts_run_batch + sts_copy_pcm_host
    offs = syn.phoneme_offsets(sum(lens))
    for b in range(3):
        assert np.array_equal(batch[b], alone[b]), (kind, rate, b)
    assert offs[lens[0]] == 0 and offs[lens[0] + lens[1]] == 0                     # offsets are per utterance
    assert all(np.array_equal(a, b) for a, b in zip(syn.infer_batch(ids), free))   # consumed: the next batch is plain
    syn.close()
    syn = engine.Synthesizer(blob)                                                 # pool and multi run unpinned engines: against an unpinned one
    syn.set_output_rate(rate)
    single = []
    for a, p in zip(ids, plans):
        syn.set_pitch_plan([len(a)], [p])
        single.append(syn.infer_ids(a))
    pool = engine.Pool(blob, device=0, n_engines=2, max_batch=1)
    pool.set_output_rate(rate)
    t = [pool.submit(a, pitch=p) if p is not None else pool.submit(a) for a, p in zip(ids, plans)]
    got = [pool.wait(k) for k in t]
    assert all(np.array_equal(g, s) for g, s in zip(got, single))
    with pytest.raises(engine.StsError):
        pool.submit(ids[0], pitch=np.full(lens[0], 601, np.int32))
    pool.close()
    md = engine.MultiDevice(blob, [0, 0], gather="download")
    md.set_output_rate(rate)
    shard = md.shard_of(lens)
    md.set_pitch_plan(lens, plans)
    multi = md.infer_batch(ids)
    after = md.infer_batch(ids)                                                    # consumed
    md.set_pitch_plan(lens[:2], plans[:2])
    with pytest.raises(engine.StsError):
        md.infer_batch(ids)                                                        # set for another batch
    md.close()
    for sh in sorted(set(int(v) for v in shard)):
        mem = [b for b in range(3) if int(shard[b]) == sh]
        syn.set_pitch_plan([lens[b] for b in mem], [plans[b] for b in mem])
        ref = syn.infer_batch([ids[b] for b in mem])
        plain = syn.infer_batch([ids[b] for b in mem])
        for k, b in enumerate(mem):
            assert np.array_equal(multi[b], ref[k]) and np.array_equal(after[b], plain[k]), (sh, b)
    syn.close()


def test_refusals_drop_the_plan():
    cfg, blob = _tiny("hifigan_fix", 3)
    ids = sb.synthetic_ids(7, cfg.vocab)
    cents = [600, -600, 0, 1, -1, 300, -300]
    syn = engine.Synthesizer(blob)
    plain = syn.infer_ids(ids)
    calls = [lambda: syn.infer_ids_stream(ids, 4), lambda: syn.infer_batch_stream([ids], 4), lambda: syn.infer_joined([ids]),
             lambda: syn.infer_joined_stream([ids], 4), lambda: syn.stream_open(4, 2, 4096), lambda: syn.stream_open(4, 2, 4096, 64),
             lambda: syn.para_open(4, 2, 4096)]
    for k, call in enumerate(calls):
        syn.set_pitch_plan([7], [cents])
        with pytest.raises(engine.StsError):
            call()
        assert np.array_equal(syn.infer_ids(ids), plain), k                        # nothing is open, and the plan is gone
    # a planned open stream lets the setter through and refuses the admission; a paragraph and an unplanned stream refuse the setter
    syn.stream_open(4, 2, 4096, 64)
    syn.set_pitch_plan([7], [cents])
    with pytest.raises(engine.StsError):
        syn.stream_admit([ids])
    assert syn.stream_info()["live"] == 0
    syn.stream_close()
    assert np.array_equal(syn.infer_ids(ids), plain)
    syn.stream_open(4, 2, 4096)
    with pytest.raises(engine.StsError):
        syn.set_pitch_plan([7], [cents])
    syn.stream_close()
    syn.para_open(4, 2, 4096)
    with pytest.raises(engine.StsError):
        syn.set_pitch_plan([7], [cents])
    syn.para_close()
    # validity at the set call; an invalid plan leaves an earlier one in force; another batch; a failed run consumes the plan
    syn.set_pitch_plan([7], [cents])
    shifted = syn.infer_ids(ids)
    assert shifted.size != plain.size
    syn.set_pitch_plan([7], [cents])
    for bad in ([601] + [0] * 6, [0] * 6 + [-601]):
        with pytest.raises(engine.StsError):
            syn.set_pitch_plan([7], [bad])
    with pytest.raises(engine.StsError):
        syn.set_pitch_plan([0], [None])
    assert np.array_equal(syn.infer_ids(ids), shifted)
    for n_set, call in (([8], lambda: syn.infer_ids(ids)), ([7, 7], lambda: syn.infer_ids(ids)), ([7], lambda: syn.infer_batch([ids, ids]))):
        syn.set_pitch_plan(n_set, [[100] * n_set[0]] + [None] * (len(n_set) - 1))
        with pytest.raises(engine.StsError, match="another batch"):
            call()
        assert np.array_equal(syn.infer_ids(ids), plain)
    syn.set_pitch_plan([7], [cents])
    with pytest.raises(engine.StsError):
        syn.infer_ids([0, 1, 2, 3, 4, 5, cfg.vocab])
    assert np.array_equal(syn.infer_ids(ids), plain)
    syn.set_pitch_plan([7], [cents]); syn.set_pitch_plan(None)
    assert np.array_equal(syn.infer_ids(ids), plain)
    syn.close()


def test_a_poisoned_workspace_changes_nothing():
    """as tests/test_poison_gpu.py fills it: every arena and host output starts out as a NaN pattern; a batch with a planned, an unplanned
    and an all-0-cents member at 44.1 kHz under the limiter"""
    cfg, blob = _tiny("mbb_fix", 9)
    lens = (21, 6, 13)
    ids = [sb.synthetic_ids(k, cfg.vocab, salt=k) for k in lens]
    plans = [_cents(lens[0], 1), None, np.zeros(lens[2], np.int32)]

    def run(poison):
        syn = engine.Synthesizer(blob)
        if poison:
            syn.debug_set("poison", 0x7FC00000)
        syn.set_output_rate(44100)
        syn.set_limiter(engine.LIMITER_ON, 3.0, -2.0, 1.5)
        syn.set_record_taps(True)
        syn.set_pitch_plan(lens, plans)
        pcm = syn.infer_batch(ids)
        out = [p.tobytes() for p in pcm] + [syn.tap(k).tobytes() for k in ("wave", "wave_pitch", "wave_out", "wave_lim")]
        out.append(syn.phoneme_offsets(sum(lens)).tobytes())
        syn.set_record_taps(False)
        syn.set_pitch_plan(lens, plans)
        out += [p.tobytes() for p in syn.infer_batch(ids)]
        syn.close()
        return out
    assert run(True) == run(False)


def test_the_split_bf16_repeat_applies_the_plan_once():
    """as tests/test_gain_plan_gpu.py provokes the repeat: conv_pre of a synthetic blob scaled up until the trunk leaves fp16's range"""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 5)
    ids = sb.synthetic_ids(20, cfg.vocab)
    w = sb._W(5, cfg.stats)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._gen_hdr(w, cfg)
    assert tuple(blob[w.n:w.n + 3].astype(int)) == (cfg.up_init, cfg.inter, 7)
    start = w.n + 6
    big = blob.copy()
    big[start:start + cfg.up_init * 7 * cfg.inter] *= np.float32(3.0e6)
    cents = _cents(len(ids), 3)
    syn = engine.Synthesizer(big)
    syn.set_conv_math("bf16x3")
    plain = syn.infer_ids(ids)
    syn.set_pitch_plan([len(ids)], [cents])
    want = syn.infer_ids(ids)
    assert want.size != plain.size
    before = syn.profile()["conv_math_fallbacks"]
    syn.set_conv_math("f16x2")
    syn.set_pitch_plan([len(ids)], [cents])
    got = syn.infer_ids(ids)
    assert syn.profile()["conv_math_fallbacks"] == before + 1
    assert np.array_equal(got, want)
    syn.close()
