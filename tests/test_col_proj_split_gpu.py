"""GPU suite (MI355X): the launch forms of col_proj_kernel (col_layer.hip) through the engine.  The text encoder's q/k/v projection and
the producer of its input run as one launch; `col_proj` 2 keeps all three passes in one workgroup per 16 phonemes, 3 gives every (column
block, pass) pair a workgroup of its own, 1 chooses (split below 24 column blocks), 0 is the separate producer plus conv.  Per pass the
arithmetic is the same, so 1, 2 and 3 must return the same bits of every tap, the durations and the PCM; 0 sums in another order and
stays within the tap tolerance.  Which form ran is read from the text encoder's traffic account: a split launch books the input
stage's reads once per workgroup.

`sdp_pre_ride` 1 takes the stochastic duration predictor's `pre` conv (single speaker, hidden -> hidden) into the launch of the
encoder's output projection, 0 leaves it a conv launch of its own.

Lengths sit on and around the 16-phoneme column block and on both sides of the 24-block threshold (368 phonemes = 23 blocks, 369 = 24)."""
import dataclasses
import functools

import numpy as np
import pytest

import noise_ref as nr
import spline_ref as sr
from conftest import TAP_MAXABS_TOL
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

LENGTHS = [1, 15, 16, 17, 33, 368, 369]
BATCH = (5, 16, 21)
CASES = [(T,) for T in LENGTHS] + [BATCH]
POISON = (0x7FC00000, 0x7BFF7BFF)             # tests/test_spline_gpu.py: a quiet NaN per float; fp16 maxima
BLOB_SEED = 47


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case_id(case):
    return "T" + "_".join(str(t) for t in case)


@functools.lru_cache(maxsize=None)
def _model(kind="hifigan_sdp", sdp_filter=None):
    cfg = sb.tiny_cfg(kind)
    if sdp_filter:
        cfg = dataclasses.replace(cfg, sdp_filter=sdp_filter)
    return cfg, sb.make_blob(cfg, BLOB_SEED)


def _ids(cfg, T):
    return sb.synthetic_ids(T, cfg.vocab, salt=T)


@functools.lru_cache(maxsize=None)
def _oracle_x_enc(T):
    """x_enc of the plain-C oracle (one frame per phoneme: the encoder does not see the durations), computed once and left unchanged."""
    cfg, blob = _model()
    x = pyref.PortModel(blob).infer_ids(_ids(cfg, T), 0, 1.0, forced_dur=[1] * T, taps=True)["x_enc"]
    x.setflags(write=False)
    return x


def _engine(blob, poison=0, **keys):
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_record_taps(True)
    if poison:
        syn.debug_set("poison", poison - (1 << 32) if poison >= (1 << 31) else poison)
    for k, v in keys.items():
        syn.debug_set(k, v)
    return syn


def _run(syn, cfg, case, sids=None):
    syn.run_batch([_ids(cfg, T) for T in case], sids)
    p = syn.profile()
    assert p["conv_math_fallbacks"] == 0, (case, "the call was repeated in the split-bf16 form")
    return {"x_enc": syn.tap("x_enc"), "m": syn.tap("m"), "logw": syn.tap("logw")[0], "dur": syn.durations(sum(case)),
            "pcm": syn.pcm_host().copy(), "bytes_te": p["bytes_text_encoder"], "bytes_dp": p["bytes_duration"], "poison_bytes": p["poison_bytes"]}


def _same_bits(a, b, what):
    for k in ("x_enc", "m", "logw"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    assert np.array_equal(a["dur"], b["dur"]), (what, "durations")
    assert np.array_equal(a["pcm"], b["pcm"]), (what, "PCM")


@functools.lru_cache(maxsize=None)
def _forms(case):
    """The case under col_proj 0, 1, 2 and 3 on one engine -> {key: results}; computed once, read by every test."""
    cfg, blob = _model()
    syn = _engine(blob)
    out = {}
    for key in (1, 2, 3, 0):
        syn.debug_set("col_proj", key)
        out[key] = _run(syn, cfg, case)
    syn.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_forms_agree_bit_for_bit(case):
    r = _forms(case)
    what = _case_id(case)
    _same_bits(r[2], r[3], what + ": in-workgroup vs pass-split")
    _same_bits(r[1], r[3], what + ": automatic vs pass-split")
    for k in ("x_enc", "m"):
        err = float(np.abs(r[0][k] - r[3][k]).max())
        print(f"COLPROJ {what} {k}: max |separate - split| = {err:.3e} of {TAP_MAXABS_TOL:.1e}")
        assert err <= TAP_MAXABS_TOL, (what, k, err)
    # which form ran: a split launch books the input stage's reads per pass; the automatic choice splits below 24 column blocks
    blocks = (sum(case) + 15) // 16
    assert r[3]["bytes_te"] > r[2]["bytes_te"], (what, "col_proj = 3 did not take the pass-split form")
    assert r[1]["bytes_te"] == (r[3] if blocks < 24 else r[2])["bytes_te"], (what, blocks, "automatic choice")


def test_separate_launches_differ_in_bits_somewhere():
    """col_proj = 0 takes its q/k/v from the split-K conv, the other values from the column kernel's 16x16x4 chain: were the bits
    equal on every case, the switch would have selected nothing."""
    assert any(not np.array_equal(_bits(_forms(c)[0]["x_enc"]), _bits(_forms(c)[3]["x_enc"])) for c in CASES)


@pytest.mark.parametrize("T", LENGTHS)
def test_both_forms_match_the_oracle(T):
    want = _oracle_x_enc(T)
    r = _forms((T,))
    for key, name in ((3, "pass-split"), (2, "in-workgroup")):
        err = float(np.abs(r[key]["x_enc"] - want).max())
        print(f"COLPROJ oracle T={T} {name}: max |x_enc - oracle| = {err:.3e} of {TAP_MAXABS_TOL:.1e}")
        assert err <= TAP_MAXABS_TOL, (T, name, err)


@pytest.mark.parametrize("pattern", POISON, ids=hex)
def test_split_form_does_not_read_stale_memory(pattern):
    """Every pass workgroup forms x from global memory itself and only z = 0 writes it: with the workspace filled with a pattern before
    the call, the ragged batch returns the bits of an engine that was never poisoned."""
    cfg, blob = _model()
    clean = _forms(BATCH)[3]
    assert clean["poison_bytes"] == 0
    syn = _engine(blob, pattern, col_proj=3)
    got = _run(syn, cfg, BATCH)
    syn.close()
    assert got["poison_bytes"] > 0
    _same_bits(got, clean, hex(pattern))


def test_a_batch_member_equals_the_utterance_alone():
    cfg, blob = _model()
    batch = _forms(BATCH)[3]["x_enc"]
    syn = _engine(blob, col_proj=3)
    off = 0
    for T in BATCH:
        alone = _run(syn, cfg, (T,))["x_enc"]
        assert np.array_equal(_bits(alone), _bits(batch[:, off:off + T])), (T, "x_enc of a batch member != the utterance alone")
        off += T
    syn.close()


def test_full_width_once():
    """The upstream-sized model, 64 phonemes: 4 column blocks of col_proj_kernel<12> in both forms, and the automatic choice (split q/k/v,
    the duration predictor's `pre` conv inside the encoder's last launch) against the separate launches (col_proj 0, sdp_pre_ride 0)."""
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, BLOB_SEED)
    sec = nr.SdpSection(blob, cfg, BLOB_SEED)
    T = 64
    syn = _engine(blob)
    r = {}
    for key in (1, 2, 3, 0):
        syn.debug_set("col_proj", key)
        syn.debug_set("sdp_pre_ride", 1 if key else 0)
        r[key] = _run(syn, cfg, (T,))
    syn.close()
    _same_bits(r[2], r[3], "full width: in-workgroup vs pass-split")
    _same_bits(r[1], r[3], "full width: automatic vs pass-split")
    assert r[3]["bytes_te"] > r[2]["bytes_te"]
    for k in ("x_enc", "m"):
        err = float(np.abs(r[1][k] - r[0][k]).max())
        print(f"COLPROJ full width {k}: max |automatic - separate| = {err:.3e} of {TAP_MAXABS_TOL:.1e}")
        assert err <= TAP_MAXABS_TOL, (k, err)
    err = float(np.abs(r[1]["logw"] - r[0]["logw"]).max())
    print(f"COLPROJ full width logw: max |automatic - separate| = {err:.3e} of {sr.LOGW_BAR:.3e}")
    assert err <= sr.LOGW_BAR, err
    # tests/test_spline_gpu.py's rule: durations are compared where the float64 duration is clear of an integer
    zero = np.zeros(T)
    w = np.exp(nr.sdp_logw(sec, r[0]["x_enc"], zero, zero, 0))
    clear = np.abs(w - np.round(w)) > 1e-4
    assert clear.sum() >= T - 1, int(clear.sum())
    assert np.array_equal(r[1]["dur"][clear], r[0]["dur"][clear])
    assert np.array_equal(r[0]["dur"][clear], nr.durations(np.log(w))[clear])


# ---- the duration predictor's `pre` conv inside the encoder's last launch ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ride(kind, case, sid):
    """(kind with a hidden -> hidden `pre` conv) under sdp_pre_ride 1 and 0, col_proj 1 / 2 / 3 with the ride on -> results."""
    cfg, blob = _model(kind, 64)
    syn = _engine(blob)
    sids = [sid] * len(case)
    out = {}
    for name, ride, key in (("ride", 1, 1), ("ride2", 1, 2), ("ride3", 1, 3), ("separate", 0, 1)):
        syn.debug_set("sdp_pre_ride", ride)
        syn.debug_set("col_proj", key)
        out[name] = _run(syn, cfg, case, sids)
    syn.close()
    return out


@pytest.mark.parametrize("case", [(1,), (17,), (33,), (369,), BATCH], ids=_case_id)
def test_sdp_pre_inside_the_encoders_last_launch(case):
    cfg, blob = _model("hifigan_sdp", 64)
    sec = nr.SdpSection(blob, cfg, BLOB_SEED)
    r = _ride("hifigan_sdp", case, 0)
    what = _case_id(case)
    _same_bits(r["ride2"], r["ride3"], what)
    _same_bits(r["ride"], r["ride3"], what)
    a, b = r["ride"], r["separate"]
    assert a["bytes_te"] > b["bytes_te"], (what, "the ride-along did not engage")
    assert a["bytes_dp"] == b["bytes_dp"], (what, "the conv's traffic left the duration stage's account")
    for k in ("x_enc", "m"):       # (the encoder's own outputs: the extra workgroup changes nothing in them)
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    err = float(np.abs(a["logw"] - b["logw"]).max())
    print(f"COLPROJ ride {what}: max |logw inside - logw separate| = {err:.3e} of {sr.LOGW_BAR:.3e}")
    assert err <= sr.LOGW_BAR, (what, err)
    off = 0
    for T in case:
        s = slice(off, off + T)
        zero = np.zeros(T)
        want = nr.sdp_logw(sec, b["x_enc"][:, s], zero, zero, 0)
        for name in ("ride", "separate"):
            e = float(np.abs(r[name]["logw"][s] - want).max())
            assert e <= sr.LOGW_BAR, (what, name, e)
        w = np.exp(want)
        clear = np.abs(w - np.round(w)) > 1e-4
        assert np.array_equal(a["dur"][s][clear], b["dur"][s][clear]) and np.array_equal(a["dur"][s][clear], nr.durations(want)[clear]), what
        off += T


def test_sdp_pre_ride_is_refused_for_a_multi_speaker_model():
    """A multi-speaker `pre` conv adds a per-utterance bias (the speaker's conditioning): it stays a launch of its own, and the switch
    changes neither the results nor the traffic account."""
    for case, sid in ((BATCH, 2), ((33,), 1)):
        r = _ride("ms_hifigan_sdp", case, sid)
        _same_bits(r["ride"], r["separate"], "multi-speaker")
        assert r["ride"]["bytes_te"] == r["separate"]["bytes_te"] and r["ride"]["bytes_dp"] == r["separate"]["bytes_dp"]
