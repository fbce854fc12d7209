"""The duration predictor's inverse rational-quadratic spline on the MI355X, in every form the engine reaches it, against the float64
checker of tests/spline_ref.py at inputs that take every branch: all ten bins, both tails, the knots and their float32 neighbours, +-5.

Kernel level (sts_debug_spline_step = spline_step_kernel on caller data).  Inputs: spline_ref.kernel_inputs, seed 20261018 -- four cases
(sigma in {0.5, 2} x filter in {24, 192}) of 4096 parameter columns, rows 0-19 ~ N(0, sigma^2) sqrt(filter), rows 20-28 ~ N(0, 4); 17158
(column, x) positions each: a sweep of (-6, 6), +-5 and their neighbours, the 11 float32 knots of 256 columns with both neighbours, 0, the
last knot + 1e-6, and 64 columns at 64 sorted x.  What float32 costs in this formula, measured on the CPU with a float32 restatement of
the reference's own operation order against the checker over all 68632 positions (tests/test_spline_cpu.py):

    E_max = 5.27e-3     E_rms = 2.14e-5     (over the 68630 positions where the restatement has a value: see below)

and the bars here are 4 E_max for the largest and 2 E_rms for the root-mean-square error of a case (the device's expf / logf / sqrtf /
division differ from libm by a few ulp, through the same conditioning); every position is compared.  E_max is large because the inverse
is ill-conditioned where a flat bin meets steep ends (slope up to 5e5 at sigma = 2).  The pooled E_rms is nearly all one position of
the third case (5.27e-3 / sqrt(68630) = 2.0e-5), so each case is also held to twice its own E_rms (spline_ref.E_RMS_CASE: 5.86e-6,
5.68e-6, 4.15e-5, 6.55e-6), which is the sharp bar against a systematic error in the three other cases.  Measured on the
MI355X: max 1.8e-4 / 2.5e-4 / 5.4e-3 / 2.3e-4 and rms 5.2e-6 / 5.6e-6 / 4.17e-5 / 5.4e-6 for the four cases -- the third case's rms is one
position (x = 3.3003, error 5.4e-3 on the device, 5.3e-3 in the restatement) and sits 2 % under the bar.

Engine level: tiny models (spline_ref.engine_cfg) with noise_scale = 0, noise_scale_w = 3, one utterance of T = 256 and one ragged batch
(37, 16, 1, 49, 130), per-model seeds chosen on the CPU so that every spline step selects every bin and both tails.  logw against
noise_ref.sdp_logw on the engine's own x_enc tap under min(4 x 1.42e-4, 1e-3) = 5.68e-4, where 1.42e-4 is the largest float32 cost of
logw over the models' utterances (the same restatement inside the float64 predictor).

The kernel carries two guards the reference lacks (devmath.hpp; the same bits wherever the reference's fp32 result is finite):

* softplus(h) = h where e^h overflows.  A derivative logit above 88.7 makes the reference's softplus inf and its quadratic inf - inf;
  the synthetic models reach logits of 120 (tiny, multi-speaker, sdp_filter 48) and 180 (full size), so without the guard
  test_engine_form_under_a_wide_latent[ms_hifigan_sdp-filter_48] and test_full_width_fused_tail_under_a_wide_latent see NaN logw.
* the root of max(disc, 0).  The float32 restatement has a negative discriminant (NaN) at the float32 number just below a knot with
  a small derivative in a steep bin, 1-3 positions per sigma = 2 case whatever the seed (tests/test_spline_cpu.py test_input_audit).
  On the device b * b - 4 a c is contracted into an FMA and these very positions come out >= 0, so no test here depends on this
  guard; only the restatement's ``guarded`` form covers it.
"""
import functools

import numpy as np
import pytest

import noise_ref as nr
import spline_ref as sr
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(sigma, filt):
    c = sr.kernel_inputs(sigma, filt)
    c["want"] = sr.rq_inverse(c["x"], c["h"], c["fs"])[0]
    hz = np.ascontiguousarray(c["h"][:, c["sweep"]])                  # (every column once)
    c["want0"] = sr.rq_inverse(np.zeros(sr.N_COLS, np.float32), hz, c["fs"])[0]
    c["hz"] = hz
    rng = np.random.default_rng(filt)
    keep = rng.standard_normal(c["x"].size).astype(np.float32)
    keep[:6] = np.array([-0.0, np.inf, -np.inf, 1e-45, 3.0e38, np.nan], np.float32)      # (carried over, never computed with)
    c["keep"] = keep
    return c


def _hold(label, got, want, x, case):
    e_max, e_rms, _, each = sr.fp32_cost()
    assert np.isfinite(got).all(), (label, np.nonzero(~np.isfinite(got))[0][:8], x[~np.isfinite(got)][:8])
    err = got.astype(np.float64) - want
    worst, rms = float(np.abs(err).max()), float(np.sqrt((err * err).mean()))
    print(label, "max |o0 - f64|", worst, "of", 4 * e_max, " rms", rms, "of", 2 * e_rms, " at x =", float(x[np.abs(err).argmax()]))
    assert worst <= 4 * e_max, (label, worst)
    assert rms <= 2 * e_rms, (label, rms)
    assert rms <= 2 * each[case], (label, rms, each[case])


@pytest.mark.parametrize("sigma,filt", sr.KERNEL_CASES)
def test_spline_step_kernel_against_the_float64_checker(sigma, filt):
    c = _case(sigma, filt)
    x, h, fs, keep = c["x"], c["h"], c["fs"], c["keep"]
    tails = ~((x > -5) & (x < 5))
    assert tails.sum() > 1000 and (~tails).sum() > 10000
    # both halves given
    o0, o1 = engine.debug_spline_step(h, fs, keep, x)
    assert np.array_equal(_bits(o1), _bits(keep)), "o1 is r0, bit for bit"
    assert np.array_equal(_bits(o0)[tails], _bits(x)[tails]), "the tails are the identity, bit for bit"
    _hold(f"sigma {sigma} filter {filt}, r0 and r1", o0, c["want"], x, (sigma, filt))
    mono = o0[c["mono"]].reshape(sr.N_MONO, sr.N_MONO)
    assert (np.diff(mono, axis=1) >= 0).all(), "not monotone in x"
    # r0 = NULL: zeros come back in its place, the spline half is the same computation
    p0, p1 = engine.debug_spline_step(h, fs, None, x)
    assert not _bits(p1).any() and np.array_equal(_bits(p0), _bits(o0))
    # r1 = NULL: x = 0 at every column
    q0, q1 = engine.debug_spline_step(c["hz"], fs, keep[:sr.N_COLS], None)
    assert np.array_equal(_bits(q1), _bits(keep[:sr.N_COLS]))
    _hold(f"sigma {sigma} filter {filt}, r1 = NULL", q0, c["want0"], np.zeros(sr.N_COLS, np.float32), (sigma, filt))
    assert np.array_equal(_bits(q0[:sr.N_KNOT_COLS]), _bits(o0[c["zero"]]))          # (the same columns at an explicit x = 0)
    z0, z1 = engine.debug_spline_step(c["hz"], fs, None, None)
    assert np.array_equal(_bits(z0), _bits(q0)) and not _bits(z1).any()


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_spline_step_writes_nothing_past_n(n):
    """Around the edge of the 128-thread workgroup: the caller's buffers, filled with a pattern, keep it behind entry n (and the entry
    itself fails if the kernel touched the device rows' guards, which reach past the launch's last workgroup); the first n results do
    not depend on n -- they are the bits the same columns give inside the 17158-position launch."""
    c = _case(2.0, 24)
    s = c["knots"]
    idx = np.arange(s.start + 5, s.start + 5 + n)
    h, x, keep = np.ascontiguousarray(c["h"][:, idx]), c["x"][idx], c["keep"][idx]
    full0, full1 = engine.debug_spline_step(c["h"], c["fs"], c["keep"], c["x"])
    for r0, r1 in ((keep, x), (None, x), (keep, None)):
        buf0, buf1 = np.full(n + 300, 0x7BFF7BFF, np.uint32).view(np.float32), np.full(n + 300, 0x7BFF7BFF, np.uint32).view(np.float32)
        o0, o1 = engine.debug_spline_step(h, c["fs"], r0, r1, o0=buf0, o1=buf1)
        assert (_bits(buf0)[n:] == 0x7BFF7BFF).all() and (_bits(buf1)[n:] == 0x7BFF7BFF).all()
        assert o0.size == o1.size == n and np.shares_memory(o0, buf0)
        if r1 is not None:
            assert np.array_equal(_bits(o0), _bits(full0[idx]))
        else:
            assert np.isfinite(o0).all() and (_bits(o0) != 0x7BFF7BFF).all()
        assert np.array_equal(_bits(o1), _bits(full1[idx]) if r0 is not None else np.zeros(n, np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# the engine's forms under a wide latent

FORMS = {          # name -> (model of spline_ref.engine_cfg, engine setup)
    "default": ("base", lambda syn: None),                              # col_layer_kernel<2, true>, the ConvFlow's pre conv folded in
    "dds_tail_0": ("base", lambda syn: syn.debug_set("dds_tail", 0)),   # fused layers, then the projection conv and spline_step_kernel
    "conv_mode_1": ("base", lambda syn: syn.set_conv_mode(1)),          # every conv on its own: pre conv, unfused layers, spline_step_kernel
    "filter_48": ("f48", lambda syn: None),                             # no column kernel at this width
    "filter_64": ("f64", lambda syn: None),                             # col_layer_kernel<4, true>
    "width_32": ("w32", lambda syn: None),                              # text encoder and predictor 32 wide
}
POISON = (0x7FC00000, 0x7BFF7BFF)


@functools.lru_cache(maxsize=None)
def _model(kind, model):
    cfg = sr.engine_cfg(kind, model)
    blob = sb.make_blob(cfg, sr.ENGINE_BLOB_SEED)
    return cfg, blob, nr.SdpSection(blob, cfg, sr.ENGINE_BLOB_SEED), sr.engine_ids(cfg), sr.ENGINE_SEEDS[kind, model]


def _engine(blob, setup, poison=0):
    syn = engine.Synthesizer(blob)
    setup(syn)
    if poison:
        syn.debug_set("poison", poison - (1 << 32) if poison >= (1 << 31) else poison)
    syn.set_record_taps(True)
    return syn


def _one(syn, ids, sid, seed):
    syn.set_noise(0.0, sr.ENGINE_NSW, seed)
    syn.infer_ids(ids, sid, 1.0)
    return syn.tap("x_enc"), syn.tap("logw")[0], syn.durations(len(ids))


def _batch(syn, ids, sids, seed):
    syn.set_noise(0.0, sr.ENGINE_NSW, seed)
    syn.run_batch(ids, sids)
    return syn.tap("x_enc"), syn.tap("logw")[0], syn.durations(sum(len(a) for a in ids))


def _against_checker(label, sec, x, logw, dur, sid, seed, audit=False):
    r0, r1 = nr.sdp_latent(seed, sr.ENGINE_NSW, x.shape[1])
    trace = []
    want = nr.sdp_logw(sec, x, r0, r1, sid, trace=trace)
    if audit:
        assert len(trace) == sec.n_flows - 1 and sr.bins_hit(trace) >= 1, (label, "a bin or tail is never selected")
    assert np.isfinite(logw).all(), (label, np.nonzero(~np.isfinite(logw))[0])
    err = float(np.abs(logw - want).max())
    print(label, "max |logw - f64|", err, "of", sr.LOGW_BAR)
    assert err <= sr.LOGW_BAR, (label, err)
    w = np.exp(want)
    clear = np.abs(w - np.round(w)) > 1e-4
    assert np.array_equal(dur[clear], nr.durations(want)[clear]), label
    assert dur.min() >= 1 and dur.max() < 100000, (label, dur.min(), dur.max())
    return int((~clear).sum())          # phonemes whose duration the rounding of logw may decide


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", sr.ENGINE_KINDS)
def test_engine_form_under_a_wide_latent(kind, form):
    model, setup = FORMS[form]
    cfg, blob, sec, (ids, sid, bids, bsid), seed = _model(kind, model)
    syn = _engine(blob, setup)
    x, logw, dur = _one(syn, ids, sid, seed)
    assert _against_checker(f"{kind} {form} T = {sr.ENGINE_T}", sec, x, logw, dur, sid, seed, audit=True) <= 0.02 * sr.ENGINE_T
    # the ragged batch: against the checker, and bit for bit what the same utterances give one at a time (utterance b draws seed + b)
    xb, logwb, durb = _batch(syn, bids, bsid, seed)
    off = np.concatenate([[0], np.cumsum(sr.ENGINE_LENS)])
    excused = 0
    for b, a in enumerate(bids):
        s = slice(off[b], off[b + 1])
        excused += _against_checker(f"{kind} {form} batch member {b}", sec, xb[:, s], logwb[s], durb[s], bsid[b], seed + b)
        x1, logw1, dur1 = _one(syn, a, bsid[b], seed + b)
        assert np.array_equal(_bits(logw1), _bits(logwb[s])) and np.array_equal(dur1, durb[s]), (kind, form, b, "batch != one at a time")
    assert excused <= 0.02 * off[-1]
    syn.close()
    # the same batch on engines whose workspaces start out as a pattern
    for pattern in POISON:
        syn = _engine(blob, setup, pattern)
        xp, logwp, durp = _batch(syn, bids, bsid, seed)
        assert syn.profile()["poison_bytes"] > 0
        assert np.array_equal(_bits(logwp), _bits(logwb)) and np.array_equal(durp, durb), (kind, form, hex(pattern))
        syn.close()


def _tail_pair(blob, ids, sid, seed):
    """(x_enc, logw, durations, bytes the duration stage accounts for) with the fused tail on and off."""
    out = []
    for v in (1, 0):
        syn = _engine(blob, lambda s: s.debug_set("dds_tail", v))
        syn.set_profiling(True)
        out.append(_one(syn, ids, sid, seed) + (syn.profile()["bytes_duration"],))
        syn.close()
    return out


@pytest.mark.parametrize("kind", sr.ENGINE_KINDS)
def test_fused_tail_and_three_launch_form_agree(kind):
    """dds_tail = 1 (the projection as an fp32 FMA chain inside the last layer's launch) and dds_tail = 0 (the projection conv, then
    spline_step_kernel) are each within the bar of the checker (test_engine_form_under_a_wide_latent), so within twice the bar of each
    other.  At the tiny models' 32 channels the projection conv is conv_generic_kernel, the same sequential FMA chain from zero with the
    bias added last, and the two forms come out bit-identical on the MI355X -- so equal bits cannot tell whether the switch selected
    anything here; the duration stage's traffic account can: the fused launch and the three launches book different byte counts."""
    cfg, blob, sec, (ids, sid, bids, bsid), seed = _model(kind, "base")
    (x1, w1, d1, b1), (x0, w0, d0, b0) = _tail_pair(blob, ids, sid, seed)
    assert np.array_equal(_bits(x1), _bits(x0))
    assert float(np.abs(w1 - w0).max()) <= 2 * sr.LOGW_BAR
    print(kind, "fused tail vs three launches: equal bits", np.array_equal(_bits(w1), _bits(w0)), "bytes", b1, b0)
    assert b1 != b0, "the fused tail did not engage"


def test_full_width_fused_tail_under_a_wide_latent():
    """The 12-wave tail of the upstream-sized model (sdp_filter 192: every production call), which no tiny model reaches, and its
    three-launch form, whose projection runs on the matrix cores: 64 phonemes under noise_scale_w = 3 against the checker on the
    engine's x_enc.  This model's derivative logits reach 180, past the overflow of the reference's softplus."""
    cfg = sr.engine_cfg("hifigan_sdp", "full")
    blob = sb.make_blob(cfg, sr.ENGINE_BLOB_SEED)
    sec = nr.SdpSection(blob, cfg, sr.ENGINE_BLOB_SEED)
    ids, seed = sb.synthetic_ids(64, cfg.vocab, salt=3), 5
    (x1, w1, d1, b1), (x0, w0, d0, b0) = _tail_pair(blob, ids, 0, seed)
    assert _against_checker("full model, fused tail", sec, x1, w1, d1, 0, seed) <= 1
    assert _against_checker("full model, three launches", sec, x0, w0, d0, 0, seed) <= 1
    print("full model, fused tail vs three launches: equal bits", np.array_equal(_bits(w1), _bits(w0)), "bytes", b1, b0)
    assert b1 != b0, "the fused tail did not engage"
