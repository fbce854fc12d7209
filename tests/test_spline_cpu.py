"""CPU suite: the references of the duration predictor's spline (tests/spline_ref.py) on their own account, the audit of the inputs that
tests/test_spline_gpu.py feeds the kernels, and the measured float32 cost that sets its bars.  No GPU."""
import os
import re

import numpy as np
import pytest

import noise_ref as nr
import spline_ref as sr
from conftest import ROOT
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

GROUPS = ("sweep", "bound", "knots", "zero", "past", "mono")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for sigma, filt in sr.KERNEL_CASES:
        c = sr.kernel_inputs(sigma, filt)
        c["f64"] = sr.rq_inverse(c["x"], c["h"], c["fs"])
        c["f32"] = sr.rq_inverse_f32(c["x"], c["h"], c["fs"])
        out[sigma, filt] = c
    return out


def test_entry_is_declared_exported_and_bound():
    """sts_debug_spline_step in the header, the library, the binding and INTEGRATION.md's list; the binding checks its arguments."""
    lib = engine.load_library() if os.path.exists(engine.LIB_PATH) else (engine.build_library(), engine.load_library())[1]
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    assert re.search(r"\bint sts_debug_spline_step\(int device, const float\* h, int64_t n, float filter_sqrt, const float\* r0, "
                     r"const float\* r1, float\* o0, float\* o1\);", hdr)
    assert hasattr(lib, "sts_debug_spline_step") and "sts_debug_spline_step" in engine.EXPORTED_SYMBOLS
    assert len(lib.sts_debug_spline_step.argtypes) == 8
    assert "#define STS_ABI_VERSION %d\n" % lib.sts_abi_version() in hdr
    assert "`sts_debug_spline_step`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    with pytest.raises(ValueError):
        engine.debug_spline_step(np.zeros((28, 4), np.float32), 1.0)
    with pytest.raises(ValueError):
        engine.debug_spline_step(np.zeros((29, 4), np.float32), 1.0, r0=np.zeros(3, np.float32))


def test_input_recipe(cases):
    for (sigma, filt), c in cases.items():
        x, n = c["x"], c["x"].size
        assert x.dtype == np.float32 and c["h"].dtype == np.float32 and c["h"].shape == (29, n) and c["h"].flags.c_contiguous
        assert [c[g].stop - c[g].start for g in GROUPS] == [4096, 6, 256 * 33, 256, 256, 64 * 64] and c["mono"].stop == n
        sw = x[c["sweep"]]
        assert -6 < sw.min() < -5.99 and 5.99 < sw.max() < 6 and np.allclose(np.diff(sw), 12 / 4096, atol=1e-6)
        five = np.float32(5)
        assert set(x[c["bound"]].tolist()) == {-5.0, 5.0, float(np.nextafter(five, np.float32(9))), float(np.nextafter(five, np.float32(0))),
                                               float(-np.nextafter(five, np.float32(9))), float(-np.nextafter(five, np.float32(0)))}
        kn = x[c["knots"]].reshape(256, 11, 3)
        assert np.array_equal(kn[:, :, 1], sr.knots_f32(c["h"][:, c["zero"]], c["fs"]).T)          # (the zero group holds columns 0..255 once)
        assert np.array_equal(kn[:, :, 0], np.nextafter(kn[:, :, 1], np.float32(-9))) and np.array_equal(kn[:, :, 2], np.nextafter(kn[:, :, 1], np.float32(9)))
        assert (kn[:, 0, 1] == -5).all() and (kn[:, 10, 1] == 5).all() and (np.diff(kn[:, :, 1], axis=1) > 0).all()
        assert not x[c["zero"]].any() and (x[c["past"]] == np.float32(5) + np.float32(1e-6)).all() and (x[c["past"]] > 5).all()
        mono = x[c["mono"]].reshape(64, 64)
        assert (np.diff(mono, axis=1) >= 0).all() and np.array_equal(c["col"][c["mono"]].reshape(64, 64), np.repeat(np.arange(64), 64).reshape(64, 64))
        rows = c["h"][:20] / np.sqrt(filt)
        assert abs(rows.std() / sigma - 1) < 0.02 and abs(c["h"][20:].std() / 2 - 1) < 0.02
        wid = np.diff(np.asarray(sr.tables(c["h"], c["fs"])[1], np.float64), axis=0)
        if sigma == 2.0:
            assert wid.min() < 0.0101 and wid.max() > 5          # (bins from the 1e-3 * 10 floor to more than 5 wide)


def test_checker_round_trip(cases):
    """Forward (the VITS formulas) and inverse (the quadratic's root) are written independently; each undoes the other to 1e-12 on every
    kernel input.  The value handed from one to the other stays in the extended precision both work in: the spline's slope reaches 5e5
    in a flat bin between steep ends (sigma = 2), so rounding the intermediate to float64 alone would cost up to 2e-10."""
    assert np.finfo(np.longdouble).eps < 1e-18, "the float64 references need x87 extended precision"
    for key, c in cases.items():
        x, h, fs = c["x"], c["h"], c["fs"]
        y, by, _ = sr.rq_inverse(x, h, fs, exact=True)
        back, bb = sr.rq_forward(y, h, fs, exact=True)
        e1 = float(np.abs(back - x).max())
        z, bz = sr.rq_forward(x, h, fs, exact=True)
        back2 = sr.rq_inverse(z, h, fs, exact=True)[0]
        e2 = float(np.abs(back2 - x).max())
        print(key, "forward(inverse(x)) - x", e1, "inverse(forward(x)) - x", e2)
        assert e1 <= 1e-12 and e2 <= 1e-12, (key, e1, e2)
        tails = ~((x > -5) & (x < 5))
        assert np.array_equal(np.asarray(y, np.float64)[tails], x[tails].astype(np.float64)) and np.array_equal(np.asarray(z, np.float64)[tails], x[tails].astype(np.float64))
        assert (np.diff(np.asarray(y[c["mono"]], np.float64).reshape(64, 64), axis=1) >= 0).all()          # the checker itself is monotone


def test_input_audit(cases):
    """From the references alone: every bin and both tails at least 64 times, the float64 discriminant positive everywhere, continuity at
    the knots, and where the float32 restatement of the reference is finite.

    Finite everywhere is what one would expect of it and is NOT the case: in each sigma = 2 case its discriminant comes out negative (NaN
    result) at one position, the float32 number just below a knot with a small derivative d1 in a steep bin.  There the exact
    discriminant is (h d1)^2 against a b^2 of (h (2 delta - d1))^2, below float32's rounding of b^2 once d1 / delta < ~5e-4; twelve
    consecutive seeds each gave 1-3 such positions, so this is the recipe, not the seed.  It is the reference's own hazard (a NaN logw for
    that phoneme); the HIP kernel takes the root of max(disc, 0).  So the audit pins down exactly that: the
    restatement is finite wherever its discriminant is >= 0, the others are 'just below an inner knot' inputs, at most 3 per case, and
    with the kernel's guard the restatement is finite everywhere and, at those positions, within E_max of the checker."""
    e_max = sr.fp32_cost()[0]
    for (sigma, filt), c in cases.items():
        x, h, fs = c["x"], c["h"], c["fs"]
        v, b, disc = c["f64"]
        v32, b32, d32 = c["f32"]
        cnt = np.bincount(b + 1, minlength=12)
        print((sigma, filt), "selected (lower tail, bins 0-9, upper tail)", cnt.tolist(), "min float64 discriminant", disc.min())
        assert cnt.size == 12 and cnt.min() >= 64
        assert np.bincount(b32 + 1, minlength=12).min() >= 64
        assert (disc > 0).all() and np.isfinite(v).all()
        neg = np.nonzero(d32 < 0)[0]
        assert np.array_equal(np.nonzero(~np.isfinite(v32))[0], neg)
        print((sigma, filt), "negative float32 discriminants at", [(int(i), float(x[i]), float(d32[i]), float(disc[i])) for i in neg])
        assert neg.size <= 3 and (neg.size == 0 or sigma == 2.0)
        for i in neg:          # the float32 number just below an inner knot
            j = i - c["knots"].start
            assert 0 <= j < 256 * 33 and j % 3 == 0 and 1 <= (j // 3) % 11 <= 9
        guarded = sr.rq_inverse_f32(x, h, fs, guarded=True)[0]
        assert np.isfinite(guarded).all() and np.array_equal(guarded[d32 >= 0], v32[d32 >= 0])
        assert (np.abs(guarded[neg] - v[neg]) <= e_max).all()
        # continuity: at each inner knot of the checker the value is the same from the bin below and the bin above.  (At the float32
        # knots, a few 1e-7 off, the neighbouring bin's formula would be an extrapolation past its own end, and next to a flat knot it
        # is off by 1e-4 or has no real root: the kernel's knot and the checker's need not agree on the bin because the checker's value
        # is continuous across its knot, not because either formula holds outside its bin.)
        cols = np.repeat(np.arange(256), 9)
        kk = np.tile(np.arange(1, 10), 256)
        hk = c["h"][:, c["zero"]][:, cols]
        xk = sr._pick(sr.tables(hk, fs)[1], kk)
        lo, hi = sr.rq_inverse(xk, hk, fs, bins=kk - 1, exact=True)[0], sr.rq_inverse(xk, hk, fs, bins=kk, exact=True)[0]
        assert float(np.abs(lo - hi).max()) <= 1e-12
        assert float(np.abs(hi - sr._pick(sr.tables(hk, fs)[0], kk)).max()) <= 1e-12          # and it is the knot of the widths


def test_measured_fp32_cost():
    e_max, e_rms, bad, each = sr.fp32_cost()
    print("per case", each)
    print("E_max", e_max, "E_rms", e_rms, "positions without a float32 root", bad)
    assert bad == sr.N_NEGATIVE and abs(e_max / sr.E_MAX - 1) < 0.01 and abs(e_rms / sr.E_RMS - 1) < 0.01
    assert set(each) == set(sr.E_RMS_CASE) and all(abs(each[k] / sr.E_RMS_CASE[k] - 1) < 0.01 for k in each), each
    assert e_max < 0.05 and e_rms < 1e-3          # (bars built on them would mean nothing otherwise)


@pytest.fixture(scope="module")
def engine_cases():
    out = {}
    for kind in sr.ENGINE_KINDS:
        for model in sr.ENGINE_MODELS:
            cfg = sr.engine_cfg(kind, model)
            blob = sb.make_blob(cfg, sr.ENGINE_BLOB_SEED)
            ids, sid, bids, bsid = sr.engine_ids(cfg)
            port = pyref.PortModel(blob)
            x = port.infer_ids(ids, sid, 1.0, forced_dur=[1] * len(ids), taps=True)["x_enc"]
            xb = [port.infer_ids(a, s, 1.0, forced_dur=[1] * len(a), taps=True)["x_enc"] for a, s in zip(bids, bsid)]
            out[kind, model] = (nr.SdpSection(blob, cfg, sr.ENGINE_BLOB_SEED), x, sid, xb, bsid)
    return out


def test_engine_latents_reach_every_bin_and_tail(engine_cases):
    """The wide latent (noise_scale_w = 3) of the T = 256 utterance, through the float64 checker on the oracle's encoder output: every
    spline step of every model selects every bin and both tails (twice at least, so that the engine's own encoder output, 1e-6 away,
    still selects each once), and the seed of record is the first that does."""
    for key, (sec, x, sid, _, _) in engine_cases.items():
        for seed in range(1, sr.ENGINE_SEEDS[key] + 1):
            r0, r1 = nr.sdp_latent(seed, sr.ENGINE_NSW, sr.ENGINE_T)
            tr = []
            logw = nr.sdp_logw(sec, x, r0, r1, sid, trace=tr)
            assert len(tr) == sec.n_flows - 1 == 3
            assert (sr.bins_hit(tr) >= 2) == (seed == sr.ENGINE_SEEDS[key]), (key, seed)
        d = nr.durations(logw)
        assert d.min() >= 1 and d.max() < 100000


def test_measured_fp32_cost_of_logw(engine_cases):
    """What float32 costs logw (the spline in rq_inverse_f32, everything else float64), per model; the largest is the figure of record
    that sets the engine bar.  The restatement has no value at a few phonemes of one model (a derivative logit of 120 there: e^h overflows in
    the reference's softplus, a hazard the kernel guards like the negative discriminant of test_input_audit), and the later flows' convs
    spread that NaN to the neighbours: those phonemes are counted, not measured."""
    worst, nans = {}, {}
    for key, (sec, x, sid, xb, bsid) in engine_cases.items():
        seed = sr.ENGINE_SEEDS[key]
        runs = [sr.logw_fp32_cost(sec, x, *nr.sdp_latent(seed, sr.ENGINE_NSW, sr.ENGINE_T), sid)]
        runs += [sr.logw_fp32_cost(sec, xb[i], *nr.sdp_latent(seed + i, sr.ENGINE_NSW, t), bsid[i]) for i, t in enumerate(sr.ENGINE_LENS)]
        worst[key], nans[key] = max(r[0] for r in runs), sum(r[1] for r in runs)
        print(key, "float32 cost of logw", worst[key], "phonemes without a float32 value", nans[key], "of", sr.ENGINE_T + sum(sr.ENGINE_LENS))
    top = max(worst.values())
    assert abs(top / sr.LOGW_COST - 1) < 0.05, worst
    assert sr.LOGW_BAR == 4 * sr.LOGW_COST < 1e-3
    assert {k: v for k, v in nans.items() if v} == sr.LOGW_NAN, nans          # (left out of the maximum: exactly these)
