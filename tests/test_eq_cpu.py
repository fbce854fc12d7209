"""CPU suite of the parametric equaliser (include/summertts_hip.h sts_set_eq): the new symbols and the ctypes mirror, the library's biquad
design against the cookbook formulas restated in eq_ref, the validity rules bound by bound, and the float64 restatement of the kernel's
scan order against the sequential definition (the evidence that the GPU tolerance is reachable)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import eq_ref
from conftest import ROOT
from summertts_amd import engine

NEW_SYMBOLS = ["sts_set_eq", "sts_get_eq", "sts_eq_check", "sts_eq_design", "sts_eq_apply", "sts_pool_set_eq", "sts_multi_set_eq"]
RATES = (8000, 16000, 22050, 48000)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_new_symbols_are_exported_declared_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    declared = set(re.findall(r"\b(sts_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert s in declared, s
    assert lib.sts_abi_version() == 18
    assert int(re.search(r"#define STS_ABI_VERSION (\d+)", hdr).group(1)) == 18
    for name, val in (("MAX_BANDS", 4), ("PEAK", 1), ("LOWSHELF", 2), ("HIGHSHELF", 3), ("HIGHPASS", 4), ("LOWPASS", 5)):
        assert int(re.search(r"#define STS_EQ_%s (\d+)" % name, hdr).group(1)) == val == getattr(engine, "EQ_" + name) == getattr(eq_ref, name)


def test_band_mirror_has_the_header_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    body = re.search(r"typedef struct sts_eq_band \{(.*?)\} sts_eq_band;", hdr, re.S).group(1)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    ctypes_of = {"float": C.c_float, "int32_t": C.c_int32}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(engine.EqBand._fields_)
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "summertts_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu", '
                    "sizeof(sts_eq_band), offsetof(sts_eq_band, type), offsetof(sts_eq_band, freq_hz), offsetof(sts_eq_band, gain_db), "
                    "offsetof(sts_eq_band, q)); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    m = engine.EqBand
    assert got == [C.sizeof(m), m.type.offset, m.freq_hz.offset, m.gain_db.offset, m.q.offset] == [16, 0, 4, 8, 12]


# ---- design
def _bands_for(rate):
    """every type, at frequencies and q inside the rules at this rate"""
    return [(eq_ref.PEAK, 1000.0, 6.0, 2.0), (eq_ref.PEAK, 0.4 * rate, -9.5, 0.3), (eq_ref.LOWSHELF, 200.0, -12.0, 0.7),
            (eq_ref.HIGHSHELF, 0.3 * rate, 12.0, 0.707), (eq_ref.HIGHPASS, 80.0, 0.0, 0.5), (eq_ref.LOWPASS, 3400.0, 3.0, 1.3),
            (eq_ref.PEAK, 20.0, 24.0, 2.5)]


@pytest.mark.parametrize("rate", RATES)
def test_design_matches_the_cookbook_formulas(lib, rate):
    for band in _bands_for(rate):
        assert eq_ref.check(rate, [band]), band
        got = engine.eq_design(rate, [band])
        want = eq_ref.design(rate, [band])
        assert got.shape == (1, 5)
        assert np.abs(got - want).max() <= 1e-12, (band, got, want)
        poles = np.roots([1.0, got[0, 3], got[0, 4]])
        assert np.abs(poles).max() < 1.0, (band, poles)
    four = _bands_for(rate)[:4]
    assert np.abs(engine.eq_design(rate, four) - eq_ref.design(rate, four)).max() <= 1e-12
    assert engine.eq_design(rate, []).shape == (0, 5)


@pytest.mark.parametrize("rate", RATES)
def test_design_has_the_magnitude_it_promises_at_f0(lib, rate):
    freqz = pytest.importorskip("scipy.signal").freqz

    def mag_db(c, f0):
        _, h = freqz([c[0], c[1], c[2]], [1.0, c[3], c[4]], worN=[2.0 * math.pi * f0 / rate])
        return 20.0 * math.log10(abs(h[0]))

    for g, q, f0 in ((6.0, 2.0, 1000.0), (-12.0, 8.0, 3000.0), (24.0, 0.1, 0.45 * rate), (-24.0, 1.0, 100.0)):
        f0 = float(np.float32(f0))
        c = engine.eq_design(rate, [(eq_ref.PEAK, f0, g, q)])[0]
        assert abs(mag_db(c, f0) - g) <= 1e-9, (g, q, f0)
    for t in (eq_ref.HIGHPASS, eq_ref.LOWPASS):
        for f0 in (300.0, 0.25 * rate):
            f0 = float(np.float32(f0))
            c = engine.eq_design(rate, [(t, f0, 0.0, float(np.float32(1.0 / math.sqrt(2.0))))])[0]
            assert abs(mag_db(c, f0) - (-3.0103)) <= 1e-6, (t, f0)


def test_the_worst_allowed_pole_stays_inside_the_unit_circle(lib):
    # q fs / f0 = 6400 exactly: 20 Hz, q 8 at 16 kHz -- the corner the numerical tolerance is stated for.  alpha = sin w0 / (2 q) is then
    # 4.9e-4; a pole's modulus is sqrt(a2), about 1 - alpha / A for a peak: at +24 dB (A = 4) 1.2e-4 inside the unit circle, the least
    for t in (1, 2, 3, 4, 5):
        for g in (-24.0, 24.0):
            c = engine.eq_design(16000, [(t, 20.0, g, 8.0)])[0]
            r = np.abs(np.roots([1.0, c[3], c[4]])).max()
            assert r < 1.0 - 1e-4, (t, g, r)


# ---- validity
def _ok(rate, bands):
    n, arr = engine._eq_bands(bands)
    return engine.load_library().sts_eq_check(int(rate), n, arr) == 0


def _next(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def test_check_accepts_each_bound_just_inside_and_refuses_it_just_outside(lib):
    fs = 16000
    good = (eq_ref.PEAK, 1000.0, 3.0, 1.0)
    assert _ok(fs, [good]) and _ok(fs, []) and _ok(fs, [good] * 4)
    assert not _ok(fs, [good] * 5)                                       # n_bands 5
    assert engine.load_library().sts_eq_check(fs, -1, None) != 0
    assert engine.load_library().sts_eq_check(fs, 1, None) != 0          # bands missing
    for t in (1, 2, 3, 4, 5):
        assert _ok(fs, [(t, 1000.0, 3.0, 1.0)])
    for t in (0, 6, -1):
        assert not _ok(fs, [(t, 1000.0, 3.0, 1.0)])
    # freq_hz in [20, 0.45 fs]
    assert _ok(fs, [(1, 20.0, 0.0, 0.1)]) and not _ok(fs, [(1, _next(20.0, False), 0.0, 0.1)])
    assert _ok(fs, [(1, 7200.0, 0.0, 1.0)]) and not _ok(fs, [(1, _next(7200.0, True), 0.0, 1.0)])
    assert _ok(48000, [(1, 21600.0, 0.0, 1.0)]) and not _ok(48000, [(1, _next(21600.0, True), 0.0, 1.0)])
    # q in [0.1, 8]  (float32(0.1) is just above 0.1)
    assert _ok(fs, [(1, 1000.0, 0.0, 0.1)]) and not _ok(fs, [(1, 1000.0, 0.0, _next(0.1, False))])
    assert _ok(fs, [(1, 1000.0, 0.0, 8.0)]) and not _ok(fs, [(1, 1000.0, 0.0, _next(8.0, True))])
    # gain_db in [-24, 24], also for the passes that ignore it
    for t in (1, 4):
        assert _ok(fs, [(t, 1000.0, 24.0, 1.0)]) and not _ok(fs, [(t, 1000.0, _next(24.0, True), 1.0)])
        assert _ok(fs, [(t, 1000.0, -24.0, 1.0)]) and not _ok(fs, [(t, 1000.0, _next(-24.0, False), 1.0)])
    # everything finite
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert not _ok(fs, [(1, bad, 0.0, 1.0)]) and not _ok(fs, [(1, 1000.0, bad, 1.0)]) and not _ok(fs, [(1, 1000.0, 0.0, bad)])
        assert not _ok(fs, [(4, 1000.0, bad, 1.0)])
    # q fs / f0 <= 6400
    assert _ok(16000, [(1, 20.0, 24.0, 8.0)])                            # exactly 6400
    assert not _ok(48000, [(1, 20.0, 0.0, 8.0)]) and _ok(48000, [(1, 60.0, 0.0, 8.0)]) and not _ok(48000, [(1, _next(60.0, False), 0.0, 8.0)])
    assert _ok(22050, [(4, 27.5625, 0.0, 8.0)]) and not _ok(22050, [(4, _next(27.5625, False), 0.0, 8.0)])
    assert _ok(48000, [(1, 20.0, 0.0, 2.6)]) and not _ok(48000, [(1, 20.0, 0.0, 2.7)])
    # the rate
    assert not _ok(7999, [good]) and not _ok(48001, [good]) and _ok(8000, [good]) and _ok(48000, [good])
    # a band that fits one rate and not another (what a run re-checks after sts_set_output_rate)
    assert _ok(16000, [(1, 3700.0, 0.0, 1.0)]) and not _ok(8000, [(1, 3700.0, 0.0, 1.0)])             # 0.45 x 8000 = 3600
    # one bad band among good ones
    assert not _ok(fs, [good, good, (1, 10.0, 0.0, 1.0), good])
    with pytest.raises(engine.StsError, match="q"):
        engine.eq_check(fs, [(1, 1000.0, 0.0, 9.0)])
    with pytest.raises(engine.StsError):
        engine.eq_design(fs, [(1, 1000.0, 0.0, 9.0)])


def test_checker_and_library_agree_on_validity(lib):
    rng = np.random.default_rng(5)
    for _ in range(300):
        rate = int(rng.choice(RATES))
        band = (int(rng.integers(0, 7)), float(np.float32(rng.choice([10.0, 20.0, 25.0, 300.0, 3500.0, 0.45 * rate, 0.46 * rate]))),
                float(np.float32(rng.choice([-25.0, -24.0, 0.0, 24.0, 24.5]))), float(np.float32(rng.choice([0.05, 0.1, 1.0, 8.0, 8.5]))))
        assert _ok(rate, [band]) == eq_ref.check(rate, [band]), (rate, band)


def test_apply_refuses_without_touching_a_device(lib):
    x = np.zeros(8, np.float32)
    lens = np.asarray([8], np.int64)
    n, arr = engine._eq_bands([(1, 1000.0, 0.0, 9.0)])
    assert lib.sts_eq_apply(0, x.ctypes.data, lens.ctypes.data, 1, 16000, n, arr, None, None) != 0      # invalid band
    assert lib.sts_eq_apply(0, x.ctypes.data, lens.ctypes.data, 1, 16000, 0, None, None, None) != 0      # nothing to apply
    n, arr = engine._eq_bands([(1, 1000.0, 0.0, 1.0)])
    assert lib.sts_eq_apply(0, x.ctypes.data, None, 1, 16000, n, arr, None, None) != 0
    assert lib.sts_eq_apply(0, x.ctypes.data, lens.ctypes.data, 0, 16000, n, arr, None, None) != 0
    assert lib.sts_set_eq(None, 0, None) != 0 and lib.sts_get_eq(None, None, None, 0) != 0
    assert lib.sts_pool_set_eq(None, 0, None) != 0 and lib.sts_multi_set_eq(None, 0, None) != 0


# ---- the scan order of the kernel against the sequential definition
SCAN_LENGTHS = (1, 2, 33, eq_ref.TILE - 1, eq_ref.TILE, eq_ref.TILE + 1, 3 * eq_ref.TILE + 5)


@pytest.mark.parametrize("which", range(len(eq_ref.FILTER_SETS)))
def test_scan_restatement_stays_within_2_to_the_minus_29_of_the_definition(which):
    """Measured (float64, noise at 0.3, 3 tiles + 5 samples): 3.7e-12 for the 4-band set at 48 kHz, 1.5e-11 (2^-35.9) for the
    q fs / f0 = 6400 corner at 16 kHz, 2.4e-15 for the telephone band at 8 kHz -- relative to the output's peak."""
    rate, bands = eq_ref.FILTER_SETS[which]
    assert eq_ref.check(rate, bands)
    c = eq_ref.design(rate, bands)
    rng = np.random.default_rng(100 + which)
    for N in SCAN_LENGTHS:
        x = (0.3 * rng.standard_normal(N)).astype(np.float32)
        ref = eq_ref.apply_df1(x, c)
        got = eq_ref.scan(x, c)
        dev = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"rate {rate} N {N}: scan deviation {dev:.3e}")
        assert dev <= 2.0 ** -29, (rate, N, dev)
        # and the vectorised form of the definition the GPU tests use is the definition
        assert np.abs(eq_ref.apply(x, c) - ref).max() <= 1e-11 * np.abs(ref).max()


def test_chunk_map_powers_are_block_lower_triangular_and_compose():
    rate, bands = eq_ref.FILTER_SETS[0]
    Mp = eq_ref.chunk_map_powers(eq_ref.design(rate, bands))
    assert Mp.shape == (9, 8, 8)
    for d in range(9):
        for i in range(8):
            assert not Mp[d][i, 2 * (i // 2) + 2:].any()
    for d in range(8):
        assert np.abs(Mp[d] @ Mp[d] - Mp[d + 1]).max() <= 1e-12 * max(1.0, np.abs(Mp[d + 1]).max())
