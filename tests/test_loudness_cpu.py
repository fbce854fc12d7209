"""CPU suite for loudness (include/summertts_hip.h sts_set_loudness): the float64 checker against the published BS.1770-4 numbers, and the
library's host-only K-weighting (sts_kweight_coeffs) against the checker."""
import os
import re

import numpy as np
import pytest

import loudness_ref as lr
from conftest import ROOT
from summertts_amd import engine


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_checker_reproduces_the_bs1770_coefficient_tables_at_48k():
    b1, a1, b2, a2 = lr.kweight(48000)
    assert np.abs(b1 - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() < 1e-12
    assert np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585]).max() < 1e-12
    assert np.abs(b2 - [1.0, -2.0, 1.0]).max() == 0.0
    assert np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621]).max() < 1e-12


def _sine(fs, amp, seconds=5.0, f=997.0):
    n = int(seconds * fs)
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / fs)).astype(np.float32)


def test_full_scale_997hz_sine():
    L, n = lr.measure(_sine(48000, 1.0), 48000)
    assert abs(L - (-3.010)) <= 0.005 and n == 47
    L01, _ = lr.measure(_sine(48000, 0.1), 48000)
    assert abs((L - L01) - 20.0) <= 1e-3
    for fs in (8000, 16000, 22050, 44100):
        Lf, _ = lr.measure(_sine(fs, 1.0), fs)
        assert abs(Lf - (-3.01)) <= 0.05, (fs, Lf)
    assert abs(lr.measure(_sine(16000, 1.0), 16000)[0] - (-2.970)) <= 0.005


def test_unmeasured_signals_and_the_gain_rule():
    fs = 16000
    S = lr.sub_block(fs)
    for x in (np.zeros(fs * 3, np.float32), _sine(fs, 0.5)[: 4 * S - 1], np.full(4 * S - 1, 0.25, np.float32), np.zeros(0, np.float32)):
        r = lr.loudness(x, fs, -16.0, -1.0)
        assert r["lufs"] == -np.inf and r["blocks"] == 0
        p = r["peak"]
        want = np.float32(min(1.0, 10 ** (-1 / 20) / p)) if p > 0 else np.float32(1.0)
        assert r["gain"] == want
    # DC: the high-pass removes it; from zero state only its onset (a step) passes the gates, and added to a sine it changes nothing
    r = lr.loudness(np.full(fs * 3, 0.5, np.float32), fs, -16.0, -1.0)
    assert 1 <= r["blocks"] <= 4 and r["lufs"] < -30.0
    s = _sine(fs, 0.5)
    assert abs(lr.measure(s + np.float32(0.25), fs)[0] - lr.measure(s, fs)[0]) < 0.01
    # the peak alone: an unmeasured signal with samples above the ceiling gets the ceiling's gain
    r = lr.loudness(np.full(4 * S - 1, 2.0, np.float32), fs, -16.0, -1.0)
    assert r["lufs"] == -np.inf and r["gain"] == np.float32(10 ** (-1 / 20) / 2.0)
    # a loud sine: the ceiling binds
    r = lr.loudness(_sine(fs, 1.5), fs, 0.0, -1.0)
    assert np.isfinite(r["lufs"]) and r["gain"] == np.float32(10 ** (-1 / 20) / r["peak"])


def test_relative_gate_drops_quiet_blocks():
    fs = 16000
    x = np.concatenate([_sine(fs, 0.5, 3.0), _sine(fs, 0.5e-3, 3.0)])      # -60 dB second half: above -70, below the relative gate
    L, n = lr.measure(x, fs)
    z = lr.block_energies(x, fs)
    L_loud, n_loud = lr.measure(_sine(fs, 0.5, 3.0), fs)
    assert n < z.size and (lr._lufs(z) > lr.ABS_GATE).all()                  # every block passes the absolute gate, not all the relative one
    assert abs(L - L_loud) < 0.5 and L > lr._lufs(z.mean()) + 2.0


def test_library_kweight_matches_the_checker(lib):
    for fs in (8000, 16000, 22050, 44100, 48000):
        got = engine.kweight_coeffs(fs).ravel()
        assert np.abs(got - lr.coeffs10(fs)).max() <= 1e-12, fs
    for bad in (7999, 48001, 0, -16000):
        with pytest.raises(engine.StsError):
            engine.kweight_coeffs(bad)


def test_abi_11_and_the_header_declares_the_loudness_entries(lib):
    assert lib.sts_abi_version() >= 11
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    for name in ("sts_set_loudness", "sts_get_loudness_mode", "sts_get_loudness", "sts_pool_set_loudness", "sts_multi_set_loudness",
                 "sts_kweight_coeffs", "sts_loudness_measure"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in engine.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name, v in (("STS_LOUD_OFF", 0), ("STS_LOUD_MEASURE", 1), ("STS_LOUD_NORMALIZE", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(v) + r"\b", hdr), name
    assert "typedef struct sts_loudness { float lufs; float peak; float gain; int32_t blocks; } sts_loudness;" in hdr
    assert engine.LOUDNESS_DTYPE.itemsize == 16
