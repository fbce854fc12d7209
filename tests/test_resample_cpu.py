"""Output sample-rate conversion, host side: the library's filter table (sts_resample_table) against the float64 checker of
tests/resample_ref.py, the rejections, the new C ABI, and the properties of the design itself."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as rr
from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000]
NEW = ("sts_set_output_rate", "sts_get_output_rate", "sts_resample_table", "sts_pool_set_output_rate", "sts_multi_set_output_rate")


def test_abi_version_and_header():
    lib = engine.load_library()
    assert lib.sts_abi_version() >= 9
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    for s in NEW:
        assert s + "(" in hdr, s
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)


@pytest.mark.parametrize("rate", RATES)
def test_library_table_matches_the_checker(rate):
    lib = engine.load_library()
    P, Q, taps = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.sts_resample_table(16000, rate, C.byref(P), C.byref(Q), C.byref(taps), None, 0) == 0
    p, q, k = rr.design(rate)[:3]
    assert (P.value, Q.value, taps.value) == (p, q, 2 * k)
    got = engine.resample_table(16000, rate)[2]
    want = rr.table(rate).astype(np.float32)
    assert got.shape == want.shape == (p, 2 * k)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp.astype(np.float64)).all(), rate


def test_listed_tap_counts():
    assert [2 * rr.design(r)[2] for r in (48000, 8000, 11025)] == [72, 144, 104]
    assert rr.design(44100)[:2] == (441, 160)


@pytest.mark.parametrize("rate", [7999, 48001, 47999, 0, -16000, -1])
def test_invalid_rates_are_rejected(rate):
    lib = engine.load_library()
    P = C.c_int32(-7)
    assert lib.sts_resample_table(16000, rate, C.byref(P), None, None, None, 0) == -1       # STS_EINVAL
    assert P.value == -7
    assert not rr.valid(rate)


def test_undersized_table_is_rejected():
    lib = engine.load_library()
    P, taps = C.c_int32(), C.c_int32()
    assert lib.sts_resample_table(16000, 44100, C.byref(P), None, C.byref(taps), None, 0) == 0
    n = P.value * taps.value
    buf = np.zeros(n, np.float32)
    assert lib.sts_resample_table(16000, 44100, None, None, None, buf.ctypes.data, n - 1) == -1
    assert not buf.any()
    assert lib.sts_resample_table(16000, 44100, None, None, None, buf.ctypes.data, n) == 0 and buf.any()


def test_setters_validate_without_a_gpu():
    lib = engine.load_library()
    assert lib.sts_set_output_rate(None, 48000) < 0
    assert lib.sts_get_output_rate(None) < 0
    assert lib.sts_pool_set_output_rate(None, 48000) < 0
    assert lib.sts_multi_set_output_rate(None, 48000) < 0


def test_length_and_phase_arithmetic():
    assert rr.out_len(171008, 48000) == 513024
    assert rr.out_len(171008, 8000) == 85504
    assert rr.out_len(1, 44100) == 3 and rr.out_len(1, 8000) == 1 and rr.out_len(3, 8000) == 2
    phi, n0 = rr.phase_base(np.arange(10), 44100)
    assert np.array_equal(phi, (np.arange(10) * 160) % 441) and np.array_equal(n0, (np.arange(10) * 160) // 441)


@pytest.mark.parametrize("rate", RATES)
def test_each_phase_sums_to_one(rate):
    assert np.abs(rr.table(rate).sum(axis=1) - 1.0).max() < 1e-12


@pytest.mark.parametrize("rate", RATES)
def test_passband_ripple_and_stopband_attenuation(rate):
    lo = min(16000, rate) / 2
    f, H = rr.prototype_spectrum(rate)
    band = f <= 0.8 * lo
    ripple_db = 20 * np.log10(H[band])
    assert np.abs(ripple_db).max() <= 0.001, np.abs(ripple_db).max()
    stop = f >= lo
    att_db = -20 * np.log10(H[stop].max())
    assert att_db >= 95.0, att_db
    # (the exact DTFT at a few edge frequencies agrees with the FFT grid)
    edges = np.array([0.0, 0.8 * lo, lo])
    Hx = rr.prototype_response(rate, edges)
    assert abs(Hx[0] - 1) < 1e-5 and abs(Hx[1] - 1) < 1e-4 and Hx[2] < 10 ** (-95 / 20)


def test_tone_round_trip_through_48k():
    n = 16000
    t = np.arange(n) / 16000.0
    x = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    up = rr.resample(x, 48000)
    assert up.size == 3 * n
    back = rr.resample(up, 16000, in_rate=48000)
    assert back.size == n
    mid = slice(400, n - 400)
    err = np.sqrt(np.mean((back[mid] - x[mid]) ** 2)) / np.sqrt(np.mean(x[mid] ** 2))
    assert 20 * np.log10(err) <= -60.0, 20 * np.log10(err)
    # the 48 kHz version is the same tone at the new rate
    t3 = np.arange(3 * n) / 48000.0
    ref = 0.5 * np.sin(2 * np.pi * 1000.0 * t3)
    assert np.abs(up[1200:-1200] - ref[1200:-1200]).max() < 1e-3


def test_pcm_cast_matches_the_reference_cast():
    y = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 70000.0, np.nan], np.float32)
    got = rr.pcm_cast(y)
    assert got[0] == 0 and got[1] == 16368 and got[2] == -16368 and got[3] == 32737 and got[4] == -32737
    assert got[5] == 49105 - 65536          # 1.5 * 32737 = 49105.5: truncated, then wrapped into int16
    assert got[6] == 0 and got[7] == 0
