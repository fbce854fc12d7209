"""CPU suite for the look-ahead peak limiter (include/summertts_hip.h sts_set_limiter): the ABI, the library's host-only design
(sts_limiter_design) against the checker, and the checker of tests/limiter_ref.py against the three consequences the definition
states: the ceiling always holds, an untouched neighbourhood passes through exactly, and y[n] depends on x[n - 2H .. n + 2H] only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import limiter_ref as lm
from conftest import ROOT
from summertts_amd import engine

STS_EINVAL = -1
HEADER = os.path.join(ROOT, "include", "summertts_hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_abi_version_and_symbols(lib):
    assert lib.sts_abi_version() >= 13
    for s in ("sts_set_limiter", "sts_get_limiter_mode", "sts_get_limiter", "sts_limiter_design", "sts_limiter_apply",
              "sts_pool_set_limiter", "sts_multi_set_limiter"):
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
    h = open(HEADER).read()
    assert re.search(r"typedef struct sts_limiter_stats \{ float gain; float min_gain; float peak_out; int32_t limited; \} sts_limiter_stats;", h)
    assert re.search(r"int sts_set_limiter\(sts_engine\* e, int mode, float gain_db, float ceiling_dbfs, float lookahead_ms\);", h)
    assert re.search(r"int sts_limiter_design\(int32_t rate, float gain_db, float ceiling_dbfs, float lookahead_ms, int32_t\* H, double\* c, double\* G\);", h)
    assert engine.LIMITER_DTYPE.itemsize == 16
    assert len(lib.sts_limiter_apply.argtypes) == 11 and len(lib.sts_set_limiter.argtypes) == 5


H_TABLE = [  # (rate, lookahead_ms, H): both ends of the range, and products that end in .5 (rounded up)
    (8000, 0.25, 2), (48000, 10.0, 480), (8000, 10.0, 80), (48000, 0.25, 12), (16000, 5.0, 80), (22050, 5.0, 110),
    (8000, 0.3125, 3), (8000, 0.4375, 4), (16000, 0.28125, 5), (44100, 1.0, 44), (22050, 1.0, 22), (11025, 1.0, 11),
    (11025, 2.0, 22), (48000, 0.28125, 14), (16000, 0.25, 4), (24000, 9.9999, 240), (32000, 2.515625, 81),
]


@pytest.mark.parametrize("rate,ms,H", H_TABLE)
def test_design_H(lib, rate, ms, H):
    assert engine.limiter_design(rate, 0.0, -1.0, ms)[0] == H
    assert lm.design_H(rate, ms) == H


def test_design_c_and_G_match_numpy(lib):
    for g, cdb in ((0.0, 0.0), (-40.0, -30.0), (40.0, -1.0), (12.0, -0.1), (-3.5, -6.0), (6.0206, -12.5)):
        H, c, G = engine.limiter_design(16000, g, cdb, 5.0)
        wc = np.power(10.0, np.float64(np.float32(cdb)) / 20.0)
        wG = np.power(10.0, np.float64(np.float32(g)) / 20.0)
        assert abs(c / wc - 1.0) <= 1e-15 and abs(G / wG - 1.0) <= 1e-15, (g, cdb, c, wc, G, wG)
    assert engine.limiter_design(16000, 0.0, 0.0, 5.0)[1:] == (1.0, 1.0)
    # each output is optional
    H = C.c_int32()
    assert lib.sts_limiter_design(16000, 0.0, -1.0, 5.0, C.byref(H), None, None) == 0 and H.value == 80
    assert lib.sts_limiter_design(16000, 0.0, -1.0, 5.0, None, None, None) == 0


def test_design_refuses_invalid_arguments(lib):
    nan, inf = float("nan"), float("inf")
    H, c, G = C.c_int32(-7), C.c_double(-7.0), C.c_double(-7.0)
    for rate, g, cdb, ms in ((7999, 0, -1, 5), (48001, 0, -1, 5), (0, 0, -1, 5), (-16000, 0, -1, 5),
                             (16000, 40.5, -1, 5), (16000, -40.5, -1, 5), (16000, nan, -1, 5), (16000, inf, -1, 5),
                             (16000, 0, 0.1, 5), (16000, 0, -30.5, 5), (16000, 0, nan, 5), (16000, 0, -inf, 5),
                             (16000, 0, -1, 0.2), (16000, 0, -1, 10.5), (16000, 0, -1, nan), (16000, 0, -1, inf), (16000, 0, -1, 0.0)):
        assert lib.sts_limiter_design(rate, g, cdb, ms, C.byref(H), C.byref(c), C.byref(G)) == STS_EINVAL, (rate, g, cdb, ms)
        assert (H.value, c.value, G.value) == (-7, -7.0, -7.0)
    # the stand-alone call checks its arguments before it touches a device
    assert lib.sts_limiter_apply(0, None, None, 0, 16000, 0.0, -1.0, 5.0, None, None, None) == STS_EINVAL
    lens = np.asarray([4], np.int64)
    x = np.zeros(4, np.float32)
    for rate, g, cdb, ms in ((7000, 0, -1, 5), (16000, 41, -1, 5), (16000, 0, 1, 5), (16000, 0, -1, 11), (16000, 0, -1, nan)):
        assert lib.sts_limiter_apply(0, x.ctypes.data, lens.ctypes.data, 1, rate, g, cdb, ms, None, None, None) == STS_EINVAL
    bad = np.asarray([-1], np.int64)
    assert lib.sts_limiter_apply(0, x.ctypes.data, bad.ctypes.data, 1, 16000, 0.0, -1.0, 5.0, None, None, None) == STS_EINVAL


# ---- the checker itself -------------------------------------------------------------------------------------------------------------
def _planted(rng, n, H, kind):
    x = (0.05 * rng.standard_normal(n)).astype(np.float32)
    if kind == "first":
        x[0] = 3.0
    elif kind == "last":
        x[-1] = -2.5
    elif kind == "isolated":
        x[n // 2] = 1.7
    elif kind == "run":
        x[n // 3:n // 3 + 4 * H + 5] = np.float32(2.3) * np.sign(rng.standard_normal(4 * H + 5)).astype(np.float32)
    elif kind == "nonfinite":
        x[n // 4] = np.nan; x[n // 2] = np.inf; x[3 * n // 4] = -np.inf
    return x


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 48000])
@pytest.mark.parametrize("ms", [0.25, 10.0])
def test_checker_properties(rate, ms):
    H = lm.design_H(rate, ms)
    rng = np.random.default_rng(rate + int(ms * 100))
    for cdb, gdb in ((-1.0, 0.0), (-6.0, 12.0), (0.0, -3.0)):
        c = 10.0 ** (cdb / 20.0)
        g0 = lm.static_gain(10.0 ** (gdb / 20.0))
        for kind in ("first", "last", "isolated", "run", "nonfinite"):
            n = 12 * H + 301
            x = _planted(rng, n, H, kind)
            y, s, S = lm.limit(x, g0, H, c)
            v = (x * g0).astype(np.float32)
            fin = np.isfinite(v)
            a = np.abs(v[fin]).astype(np.float64)
            # the ceiling: s <= c / a (float32 rounding of s may exceed the float64 bound by half an ulp), and the PCM bound exactly
            assert (s[fin].astype(np.float64) * a <= c * (1 + 2.0 ** -23)).all(), (kind, cdb)
            pcm = lm.pcm_cast(y[fin])
            assert np.abs(pcm.astype(np.int64)).max() <= lm.ceiling_pcm(c), (kind, cdb)
            assert (np.sign(pcm[pcm != 0]) == np.sign(v[fin][pcm != 0])).all()         # never wraps
            assert (s[~fin] == 0).all()
            # untouched where no sample within 2H exceeds the ceiling
            over = ~(np.abs(v).astype(np.float64) <= c)
            near = np.convolve(over.astype(np.int64), np.ones(4 * H + 1, np.int64), mode="same") > 0
            assert (s[~near] == np.float32(1.0)).all() and np.array_equal(y[~near], v[~near]), (kind, cdb)
            assert (S[~near] == (2 * H + 1) * lm.ONE).all()
            assert (S[over] < (2 * H + 1) * lm.ONE).all()
            st = lm.stats(y[fin], s[fin], S[fin], g0, H)
            assert st["limited"] > 0 and st["min_gain"] < 1.0
        # a quiet signal passes through bit for bit
        x = (0.01 * rng.standard_normal(5 * H + 17)).astype(np.float32)
        y, s, S = lm.limit(x, g0, H, c)
        assert np.array_equal(y, (x * g0).astype(np.float32)) and (s == 1.0).all()
        st = lm.stats(y, s, S, g0, H)
        assert st["limited"] == 0 and st["min_gain"] == np.float32(1.0)


@pytest.mark.parametrize("rate,ms", [(8000, 0.25), (16000, 5.0), (22050, 3.3), (48000, 10.0)])
def test_checker_slice_equals_whole(rate, ms):
    H = lm.design_H(rate, ms)
    rng = np.random.default_rng(5)
    n = 20 * H + 1000
    x = (0.05 * rng.standard_normal(n)).astype(np.float32)
    x[rng.integers(0, n // 2, 12)] = np.float32(1.5)          # peaks in the first half only: the tail of the second half is untouched
    c = 10.0 ** (-3.0 / 20.0)
    g0 = lm.static_gain(10.0 ** (4.0 / 20.0))
    y, s, S = lm.limit(x, g0, H, c)
    assert (S < (2 * H + 1) * lm.ONE).any() and (s == 1.0).any()
    for a, b in ((0, 1), (0, 3 * H), (5 * H + 3, 5 * H + 4), (7 * H, 13 * H + 11), (n - 2 * H - 1, n), (n - 1, n), (0, n)):
        lo, hi = max(0, a - 2 * H), min(n, b + 2 * H)
        # the slice carries its true distance to the utterance's edges: beyond them q is 2^30 anyway, inside the slice it must be real
        ys, _, _ = lm.limit(x[lo:hi], g0, H, c)
        assert np.array_equal(ys[a - lo:b - lo], y[a:b]), (a, b)


def test_checker_empty_and_tiny_signals():
    H, c = 4, 0.5
    y, s, S = lm.limit(np.zeros(0, np.float32), np.float32(1.0), H, c)
    assert y.size == 0 and lm.stats(y, s, S, np.float32(1.0), H) == {"gain": np.float32(1.0), "min_gain": np.float32(1.0),
                                                                     "peak_out": np.float32(0.0), "limited": 0}
    y, s, S = lm.limit(np.asarray([2.0], np.float32), np.float32(1.0), H, c)
    # one loud sample: every minimum window within H of it holds it, so S = (2H + 1) q and s = float32(q / 2^30)
    assert S[0] == (2 * H + 1) * (lm.ONE // 4) and s[0] == np.float32(0.25) and y[0] == np.float32(0.5)
