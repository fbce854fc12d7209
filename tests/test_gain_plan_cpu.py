"""Gain plans without a GPU: the new symbols in the library, the Python list and the header; the host-only design (sts_gain_design) against
the NumPy restatement of tests/gain_ref.py; every refusal of sts_gain_plan_check; and the properties of the restatement itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gain_ref as gr
from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sts_set_gain_plan", "sts_gain_plan_check", "sts_gain_design", "sts_gain_plan_apply", "sts_pool_submit_gain", "sts_multi_set_gain_plan"]
STS_EINVAL = -1
INF, NAN = float("inf"), float("nan")


def test_symbols_are_in_the_library_the_list_and_the_header():
    lib = engine.load_library()
    header = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\s*\(", header), s
    assert "typedef struct sts_gain_plan" in header
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18" in header
    assert C.sizeof(engine.Profile) == 200                      # sts_profile did not grow


# dB values whose 10^(dB / 20) 2^20 is not within 1e-6 of a half-integer (asserted below), the limits and the mute
DB_TABLE = [-INF, -96.0, -95.5, -60.0, -40.25, -20.0, -12.0, -6.0, -3.0, -0.5, 0.0, 0.5, 3.0, 6.0, 12.0, 23.75, 24.0]


def test_gain_design_against_the_reference():
    finite = np.asarray([g for g in DB_TABLE if np.isfinite(g)], np.float32).astype(np.float64)
    frac = np.mod(np.power(10.0, finite / 20.0) * gr.ONE, 1.0)
    assert (np.abs(frac - 0.5) > 1e-6).all()                     # libm and NumPy cannot land on different sides of the rounding
    for ramp in (0.0, 0.06, 0.0625, 1.0, 12.34, 50.0):
        q, h = engine.gain_design(DB_TABLE, len(DB_TABLE), ramp)
        wq, wh = gr.design(DB_TABLE, len(DB_TABLE), ramp)
        assert q.dtype == np.int32 and np.array_equal(q, wq) and h == wh, ramp
    q, h = engine.gain_design(DB_TABLE, len(DB_TABLE), 50.0)
    assert h == 400 and q[0] == 0 and q[DB_TABLE.index(0.0)] == gr.ONE and q[1] == 17 and q[-1] == 16618810
    assert engine.gain_design(DB_TABLE, len(DB_TABLE), 0.0)[1] == 0
    q, h = engine.gain_design(None, 5, 2.0)                      # gain_db == NULL: unit gain
    assert q.tolist() == [gr.ONE] * 5 and h == 16
    lib = engine.load_library()
    hh = C.c_int32(-1)
    g = np.zeros(3, np.float32)
    assert lib.sts_gain_design(g.ctypes.data, 3, 1.0, None, C.byref(hh)) == 0 and hh.value == 8     # each output is optional
    assert lib.sts_gain_design(g.ctypes.data, 3, 1.0, None, None) == 0
    assert lib.sts_gain_design(g.ctypes.data, 0, 1.0, None, None) == STS_EINVAL
    assert lib.sts_gain_design(g.ctypes.data, 3, 50.5, None, None) == STS_EINVAL


@pytest.mark.parametrize("bad", [{"gain_db": [0, NAN, 0]}, {"gain_db": [24.01, 0, 0]}, {"gain_db": [0, 0, -96.01]}, {"gain_db": [0, INF, 0]},
                                 {"gain_db": [0, 0, 0], "ramp_ms": -1.0}, {"gain_db": [0, 0, 0], "ramp_ms": 50.01}, {"ramp_ms": NAN},
                                 {"gain_db": [0, 0, 0], "ramp_ms": INF}], ids=str)
def test_check_refuses(bad):
    with pytest.raises(engine.StsError):
        engine.gain_plan_check([3], [bad])
    with pytest.raises(engine.StsError):
        engine.gain_plan_check([2, 3], [{"gain_db": [0, 0]}, bad])        # anywhere in the batch


def test_check_accepts_the_limits_and_refuses_a_null_n():
    engine.gain_plan_check([3, 1, 2], [{"gain_db": [-96, 24, -INF], "ramp_ms": 50.0}, None, {"gain_db": [0, -0.0], "ramp_ms": 0.0}])
    lib = engine.load_library()
    arr = (engine.GainPlan * 1)()
    n = np.asarray([3], np.int32)
    assert lib.sts_gain_plan_check(1, None, arr) == STS_EINVAL
    assert lib.sts_gain_plan_check(1, n.ctypes.data, None) == STS_EINVAL
    assert lib.sts_gain_plan_check(-1, n.ctypes.data, arr) == STS_EINVAL
    assert lib.sts_gain_plan_check(0, None, None) == 0
    zero = np.asarray([0], np.int32)
    assert lib.sts_gain_plan_check(1, zero.ctypes.data, arr) == STS_EINVAL


# ---- properties of the restatement itself -------------------------------------------------------------------------------------------------
def test_all_gains_zero_db_is_exactly_one():
    for h_ms in (0.0, 0.125, 50.0):
        q, h = gr.design([0.0] * 4, 4, h_ms)
        env = gr.envelope(q, h, [3, 0, 2, 1], 7)
        assert env.dtype == np.float32 and env.size == 6 * 7 and (env == np.float32(1.0)).all()
        x = np.random.default_rng(1).standard_normal(42).astype(np.float32)
        assert gr.apply(x, [3, 0, 2, 1], 7, [0.0] * 4, h_ms).tobytes() == x.tobytes()
        assert gr.apply(x, [3, 0, 2, 1], 7, None, h_ms).tobytes() == x.tobytes()


def test_zero_ramp_is_the_bare_step_function():
    db = [-6.0, 3.0, -INF, 12.0]
    dur = [2, 1, 3, 1]
    q, h = gr.design(db, 4, 0.0)
    assert h == 0
    env = gr.envelope(q, h, dur, 5)
    want = np.repeat((q.astype(np.float64) / gr.ONE).astype(np.float32), np.asarray(dur) * 5)
    assert np.array_equal(env, want) and (env[15:30] == 0).all()


def test_prefix_sums_equal_the_window_sums():
    rng = np.random.default_rng(2)
    for h in (0, 1, 7, 400):
        for n, hop in ((1, 3), (9, 1), (40, 6)):
            dur = rng.integers(0, 4, n)
            q = rng.integers(0, 1 << 24, n)
            Q = gr.step(q, dur, hop)
            S = gr.window_sums(Q, h)
            assert S.dtype == np.int64 and np.array_equal(S, gr.window_sums_brute(Q, h)), (h, n, hop)
            assert S.max() < 1 << 34


def test_a_zero_length_phoneme_owns_nothing():
    q = [gr.ONE, 0, 2 * gr.ONE, 0, 0]
    with_zeros = gr.step(q, [2, 0, 3, 0, 0], 4)
    assert np.array_equal(with_zeros, gr.step([gr.ONE, 2 * gr.ONE], [2, 3], 4))
    assert np.array_equal(gr.window_sums(with_zeros, 3), gr.window_sums(gr.step([gr.ONE, 2 * gr.ONE], [2, 3], 4), 3))
    # no fade at the edges: before the first sample the first gain, behind the last one the last gain
    env = gr.envelope(np.asarray([gr.ONE // 2, gr.ONE]), 5, [4, 4], 4)
    assert env[0] == np.float32(0.5) and env[-1] == np.float32(1.0)


def test_all_zero_durations_give_one_frame_at_unit_gain():
    q, h = gr.design([-INF, -20.0, 6.0], 3, 5.0)
    env = gr.envelope(q, h, [0, 0, 0], 6)
    assert env.size == 6 and (env == np.float32(1.0)).all()
    x = np.arange(6, dtype=np.float32)
    assert gr.apply(x, [0, 0, 0], 6, [-INF, -20.0, 6.0], 5.0).tobytes() == x.tobytes()


def test_the_cast_truncates_wraps_and_zeroes():
    y = np.asarray([0.0, 0.5, -0.5, 1.0, 1.0009, 1.001, -1.001, 3.0e5, -3.0e5, NAN, INF], np.float32)
    got = gr.pcm_cast(y)
    assert got.dtype == np.int16
    assert got[:4].tolist() == [0, 16368, -16368, 32737]
    assert got[4] == 32766 and got[5] < 0 and got[6] > 0          # past 1.0009 the cast wraps, as the reference's does
    assert got[7:].tolist() == [0, 0, 0, 0]                        # beyond int32, NaN: 0x80000000 -> 0
