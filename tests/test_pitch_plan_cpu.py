"""Pitch plans without a GPU: the new symbols in the library, the Python list and the header; the host-only design, layout and prototype
(sts_pitch_design, sts_pitch_layout, sts_pitch_table) against the NumPy restatement of tests/pitch_ref.py; every refusal of
sts_pitch_plan_check; the layout arithmetic as a stand-alone program under UBSan; and the properties of the restatement itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pitch_ref as pr
from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
NEW = ["sts_pitch_plan_check", "sts_pitch_design", "sts_pitch_layout", "sts_pitch_table", "sts_pitch_apply"]
STS_EINVAL = -1


def test_symbols_are_in_the_library_the_list_and_the_header():
    lib = engine.load_library()
    header = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\s*\(", header), s
    assert "typedef struct sts_pitch_plan" in header
    assert "THE FORMANTS MOVE WITH THE PITCH" in header and "NOT COMPENSATED" in header
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18" in header
    assert C.sizeof(engine.Profile) == 200                      # sts_profile did not grow
    assert C.sizeof(engine.PitchPlan) == C.sizeof(C.c_void_p)


# ---- validity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [[601, 0, 0], [0, -601, 0], [0, 0, 2 ** 31 - 1], [-2 ** 31, 0, 0]], ids=str)
def test_check_refuses(bad):
    with pytest.raises(engine.StsError):
        engine.pitch_plan_check([3], [{"cents": bad}])
    with pytest.raises(engine.StsError):
        engine.pitch_plan_check([2, 3], [{"cents": [0, 0]}, bad])          # anywhere in the batch


def test_cents_are_integers():
    for bad in ([0.5, 0, 0], [float("nan"), 0, 0], [100.0, 0, 0]):
        with pytest.raises(ValueError):
            engine.pitch_plan_check([3], [bad])
    with pytest.raises(ValueError):
        engine.pitch_plan_check([3], [[0, 0]])                             # one entry per phoneme
    with pytest.raises(ValueError):
        engine.pitch_plan_check([3, 2], [[0, 0, 0]])                       # one plan (or None) per utterance


def test_check_accepts_the_limits_and_refuses_a_null_n():
    engine.pitch_plan_check([3, 1, 2], [{"cents": [-600, 600, 0]}, None, [1, -1]])
    lib = engine.load_library()
    arr = (engine.PitchPlan * 1)()
    n = np.asarray([3], np.int32)
    assert lib.sts_pitch_plan_check(1, None, arr) == STS_EINVAL
    assert lib.sts_pitch_plan_check(1, n.ctypes.data, None) == STS_EINVAL
    assert lib.sts_pitch_plan_check(-1, n.ctypes.data, arr) == STS_EINVAL
    assert lib.sts_pitch_plan_check(0, None, None) == 0
    assert lib.sts_pitch_plan_check(1, n.ctypes.data, arr) == 0                # cents == NULL: no plan for this utterance
    for bad_n in (0, -1):
        z = np.asarray([bad_n], np.int32)
        assert lib.sts_pitch_plan_check(1, z.ctypes.data, arr) == STS_EINVAL
        assert lib.sts_pitch_design(None, bad_n, None, None) == STS_EINVAL


# ---- design -----------------------------------------------------------------------------------------------------------------------------------
def test_pitch_design_against_the_reference():
    cents = np.arange(-600, 601)
    frac = np.mod(np.power(2.0, cents / 1200.0) * 4294967296.0, 1.0)
    assert (np.abs(frac - 0.5) > 1e-5).all()                     # libm and NumPy cannot land on different sides of the rounding
    ratio, step = engine.pitch_design(cents, cents.size)
    wr, ws = pr.design(cents)
    assert step.dtype == np.int64 and np.array_equal(step, ws)
    assert ratio.dtype == np.float32 and np.array_equal(ratio, wr)
    assert step[600] == 1 << 32 and ratio[600] == np.float32(1.0)
    assert step[0] == 3037000500 and step[-1] == 6074001000     # the limits pitch_layout.hpp names
    ratio, step = engine.pitch_design(None, 4)                    # cents == NULL
    assert step.tolist() == [1 << 32] * 4 and ratio.tolist() == [1.0] * 4
    lib = engine.load_library()
    c = np.asarray([0, 601], np.int32)
    assert lib.sts_pitch_design(c.ctypes.data, 2, None, None) == STS_EINVAL
    assert lib.sts_pitch_design(c.ctypes.data, 1, None, None) == 0            # each output is optional


# ---- layout -----------------------------------------------------------------------------------------------------------------------------------
def _layout_case(d, cents, hop):
    step = pr.design(cents)[1]
    o, e = engine.pitch_layout(d, step, hop)
    wo, we = pr.layout(d, step, hop)
    assert o.tolist() == wo and e.tolist() == we, (d, cents, hop)
    return wo, we


def test_layout_steps_over_one_frame_phonemes_at_hop_1():
    o, e = _layout_case([1] * 40, [600] * 40, 1)
    n = np.diff(o)
    assert (n == 0).sum() >= 10 and o[-1] == 29                 # ceil(40 / sqrt 2): some phonemes emit nothing, and e carries across them
    assert all(0 <= v < 6074001000 for v in e)
    for i in np.flatnonzero(n == 0):
        assert e[i + 1] == e[i] - (1 << 32)
    _layout_case([1, 1, 0, 1, 1, 1], [600, -600, 0, 600, 600, 600], 1)


def test_layout_runs_of_empty_phonemes():
    for d in ([0, 0, 0, 4, 5], [4, 0, 0, 0, 5], [4, 5, 0, 0, 0], [0, 0, 3, 0, 0, 2, 0, 0]):
        for cents in (600, -600, 37):
            o, e = _layout_case(d, [cents] * len(d), 6)
            for i, di in enumerate(d):
                if di == 0:
                    assert o[i + 1] == o[i]
                    assert e[i + 1] == e[i]


def test_layout_all_zero_and_neighbours():
    o, e = _layout_case([0, 0, 0], [600, 0, -600], 256)
    assert o == [0] * 4 and e == [0] * 4
    assert pr.warped_length([0, 0, 0], pr.design([600, 0, -600])[1], 256) == 256     # the frame nobody owns: step 2^32
    o, e = _layout_case([5, 5, 5, 5], [-600, 600, -600, 600], 16)
    assert abs(o[-1] - (160 * 2 ** 0.5 + 160 / 2 ** 0.5)) < 2
    _layout_case([5, 0, 7, 3], [0, 0, 0, 0], 16)
    assert [pr.warped_length([5, 0, 7, 3], pr.design([c] * 4)[1], 16) for c in (-600, -100, 37, 600)] == [340, 255, 235, 170]


def test_layout_refusals():
    lib = engine.load_library()
    d, s = np.asarray([3, 4], np.int32), np.asarray([1 << 32, 1 << 32], np.int64)
    o = np.zeros(3, np.int64)

    def call(dd, ss, n, hop):
        return lib.sts_pitch_layout(dd.ctypes.data, ss.ctypes.data, n, hop, o.ctypes.data, None)
    assert call(d, s, 2, 16) == 0 and o.tolist() == [0, 48, 112]
    assert call(d, s, 0, 16) == STS_EINVAL and call(d, s, 2, 0) == STS_EINVAL and call(d, s, 2, (1 << 20) + 1) == STS_EINVAL
    assert call(np.asarray([3, -1], np.int32), s, 2, 16) == STS_EINVAL
    assert call(np.asarray([3, 100001], np.int32), s, 2, 16) == STS_EINVAL
    assert call(d, np.asarray([1 << 32, 3037000499], np.int64), 2, 16) == STS_EINVAL
    assert call(d, np.asarray([6074001001, 1 << 32], np.int64), 2, 16) == STS_EINVAL
    assert call(np.asarray([1024, 0], np.int32), s, 2, 1 << 20) == STS_EINVAL          # N = 2^30
    assert call(np.asarray([1023, 0], np.int32), s, 2, 1 << 20) == 0


def test_layout_program_under_ubsan(tmp_path):
    """tests/pitch_layout_check.cpp: the header's arithmetic at the largest admitted signals and on seeded random cases, every line against
    the restatement's Python integers"""
    exe = tmp_path / "pitch_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "pitch_layout_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-400:], r.stderr[-400:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) >= 230
    refused = 0
    for line in lines:
        parts = [p.split() for p in line.split("|")]
        hop, n = int(parts[0][0]), int(parts[0][1])
        d, cents = [int(v) for v in parts[1]], [int(v) for v in parts[2]]
        assert len(d) == n and len(cents) == n
        if parts[3] == ["refused"]:
            assert max(1, sum(d)) * hop >= 1 << 30, line
            refused += 1
            continue
        assert max(1, sum(d)) * hop < 1 << 30, line
        step = pr.design(cents)[1]
        assert [int(v) for v in parts[3]] == step.tolist()
        o, e = pr.layout(d, step, hop)
        assert [int(v) for v in parts[4]] == o and [int(v) for v in parts[5]] == e, line
    assert refused == 4


# ---- prototype --------------------------------------------------------------------------------------------------------------------------------
def test_pitch_table_against_numpy():
    t = engine.pitch_table()
    w = pr.table()
    assert t.dtype == np.float32 and t.size == engine.PITCH_TABLE_FLOATS == pr.PROTO + 2
    assert t.tobytes() == w.tobytes()
    assert t[0] == 1.0 and t[pr.PROTO] == 0 and t[pr.PROTO + 1] == 0
    assert (np.abs(t[pr.RES::pr.RES]) < 1e-7).all()              # the sinc's zero crossings
    lib = engine.load_library()
    assert lib.sts_pitch_table(t.ctypes.data, pr.PROTO + 1) == STS_EINVAL and lib.sts_pitch_table(None, 1 << 20) == STS_EINVAL


# ---- properties of the restatement itself -----------------------------------------------------------------------------------------------------
SINE_CASES = {}


def _sine_case(cents):
    if cents not in SINE_CASES:
        hop, d, f0 = 16, [5, 0, 7, 3], 0.11
        step = pr.design([cents] * 4)[1]
        x = np.sin(2 * np.pi * f0 * np.arange(sum(d) * hop)).astype(np.float32)
        y, S = pr.warp(x, d, step, hop)
        ye, _ = pr.warp(x, d, step, hop, exact=True)
        SINE_CASES[cents] = (x, y, ye, int(step[0]))
    return SINE_CASES[cents]


@pytest.mark.parametrize("cents,length", [(-600, 340), (-100, 255), (37, 235), (600, 170)])
def test_a_sine_comes_out_at_the_warped_positions(cents, length):
    x, y, ye, step = _sine_case(cents)
    assert y.size == length
    pos = np.arange(y.size) * step / 4294967296.0
    ref = np.sin(2 * np.pi * 0.11 * pos)
    err = np.abs(y - ref)[80:-80].max()
    tab = np.abs(y - ye).max()
    print(f"cents {cents}: sine error in the middle {err:.3g}, table against the closed-form window {tab:.3g}")
    assert err <= 1e-5                                            # (measured 3.7e-6; the margin covers libm differences)
    assert tab <= 2e-6                                            # (measured 9.5e-7)


def test_identity_and_copy():
    rng = np.random.default_rng(0)
    d, hop = [3, 4], 16
    x = rng.standard_normal(sum(d) * hop).astype(np.float32)
    y, S, y64 = pr.apply(x, d, hop, [0, 0])
    assert y.size == x.size and not np.array_equal(y, x)            # all cents 0 keeps the length; the member is filtered all the same (c = 0.9)
    y, S, y64 = pr.apply(x, d, hop, None)
    assert y.tobytes() == x.tobytes()
    y, S, y64 = pr.apply(np.ones(6, np.float32), [0, 0], 6, [600, -600])
    assert y.size == 6
