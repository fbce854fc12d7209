"""Paragraph join without a GPU: the new symbols in the library, the Python list and the header; the ctypes mirror of sts_join; every
refusal of sts_join_check; the host-only layout (sts_join_layout) against the NumPy restatement of tests/join_ref.py; and the properties of
the restatement's envelope."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import join_ref as jr
from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sts_join_check", "sts_join_layout", "sts_join_apply", "sts_infer_ids_joined", "sts_get_join_offsets", "sts_pool_submit_joined"]
STS_EINVAL = -1
INF, NAN = float("inf"), float("nan")


def _header():
    return open(os.path.join(ROOT, "include", "summertts_hip.h")).read()


def test_symbols_are_in_the_library_the_list_and_the_header():
    lib = engine.load_library()
    header = _header()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\s*\(", header), s
    assert "typedef struct sts_join" in header
    for name in ("join_check", "join_layout", "join_apply"):
        assert callable(getattr(engine, name)), name
    for cls, name in ((engine.Synthesizer, "infer_joined"), (engine.Synthesizer, "join_offsets"), (engine.Pool, "submit_joined")):
        assert callable(getattr(cls, name)), name


def test_the_abi_version_is_still_15():
    lib = engine.load_library()
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18" in _header()
    assert C.sizeof(engine.Profile) == 200                      # sts_profile did not grow


def test_the_ctypes_mirror_matches_the_header():
    m = re.search(r"typedef struct sts_join \{(.*?)\} sts_join;", _header(), re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        t = re.match(r"(const\s+int32_t\s*\*|int32_t|float)", decl)
        ctype, names = t.group(1).replace(" ", ""), decl[t.end():]
        for name in names.split(","):
            fields.append((name.strip(), ctype))
    want = {"constint32_t*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, want[t]) for n, t in fields] == [(n, t) for n, t in engine.Join._fields_]
    assert [n for n, _ in fields] == ["gap_frames", "lead_frames", "trail_frames", "fade_ms"]
    assert C.sizeof(engine.Join) == 24 and engine.Join.lead_frames.offset == 8 and engine.Join.fade_ms.offset == 16


@pytest.mark.parametrize("B,bad", [(2, {"fade_ms": NAN}), (2, {"fade_ms": 50.0001}), (2, {"fade_ms": -0.5}), (2, {"fade_ms": INF}),
                                   (3, {"gap_frames": [0, -1]}), (3, {"gap_frames": [100001, 0]}), (0, {}), (0, None),
                                   (1, {"lead_frames": -1}), (1, {"lead_frames": 100001}), (1, {"trail_frames": -1}),
                                   (1, {"trail_frames": 100001})], ids=str)
def test_check_refuses(B, bad):
    with pytest.raises(engine.StsError):
        engine.join_check(B, bad)
    lib = engine.load_library()
    jp, keep = engine._join(B, bad)
    assert lib.sts_join_check(B, jp) == STS_EINVAL
    f = np.ones(max(B, 1), np.int32)
    total = C.c_int64(-7)
    assert lib.sts_join_layout(B, f.ctypes.data, 4, jp, None, C.byref(total), None) == STS_EINVAL and total.value == -7


def test_check_accepts_the_limits():
    engine.join_check(1, None)
    engine.join_check(1, {})
    engine.join_check(3, {"gap_frames": [0, 100000], "lead_frames": 100000, "trail_frames": 100000, "fade_ms": 50.0})
    engine.join_check(4, {"gap_frames": None, "fade_ms": 0.0})
    engine.join_check(1, {"gap_frames": []})
    lib = engine.load_library()
    jp, keep = engine._join(2, {"gap_frames": [5]})
    f = np.asarray([3, 0], np.int32)
    assert lib.sts_join_layout(2, f.ctypes.data, 4, jp, None, None, None) == STS_EINVAL        # a sentence without frames
    assert lib.sts_join_layout(2, None, 4, jp, None, None, None) == STS_EINVAL
    f[1] = 1
    assert lib.sts_join_layout(2, f.ctypes.data, 0, jp, None, None, None) == STS_EINVAL
    assert lib.sts_join_layout(2, f.ctypes.data, 4, jp, None, None, None) == 0                 # every output is optional


@pytest.mark.parametrize("hop", [1, 4, 256])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_layout_equals_the_reference(hop, B):
    rng = np.random.default_rng(100 * hop + B)
    for trial in range(6):
        frames = rng.integers(1, 400, B)
        frames[rng.integers(0, B)] = 1                                        # a one-frame sentence
        gaps = rng.integers(0, 100001, max(B - 1, 0))
        if B > 1:
            gaps[rng.integers(0, B - 1)] = 0                                  # a butt join
        for join in (None, {}, {"gap_frames": gaps}, {"gap_frames": gaps, "lead_frames": 100000, "trail_frames": int(rng.integers(0, 9)),
                                                       "fade_ms": float(rng.uniform(0, 50))},
                     {"lead_frames": 3, "fade_ms": 50.0}, {"trail_frames": 100000, "fade_ms": 0.03125}):
            start, total, h = engine.join_layout(frames, hop, join)
            ws, wt, wh = jr.layout(frames, hop, join)
            assert start.dtype == np.int64 and np.array_equal(start, ws) and total == wt and h == wh, (hop, B, trial, join)
            assert (start % hop == 0).all() and total % hop == 0
    # back to back without a join: the packed batch's own offsets
    frames = np.arange(1, B + 1)
    start, total, h = engine.join_layout(frames, hop, None)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(frames)[:-1]]) * hop) and total == frames.sum() * hop and h == 0


def test_design_rounds_half_up():
    for ms, want in ((0.0, 0), (0.03, 0), (0.03125, 1), (0.0625, 1), (0.09375, 2), (5.0, 80), (50.0, 800)):
        assert jr.design(ms) == want and engine.join_layout([1], 4, {"fade_ms": ms})[2] == want, ms


# ---- properties of the restatement's envelope -------------------------------------------------------------------------------------------
def test_no_fade_is_all_ones():
    for n in (1, 2, 7, 4096):
        e = jr.envelope(n, 0)
        assert e.dtype == np.float32 and e.size == n and (e == np.float32(1.0)).all()
    x = np.random.default_rng(1).standard_normal(24).astype(np.float32)
    J, pcm = jr.join([x[:8], x[8:]], [2, 4], 4, None)
    assert J.tobytes() == x.tobytes() and np.array_equal(pcm, jr.pcm_cast(x))


def test_the_envelope_is_symmetric_and_below_one_only_within_h_of_an_edge():
    for n, h in ((1000, 80), (161, 80), (160, 80), (2000, 800), (5, 1), (9, 3)):
        e = jr.envelope(n, h)
        assert np.array_equal(e, e[::-1]), (n, h)
        below = np.flatnonzero(e < np.float32(1.0))
        t = np.arange(n)
        assert np.array_equal(below, np.flatnonzero((t < h) | (t >= n - h))), (n, h)
        assert (e > 0).all() and (e <= np.float32(1.0)).all()
        assert e[0] == np.float32(np.float64(1) / np.float64(h + 1))
        if n >= 2 * h + 1:
            assert e[h] == np.float32(1.0) and e[n - 1 - h] == np.float32(1.0)


def test_a_three_sample_sentence_under_the_longest_fade():
    e = jr.envelope(3, 800)
    want = np.asarray([1, 2, 1], np.float64) / 801.0
    assert np.array_equal(e, want.astype(np.float32)) and e.max() < np.float32(1.0)        # never reaches 1
    x = np.asarray([0.5, -1.5, 2.0], np.float32)
    J, pcm = jr.join([x], [3], 1, {"fade_ms": 50.0, "lead_frames": 2, "trail_frames": 1})
    assert J.size == 6 and J[:2].tolist() == [0.0, 0.0] and J[5] == 0.0 and not np.signbit(J[[0, 1, 5]]).any()
    assert np.array_equal(J[2:5], x * e)


def test_silence_is_positive_zero_and_casts_to_zero():
    x = np.full(8, -0.25, np.float32)
    J, pcm = jr.join([x, x], [2, 2], 4, {"gap_frames": [3], "lead_frames": 1, "trail_frames": 2})
    sil = np.r_[0:4, 12:24, 32:40]
    assert J.size == 40 and (J[sil].view(np.uint32) == 0).all() and (pcm[sil] == 0).all()
    assert (J[4:12] == x).all() and (J[24:32] == x).all()


def test_a_float64_reciprocal_rounds_like_the_quotient():
    """join.hip evaluates the fade as float32(m * (1.0 / (h + 1))) -- one division per lane instead of one per sample; for every h and m
    the definition allows that is the float32 the quotient rounds to"""
    for h in range(0, 801):
        m = np.arange(1, h + 2, dtype=np.float64)
        assert np.array_equal((m * (1.0 / np.float64(h + 1))).astype(np.float32), (m / np.float64(h + 1)).astype(np.float32)), h
