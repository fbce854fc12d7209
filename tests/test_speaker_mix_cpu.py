"""CPU suite of speaker blending (sts_set_speaker_mix): the header / library surface, the layout of sts_speaker_mix against its ctypes
mirror, the validity rules of sts_speaker_mix_check against tests/speaker_ref.py, and worked examples of the NumPy blend.  Nothing here
touches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import speaker_ref as sr
from conftest import ROOT
from summertts_amd import engine, synth_blob as sb

STS_EINVAL = -1
HEADER = os.path.join(ROOT, "include", "summertts_hip.h")
NEW = (("sts_set_speaker_mix", 3), ("sts_speaker_mix_check", 4), ("sts_get_speaker_embedding", 4), ("sts_speaker_blend", 8),
       ("sts_pool_submit_mix", 9), ("sts_multi_set_speaker_mix", 3))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def _arg_count(name, src):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_surface_and_an_abi_that_did_not_grow(lib, tmp_path):
    src = open(HEADER).read()
    assert re.search(r"#define STS_ABI_VERSION (\d+)", src).group(1) == "18" and lib.sts_abi_version() == 18
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NEW:
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS, name
        assert _arg_count(name, code) == nargs, name
    # existing signatures are what they were
    for name, nargs in (("sts_infer_ids", 7), ("sts_infer_ids_batch", 8), ("sts_run_batch", 8), ("sts_infer_ids_stream", 9),
                        ("sts_infer_ids_batch_stream", 10), ("sts_pool_submit", 5), ("sts_pool_submit_ex", 8), ("sts_pool_submit_plan", 11),
                        ("sts_multi_infer_ids_batch", 8), ("sts_set_duration_plan", 4)):
        assert _arg_count(name, code) == nargs, name
    # the reference's class surface knows nothing of it
    assert "mix" not in open(os.path.join(ROOT, "include", "SynthesizerTrn.h")).read().lower()
    # the struct as the C compiler lays it out against the ctypes mirror; sts_profile keeps its size
    fields = ("k", "sid", "weight", "vector", "vector_weight")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "summertts_hip.h"\nint main(void) { printf("%zu %zu", sizeof(sts_profile), '
                    'sizeof(sts_speaker_mix)); ' + " ".join('printf(" %%zu", offsetof(sts_speaker_mix, %s));' % f for f in fields) + " return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(engine.Profile) == 200
    assert vals[1] == C.sizeof(engine.SpeakerMix)
    assert vals[2:] == [getattr(engine.SpeakerMix, f).offset for f in fields]


def _rc(lib, speaker_num, gin, mixes):
    arr, keep = engine._speaker_mixes(mixes)
    return lib.sts_speaker_mix_check(speaker_num, gin, len(mixes), C.cast(arr, C.c_void_p))


def test_check_rules(lib):
    nan, inf = float("nan"), float("inf")
    v4 = [0.5, -1.0, 0.0, 2.0]
    good = [None, {}, {"sid": [0], "weight": [1.0]}, {"sid": [2, 2, 0], "weight": [16.0, -16.0, 0.0]}, {"vector": v4},
            {"vector": v4, "vector_weight": -16.0}, {"sid": [1, 0], "weight": [1.5, -0.5], "vector": v4, "vector_weight": 0.25},
            {"sid": list(range(3)) * 5 + [0], "weight": [0.1] * 16}]
    bad = [{"sid": [3], "weight": [1.0]}, {"sid": [-1], "weight": [1.0]}, {"sid": [0, 1], "weight": [1.0, nan]}, {"sid": [0], "weight": [inf]},
           {"sid": [0], "weight": [-inf]}, {"sid": [0], "weight": [16.000002]}, {"sid": [0], "weight": [-17.0]},
           {"sid": [0] * 17, "weight": [0.0] * 17}, {"vector": [0.0, nan, 0.0, 0.0]}, {"vector": [inf, 0.0, 0.0, 0.0]},
           {"vector": v4, "vector_weight": nan}, {"vector": v4, "vector_weight": 16.5}, {"vector": v4, "vector_weight": inf}]
    for m in good:
        assert sr.valid(3, 4, m) and _rc(lib, 3, 4, [m]) == 0, m
    for m in bad:
        assert not sr.valid(3, 4, m) and _rc(lib, 3, 4, [m]) == STS_EINVAL, m
        assert _rc(lib, 3, 4, [good[2], m, None]) == STS_EINVAL, m            # one bad entry refuses the batch
        with pytest.raises(engine.StsError, match="speaker mix"):
            engine.speaker_mix_check(3, 4, [m])
    assert _rc(lib, 3, 4, good) == 0
    engine.speaker_mix_check(3, 4, good)
    # a single-speaker model (speaker_num 0) takes empty entries only
    for m in good:
        assert (_rc(lib, 0, 0, [m]) == 0) == sr.is_empty(m) == sr.valid(0, 0, m), m
    # k outside 0..16 and null arrays with k > 0, which the Python front end cannot express
    one = (engine.SpeakerMix * 1)()
    s = np.zeros(20, np.int32); w = np.ones(20, np.float32)
    for k, sp, wp, want in ((-1, s, w, STS_EINVAL), (17, s, w, STS_EINVAL), (16, s, w, 0), (1, None, w, STS_EINVAL), (1, s, None, STS_EINVAL),
                            (0, None, None, 0)):
        one[0].k = k; one[0].sid = None if sp is None else sp.ctypes.data; one[0].weight = None if wp is None else wp.ctypes.data
        assert lib.sts_speaker_mix_check(3, 4, 1, C.cast(one, C.c_void_p)) == want, (k, sp is None, wp is None)
    assert lib.sts_speaker_mix_check(3, 4, 1, None) == STS_EINVAL and lib.sts_speaker_mix_check(3, 4, -1, C.cast(one, C.c_void_p)) == STS_EINVAL
    assert lib.sts_speaker_mix_check(3, 4, 0, None) == 0


def test_reference_on_worked_examples():
    rng = np.random.default_rng(11)
    table = rng.standard_normal((16, 5)).astype(np.float32)
    for s in range(5):                                                   # one-hot equals the row
        assert np.array_equal(sr.blend(table, {"sid": [s], "weight": [1.0]}).view(np.uint32), table[:, s].view(np.uint32))
        assert np.array_equal(sr.blend(table, None, s), table[:, s]) and np.array_equal(sr.blend(table, {}, 7), table[:, 0])
    v = rng.standard_normal(16).astype(np.float32)                      # vector-only equals the vector
    assert np.array_equal(sr.blend(table, {"vector": v}).view(np.uint32), v.view(np.uint32))
    # exact small cases: 0.5 a + 0.5 b of representable halves; an extrapolation
    t = np.asarray([[1.0, 3.0], [-2.0, 6.0]], np.float32)
    assert sr.blend(t, {"sid": [0, 1], "weight": [0.5, 0.5]}).tolist() == [2.0, 2.0]
    assert sr.blend(t, {"sid": [0, 1], "weight": [1.5, -0.5], "vector": [1.0, 1.0], "vector_weight": 2.0}).tolist() == [2.0, -4.0]
    # ONE rounding: 1 + 2^-24 + 2^-24 is 1 + 2^-23 in float64 accumulation; rounding after every term would stay at 1
    t = np.asarray([[1.0, 2.0 ** -24]], np.float32)
    assert sr.blend(t, {"sid": [0, 1, 1], "weight": [1.0, 1.0, 1.0]})[0] == np.float32(1.0 + 2.0 ** -23)
    # the order of the terms matters only in the last float64 bit: across random three-term mixes the float64 sums of two orders differ by at
    # most two units in the last place of the sum of magnitudes, and the float32 results are nearly always the same bits
    same = 0
    for trial in range(200):
        sid = rng.integers(0, 5, 3); w = rng.uniform(-2, 2, 3).astype(np.float32)
        a = sr.blend(table, {"sid": sid, "weight": w}); b = sr.blend(table, {"sid": sid[::-1], "weight": w[::-1]})
        p = w.astype(np.float64)[:, None] * table[:, sid].T.astype(np.float64)
        fwd = (p[0] + p[1]) + p[2]; rev = (p[2] + p[1]) + p[0]
        assert (np.abs(fwd - rev) <= 2 * np.spacing(np.abs(p).sum(axis=0))).all()      # (two additions per order, half a unit each)
        assert (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= 1).all()
        same += int(np.array_equal(a, b))
    assert same >= 190


def test_blob_b_is_blob_a_with_more_speakers():
    cfg = sb.tiny_cfg("ms_hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    head, table = sr.blob_tail(blob, cfg.spk_num, cfg.gin)
    assert table.shape == (cfg.gin, cfg.spk_num) and head.size + 2 + table.size == blob.size
    cols = sr.blend_batch(table, [{"sid": [0, 3], "weight": [0.6, 0.4]}, {"sid": [1], "weight": [1.0]}])
    blob_b = sr.blob_with_extra_speakers(blob, cfg.spk_num, cfg.gin, cols)
    assert blob_b.size == blob.size + 2 * cfg.gin and np.array_equal(blob_b[:head.size], head)
    _, table_b = sr.blob_tail(blob_b, cfg.spk_num + 2, cfg.gin)
    assert np.array_equal(table_b[:, :cfg.spk_num], table) and np.array_equal(table_b[:, cfg.spk_num:].T, cols)
    assert np.array_equal(table_b[:, cfg.spk_num + 1], table[:, 1])
    import dataclasses
    assert np.array_equal(blob_b[:head.size], sb.make_blob(dataclasses.replace(cfg, spk_num=cfg.spk_num + 2), 1234)[:head.size])
