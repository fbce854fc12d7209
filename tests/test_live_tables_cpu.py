"""Planned open streams, host side: the four new entries are exported, declared with the header's prototypes and listed; the ABI revision
stays 18; the header names the old open entry as the capacity_phonemes == 0 case; what the entries answer without a device; and
live_stream.hpp's three resources -- slots, frame ranges, phoneme ranges -- through seeded random schedules against brute force in a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
STS_EINVAL = -1
NEW_SYMBOLS = ("sts_stream_open_ex", "sts_stream_tables_info", "sts_pool_submit_stream_ex", "sts_debug_adopt_tables")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def _raw_header():
    return open(os.path.join(ROOT, "include", "summertts_hip.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", " ", _raw_header(), flags=re.S)


def test_new_symbols_are_exported_declared_and_listed(lib):
    hdr = _header()
    declared = set(re.findall(r"\b(sts_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert s in declared, s
    # additive: the revision does not move, and the header says how the entries are found
    assert lib.sts_abi_version() == 18 == int(re.search(r"#define STS_ABI_VERSION (\d+)", hdr).group(1))
    raw = " ".join(_raw_header().split())
    assert "detected by symbol" in raw and "detect them by symbol" in raw
    assert "sts_stream_open is the capacity_phonemes == 0 case of sts_stream_open_ex" in raw
    assert "capacity_phonemes == 0 is sts_stream_open exactly" in raw
    # what stays refused is said where the entries are declared
    for word in ("EQ and loudness in an open stream", "record taps", "sts_para_*", "sts_multi_*"):
        assert word in raw, word
    codes = dict(re.findall(r"\b(STS_E[A-Z]+)\s*=\s*(-?\d+)", hdr))
    assert codes == {"STS_EINVAL": "-1", "STS_EMODEL": "-2", "STS_EDEVICE": "-3", "STS_ESTATE": "-4"}


def test_python_argtypes_match_the_header(lib):
    """the ctypes argtypes name the header's parameter types in the header's order (pointers as c_void_p, the callback as CHUNK_CB)"""
    hdr = _header()
    of = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "sts_chunk_cb": engine.CHUNK_CB}
    for s in NEW_SYMBOLS:
        ret, params = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % s, hdr).groups()
        assert ret == ("int64_t" if s == "sts_pool_submit_stream_ex" else "int"), s
        want = []
        for p in params.split(","):
            p = " ".join(p.split())
            want.append(C.c_void_p if "*" in p else of[p.replace("const ", "").split()[0]])
        assert list(getattr(lib, s).argtypes) == want, s
    assert lib.sts_pool_submit_stream_ex.restype == C.c_int64
    for m in ("stream_open", "stream_tables_info"):
        assert callable(getattr(engine.Synthesizer, m)), m
    assert callable(engine.debug_adopt_tables)
    import inspect
    assert inspect.signature(engine.Synthesizer.stream_open).parameters["capacity_phonemes"].default == 0
    for k in ("plan", "mix", "gain"):
        assert inspect.signature(engine.Pool.submit_stream).parameters[k].default is None


def test_bad_arguments_before_a_device_is_touched(lib):
    """(an engine needs a GPU: tests/test_live_plans_gpu.py drives one)"""
    assert lib.sts_stream_open_ex(None, 8, 4, 1000, 64) == STS_EINVAL
    assert lib.sts_stream_open_ex(None, 8, 4, 1000, 0) == STS_EINVAL
    assert lib.sts_stream_tables_info(None, None, None, None) == STS_EINVAL
    cb = engine.CHUNK_CB(lambda *a: 0)
    ids = np.arange(5, dtype=np.int32)
    assert lib.sts_pool_submit_stream_ex(None, ids.ctypes.data, 5, 0, 1.0, 0.0, 0.0, 0, 4, cb, None, None, None, None) == STS_EINVAL
    # an invalid plan is refused at submit, by the checks of sts_pool_submit_plan / _gain, before the pool is looked at
    lib.sts_pool_last_error.restype = C.c_char_p
    rate = np.array([1.0, 1.0, 1000.0, 1.0, 1.0], np.float32)
    bad = engine.DurPlan(rate.ctypes.data, None, 0)
    assert lib.sts_pool_submit_stream_ex(None, ids.ctypes.data, 5, 0, 1.0, 0.0, 0.0, 0, 4, cb, None, C.addressof(bad), None, None) == STS_EINVAL
    assert b"rate" in lib.sts_pool_last_error()
    db = np.array([0.0, 0.0, 30.0, 0.0, 0.0], np.float32)
    badg = engine.GainPlan(db.ctypes.data, 5.0)
    assert lib.sts_pool_submit_stream_ex(None, ids.ctypes.data, 5, 0, 1.0, 0.0, 0.0, 0, 4, cb, None, None, None, C.addressof(badg)) == STS_EINVAL
    assert b"gain" in lib.sts_pool_last_error()
    # the kernel entry checks its tables before it looks for a device
    cum = np.arange(1, 17, dtype=np.int32)
    q = np.full(16, 1 << 20, np.int32)
    pool = np.zeros((2, 9), np.int32)
    words = np.zeros((3, 4), np.int32)
    g = np.zeros((3, 2), np.float32)
    gpool = np.zeros((3, 4), np.float32)

    def adopt(slot, so, n, do, B=None, with_g=True, cap=8, max_live=4):
        a = [np.asarray(v, np.int32) for v in (slot, so, n, do, [0] * len(slot))]
        return lib.sts_debug_adopt_tables(0, g.ctypes.data if with_g else None, 3 if with_g else 0, len(slot) if B is None else B,
                                          gpool.ctypes.data if with_g else None, max_live, cum.ctypes.data, q.ctypes.data, 16, pool.ctypes.data, cap,
                                          words.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data)
    assert adopt([0, 1], [0, 4], [4, 4], [0, 4], B=0) == STS_EINVAL and adopt([0, 1], [0, 4], [4, 4], [0, 4], B=65536) == STS_EINVAL
    assert adopt([0, 1], [13, 0], [4, 4], [0, 4]) == STS_EINVAL           # a source range leaves cum / q
    assert adopt([0, 1], [0, 4], [4, 4], [0, 5]) == STS_EINVAL            # a destination range leaves the pool (its last column is not for plans)
    assert adopt([0, 1], [0, 4], [4, 4], [-1, 4]) == STS_EINVAL and adopt([0, 1], [0, 4], [-1, 4], [0, 4]) == STS_EINVAL
    assert adopt([0, 1], [0, 4], [4, 4], [0, 3]) == STS_EINVAL and b"overlap" in lib.sts_last_error()
    assert adopt([0, 0], [0, 4], [4, 4], [0, 4]) == STS_EINVAL and adopt([0, 4], [0, 4], [4, 4], [0, 4]) == STS_EINVAL      # a slot twice, a slot outside
    assert adopt([0, 1], [0, 4], [4, 4], [0, 4], cap=0) == STS_EINVAL
    assert lib.sts_debug_adopt_tables(0, g.ctypes.data, 3, 2, None, 4, cum.ctypes.data, q.ctypes.data, 16, pool.ctypes.data, 8, words.ctypes.data,
                                      None, None, None, None, None) == STS_EINVAL


def test_the_planned_stream_is_wired_through_one_builder_and_one_launch():
    eng, tab, ls, hpp = (open(os.path.join(CSRC, f)).read() for f in ("engine.hip", "stream_step.hpp", "live_stream.hip", "live_stream.hpp"))
    # one builder: the planned stream's slot rides in StepWin, no second step_build
    assert tab.count("static inline const char* step_build(") == 1 and "u.tab >= 0 ? u.tab : u.b" in tab
    # one launch next to adopt_z, its table in the admission's one upload
    once = eng[eng.index("int Engine::stream_admit_once("):eng.index("int Engine::stream_admit(")]
    assert once.count("adopt_tables(a, max_n, stream)") == 1 and once.count("hipMemcpyAsync(L.tab_dev") == 1
    # the tables are consumed behind the last attempt, not inside stream_admit_once
    assert "drop_tables" not in once and "drop_tables" in eng[eng.index("int Engine::stream_admit("):eng.index("int Engine::stream_step(")]
    # the gain kernel itself is not touched by the pools: the new kernel has no LDS and no gain arithmetic
    kern = ls[ls.index("void adopt_tables_kernel("):]
    assert "__shared__" not in kern
    # the state struct stays plain C++
    assert "hip" not in re.sub(r"//.*", "", hpp).lower() and "engine.hpp" not in hpp
    # the pool's phoneme capacity follows a stated rule next to live_capacity_rule
    assert hpp.index("live_capacity_rule(int") < hpp.index("live_phoneme_rule(int") and "live_phoneme_rule(" in open(os.path.join(CSRC, "pool.hip")).read()


def test_three_resources_against_brute_force_under_the_sanitizers(tmp_path):
    """tests/live_tables_check.cpp: nothing overlaps in either pool, a refused admission changes nothing (slots, frame ranges, phoneme
    ranges, counters), a full drain leaves one range in each list, the lowest free slot, first fit in both -- and the refusals are mostly
    the phoneme pool's own: the new path is what runs"""
    exe = tmp_path / "live_tables_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "live_tables_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-400:], r.stderr[-400:])
    schedules, admissions, refused, refused_phonemes, steps = (int(v) for v in r.stdout.split()[1:6])
    assert schedules >= 100 and admissions > 1000 and refused_phonemes > 100 and refused >= refused_phonemes and steps > 1000
