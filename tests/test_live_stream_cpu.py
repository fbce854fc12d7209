"""Open streams, host side: the new entries are exported, declared and listed; the ABI revision; the Python argtypes against the header's
prototypes; what the entries answer without an engine; the layout pins of class Engine; and live_stream.hpp -- the slot table, the first-fit
allocator and the window geometry -- through seeded random schedules in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
STS_EINVAL, STS_ESTATE = -1, -4
NEW_SYMBOLS = ("sts_stream_open", "sts_stream_admit", "sts_stream_step", "sts_stream_info", "sts_stream_close", "sts_debug_adopt_z",
               "sts_pool_set_stream_admission", "sts_pool_get_stream_admission", "sts_pool_stream_stats")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "summertts_hip.h")).read(), flags=re.S)


def test_new_symbols_are_exported_declared_and_listed(lib):
    hdr = _header()
    declared = set(re.findall(r"\b(sts_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert s in declared, s
    assert lib.sts_abi_version() == 18 == int(re.search(r"#define STS_ABI_VERSION (\d+)", hdr).group(1))
    assert re.search(r"typedef struct sts_stream_noise \{ float noise_scale, noise_scale_w; uint64_t seed; \} sts_stream_noise;", hdr)
    assert C.sizeof(engine.StreamNoise) == 16 and [n for n, _ in engine.StreamNoise._fields_] == ["noise_scale", "noise_scale_w", "seed"]
    # no error code was added
    codes = dict(re.findall(r"\b(STS_E[A-Z]+)\s*=\s*(-?\d+)", hdr))
    assert codes == {"STS_EINVAL": "-1", "STS_EMODEL": "-2", "STS_EDEVICE": "-3", "STS_ESTATE": "-4"}


def test_python_argtypes_match_the_header(lib):
    """the ctypes argtypes name the header's parameter types in the header's order (pointers as c_void_p, the callback as BATCH_CHUNK_CB)"""
    hdr = _header()
    of = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "sts_batch_chunk_cb": engine.BATCH_CHUNK_CB}
    for s in NEW_SYMBOLS:
        ret, params = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % s, hdr).groups()
        assert ret == "int"
        want = []
        for p in params.split(","):
            p = " ".join(p.split())
            want.append(C.c_void_p if "*" in p else of[p.replace("const ", "").split()[0]])
        assert list(getattr(lib, s).argtypes) == want, s
    for m in ("stream_open", "stream_admit", "stream_step", "stream_info", "stream_close"):
        assert callable(getattr(engine.Synthesizer, m)), m
    assert callable(engine.debug_adopt_z) and callable(engine.Pool.set_stream_admission) and callable(engine.Pool.stream_stats)


def test_null_handles_and_bad_arguments_before_a_device_is_touched(lib):
    """(an engine needs a GPU: tests/test_live_stream_gpu.py drives one)"""
    one = C.c_int32(7)
    assert lib.sts_stream_open(None, 8, 4, 1000) == STS_EINVAL
    assert lib.sts_stream_admit(None, 1, None, None, None, None, None, None, None, C.addressof(one)) == STS_EINVAL
    assert lib.sts_stream_step(None, engine.BATCH_CHUNK_CB(lambda *a: 0), None, None) == STS_EINVAL
    assert lib.sts_stream_info(None, None, None, None, None, None) == STS_EINVAL
    assert lib.sts_stream_close(None) == STS_EINVAL
    assert lib.sts_pool_set_stream_admission(None, 1) == STS_EINVAL
    assert lib.sts_pool_get_stream_admission(None) == 0
    assert lib.sts_pool_stream_stats(None, None, None) == STS_EINVAL
    # the kernel entry checks its tables before it looks for a device
    src = np.zeros((3, 16), np.float32)
    dst = np.zeros((3, 16), np.float32)

    def adopt(so, do, ln, B=None, C_=3):
        so, do, ln = np.asarray(so, np.int64), np.asarray(do, np.int64), np.asarray(ln, np.int32)
        return lib.sts_debug_adopt_z(0, src.ctypes.data, C_, 16, dst.ctypes.data, 16, so.ctypes.data, do.ctypes.data, ln.ctypes.data,
                                     len(ln) if B is None else B)
    assert adopt([0], [0], [4], B=0) == STS_EINVAL and adopt([0], [0], [4], C_=0) == STS_EINVAL
    assert adopt([13], [0], [4]) == STS_EINVAL and adopt([0], [13], [4]) == STS_EINVAL and adopt([-1], [0], [4]) == STS_EINVAL
    assert adopt([0, 4], [0, 3], [4, 4]) == STS_EINVAL and b"overlap" in lib.sts_last_error()
    assert lib.sts_debug_adopt_z(0, None, 3, 16, dst.ctypes.data, 16, None, None, None, 1) == STS_EINVAL


def test_the_engine_keeps_its_pinned_layout():
    """the open stream's members stand behind run_joined_stream and in front of loud_streaming; eq_streaming stays the last declaration"""
    src = open(os.path.join(CSRC, "engine.hpp")).read()
    body = src[src.index("class Engine {"):]
    assert body.index("int run_joined_stream(") < body.index("int stream_open(") < body.index("LiveStream* live_ = nullptr;") < \
        body.index("bool loud_streaming = false;") < body.index("bool eq_streaming = false;")
    assert body[body.index("bool eq_streaming = false;") + len("bool eq_streaming = false;"):].split("}  // namespace sts")[0].strip() == "};"
    # the state struct is plain C++: no HIP, no engine type
    hpp = open(os.path.join(CSRC, "live_stream.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", hpp).lower() and "engine.hpp" not in hpp
    # the pool is not in the frame arena, and the closed call and the open stream share one step loop and one window definition
    eng = open(os.path.join(CSRC, "engine.hip")).read()
    opened = eng[eng.index("int Engine::stream_open("):eng.index("int Engine::stream_close(")]
    assert "hipMalloc((void**)&L->zpool" in opened and "arenaF_" not in opened
    step = eng[eng.index("int Engine::stream_step("):]
    assert "run_stream_steps(c)" in step
    # (the one call of the window definition: the plain builder of stream_step.hpp, which run_stream_steps calls for both)
    dec, tab = (open(os.path.join(CSRC, f)).read() for f in ("decoder.hip", "stream_step.hpp"))
    assert (eng + dec + tab).count("stream_window(") == 1
    plain = tab[tab.index("static inline const char* step_build("):tab.index("static inline const char* step_build_joined(")]
    assert "stream_window(" in plain
    loop = eng[eng.index("int Engine::run_stream_steps("):]
    assert "step_build(call," in loop and "step_build_joined(call," in loop


def test_slot_table_allocator_and_windows_under_the_sanitizers(tmp_path):
    """tests/live_stream_check.cpp: allocated ranges never overlap and stay inside [0, capacity), freed ranges coalesce (a full drain leaves
    one), first fit and the lowest free slot against brute force, the same schedule twice places alike, a slot's window sequence is a
    function of (F, C, halo, P, Q, H) whatever the schedule, a refused admission leaves the state untouched"""
    exe = tmp_path / "live_stream_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "live_stream_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-400:], r.stderr[-400:])
    schedules, admissions, refused, steps = (int(v) for v in r.stdout.split()[1:5])
    assert schedules >= 100 and admissions > 1000 and refused > 100 and steps > 1000
