"""Per-slot filter state of an open stream, host side: sts_stream_get_loudness is exported, declared, listed and bound without a new ABI
revision; what it answers without an engine; the structure no GPU test sees; and live_stream.hpp's
four resources -- slots, frame ranges, phoneme ranges, tiles -- with the consumed positions and the one parity, through seeded random
schedules against brute force in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import pytest

from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
STS_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_entry_is_exported_declared_listed_and_bound(lib):
    raw = _read("include", "summertts_hip.h")
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert hasattr(lib, "sts_stream_get_loudness") and "sts_stream_get_loudness" in engine.EXPORTED_SYMBOLS
    assert "int sts_stream_get_loudness(sts_engine* e, int32_t* slot_out, sts_loudness* out, int64_t capacity);" in hdr
    # (a C compiler needs the struct in front of the prototype)
    assert hdr.index("} sts_loudness;") < hdr.index("int sts_stream_get_loudness(")
    assert list(lib.sts_stream_get_loudness.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    assert lib.sts_abi_version() == 18 == int(re.search(r"#define STS_ABI_VERSION (\d+)", hdr).group(1))
    assert callable(engine.Synthesizer.stream_loudness)
    assert lib.sts_stream_get_loudness(None, None, None, 0) == STS_EINVAL


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "summertts_hip.h"\nint main(void) { return sizeof(sts_loudness) == 16 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "h")], check=True)
    assert subprocess.run([str(tmp_path / "h")]).returncode == 0


def test_the_documents_no_longer_promise_it():
    raw = " ".join(_read("include", "summertts_hip.h").split())
    assert "filter state, the next step" not in raw and "filter state: later work" not in raw
    assert "filter state is the next step" not in " ".join(_read("README.md").split())
    design = _read("DESIGN.md")
    assert "Per-slot filter state" in design and "sts_stream_get_loudness" in design


def test_the_structure_no_gpu_test_sees():
    """(what the entries answer is tests/test_live_filters_gpu.py's)"""
    eng, hpp, step = (_read("summertts_amd", "csrc", f) for f in ("engine.hip", "live_stream.hpp", "stream_step.hpp"))
    opened = eng[eng.index("int Engine::stream_open("):eng.index("int Engine::stream_close(")]
    closed = eng[eng.index("int Engine::stream_close("):eng.index("int Engine::stream_admit_once(")]
    # one allocation for all the filter pools, freed at close
    assert opened.count("hipMalloc(&L->filters_dev") == 1 and "hipFree(live_->filters_dev)" in closed
    # a stream's result lists begin and end with it
    assert "loud_slots.clear()" in opened and "loud_slots.clear()" in closed
    # open paragraphs open no filter pools
    assert "open_filters" not in eng[eng.index("int Engine::para_open("):eng.index("int Engine::para_step(")]
    # one builder for closed and open steps
    assert step.count("static inline const char* step_build(") == 1
    # the header stays plain C++
    assert "hip" not in re.sub(r"//.*", "", hpp).lower() and "engine.hpp" not in hpp


def test_four_resources_positions_and_parity_against_brute_force_under_the_sanitizers(tmp_path):
    """tests/live_filters_check.cpp: nothing overlaps in any pool, admission is all or nothing over slots, frames, phonemes and tiles and
    leaves positions and parity alone when refused, a full drain leaves one range in every list, one utterance that fits the empty frame pool fits
    the empty tile pool, every row of an open step passes eqs_row_check / lds_row_check, names its slot, continues where that slot's state
    ends and reads the state slot that state lies in (the one global parity), writes tiles of its own range only, and a step repeated
    after drop() builds the same rows"""
    exe = tmp_path / "live_filters_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "live_filters_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-400:], r.stderr[-400:])
    schedules, admissions, refused, refused_tiles, steps, repeats, rows = (int(v) for v in r.stdout.split()[1:8])
    assert schedules >= 100 and admissions > 1000 and refused > 100 and steps > 1000 and repeats > 100 and rows > 3000
    assert refused_tiles > 0          # fragmentation of the tile pool alone refuses some: the third list decides, not only mirrors
