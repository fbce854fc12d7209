"""The per-call tables in one place (summertts_amd/csrc/utt_tables.hpp): the staging layout, the owning copy of one utterance's tables and
the same-batch check in a stand-alone program under AddressSanitizer and UBSan; and, from the sources, that the tables reach an engine
through one forwarder."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
SETTERS = ("set_duration_plan", "set_speaker_mix", "set_gain_plan", "set_pitch_plan")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _member_calls(text, setter):
    """calls of an engine's setter through an object (`x.set_..(`, `x->set_..(`): neither its definition nor a C entry's name"""
    return re.findall(r"(?:\.|->)%s\(" % setter, re.sub(r"//.*", "", text))


def test_layout_tables_and_same_batch_check_under_the_sanitizers(tmp_path):
    """tests/utt_tables_check.cpp: every offset and both totals of the staging block equal the hand-written expressions over B x Ttot x
    every legal combination of tables; assign -> view round-trips every kind bit for bit from freed sources; table_matches"""
    exe = tmp_path / "utt_tables_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "utt_tables_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-400:], r.stderr[-400:])
    layouts, trips = (int(v) for v in r.stdout.split()[1:3])
    # 4 B x 3 Ttot x 3 mixes x 2 gains x (join, plan, forced, pitch: 16, less the 4 with plan and forced, less the 3 of the rest with join and pitch)
    assert layouts == 4 * 3 * 3 * 2 * 9 and trips >= 256


def test_the_header_is_plain_cpp():
    hpp = _src("utt_tables.hpp")
    assert "hip/" not in hpp and "__global__" not in hpp and "engine.hpp" not in hpp
    assert "hip" not in re.sub(r"//.*", "", hpp).lower().replace("summertts_hip.h", "")
    assert '#include "utt_tables.hpp"' in _src("kernels.hpp") and "struct SpeakerMixCopy" not in _src("kernels.hpp")


def test_one_forwarder_sets_the_tables_in_order():
    eng = _src("engine.hip")
    fwd = eng[eng.index("int apply_utt_tables("):]
    fwd = fwd[:fwd.index("\n}\n")]
    at = [fwd.index("eng.%s(" % s) for s in SETTERS]
    assert at == sorted(at) and all(fwd.count("eng.%s(" % s) == 1 for s in SETTERS)
    assert "eng.drop_tables()" in fwd[at[-1]:]
    # the engine's own file calls a setter nowhere else; the pool and the multi-device handle go through the forwarder only; outside
    # engine.hip the one caller of each setter is its C entry
    for s in SETTERS:
        assert len(_member_calls(eng, s)) == 1, s
        assert not _member_calls(_src("pool.hip"), s) and not _member_calls(_src("multi.hip"), s), s
        others = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp")) and f != "engine.hip" and _member_calls(_src(f), s)]
        assert others == ["capi.hip"] and len(_member_calls(_src("capi.hip"), s)) == 1, (s, others)
    assert _src("pool.hip").count("apply_utt_tables(") == 1 and _src("multi.hip").count("apply_utt_tables(") == 1


def test_the_layout_and_the_message_are_spelled_once():
    eng = _src("engine.hip")
    assert not re.search(r"mix_ints\s*\+\s*gain_ints", eng) and "join_ints" not in eng
    assert eng.count("StageLayout L(") == 1
    spelled = [f for f in sorted(os.listdir(CSRC)) if "was set for another batch" in _src(f)]
    assert spelled == ["utt_tables.hpp"]
    assert eng.count("table_matches(") == 3 and _src("multi.hip").count("table_matches(") == 3
