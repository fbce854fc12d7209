"""CPU suite of loudness in a stream (include/summertts_hip.h sts_set_loudness_streaming, DESIGN.md 9d "streamed"): the new symbols, the
ABI revision, the ctypes mirror, the switch on null handles; the float64 restatement of the CARRIED-STATE evaluation
(tests/loudness_stream_ref.py) against its whole-signal form bit for bit -- the evidence that a stream can return the whole call's
sts_loudness for every chunking -- and both against the definition (tests/loudness_ref.py); the chain planner with the new trailing
fact; the host-side row arithmetic (loud_stream.hpp) as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref
import loudness_stream_ref as lsr
from conftest import ROOT
from summertts_amd import engine

NEW_SYMBOLS = ["sts_set_loudness_streaming", "sts_get_loudness_streaming", "sts_loudness_measure_chunked"]
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
R, T = lsr.R, lsr.TILE
STS_EINVAL = -1


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


def test_python_argtypes_match_the_header(lib):
    """the ctypes argtypes name the header's parameter types in the header's order (pointers as c_void_p)"""
    hdr = _header()
    of = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    for s in NEW_SYMBOLS:
        ret, params = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % s, hdr).groups()
        assert ret == "int"
        want = []
        for p in params.split(","):
            p = p.strip()
            want.append(C.c_void_p if "*" in p else of[p.replace("const ", "").split()[0]])
        assert list(getattr(lib, s).argtypes) == want, s
    assert callable(engine.Synthesizer.set_loudness_streaming) and callable(engine.Synthesizer.loudness_streaming)
    assert callable(engine.loudness_measure_chunked)


def test_the_switch_on_null_handles_and_its_default(lib):
    """(an engine needs a GPU: tests/test_loudness_stream_gpu.py reads the default, sets and gets on one)"""
    assert lib.sts_get_loudness_streaming(None) == 0
    assert lib.sts_set_loudness_streaming(None, 1) == STS_EINVAL
    src = open(os.path.join(CSRC, "engine.hpp")).read()
    assert re.search(r"bool loud_streaming = false;", src)
    # behind every member that existed before the streamed EQ's switch (whose place at the very end an older test pins): the layout of
    # the members in front stays what it was
    body = src[src.index("class Engine {"):]
    assert body.index("int run_joined_stream(") < body.index("bool loud_streaming = false;") < body.index("bool eq_streaming = false;")
    between = body[body.index("bool loud_streaming = false;") + len("bool loud_streaming = false;"):body.index("bool eq_streaming = false;")]
    assert all(ln.strip().startswith("//") for ln in between.strip().splitlines())


def test_chunked_entry_refuses_bad_arguments_before_touching_a_device(lib):
    x = np.zeros(100, np.float32)
    lens = np.asarray([100], np.int64)
    out = np.zeros(2, engine.LOUDNESS_DTYPE)

    def call(bounds, back=0, nb=None, rate=16000, target=-16.0, o=out, B=1):
        b = np.asarray(bounds, np.int64)
        return lib.sts_loudness_measure_chunked(0, x.ctypes.data, lens.ctypes.data, B, rate, target, -1.0, b.ctypes.data,
                                                len(bounds) if nb is None else nb, back, None if o is None else o.ctypes.data, None)
    for bounds in ([1, 5], [0, 5, 5], [0, 9, 5]):
        assert call(bounds) == STS_EINVAL, bounds
    assert b"loudness stream" in lib.sts_last_error()
    assert call([0], nb=0) == STS_EINVAL and call([0], back=-1) == STS_EINVAL and call([0], back=2049) == STS_EINVAL
    assert call([0], rate=7000) == STS_EINVAL and call([0], target=1.0) == STS_EINVAL
    assert call([0], o=None) == STS_EINVAL and call([0], B=0) == STS_EINVAL


# ---- the carried-state restatement against the whole form and the definition ----------------------------------------------------------
def _signal(N):
    """noise at amplitude 0.3 with a middle third 50 dB down and a stretch of digital silence: both gates act"""
    x = (0.3 * np.random.default_rng(N).standard_normal(N)).astype(np.float32)
    x[N // 3:2 * N // 3] *= np.float32(0.003)
    x[2 * N // 3:2 * N // 3 + N // 6] = 0
    return x


CASES = [(2 * T + 5, 16000), (3 * T + 5, 16000), (2 * T + 5, 8000), (3 * T + 5, 8000), (7 * T + 5, 48000)]
FINAL_SETS = {(3 * T + 5, 16000): (8, 12), (3 * T + 5, 8000): (16, 27), (7 * T + 5, 48000): (5, 8)}      # (final set, blocks) by loudness_ref


def _step_lists(N, S):
    return {"every sample of the first 70": list(range(0, 71)),
            "chunk and tile edges": [0, R - 1, R, R + 1, 2 * R + 5, T - 1, T, T + 1, 2 * T + 5],
            "sub-block edges": [0, S - 1, S, S + 1, 4 * S],
            "one step": [0],
            "steps of 1000": list(range(0, N, 1000))}


_cache = {}


def _whole(N, fs):
    if (N, fs) not in _cache:
        k = lsr.Coef(fs)
        x = _signal(N)
        ts, tp = lsr.whole(x, k)
        _cache[(N, fs)] = (k, x, ts, tp, lsr.gate(ts, tp, N, k))
    return _cache[(N, fs)]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("N,fs", CASES)
def test_carried_state_equals_the_whole_form_bit_for_bit(N, fs):
    """every step list, the window widened by 0, 7 and 1920 samples: the tiles' sums and peaks, and the gated result"""
    k, x, ts, tp, want = _whole(N, fs)
    for name, bounds in _step_lists(N, k.S).items():
        for back in (0, 7, 1920):
            cs, cp = lsr.chunked(x, k, bounds, back)
            assert _bits(cs) == _bits(ts) and _bits(cp) == _bits(tp), (name, back)
            got = lsr.gate(cs, cp, N, k)
            assert _bits(np.float64(got["lufs"])) == _bits(np.float64(want["lufs"])) and got["blocks"] == want["blocks"], (name, back)
            assert got["peak"] == want["peak"] and _bits(got["gain"]) == _bits(want["gain"]), (name, back)


@pytest.mark.parametrize("N,fs", CASES)
def test_both_forms_agree_with_the_definition_and_both_gates_act(N, fs):
    k, x, ts, tp, got = _whole(N, fs)
    ref = loudness_ref.loudness(x, fs)
    assert np.isfinite(ref["lufs"]) and abs(got["lufs"] - ref["lufs"]) <= 0.01, (got, ref)
    assert got["peak"] == ref["peak"] and got["blocks"] == ref["blocks"]
    assert abs(float(got["gain"]) - float(ref["gain"])) <= 1e-4 * float(ref["gain"])
    assert 0 < got["blocks"] < N // k.S - 3                 # (the test cannot pass with the gates idle)
    if (N, fs) in FINAL_SETS:
        assert (got["blocks"], N // k.S - 3) == FINAL_SETS[(N, fs)]


def test_a_stopped_stream_measures_what_was_consumed():
    """the tables behind a step are those of the signal cut there: the open tile's provisional sums are the cut signal's own"""
    N, fs = 2 * T + 5, 16000
    k, x, _, _, _ = _whole(N, fs)
    for cut in (4 * k.S, T, T + 1, T + 2000):
        st = lsr.Stream(k, N)
        st.step(x[:1000], 0, 1000)
        st.step(x[993:cut + 7], 993, cut)
        ws, wp = lsr.whole(x[:cut], k)
        nt = (cut + T - 1) // T
        assert _bits(st.tsum[:nt]) == _bits(ws) and _bits(st.tpeak[:nt]) == _bits(wp), cut
    with pytest.raises(AssertionError):
        st.step(x[cut + 1:cut + 50], cut + 1, cut + 50)     # a gap: the window must hold [e, j1)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
# sha256 of the tables tests/out_chain_check.cpp and tests/eq_stream_chain_check.cpp printed before the fact loud_stream existed
TABLE_BEFORE = "27d93bf110378c856444173f87adcec961ce823b620894d7ec73c4b894eeb9a3"
EQ_TABLE_BEFORE = "8034407d7cf1c7d56c8224ee832fd7a655ca6ec59a4b15fde924eca4d7f3bc1c"


def _build(tmp_path, src, name, extra=()):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, os.path.join(ROOT, "tests", src), "-o", str(exe)], check=True)
    return str(exe)


def _parse(line):
    head, stages, tail = (p.strip() for p in line.split("|"))
    facts = {k: int(v) for k, v in (t.split("=") for t in head.split())}
    st = {}
    for t in stages.split():
        name, rest = t.split("=")
        run, src, wave = rest.split(":")
        st[name] = (int(run), None if src == "-" else src, int(wave))
    flags = dict(t.split("=") for t in tail.split())
    return facts, st, flags


def test_planner_with_the_fact_false_is_todays_and_with_it_true_follows_the_rules(tmp_path):
    run = lambda *a: subprocess.run(list(a), capture_output=True, text=True, check=True).stdout
    old = run(_build(tmp_path, "out_chain_check.cpp", "out_chain_check"))
    old_eq = run(_build(tmp_path, "eq_stream_chain_check.cpp", "eq_stream_chain_check"))
    exe = _build(tmp_path, "loud_stream_chain_check.cpp", "loud_stream_chain_check")
    assert run(exe, "base") == old and hashlib.sha256(old.encode()).hexdigest() == TABLE_BEFORE
    assert hashlib.sha256(old_eq.encode()).hexdigest() == EQ_TABLE_BEFORE
    plans = {}
    for ln in run(exe).splitlines():
        f, st, fl = _parse(ln)
        plans[tuple(f[k] for k in "SBRGJELMTD") + (f["ES"], f["LS"])] = (f, st, fl, ln)
    # every admissible combination: whole calls B x (R G J E) x L x (M T D) x (ES LS); streams (B R G J M T D) x (E, ES) in (0,0) (0,1)
    # (1,1) x (L, LS) in (0,0) (0,1) (1,1)
    assert sum(1 for key in plans if not key[0]) == 2 * 2 ** 4 * 3 * 2 ** 3 * 4
    assert sum(1 for key in plans if key[0]) == 2 ** 7 * 3 * 3
    # the older tables, line by line, where both trailing facts are false / only eq_stream is set
    strip = lambda ln: re.sub(r" ES=\d LS=\d", "", re.sub(r" eqws=\d eqst=\d lst=\d", "", ln))
    by_old = {ln.split("|")[0]: ln for ln in old.splitlines()}
    for key, (f, st, fl, ln) in plans.items():
        if key[10] == 0 and key[11] == 0 and strip(ln).split("|")[0] in by_old:
            assert strip(ln) == by_old[strip(ln).split("|")[0]], ln
    for ln in old_eq.splitlines():
        f, st, fl = _parse(ln)
        mine = plans[tuple(f[k] for k in "SBRGJELMTD") + (1, 0)]
        assert (mine[1], {k: v for k, v in mine[2].items() if k != "lst"}) == (st, fl) and mine[2]["lst"] == "0", ln
    measured = 0
    for key, (f, st, fl, ln) in plans.items():
        if not f["LS"]:
            assert fl["lst"] == "0", ln
            continue
        if not (f["S"] and f["L"] == 1):
            # mode 0 in a stream, or any whole call: the switch changes nothing
            other = plans[key[:11] + (0,)]
            assert (st, fl) == (other[1], other[2]), ln
            continue
        measured += 1
        plain = plans[key[:6] + (0,) + key[7:11] + (0,)]       # the same stream without loudness
        want_src = "eq" if f["E"] else "resample" if f["R"] else "join" if f["J"] else "gain" if f["G"] else "tail"
        assert st["loud"] == (1, want_src, 0) and st[want_src][0] == 1 and st[want_src][2] == 1, ln
        for name, v in st.items():
            if name == "loud":
                continue
            pv = plain[1][name]
            assert v == ((pv[0], pv[1], 1) if name == want_src else pv), (name, ln)
        assert fl["lst"] == "1" and fl["lws"] == "0" and fl["loud_cast"] == "0" and fl["gloud"] == "0", ln
        assert {k: v for k, v in fl.items() if k != "lst"} == {k: v for k, v in plain[2].items() if k != "lst"}, ln
        assert st["limit"][1] == plain[1]["limit"][1]
    assert measured == 2 ** 7 * 3


def test_host_row_arithmetic_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "loud_stream_check.cpp", "loud_stream_check", extra=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-400:], r.stderr[-400:])


def test_the_kernels_share_the_whole_calls_device_functions():
    """the stream kernels call ld_scan_staged / ld_tile_sums (ld_chunk, mv4, mpow_apply, the wave loop, the slot tree) -- the arithmetic
    and its order are the same code -- and the host header restates the kernel file's constants"""
    src = open(os.path.join(CSRC, "loudness.hip")).read()
    for k in ("loud_stream_scan_kernel", "loud_stream_measure_kernel"):
        body = src[src.index("void %s(LoudStreamArgs a)" % k):]
        body = body[:body.index("\n}\n")]
        assert "ld_scan_staged(a.k" in body and "lds_stage(" in body, k
    meas = src[src.index("void loud_stream_measure_kernel(LoudStreamArgs a)"):]
    assert "ld_tile_sums(a.k" in meas and "mv4(a.k.Mp[8]" in meas
    whole = src[src.index("void loud_measure_kernel(LoudArgs a)"):src.index("double ld_subblock(")]
    assert "ld_tile_sums(a.k" in whole and "ld_tile_scan(a" in whole
    sums = src[src.index("void ld_tile_sums("):src.index("void loud_measure_kernel(LoudArgs a)")]
    assert "ld_chunk<true>(" in sums and "mpow_apply(k, tid, S)" in sums and "((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]" in sums
    scan = src[src.index("void ld_tile_scan("):src.index("void loud_scan_kernel(LoudArgs a)")]
    assert "ld_scan_staged(a.k" in scan
    hdr = open(os.path.join(CSRC, "loud_stream.hpp")).read()
    assert int(re.search(r"kLdsTile = (\d+)", hdr).group(1)) == T and int(re.search(r"kLdsSlots = (\d+)", hdr).group(1)) == lsr.SLOTS
    assert "asm" not in src
