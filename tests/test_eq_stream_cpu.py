"""CPU suite of the equaliser in a stream (include/summertts_hip.h sts_set_eq_streaming, DESIGN.md 9j "streamed"): the new symbols, the
ABI revision, the ctypes mirror, the switch on null handles; the float64 restatement of the CARRIED-STATE evaluation
(tests/eq_stream_ref.py) against the whole call's scan order (eq_ref.scan) bit for bit -- the evidence that a stream can return the
whole call's bytes for every chunking; the chain planner with the new trailing fact; the host-side row arithmetic (eq_stream.hpp) as
a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eq_ref
import eq_stream_ref
from conftest import ROOT
from summertts_amd import engine

NEW_SYMBOLS = ["sts_set_eq_streaming", "sts_get_eq_streaming", "sts_pool_set_eq_streaming", "sts_eq_apply_chunked"]
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
R, T = eq_ref.R, eq_ref.TILE
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
    of = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for s in NEW_SYMBOLS:
        ret, params = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % s, hdr).groups()
        assert ret == "int"
        want = []
        for p in params.split(","):
            p = p.strip()
            want.append(C.c_void_p if "*" in p else of[p.replace("const ", "").split()[0]])
        assert list(getattr(lib, s).argtypes) == want, s
    for cls in (engine.Synthesizer, engine.Pool):
        assert callable(getattr(cls, "set_eq_streaming"))
    assert callable(engine.Synthesizer.get_eq_streaming) and callable(engine.eq_apply_chunked)


def test_the_switch_on_null_handles_and_its_default(lib):
    """(an engine needs a GPU: tests/test_eq_stream_gpu.py reads the default, sets and gets on one)"""
    assert lib.sts_get_eq_streaming(None) == 0
    assert lib.sts_set_eq_streaming(None, 1) == STS_EINVAL and lib.sts_pool_set_eq_streaming(None, 1) == STS_EINVAL
    src = open(os.path.join(CSRC, "engine.hpp")).read()
    assert re.search(r"bool eq_streaming = false;", src)
    # behind every other member of the engine (the layout of the members in front of it stays what it was)
    body = src[src.index("class Engine {"):]
    assert body.index("bool eq_streaming = false;") > body.index("int run_joined_stream(")
    assert body[body.index("bool eq_streaming = false;"):].strip().endswith("}  // namespace sts")
    assert body[body.index("bool eq_streaming = false;") + len("bool eq_streaming = false;"):].split("}  // namespace sts")[0].strip() == "};"


def test_chunked_entry_refuses_bad_arguments_before_touching_a_device(lib):
    n, arr = engine._eq_bands([(eq_ref.PEAK, 1000.0, 6.0, 2.0)])
    x = np.zeros(100, np.float32)
    lens = np.asarray([100], np.int64)

    def call(bounds, back=0, nb=None, bands=(n, arr)):
        b = np.asarray(bounds, np.int64)
        return lib.sts_eq_apply_chunked(0, x.ctypes.data, lens.ctypes.data, 1, 16000, bands[0], bands[1], b.ctypes.data,
                                        len(bounds) if nb is None else nb, back, None, None, None, 0, None)
    for bounds in ([1, 5], [0, 5, 5], [0, 9, 5]):
        assert call(bounds) == STS_EINVAL, bounds
    assert call([0], nb=0) == STS_EINVAL and call([0], back=-1) == STS_EINVAL and call([0], back=2049) == STS_EINVAL
    assert call([0], bands=(0, None)) == STS_EINVAL
    assert b"eq" in lib.sts_last_error()


# ---- the carried-state restatement against the whole call's order ---------------------------------------------------------------------
N = 2 * T + 37
X = (0.3 * np.random.default_rng(11).standard_normal(N)).astype(np.float32)
STEP_LISTS = {"every sample of the first 70": list(range(0, 71)),
              "chunk and tile edges": [0, R - 1, R, R + 1, 2 * R + 5, T - 1, T, T + 1, 2 * T + 5],
              "one step": [0],
              "steps of 1000": list(range(0, N, 1000))}
_CASES = [(w, S) for w in range(3) for S in range(1, len(eq_ref.FILTER_SETS[w][1]) + 1)]
_scan_cache = {}


def _scan(which, S):
    if (which, S) not in _scan_cache:
        rate, bands = eq_ref.FILTER_SETS[which]
        c = eq_ref.design(rate, bands[:S])
        _scan_cache[(which, S)] = (c, eq_ref.chunk_map_powers(c), eq_ref.scan(X, c))
    return _scan_cache[(which, S)]


def _same_bits(a, b):
    return a.size == b.size and np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("which,S", _CASES)
def test_carried_state_equals_the_scan_bit_for_bit(which, S):
    """the three filter sets of DESIGN.md 9j with their first S sections, noise at amplitude 0.3, N = 2T + 37: every step list, the window
    widened by 0, 7 and 1920 samples -- the assembled signal AND every step's whole window (the re-presented part comes out of the
    carried history)"""
    c, Mp, want = _scan(which, S)
    for name, bounds in STEP_LISTS.items():
        for back in (0, 7, 1920):
            y, wins = eq_stream_ref.chunked(X, c, bounds, back, Mp)
            assert _same_bits(y, want), (which, S, name, back)
            assert len(wins) == len(bounds)
            for a0, w in wins:
                assert _same_bits(w, want[a0:a0 + w.size]), (which, S, name, back, a0)


def test_the_restatement_is_not_the_sequential_carry():
    """what the stream must NOT be: float32 of the scan differs from float32 of the sequential loop on the 48 kHz and 16 kHz sets, so a
    direct-form state carried from chunk to chunk could not return the whole call's bytes"""
    for which in (0, 1):
        rate, bands = eq_ref.FILTER_SETS[which]
        c, _, want = _scan(which, len(bands))
        seq = eq_ref.apply_df1(X[:T + 100], c)
        assert (want[:T + 100].astype(np.float32) != seq.astype(np.float32)).any(), which


def test_a_step_may_reach_back_only_into_the_history_and_consumes_in_order():
    c, Mp, want = _scan(1, 1)
    st = eq_stream_ref.Stream(c, Mp)
    assert _same_bits(st.step(X[:5000], 0, 0, 5000), want[:5000])
    with pytest.raises(AssertionError):
        st.step(X[5001:6000], 5001, 5001, 6000)                     # a gap: the window must hold [e, o1)
    with pytest.raises(AssertionError):
        st.step(X[:6000], 0, 5000 - eq_stream_ref.HIST - 1, 6000)   # further back than the history
    assert _same_bits(st.step(X[4000:T + 7], 4000, 5000 - eq_stream_ref.HIST, T + 7), want[5000 - eq_stream_ref.HIST:T + 7])
    assert st.e == T + 7 and st.xt.size == 7


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
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
    old = subprocess.run([_build(tmp_path, "out_chain_check.cpp", "out_chain_check")], capture_output=True, text=True, check=True).stdout
    exe = _build(tmp_path, "eq_stream_chain_check.cpp", "eq_stream_chain_check")
    base = subprocess.run([exe, "base"], capture_output=True, text=True, check=True).stdout
    assert base == old and len(old.splitlines()) > 100
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 2 * 2 * 2 * 2 * 2 * 2 * 2                   # B x resample x gain x join x limiter x taps x direct
    seen = set()
    for ln in lines:
        f, st, fl = _parse(ln)
        seen.add((f["B"], f["R"], f["G"], f["J"], f["M"], f["T"], f["D"]))
        assert f["S"] == 1 and f["E"] == 1 and f["L"] == 0
        assert st["eq"][0] == 1 and st["eq"][2] == 1 and st["pack"][0] == 0 and st["loud"][0] == 0, ln
        # the EQ reads the nearest running stage in front of it; the limiter reads the EQ
        want_src = "resample" if f["R"] else "join" if f["J"] else "gain" if f["G"] else "tail"
        assert st["eq"][1] == want_src and st[want_src][2] == 1, ln
        assert st["limit"] == ((1, "eq", 0) if f["M"] else (0, None, 0)), ln
        assert fl["writer"] == ("limit" if f["M"] else "eq"), ln
        assert fl["in_place"] == "0" and fl["spack"] == "0" and fl["stab"] == "1" and fl["eqst"] == "1" and fl["eqws"] == "0", ln
        assert fl["pcm_nat"] == "1" and fl["pcm_rs"] == str(f["R"]) and fl["lws"] == "0" and fl["limws"] == "0", ln
    assert len(seen) == 128


def test_host_row_arithmetic_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "eq_stream_check.cpp", "eq_stream_check", extra=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-400:], r.stderr[-400:])


def test_the_kernels_share_the_whole_calls_device_functions():
    """the stream kernels call eq_scan_staged / eq_chunk / eq_mv / eq_mpow -- the arithmetic and its order are the same code -- and the
    host header restates the kernel file's constants"""
    src = open(os.path.join(CSRC, "eq.hip")).read()
    for k in ("eq_stream_scan_kernel", "eq_stream_apply_kernel"):
        body = src[src.index("void %s(EqArgs a)" % k):]
        body = body[:body.index("\n}\n")]
        assert "eq_scan_staged<S>(" in body and "eqs_stage(" in body, k
    apply = src[src.index("void eq_stream_apply_kernel(EqArgs a)"):]
    assert "eq_chunk<S, true>(" in apply and "eq_mpow<S, 8>(" in apply and "eq_mv<S>(k->Mp[8]" in apply
    whole = src[src.index("void eq_tile_scan("):src.index("void eq_load_coef(")]
    assert "eq_scan_staged<S>(" in whole
    hdr = open(os.path.join(CSRC, "eq_stream.hpp")).read()
    assert int(re.search(r"kEqsTile = (\d+)", hdr).group(1)) == T and int(re.search(r"kEqsHist = (\d+)", hdr).group(1)) == eq_stream_ref.HIST
    assert "asm" not in src
