"""A stream through the pitch warp without a GPU: the geometry header and the warped step builder as a stand-alone program under
ASan + UBSan, every printed word against the Python-integer restatement of tests/pitch_stream_ref.py; the properties of the geometry
(the chunks partition the output, the warp's input span stays inside the decoded window's interior, the halo is tight and sufficient);
sts_pitch_chunk_starts against the restatement; the symbols, the list, the header and the unchanged ABI number."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pitch_ref as pr
import pitch_stream_ref as ps
from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")
NEW = ["sts_pitch_chunk_starts", "sts_pitch_apply_range", "sts_set_pitch_streaming"]
STS_EINVAL = -1


def test_symbols_are_in_the_library_the_list_and_the_header():
    lib = engine.load_library()
    header = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in engine.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\s*\(", header), s
    assert "typedef struct sts_pitch_range" in header
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18" in header
    assert C.sizeof(engine.Profile) == 200                      # sts_profile did not grow
    assert C.sizeof(engine.PitchRange) == 48
    assert callable(engine.Synthesizer.set_pitch_streaming) and callable(engine.pitch_chunk_starts) and callable(engine.pitch_apply_range)


# ---- the restatement against the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 6, 16])
def test_Y_counts_the_positions_in_front_of_a_frame(hop):
    d = [3, 2, 0, 0, 1, 1, 1, 0, 4, 1, 0, 5]
    cents = [600, -600, 1, -1, 0, 600, 600, 600, -600, 37, 0, -1]
    u = ps.Utt(d, cents, hop)
    pos = pr.positions(d, pr.design(cents)[1], hop)
    assert all(a < b for a, b in zip(pos[:-1], pos[1:]))                     # strictly increasing over the utterance
    assert max(b - a for a, b in zip(pos[:-1], pos[1:])) <= ps.STEP_MAX      # stepped-over phonemes included
    assert [u.pos(j) for j in range(u.Nw)] == pos
    for f in range(u.F + 1):
        assert u.Y(f * hop) == u.Y_slow(f * hop)
    assert u.Y(0) == 0 and u.Y(u.N) == u.Nw
    z = ps.Utt([0, 0, 0], [600, -600, 0], hop)                                # the frame nobody owns: step 2^32
    assert z.Nw == hop and z.Y(hop) == hop and [z.pos(j) for j in range(hop)] == [j << 32 for j in range(hop)]
    p = ps.Utt(d, None, hop)
    assert p.Nw == p.N and p.Y(7 * hop) == 7 * hop


# ---- the program ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program_lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pitch_stream") / "pitch_stream_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "pitch_stream_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-400:], r.stderr[-400:])
    return r.stdout.strip().split("\n")


def _streams(lines):
    """-> list of (call ints, utterances, steps) with steps = [(S ints, [W parts])]"""
    out = []
    for line in lines:
        tag, rest = line[0], line[2:]
        assert tag in "CUSWE", line                                 # ("R reason": the builder refused a step)
        if tag == "C":
            out.append(([int(v) for v in rest.split()], [], []))
        elif tag == "U":
            parts = [p.split() for p in rest.split("|")]
            b, F, zoff, sid, planned, n = [int(v) for v in parts[0]]
            d = [int(v) for v in parts[1]]
            assert len(d) == n
            out[-1][1].append((F, zoff, sid, d, [int(v) for v in parts[2]] if planned else None))
        elif tag == "S":
            out[-1][2].append(([int(v) for v in rest.split()], []))
        elif tag == "W":
            out[-1][2][-1][1].append([[int(v) for v in p.split()] for p in rest.split("|")])
        else:
            assert int(rest) == len(out[-1][2])
    return out


def test_every_word_of_every_step_and_the_properties(program_lines):
    streams = _streams(program_lines)
    assert len(streams) == 3 * 3 * 4 * 2 + 40 + 9
    tight, seen = None, set()
    for call, utts_in, steps in streams:
        hop, Cf, P, Q, H, K, dec_halo, hl, srs, slim, B = call
        assert hl == ps.halo(dec_halo, ps.extra(K if srs else 0, H, P, Q), hop)
        utts = [ps.Utt(d, cents, hop) for (_, _, _, d, cents) in utts_in]
        zoff, sid = [u[1] for u in utts_in], [u[2] for u in utts_in]
        for u, (F, _, _, _, _) in zip(utts, utts_in):
            assert u.F == F
        assert len(steps) == max(-(-u.F // Cf) for u in utts)
        nxt = [0] * B                                               # the chunks partition [0, Nout) in order
        for k, (S, wins) in enumerate(steps):
            live = [b for b in range(B) if k * Cf < utts[b].F]
            rows, tot = ps.step_rows(utts, live, k, Cf, hl, hop, P, Q, H, K, srs, slim, zoff, sid)
            assert S[0] == k and S[1] == len(live) and S[2:9] == tot and S[9] == tot[2], (call, k)
            for i, (w, (ints, rs, lim, prow, seg, g)) in enumerate(zip(wins, rows)):
                assert w[0] == [k, i, live[i]]
                assert w[1:6] == [ints, rs, lim, prow, seg], (call, k, i)
                assert w[6] == [g["j0"], g["j1"] - g["j0"], ints[5]]
                b, u = live[i], utts[live[i]]
                assert g["j0"] == nxt[b] and g["j1"] >= g["j0"]
                nxt[b] = g["j1"]
                assert 0 <= g["yl0"] <= g["yl1"] <= u.Nw and g["yl1"] - g["yl0"] <= min(u.Nw, ps.cap(g["w1"] - g["w0"], hop))
                if g["yl1"] > g["yl0"]:
                    # every staged sample inside the utterance lies dec_halo frames inside the decoded window (an edge of the utterance
                    # needs no margin); how much of the halo is left over, in frames
                    lo = (g["w0"] + dec_halo) * hop if g["w0"] > 0 else 0
                    hi = (g["w1"] - dec_halo) * hop if g["w1"] < u.F else u.N
                    assert lo <= g["c0"] and g["c1"] <= hi, (call, k, i)
                    for slack, edge in ((g["c0"] - lo, g["w0"] > 0), (hi - g["c1"], g["w1"] < u.F)):
                        if edge and u.planned:
                            tight = slack / hop if tight is None else min(tight, slack / hop)
                if not srs and not slim:                             # the warp writes the PCM: what it keeps is what it computes
                    assert (g["yl0"], g["yl1"]) == (g["y0"], g["y1"]) == (g["j0"], g["j1"])
                if g["y1"] == g["y0"]:
                    seen.add("empty")
                    assert Cf * hop == 1                              # a chunk that owns no warped output: only when a chunk is one sample
                if g["j1"] == g["j0"] and P >= Q:
                    assert g["y1"] == g["y0"]                         # (a lower output rate thins the outputs itself)
            for b in live:
                if (k + 1) * Cf >= utts[b].F:
                    assert nxt[b] == ps.out_count(utts[b].Nw, P, Q)
    print(f"least halo left over: {tight:.4f} frames")
    assert tight is not None and 0 <= tight <= 1                    # the bound is attained within one frame and never exceeded
    assert "empty" in seen


def test_a_step_without_the_warp_is_what_it_was(program_lines):
    assert not any(line.startswith("R") for line in program_lines)   # (the program's first check: the warped sections trail the table)


# ---- sts_pitch_chunk_starts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,Cf", [(1, 1), (1, 4), (6, 3), (256, 4), (256, 32), (6, 1000)])
def test_chunk_starts_against_the_restatement(hop, Cf):
    d = [3, 2, 0, 0, 1, 1, 1, 0, 4, 1, 0, 5]
    for cents in ([600, -600, 1, -1, 0, 600, 600, 600, -600, 37, 0, -1], [0] * 12, None):
        u = ps.Utt(d, cents, hop)
        step = None if cents is None else pr.design(cents)[1]
        got = engine.pitch_chunk_starts(d, step, hop, Cf)
        assert got.dtype == np.int64 and got.tolist() == ps.chunk_starts(u, Cf), (hop, Cf, cents)
    z = engine.pitch_chunk_starts([0, 0], pr.design([600, -600])[1], hop, Cf)
    assert z.tolist() == ps.chunk_starts(ps.Utt([0, 0], [600, -600], hop), Cf) and z[-1] == hop


def test_chunk_starts_refusals():
    lib = engine.load_library()
    d, s = np.asarray([3, 4], np.int32), np.asarray([1 << 32, 1 << 32], np.int64)
    out = np.zeros(8, np.int64)

    def call(dd, ss, n, hop, Cf, cap=8):
        return lib.sts_pitch_chunk_starts(dd.ctypes.data, ss.ctypes.data if ss is not None else None, n, hop, Cf, out.ctypes.data, cap)
    assert call(d, s, 2, 16, 2) == 4 and out[:5].tolist() == [0, 32, 64, 96, 112]
    assert call(d, None, 2, 16, 7) == 1 and out[:2].tolist() == [0, 112]
    assert lib.sts_pitch_chunk_starts(d.ctypes.data, s.ctypes.data, 2, 16, 2, None, 0) == 4          # the count alone
    assert call(d, s, 2, 16, 2, 4) == STS_EINVAL                     # room for chunks + 1
    assert call(d, s, 0, 16, 2) == STS_EINVAL and call(d, s, 2, 0, 2) == STS_EINVAL and call(d, s, 2, 16, 0) == STS_EINVAL
    assert call(np.asarray([3, -1], np.int32), s, 2, 16, 2) == STS_EINVAL
    assert call(d, np.asarray([1 << 32, 3037000499], np.int64), 2, 16, 2) == STS_EINVAL
    assert call(np.asarray([1024, 0], np.int32), s, 2, 1 << 20, 2) == STS_EINVAL
