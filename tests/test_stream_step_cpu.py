"""The tables of a stream's steps without a GPU: summertts_amd/csrc/stream_step.hpp, compiled into tests/stream_step_check.cpp under the
sanitizers, walks whole streams (closed, open, joined; every step committed, one step run twice); every word of every table, the launch
dimensions and the delivery lists against the restatement of tests/stream_step_ref.py, and the invariants the kernels rely on, checked
on the program's output alone."""
import itertools
import os
import subprocess

import pytest

import join_stream_ref as jsr
import stream_step_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")

CHUNKS = (1, 7, 64)
HALO, HD, HO = 3, 2, 3                    # (a joined stream: the halo is the output side's reach Ho, in front of a decoder halo of 2 frames)
HOPS = (4, 256)
RATES = ((1, 1), (1, 2), (3, 1), (441, 160))
LIMITER_H = (0, 5)
FORMS = ("one", "batch", "open", "joined")


def _form(name, C):
    """-> form number, F, f0, zoff, sid, join"""
    if name == "one":
        return 0, (23,), (0,), (0,), (4,), None
    if name == "batch":            # windows drop out: nw changes between steps
        return 0, (5, 23, 64), (0, 0, 0), (0, 5, 28), (3, 0, 5), None
    if name == "open":             # slots at frames 0, 7 and 14 of their utterances, anywhere in the pool
        return 1, (23, 64, 9), (0, 7, 14), (100, 0, 300), (3, 0, 5), None
    # a lead, a gap longer than a chunk and the reach on both sides (a step without a window), a short gap, a trail
    return 2, (5, 23, 64), (0, 0, 0), (0, 5, 28), (3, 0, 5), {"lead_frames": 2, "gap_frames": [C + 2 * (HO + HD) + 1, 1], "trail_frames": 1}


def _cases():
    seen = set()
    for name, C, hop, (P, Q), H in itertools.product(FORMS, CHUNKS, HOPS, RATES, LIMITER_H):
        for srs, slim, seq, sld, gain in itertools.product((0, 1), repeat=5):
            # (without the resampler the ratio is 1 / 1 and without the limiter H is 0, whatever the call has set: one case each)
            key = (name, C, hop, (P, Q) if srs else (1, 1), H if slim else 0, srs, slim, seq, sld, gain)
            if key in seen:
                continue
            seen.add(key)
            form, F, f0, zoff, sid, join = _form(name, C)
            steps = -(-jsr.layout_frames(F, join)[1] // C) if form == 2 else max(-(-(f - a) // C) for f, a in zip(F, f0))
            yield dict(name=name, form=form, hop=hop, C=C, halo=HALO, P=P, Q=Q, H=H, srs=srs, slim=slim, seq=seq, sld=sld, gain=gain,
                       mix=srs ^ gain, retry=min(1, steps - 1), F=F, f0=f0, zoff=zoff, sid=sid, join=join, Hd=HD, Ho=HO)


def _line(c):
    v = [c[k] for k in ("form", "hop", "C", "halo", "P", "Q", "H", "srs", "slim", "seq", "sld", "gain", "mix", "retry")]
    v += [len(c["F"]), *c["F"], *c["f0"], *c["zoff"], *c["sid"]]
    if c["form"] == 2:
        start, FJ = jsr.layout_frames(c["F"], c["join"])
        v += [start[b] - sum(c["F"][:b]) for b in range(len(c["F"]))] + [FJ - sum(c["F"]), c["Hd"], c["Ho"]]
    return " ".join(str(x) for x in v)


STEP_KEYS = ("k", "attempt", "nw", "Wtot", "maxW", "zoff0", "wlen0", "src0", "max_rs", "max_out", "etiles", "ltiles", "dsum", "bytes", "eslot", "lslot")
OFF_KEYS = ("rs", "lim", "utt", "jrs", "jlim", "jrows", "eq", "loud")


def _parse(lines, i):
    """one case's lines -> (lsrc, attempts, next line)"""
    head = lines[i].split(); i += 1
    assert head[0] == "case", lines[i - 1]
    got = []
    while lines[i] != "end":
        w = lines[i].split(); i += 1
        if w[0] == "error":
            got.append({"error": (int(w[1]), " ".join(w[2:]))})
        elif w[0] == "step":
            got.append(dict(zip(STEP_KEYS, (int(x) for x in w[1:])), sec={}))
        elif w[0] == "off":
            got[-1]["off"] = dict(zip(OFF_KEYS, (int(x) for x in w[1:])))
        elif w[0] == "chunks":
            v = [int(x) for x in w[1:]]
            got[-1]["chunks"] = [tuple(v[q:q + 3]) for q in range(0, len(v), 3)]
        else:
            got[-1]["sec"][w[0]] = [int(x) for x in w[1:]]
    return int(head[1]), got, i + 1


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_step") / "stream_step_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "stream_step_check.cpp"), "-o", str(exe)], check=True)
    cases = list(_cases())
    r = subprocess.run([str(exe)], input="\n".join(_line(c) for c in cases) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, i, out = r.stdout.split("\n"), 0, []
    for c in cases:
        lsrc, got, i = _parse(lines, i)
        out.append((c, lsrc, got))
    assert lines[i:] == [""]
    return out


def test_the_cases_cross_every_flag_with_every_form(walked):
    n = {}
    for c, _, _ in walked:
        n.setdefault((c["name"], c["C"], c["hop"]), set()).add((c["srs"], c["slim"], c["seq"], c["sld"], c["gain"]))
    assert len(n) == len(FORMS) * len(CHUNKS) * len(HOPS) and all(len(v) == 32 for v in n.values())
    full = [c for c, _, _ in walked if c["srs"] and c["slim"]]
    assert {(c["P"], c["Q"]) for c in full} == set(RATES) and {c["H"] for c in full} == set(LIMITER_H)
    # the stage loudness reads is the chain's: the nearest running stage with a float output in front of it
    for c, lsrc, _ in walked:
        want = ssr.EQ if c["seq"] else ssr.RESAMPLE if c["srs"] else ssr.JOIN if c["form"] == 2 else ssr.GAIN if c["gain"] else ssr.TAIL
        assert lsrc == (want if c["sld"] else -1), c
    assert {lsrc for _, lsrc, _ in walked} >= {ssr.TAIL, ssr.RESAMPLE, ssr.EQ}


def test_every_word_of_every_step_is_the_restatement(walked):
    steps = silent = repeats = refused = 0
    for c, lsrc, got in walked:
        want = ssr.walk(dict(c, lsrc=lsrc))
        assert len(got) == len(want), c
        for g, w in zip(got, want):
            if "error" in w or "error" in g:
                assert g.get("error") == w.get("error"), c
                refused += 1
                continue
            tag = (c, w["k"])
            for key in ("k", "attempt", "nw", "Wtot", "maxW", "zoff0", "wlen0", "src0", "max_rs", "max_out", "etiles", "ltiles", "dsum"):
                assert g[key] == w[key], (tag, key)
            assert g["bytes"] == w["off"]["bytes"] and g["off"] == {k: w["off"][k] for k in OFF_KEYS}, tag
            assert (g["eslot"], g["lslot"]) == w["slots"] and g["chunks"] == w["chunks"], tag
            assert g["sec"] == w["sec"], tag
            steps += 1
            silent += c["form"] == 2 and g["nw"] == 0
            repeats += g["attempt"]
    # an open stream's slot that starts inside its utterance has no carried state to start from: the row checks refuse it, in the first step
    for c, _, got in walked:
        assert ("error" in got[-1]) == (c["form"] == 1 and bool(c["seq"] or c["sld"])), c
        assert "error" not in got[-1] or got[-1]["error"][0] == 0
    assert repeats == len(walked) - refused and steps > 20000 and silent > 500


def test_the_tables_keep_what_the_kernels_rely_on(walked):
    for c, lsrc, got in walked:
        P, Q = (c["P"], c["Q"]) if c["srs"] else (1, 1)
        joined, wide, hop = c["form"] == 2, bool(c["srs"] or c["seq"]), c["hop"]
        for g in got:
            if "error" in g:
                continue
            tag, nw, sec = (c, g["k"]), g["nw"], g["sec"]
            # sections in table order: inside the table, not overlapping, aligned to their words
            want = [name for name, *_ in ssr.sections(nw, c["gain"], c["seq"], c["sld"], joined)]
            assert list(sec) == want, tag
            end = 0
            for name in want:
                size = 4 if name in ("ints", "utt") else 8
                first = 0 if name == "ints" else g["off"][name]
                assert first >= end and first % size == 0, (tag, name)
                end = first + len(sec[name]) * size
            assert end == g["bytes"], tag
            # the packed destinations partition [0, dsum) in window order
            at = 0
            for j0, n, dst in g["chunks"]:
                assert dst == at and n >= 0, tag
                at += n
            assert at == g["dsum"] and len(g["chunks"]) == (1 if joined else nw), tag
            ints = sec["ints"]
            assert ints[5 * nw:] == ([0] * (nw + 1) if joined else [d for _, _, d in g["chunks"]] + [g["dsum"]]), tag
            rs = [sec["rs"][5 * i:5 * i + 5] for i in range(nw)] + ([sec["jrs"]] if joined else [])
            lim = [sec["lim"][7 * i:7 * i + 7] for i in range(nw)] + ([sec["jlim"]] if joined else [])
            for u0, L, j0, j1, obase in rs:
                assert 0 <= j0 <= j1 <= -(-L * P // Q) and 0 <= u0 <= L and obase >= 0, tag
            # what the limiter reads lies inside what the stage in front of it packed: the resampler's (the EQ's) outputs of the output
            # side's windows, else the decoded windows (a joined stream: the J window buffer)
            out_rs = rs[nw:] if joined else rs
            if wide:
                extent = sum(r[3] - r[2] for r in out_rs)
            else:
                extent = min(jsr.layout_frames(c["F"], c["join"])[1], c["C"] + 2 * c["Ho"]) * hop if joined else g["Wtot"] * hop
            for xbase, u0, xlen, N, j0, j1, dst in lim:
                assert xbase >= 0 and xlen >= 0 and xbase + xlen <= extent and 0 <= j0 <= j1 <= N, tag
            out_lim = lim[nw:] if joined else lim
            for i, m in enumerate(out_lim):
                if c["seq"]:
                    assert ssr.eq_row_check(sec["eq"][12 * i:12 * i + 12], m[3]) is None, tag
                if c["sld"]:
                    assert ssr.loud_row_check(sec["loud"][8 * i:8 * i + 8], m[3]) is None, tag
