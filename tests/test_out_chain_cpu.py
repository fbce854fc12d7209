"""The output chain's planner (summertts_amd/csrc/out_chain.hpp) on the CPU: tests/out_chain_check.cpp prints its plan for every admissible
combination of a run's facts, and every line is compared with the decisions the engine made before the planner existed, written out
below from those expressions -- nothing here is derived from the header.  Then the structural rules: exactly one writer, which is the
last running stage that can cast; every running stage reads a running stage in front of it."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["tail", "gain", "join", "resample", "pack", "eq", "loud", "limit"]


def _table(S, B, R, G, J, eq, loud_mode, M, T, D):
    """stream, batch size, resample, gain, join, eq set, loudness mode, limit, taps, stream_direct -> the expected line's fields"""
    E = eq and not S
    L1 = loud_mode != 0 and not S
    L2 = loud_mode == 2 and not S
    pack = S and not R and not M and (B > 1 or D)
    run = {"tail": True, "gain": G, "join": J, "resample": R, "pack": pack, "eq": E, "loud": L1, "limit": M}
    writer = "limit" if M else "loud" if L2 else "eq" if E else "resample" if R else "join" if J else "gain" if G else "tail"
    native = "join" if J else "gain" if G else "tail"
    rate = "resample" if R else native
    last = "eq" if E else rate
    src = {"tail": None, "gain": "tail", "join": "gain" if G else "tail", "resample": native, "pack": None, "eq": rate, "loud": last, "limit": last}
    wave = {"tail": T or R or M or L1 or E or G or J, "gain": G, "join": J, "resample": R and (E or L1 or M or (T and not S)), "pack": False,
            "eq": E, "loud": False, "limit": M and not S and T}
    stages = {s: (bool(run[s]), src[s] if run[s] else None, bool(wave[s])) for s in ORDER}
    flags = {"writer": writer, "pcm_nat": writer != "tail", "pcm_rs": R and writer != "resample", "loud_cast": L2 and not M, "no_clamp": M,
             "gloud": L2, "lws": L1, "limws": M and not S, "spack": S and not R and not M and B > 1, "stab": S,
             "in_place": S and B == 1 and not R and not M and not pack}
    return stages, {k: v if k == "writer" else int(bool(v)) for k, v in flags.items()}


def _parse(line):
    facts, stages, flags = (part.split() for part in line.split("|"))
    key = tuple(int(f.split("=")[1]) for f in facts)
    st = {}
    for item in stages:
        name, rest = item.split("=")
        run, src, wave = rest.split(":")
        st[name] = (run == "1", None if src == "-" else src, wave == "1")
    fl = {k: v if k == "writer" else int(v) for k, v in (f.split("=") for f in flags)}
    return key, st, fl


def test_every_admissible_combination_plans_what_the_engine_decided(tmp_path):
    exe = tmp_path / "out_chain_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "summertts_amd", "csrc"),
                    os.path.join(ROOT, "tests", "out_chain_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict((k, (st, fl)) for k, st, fl in map(_parse, r.stdout.splitlines()))
    combos = [c for c in itertools.product((0, 1), (1, 3), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1))]
    assert len(combos) == 1536
    admissible = [c for c in combos if not (c[0] and (c[4] or c[5] or c[6]))]
    assert sorted(got) == sorted(admissible) and len(admissible) == 832
    for c in admissible:
        st, fl = got[c]
        want_st, want_fl = _table(*c)
        assert st == want_st and fl == want_fl, (c, st, want_st, fl, want_fl)
        # structure: one writer, the last running stage that can cast (pack moves int16 samples; loudness casts only when normalising)
        S, loud_mode = c[0], c[6]
        can_cast = [s for s in ORDER if st[s][0] and s != "pack" and (s != "loud" or loud_mode == 2)]
        assert fl["writer"] == can_cast[-1], c
        writers = [s for s in can_cast if s == fl["writer"]]
        assert len(writers) == 1 and fl["loud_cast"] == int(fl["writer"] == "loud"), c
        assert fl["pcm_nat"] == int(fl["writer"] != "tail") and fl["pcm_rs"] == int(st["resample"][0] and fl["writer"] != "resample"), c
        for i, s in enumerate(ORDER):
            run, src, wave = st[s]
            if not run:
                assert src is None and not wave, (c, s)
            elif s not in ("tail", "pack"):
                # its source runs, stands in front of it, and writes the float output it reads
                assert src in ORDER[:i] and st[src][0] and st[src][2], (c, s, src)
