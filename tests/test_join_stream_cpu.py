"""A joined stream (sts_infer_ids_joined_stream, sts_join_apply_range) without a GPU: the exports; the step geometry of
summertts_amd/csrc/join_stream.hpp, compiled into tests/join_stream_check.cpp, against the restatement of tests/join_stream_ref.py and
against invariants checked by brute force; the output chain of the 64 streaming joined combinations against a table written out here."""
import itertools
import os
import subprocess

import pytest

import join_ref as jr
import join_stream_ref as jsr
import resample_ref as rr
from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summertts_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("join_stream") / "join_stream_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "join_stream_check.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_both_symbols_are_exported_and_declared():
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    for s in ("sts_infer_ids_joined_stream", "sts_join_apply_range"):
        assert hasattr(lib, s) and s in engine.EXPORTED_SYMBOLS and ("int %s(" % s) in hdr, s
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18\n" in hdr
    assert "Out of scope: a streaming form" not in hdr
    assert hasattr(engine.Synthesizer, "infer_joined_stream") and hasattr(engine, "join_apply_range")


# ---- step geometry -------------------------------------------------------------------------------------------------------------------------
SENTENCES = ((1, 3, 7, 12), (40, 9, 55), (1,) * 7)
HALOS = ((3, 0), (3, 2), (11, 5))                   # (Hd, Ho)
RATES = (16000, 8000, 44100)
LIMITER_H = (0, 16)


def _joins(B, C, Hd, Ho):
    """gap 0 next to gap 3; a gap longer than C + 2 (Ho + Hd) (at most the 100000 frames a join admits); lead only; trail only"""
    long_gap = min(jr.MAX_FRAMES, C + 2 * (Ho + Hd) + 1)
    return ({"gap_frames": [(0, 3)[b % 2] for b in range(B - 1)], "lead_frames": 2, "trail_frames": 1},
            {"gap_frames": [long_gap if b == 0 else 1 for b in range(B - 1)]},
            {"lead_frames": 5}, {"trail_frames": 4}, None)


def _reach(rate, H):
    """native samples a kept output needs beyond its own position: the resampler's K and the limiter's 2H outputs (Engine::stream_halo)"""
    P, Q, K = rr.design(rate)[:3]
    native = rate == rr.NATIVE
    return (0 if native else K) + ((-(-2 * H * Q // P) + 1) if H else 0)


def _hop(rate, H, Ho):
    """the smallest multiple of 4 at which Ho frames cover the reach (Ho == 0: any; such a case is consistent only with no reach at all)"""
    need = _reach(rate, H)
    return 4 if Ho == 0 or need == 0 else 4 * -(-need // (4 * Ho))


def _cases():
    for frames, (Hd, Ho), rate, H in itertools.product(SENTENCES, HALOS, RATES, LIMITER_H):
        halo = Hd + Ho
        for C in (1, 7, halo, 3 * halo + 1, 100000):
            for join in _joins(len(frames), C, Hd, Ho):
                P, Q = rr.design(rate)[:2]
                yield dict(frames=frames, join=join, hop=_hop(rate, H, Ho), C=C, Hd=Hd, Ho=Ho, P=P, Q=Q, H=H, rate=rate)


def _run(checker, cases):
    lines = []
    for c in cases:
        start, FJ = jsr.layout_frames(c["frames"], c["join"])
        sil = [start[b] - sum(c["frames"][:b]) for b in range(len(c["frames"]))]
        lines.append(" ".join(str(v) for v in [c["hop"], c["C"], c["Hd"], c["Ho"], c["P"], c["Q"], c["H"], len(c["frames"]), *c["frames"], *sil,
                                               FJ - sum(c["frames"])]))
    out = subprocess.run([checker, "steps"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got, i = [], 0
    for c in cases:
        head = out[i].split(); i += 1
        assert head[0] == "case", out[i - 1]
        FJ, n, work, wf = (int(v) for v in head[1:])
        steps = []
        for _ in range(n):
            v = [int(x) for x in out[i].split()]; i += 1
            nw = v[11]
            w = [tuple(v[12 + 9 * q:12 + 9 * q + 9]) for q in range(nw)]
            steps.append(dict(k=v[0], f=(v[1], v[2]), g=(v[3], v[4]), j=(v[5], v[6]), jl=(v[7], v[8]), Wtot=v[9], maxW=v[10],
                              win=[x[:4] for x in w], rows=[x[4:] for x in w]))
        got.append((FJ, work, wf, steps))
    return got


def test_step_geometry_is_the_restatement_and_keeps_its_invariants(checker):
    cases = list(_cases())
    got = _run(checker, cases)
    assert len(cases) == len(SENTENCES) * len(HALOS) * len(RATES) * len(LIMITER_H) * 5 * 5
    checked_reach = silent_steps = 0
    for c, (FJ, work, wf, steps) in zip(cases, got):
        frames, hop, C, Hd, Ho, P, Q, H = (c[k] for k in ("frames", "hop", "C", "Hd", "Ho", "P", "Q", "H"))
        want = jsr.steps(frames, c["join"], hop, C, Hd, Ho, P, Q, H)
        tag = {k: v for k, v in c.items()}
        assert (FJ, work, wf) == want[:3], tag
        assert steps == want[3], tag
        # ---- invariants, by brute force
        s, _ = jsr.layout_frames(frames, c["join"])
        NJ = FJ * hop
        L_out = -(-NJ * P // Q)
        assert len(steps) == -(-FJ // C)
        occupied = [False] * FJ
        for b, F in enumerate(frames):
            for f in range(s[b], s[b] + F):
                occupied[f] = True
        pos = 0
        consistent = Ho * hop >= _reach(c["rate"], H)
        for t in steps:
            # the kept output ranges tile [0, L_out) exactly once, in order
            assert t["j"][0] == pos and t["j"][1] >= pos, tag
            pos = t["j"][1]
            g0, g1 = t["g"]
            assert 0 <= g0 <= t["f"][0] < t["f"][1] <= g1 <= FJ and g1 - g0 <= wf, tag
            # silence-only steps have zero windows, every other step at least one
            assert bool(t["win"]) == any(occupied[g0:g1]), tag
            silent_steps += not t["win"]
            total = 0
            for (b, w0, w1, coff), (st, en, S, N, xoff) in zip(t["win"], t["rows"]):
                F = frames[b]
                assert 0 <= w0 < w1 <= F and coff == total, tag                    # inside its sentence, packed in sentence order
                total += w1 - w0
                a, e = max(g0, s[b]) - s[b], min(g1, s[b] + F) - s[b]              # the sentence's frames inside the J window
                assert a < e and (w0 == 0 or a - w0 >= Hd) and (w1 == F or w1 - e >= Hd), tag
                # the row reads only what the window decoded
                assert coff * hop <= xoff + (st - S) and xoff + (en - S) <= (coff + w1 - w0) * hop, tag
            assert total == t["Wtot"] <= work, tag                                 # the workspace bound holds at every step
            if consistent:
                # every J sample a kept output reads lies inside the J window: the limiter reads the float outputs [jl0, jl1), each of
                # which is the native sample itself or, resampled, the samples [floor(j Q / P) - K + 1, floor(j Q / P) + K] of [0, N_J)
                jl0, jl1 = t["jl"]
                want_jl = (max(0, t["j"][0] - 2 * H), min(L_out, t["j"][1] + 2 * H))
                assert (jl0, jl1) == want_jl, tag
                if jl1 > jl0:
                    K = 0 if c["rate"] == rr.NATIVE else rr.design(c["rate"])[2]
                    # (every output of a short range; of a long one -- the 100000-frame chunks -- its ends and a stride: both bounds ascend with j)
                    js = range(jl0, jl1) if jl1 - jl0 <= 4096 else [*range(jl0, jl1, 997), jl1 - 1]
                    lo = min(max(0, (j * Q) // P - (K - 1 if K else 0)) for j in js)
                    hi = max(min(NJ - 1, (j * Q) // P + K) for j in js)
                    assert g0 * hop <= lo and hi < g1 * hop, (tag, t["k"], lo, hi)
                    checked_reach += 1
        assert pos == L_out, tag
        assert max(t["Wtot"] for t in steps) == work, tag
    assert checked_reach > 10000 and silent_steps > 1000


# ---- the output chain ------------------------------------------------------------------------------------------------------------------
# (R, G, M) -> the plan's line behind the facts; B, the taps and stream_direct change nothing in a joined stream
PLANS = {
    (0, 0, 0): "tail=1:-:1 gain=0:-:0 join=1:tail:1 resample=0:-:0 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=0:-:0 | writer=join pcm_nat=1 pcm_rs=0 "
               "loud_cast=0 no_clamp=0 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (0, 0, 1): "tail=1:-:1 gain=0:-:0 join=1:tail:1 resample=0:-:0 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=1:join:0 | writer=limit pcm_nat=1 pcm_rs=0 "
               "loud_cast=0 no_clamp=1 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (0, 1, 0): "tail=1:-:1 gain=1:tail:1 join=1:gain:1 resample=0:-:0 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=0:-:0 | writer=join pcm_nat=1 pcm_rs=0 "
               "loud_cast=0 no_clamp=0 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (0, 1, 1): "tail=1:-:1 gain=1:tail:1 join=1:gain:1 resample=0:-:0 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=1:join:0 | writer=limit pcm_nat=1 pcm_rs=0 "
               "loud_cast=0 no_clamp=1 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (1, 0, 0): "tail=1:-:1 gain=0:-:0 join=1:tail:1 resample=1:join:0 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=0:-:0 | writer=resample pcm_nat=1 pcm_rs=0 "
               "loud_cast=0 no_clamp=0 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (1, 0, 1): "tail=1:-:1 gain=0:-:0 join=1:tail:1 resample=1:join:1 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=1:resample:0 | writer=limit pcm_nat=1 pcm_rs=1 "
               "loud_cast=0 no_clamp=1 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (1, 1, 0): "tail=1:-:1 gain=1:tail:1 join=1:gain:1 resample=1:join:0 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=0:-:0 | writer=resample pcm_nat=1 pcm_rs=0 "
               "loud_cast=0 no_clamp=0 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
    (1, 1, 1): "tail=1:-:1 gain=1:tail:1 join=1:gain:1 resample=1:join:1 pack=0:-:0 eq=0:-:0 loud=0:-:0 limit=1:resample:0 | writer=limit pcm_nat=1 pcm_rs=1 "
               "loud_cast=0 no_clamp=1 gloud=0 lws=0 limws=0 spack=0 stab=1 in_place=0",
}
ORDER = ["tail", "gain", "join", "resample", "pack", "eq", "loud", "limit"]
CASTS = ("tail", "gain", "join", "resample", "eq", "loud", "limit")          # (pack moves int16 samples; it writes no cast of its own)


def test_the_output_chain_of_a_joined_stream(checker):
    lines = subprocess.run([checker, "plan"], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(lines) == 64 and len(set(lines)) == 64
    seen = set()
    for line in lines:
        facts, rest = line.split(" |", 1)
        f = dict(kv.split("=") for kv in facts.split())
        assert f["S"] == "1" and f["J"] == "1" and f["E"] == "0" and f["L"] == "0"
        seen.add(facts)
        assert rest.strip() == PLANS[(int(f["R"]), int(f["G"]), int(f["M"]))], line
        # the structural rules of tests/test_out_chain_cpu.py: one writer, and it is the last running stage that can cast
        stages, tail = rest.strip().split(" | ")
        run = {kv.split("=")[0]: kv.split("=")[1].split(":")[0] == "1" for kv in stages.split()}
        writer = dict(kv.split("=") for kv in tail.split())["writer"]
        assert writer == [s for s in ORDER if run[s] and s in CASTS][-1] and not run["pack"], line
    assert len(seen) == 64
