"""Restatement of the tables of one step of a stream (summertts_amd/csrc/stream_step.hpp is the code under test), in Python integers and
written from the documented layout and the window rules: a whole stream is walked step by step, every section of every
step is a list of words, and nothing is shared with the header.  The joined geometry is tests/join_stream_ref.py's."""
import join_stream_ref as jsr

TAIL, GAIN, JOIN, RESAMPLE, PACK, EQ, LOUD, LIMIT = range(8)       # out_chain.hpp OutStage
EQ_TILE = LOUD_TILE = 8192
EQ_HIST = 4096
EQ_ROW, LOUD_ROW, RS_ROW, LIM_ROW, JOIN_ROW = 12, 8, 5, 7, 5      # 8-byte words per row


def ceil_div(a, b):
    return -((-a) // b)


def up8(v):
    return (v + 7) // 8 * 8


def layout(nw, gain, eq, loud, joined):
    """byte offsets of the sections and the table's size: ints [6 nw + 1], then 8-byte aligned the resampler's and the limiter's rows, the
    gain kernel's ints; a plain stream: 8-byte aligned the EQ's rows, 8-byte aligned loudness' rows; a joined stream: 8-byte aligned J's
    resampler row, J's limiter row, the join's rows, J's EQ row, J's loudness row"""
    o = {"ints": 0}
    o["rs"] = up8((6 * nw + 1) * 4)
    o["lim"] = o["rs"] + nw * RS_ROW * 8
    o["utt"] = o["lim"] + nw * LIM_ROW * 8
    end = o["utt"] + (4 * nw if gain else 0)
    if joined:
        o["jrs"] = up8(end)
        o["jlim"] = o["jrs"] + RS_ROW * 8
        o["jrows"] = o["jlim"] + LIM_ROW * 8
        o["eq"] = o["jrows"] + nw * JOIN_ROW * 8
        o["loud"] = o["eq"] + (EQ_ROW * 8 if eq else 0)
        end = o["loud"] + (LOUD_ROW * 8 if loud else 0)
    else:
        o["jrs"] = o["jlim"] = o["jrows"] = 0
        o["eq"] = up8(end)
        if eq:
            end = o["eq"] + nw * EQ_ROW * 8
        o["loud"] = up8(end)
        if loud:
            end = o["loud"] + nw * LOUD_ROW * 8
    o["bytes"] = end
    return o


def sections(nw, gain, eq, loud, joined):
    """[(name, first byte, bytes, word size)] of the sections a step with these flags has, in table order"""
    o = layout(nw, gain, eq, loud, joined)
    nu = 1 if joined else nw
    s = [("ints", 0, (6 * nw + 1) * 4, 4), ("rs", o["rs"], nw * RS_ROW * 8, 8), ("lim", o["lim"], nw * LIM_ROW * 8, 8)]
    if gain:
        s.append(("utt", o["utt"], nw * 4, 4))
    if joined:
        s += [("jrs", o["jrs"], RS_ROW * 8, 8), ("jlim", o["jlim"], LIM_ROW * 8, 8), ("jrows", o["jrows"], nw * JOIN_ROW * 8, 8)]
    if eq:
        s.append(("eq", o["eq"], nu * EQ_ROW * 8, 8))
    if loud:
        s.append(("loud", o["loud"], nu * LOUD_ROW * 8, 8))
    return s


def window(F, f0, C, halo, hop, P, Q, H):
    """the window of chunk frames [f0, min(F, f0 + C)) of an utterance of F frames (live_stream.hpp's comment)"""
    f1 = min(F, f0 + C)
    w0, w1 = max(0, f0 - halo), min(F, f1 + halo)
    j0, j1, Nout = ceil_div(f0 * hop * P, Q), ceil_div(f1 * hop * P, Q), ceil_div(F * hop * P, Q)
    jl0, jl1 = (max(0, j0 - 2 * H), min(Nout, j1 + 2 * H)) if H > 0 else (j0, j1)
    return dict(f1=f1, w0=w0, w1=w1, j0=j0, j1=j1, jl0=jl0, jl1=jl1, Nout=Nout)


def eq_row_check(r, N):
    b, xbase, u0, xlen, o0, o1, ybase, j0, j1, pdst, e, _ = r
    if min(b, xbase, ybase, u0, xlen) < 0:
        return "eq stream: negative geometry"
    if e < 0 or e > o1 or o1 > N:
        return "eq stream: the consumed position lies outside [0, o1], or o1 beyond the utterance"
    if o0 < 0 or o0 > o1:
        return "eq stream: empty or negative output range"
    if u0 > e or u0 + xlen < o1:
        return "eq stream: the window does not hold the input [e, o1)"
    if o0 > e:
        return "eq stream: a gap between the consumed input and the output range"
    if e - o0 > EQ_HIST:
        return "eq stream: the output range reaches further back than the carried history"
    if j0 < o0 or j1 > o1 or j0 > j1 or pdst < 0:
        return "eq stream: the kept range lies outside the output range"
    return None


def loud_row_check(r, N):
    b, xbase, u0, xlen, j1, e, tbase, _ = r
    if min(b, xbase, u0, xlen, tbase) < 0:
        return "loudness stream: negative geometry"
    if e < 0 or e > j1 or j1 > N:
        return "loudness stream: the consumed position lies outside [0, j1], or j1 beyond the utterance"
    if u0 > e or u0 + xlen < j1:
        return "loudness stream: the window does not hold the input [e, j1)"
    return None


class Track:
    """how far every utterance is consumed and which of the two state slots a step reads: a step's rows name their ends, a commit moves
    the positions there and flips the slot if any row was written, a dropped step leaves everything as it was"""

    def __init__(self, n):
        self.e, self.pend, self.slot = [0] * n, {}, 0

    def commit(self):
        for b, v in self.pend.items():
            self.e[b] = v
        self.slot ^= 1 if self.pend else 0
        self.pend = {}

    def drop(self):
        self.pend = {}


def walk(case):
    """-> list of attempts, each a dict of the step's facts and sections, or {"error": (k, text)} as the last entry.  case: form (0 a
    closed stream, 1 an open one, 2 joined), hop C halo P Q H, the flags srs slim seq sld gain mix, lsrc, retry, F f0 zoff sid per
    utterance, and for a joined stream join / Hd / Ho"""
    form, hop, C, halo = case["form"], case["hop"], case["C"], case["halo"]
    srs, slim, seq, sld, gain, mix, lsrc = (case[k] for k in ("srs", "slim", "seq", "sld", "gain", "mix", "lsrc"))
    P, Q = (case["P"], case["Q"]) if srs else (1, 1)
    H = case["H"] if slim else 0
    F, zoff, sid = case["F"], case["zoff"], case["sid"]
    B, joined = len(F), form == 2
    wide = srs or seq
    if joined:
        FJ, _, _, jsteps = jsr.steps(F, case["join"], hop, C, case["Hd"], case["Ho"], P, Q, H)
        lens = [ceil_div(FJ * hop * P, Q)]
    else:
        lens = [ceil_div(f * hop * P, Q) for f in F]
    eqt, ldt = Track(len(lens)), Track(len(lens))
    tbase = [sum(n // LOUD_TILE + 1 for n in lens[:b]) for b in range(len(lens))]
    pos = list(case["f0"])
    out, k, repeated = [], 0, False
    while True:
        t = {"k": k, "attempt": int(repeated and k == case["retry"]), "sec": {}}
        sec = t["sec"]
        err = None
        if joined:
            if k >= len(jsteps):
                break
            js = jsteps[k]
            nw = len(js["win"])
            ints = [[], [], [], [], [0] * nw, [0] * nw + [0]]
            sec["rs"], sec["lim"], sec["utt"], sec["jrows"] = [], [0] * (LIM_ROW * nw), [], []
            for (b, w0, w1, coff), row in zip(js["win"], js["rows"]):
                ints[0].append(zoff[b] + w0); ints[1].append(coff); ints[2].append(w1 - w0); ints[3].append(b if mix else sid[b])
                sec["rs"] += [w0 * hop, F[b] * hop, 0, 0, 0]
                sec["utt"].append(b)
                sec["jrows"] += list(row)
            NJ, Nout = FJ * hop, lens[0]
            (g0, g1), (j0, j1), (jl0, jl1) = js["g"], js["j"], js["jl"]
            u0, ulen, nrs, nout = g0 * hop, (g1 - g0) * hop, jl1 - jl0, j1 - j0
            sec["jrs"] = [u0, NJ, jl0, jl1, 0]
            sec["jlim"] = [0, jl0 if wide else u0, nrs if wide else ulen, Nout, j0, j1, 0]
            etiles = ltiles = 1
            if seq:
                r = [0, 0, jl0 if srs else u0, nrs if srs else ulen, jl0, jl1, 0, j0, j1, 0, eqt.e[0], 0]
                eqt.pend[0] = jl1
                err = err or eq_row_check(r, Nout)
                sec["eq"] = r
                etiles = jl1 // EQ_TILE - r[10] // EQ_TILE + 1
            if sld and not err:
                at_out = lsrc in (EQ, RESAMPLE)
                r = [0, 0, jl0 if at_out else u0, nrs if at_out else ulen, j1, ldt.e[0], tbase[0], 0]
                ldt.pend[0] = j1
                err = loud_row_check(r, Nout)
                sec["loud"] = r
                ltiles = j1 // LOUD_TILE - r[5] // LOUD_TILE + 1
            t.update(nw=nw, Wtot=js["Wtot"], maxW=js["maxW"], zoff0=ints[0][0] if nw else 0, wlen0=ints[2][0] if nw else 0, src0=0,
                     max_rs=nrs, max_out=nout, etiles=etiles, ltiles=ltiles, dsum=nout, chunks=[(j0, nout, 0)])
        else:
            live = [(b, pos[b] if form == 1 else k * C) for b in range(B)]
            live = [(b, f) for b, f in live if f < F[b]]
            nw = len(live)
            if nw == 0:
                break
            ints = [[], [], [], [], [], []]
            for s in ("rs", "lim", "utt", "eq", "loud"):
                sec[s] = []
            Wtot = rsum = dsum = maxW = max_rs = max_out = 0
            etiles = ltiles = 1
            chunks = []
            for b, f0 in live:
                w = window(F[b], f0, C, halo, hop, P, Q, H)
                wlen, nrs, nout = w["w1"] - w["w0"], w["jl1"] - w["jl0"], w["j1"] - w["j0"]
                nat = (Wtot * hop, w["w0"] * hop, wlen * hop)              # the decode window's native samples: place, first, count
                ints[0].append(zoff[b] + w["w0"]); ints[1].append(Wtot); ints[2].append(wlen); ints[3].append(b if mix else sid[b])
                ints[4].append((Wtot + f0 - w["w0"]) * hop); ints[5].append(dsum)
                sec["rs"] += [w["w0"] * hop, F[b] * hop, w["jl0"], w["jl1"], rsum if slim else dsum]
                sec["lim"] += ([rsum, w["jl0"], nrs] if wide else list(nat)) + [w["Nout"], w["j0"], w["j1"], dsum]
                sec["utt"].append(b)
                if seq:
                    r = [b] + ([rsum, w["jl0"], nrs] if srs else list(nat)) + [w["jl0"], w["jl1"], rsum, w["j0"], w["j1"], dsum, eqt.e[b], 0]
                    eqt.pend[b] = w["jl1"]
                    err = eq_row_check(r, w["Nout"])
                    if err:
                        break
                    sec["eq"] += r
                    etiles = max(etiles, w["jl1"] // EQ_TILE - r[10] // EQ_TILE + 1)
                if sld:
                    src = [rsum, w["jl0"], nrs] if lsrc == EQ else [rsum if slim else dsum, w["jl0"], nrs] if lsrc == RESAMPLE else list(nat)
                    r = [b] + src + [w["j1"], ldt.e[b], tbase[b], 0]
                    ldt.pend[b] = w["j1"]
                    err = loud_row_check(r, w["Nout"])
                    if err:
                        break
                    sec["loud"] += r
                    ltiles = max(ltiles, w["j1"] // LOUD_TILE - r[5] // LOUD_TILE + 1)
                chunks.append((w["j0"], nout, dsum))
                rsum += nrs; dsum += nout; Wtot += wlen
                maxW, max_rs, max_out = max(maxW, wlen), max(max_rs, nrs), max(max_out, nout)
            ints[5].append(dsum)
            t.update(nw=nw, Wtot=Wtot, maxW=maxW, zoff0=ints[0][0], wlen0=ints[2][0], src0=ints[4][0], max_rs=max_rs, max_out=max_out,
                     etiles=etiles, ltiles=ltiles, dsum=dsum, chunks=chunks)
        if err:
            out.append({"error": (k, err)})
            break
        sec["ints"] = [v for col in ints for v in col]
        have = {name for name, *_ in sections(nw, gain, seq, sld, joined)}
        t["sec"] = {name: v for name, v in sec.items() if name in have}
        t["off"] = layout(nw, gain, seq, sld, joined)
        t["slots"] = (eqt.slot, ldt.slot)
        out.append(t)
        if k == case["retry"] and not repeated:
            repeated = True
            eqt.drop(); ldt.drop()
            continue
        eqt.commit(); ldt.commit()
        if form == 1:
            for b, _ in live:
                pos[b] += C
        k += 1
    return out
