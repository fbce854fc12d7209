"""Restatement of a joined stream's step geometry (include/summertts_hip.h sts_infer_ids_joined_stream; summertts_amd/csrc/join_stream.hpp
is the code under test), in Python integers and written from the definition: the layout is tests/join_ref.py's, every sentence is looked
at in every step (no search), and nothing is shared with the header."""
import join_ref as jr


def ceil_div(a, b):
    return -((-a) // b)


def layout_frames(frames, join):
    """-> (first J frame of every sentence, F_J)"""
    start, total, _ = jr.layout(frames, 1, join)
    return [int(s) for s in start], int(total)


def steps(frames, join, hop, C, Hd, Ho, P=1, Q=1, H=0):
    """-> (F_J, workspace frames, J window buffer frames, list of steps); a step is a dict with the chunk frames f, the J window g, the kept
    outputs j, the limiter's widened range jl, and the windows [(b, w0, w1, coff)] with the join's rows [(st, en, S, N, xoff)] in samples"""
    s, FJ = layout_frames(frames, join)
    L_out = ceil_div(FJ * hop * P, Q)
    out, k = [], 0
    while k * C < FJ:
        f0, f1 = k * C, min((k + 1) * C, FJ)
        g0, g1 = max(0, f0 - Ho), min(FJ, f1 + Ho)
        j0, j1 = ceil_div(f0 * hop * P, Q), ceil_div(f1 * hop * P, Q)
        jl0, jl1 = (max(0, j0 - 2 * H), min(L_out, j1 + 2 * H)) if H else (j0, j1)
        win, rows, coff = [], [], 0
        for b, F in enumerate(frames):
            if s[b] < g1 and s[b] + F > g0:                   # the sentence's J frames meet the J window
                w0, w1 = max(0, g0 - s[b] - Hd), min(F, g1 - s[b] + Hd)
                win.append((b, w0, w1, coff))
                rows.append((max(g0, s[b]) * hop, min(g1, s[b] + F) * hop, s[b] * hop, F * hop, (coff - w0) * hop))
                coff += w1 - w0
        out.append(dict(k=k, f=(f0, f1), g=(g0, g1), j=(j0, j1), jl=(jl0, jl1), win=win, rows=rows, Wtot=coff,
                        maxW=max([w[2] - w[1] for w in win], default=0)))
        k += 1
    return FJ, max(t["Wtot"] for t in out), min(FJ, min(C, FJ) + 2 * Ho), out
