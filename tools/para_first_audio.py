#!/usr/bin/env python3
"""Time to first audio of a paragraph whose sentences arrive one by one (DESIGN.md 9i "Open paragraphs"), two ways in one process, alternating:

  (a) open_paragraph   sts_para_open; sentence 0 is appended the moment it is available and stepped until its first chunk is on the host;
                       the other sentences are appended one by one, each followed by the steps that have become deliverable; finish; drain
  (b) closed_stream    one sts_infer_ids_joined_stream given all the sentences at once (what a caller without open paragraphs has to do
                       once the last sentence is written)

One full-size synthetic HiFi-GAN model (hifigan_sdp, the configs[1] size), --sentences sentences (default 8) of --phonemes phonemes
(default 32), chunks of --chunk frames (default 32), gaps of 8 frames, a 5 ms fade.  Every repetition uses fresh text (ids no earlier
repetition has seen), after one warm-up of both forms.  Reported, as the median over --reps repetitions (default 20) with the 10th and
90th percentile next to it: the time from "sentence 0 available" to its first chunk on the host through (a); the time to the first chunk
of (b); the time of one step in both (a: around each sts_para_step that delivered, b: between successive chunks), over every delivered
step (with gaps of 8 frames and chunks of 32 none is silent, so these are the steps that decode).  The clock of (a) starts behind
sts_para_open: a service opens its paragraph before any text exists, so the pool's two device allocations and one pinned host allocation
are outside the first-audio figure.  Both forms must deliver the same samples.  Prints one
JSON line; --out FILE writes it there as well.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from summertts_amd import engine, synth_blob as sb  # noqa: E402

GAP, FADE = 8, 5.0


def _open_paragraph(syn, ids, chunk):
    """-> (seconds to the first chunk, per-step seconds, samples)"""
    steps, n = [], 0
    syn.para_open(chunk, len(ids), 1024 * len(ids), 0, FADE)
    try:
        t0 = time.perf_counter()                    # sentence 0 is available
        first = None
        for i, s in enumerate(ids):
            assert syn.para_append([s], gap_frames=[0 if i == 0 else GAP]) is not None
            if i + 1 == len(ids):
                syn.para_finish(0)
            while True:
                ta = time.perf_counter()
                c, ready = syn.para_step()
                tb = time.perf_counter()
                if c is None:
                    break
                if first is None:
                    first = tb - t0
                steps.append(tb - ta)
                n += c[1].size
                if ready == 0:
                    break
    finally:
        syn.para_close()
    return first, steps, n


def _closed_stream(syn, ids, chunk):
    got = []
    t0 = time.perf_counter()
    chunks = syn.infer_joined_stream(ids, chunk, join={"gap_frames": [GAP] * (len(ids) - 1), "fade_ms": FADE},
                                     on_chunk=lambda pcm, off, t: got.append(time.perf_counter()) and False)
    return got[0] - t0, list(np.diff(got)), sum(p.size for _, p in chunks)


def _pct(v):
    v = np.asarray(v, np.float64) * 1e3
    return {"p50_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4), "p90_ms": round(float(np.percentile(v, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=8)
    ap.add_argument("--phonemes", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = sb.full_cfg("hifigan_sdp")
    syn = engine.Synthesizer(sb.make_blob(cfg, 1234))

    def text(rep):
        return [sb.synthetic_ids(a.phonemes, cfg.vocab, salt=1000 * rep + u) for u in range(a.sentences)]

    for form in (_open_paragraph, _closed_stream):      # warm-up of every shape
        form(syn, text(0), a.chunk)
    first = {"open_paragraph": [], "closed_stream": []}
    step = {"open_paragraph": [], "closed_stream": []}
    for rep in range(1, a.reps + 1):
        ids = text(rep)
        order = (_open_paragraph, _closed_stream) if rep % 2 else (_closed_stream, _open_paragraph)
        n = {}
        for form in order:
            name = form.__name__[1:]
            f, s, n[name] = form(syn, ids, a.chunk)
            first[name].append(f); step[name].append(float(np.median(s)))
        assert n["open_paragraph"] == n["closed_stream"], n
    row = {"tool": "para_first_audio", "model": "hifigan_sdp", "sentences": a.sentences, "phonemes": a.phonemes, "chunk_frames": a.chunk, "reps": a.reps,
           "first_audio": {k: _pct(v) for k, v in first.items()}, "step": {k: _pct(v) for k, v in step.items()}}
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    syn.close()


if __name__ == "__main__":
    main()
