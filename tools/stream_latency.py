#!/usr/bin/env python3
"""Time to first audio of N clients that each want their utterance streamed, three ways in one process:

  (a) batched   one sts_infer_ids_batch_stream over the B utterances (chunk k of every utterance per step)
  (b) serial    B sts_infer_ids_stream calls one after another on the same engine
  (c) batch     one sts_infer_ids_batch of the B utterances (everyone hears the whole utterance at the end)

Full-size synthetic HiFi-GAN (hifigan_sdp) and MB-iSTFT (mbb_fix) models, 128-phoneme utterances (the configs[1] shape, one
distinct utterance per client), B in {1, 8, 32}, chunks of 32 and 64 frames.  Per (model, B, chunk, form): time to first chunk over
the utterances (min / p50 / max), time to the last chunk, and seconds of audio delivered per wall second; the median of --reps
timed repeats after one warm-up of every shape.  The launch-ahead memo is off, so (c) waits for its frame counts as (a) and (b) do.
--rate R: PCM at R Hz (sts_set_output_rate).  --direct 1: the batched stream's step output goes to mapped pinned memory (sts_debug_set STS_DBG_STREAM_DIRECT) instead of one
download.  --eq 1: the 4-band equaliser of DESIGN.md 9j's cost table on every call, streamed from its carried state
(sts_set_eq_streaming); --eq 0 (default) sets neither bands nor the switch.  --loud 1: every call measures its loudness (sts_set_loudness
mode 1), the streams from their carried state (sts_set_loudness_streaming; DESIGN.md 9d "streamed"); --loud 0 (default) sets neither the
mode nor the switch.  Prints one JSON line per row.

--joined: a paragraph instead -- --sentences sentences (default 32) of 64 to 256 phonemes joined with gaps of 8 frames and
a 5 ms fade, three ways:
  (a) joined_stream   one sts_infer_ids_joined_stream (chunks of the ONE joined signal, in order)
  (b) serial_streams  the sentences as sts_infer_ids_stream calls one after another (no batch for the front and the flow, no join)
  (c) whole_joined    one sts_infer_ids_joined (the reader hears the paragraph when all of it is done)
Per (model, chunk, form): time to the first and to the last chunk, seconds of audio per wall second.

--late: a late arrival at a pool of one engine (DESIGN.md 9c "Open streams") -- --clients clients (default 32) whose streaming requests
are queued together and run as one group, and one more client that submits its request when the group's second step has delivered.  Two
legs: admission off (the group is a closed stream: the late client waits until it has drained) and on (sts_pool_set_stream_admission: the
late client is admitted between two steps).  Per leg: the late client's time from submit to its first chunk, the group's first-chunk
times, and the group's last-chunk time with and without the late client.  A library without the switch (an older build) runs the off leg
only.  --plans: the late client and every second member of the group carry a duration plan, a gain plan and (a multi-speaker model) a
speaker mix (sts_pool_submit_stream_ex): the planned late client.  --eq: the pool of every leg runs the 4-band EQ, streamed -- with
admission on the group is an open stream with per-slot EQ state.
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


def _batched(syn, ids, chunk):
    t0 = time.perf_counter()
    chunks, times = syn.infer_batch_stream(ids, chunk)
    wall = time.perf_counter() - t0
    first = [t[0] for t in times]
    return first, max(t[-1] for t in times), sum(sum(c.size for c in cs) for cs in chunks), wall


def _serial(syn, ids, chunk):
    first, last, n = [], 0.0, 0
    t0 = time.perf_counter()
    for x in ids:
        got = []
        chunks, _ = syn.infer_ids_stream(x, chunk, on_chunk=lambda pcm, off, t: got.append(time.perf_counter() - t0) and False)
        first.append(got[0]); last = got[-1]
        n += sum(c.size for c in chunks)
    return first, last, n, time.perf_counter() - t0


def _batch(syn, ids, chunk):
    t0 = time.perf_counter()
    pcm = syn.infer_batch(ids)
    t = time.perf_counter() - t0
    return [t] * len(ids), t, sum(p.size for p in pcm), t


# DESIGN.md 9j's cost table: HP 100 Hz; peak 1 kHz +6 dB q 2; low shelf 300 Hz -6 dB; peak 3 kHz -9 dB q 4 (valid from 8 kHz up)
EQ_BANDS = [(engine.EQ_HIGHPASS, 100.0, 0.0, 0.707), (engine.EQ_PEAK, 1000.0, 6.0, 2.0), (engine.EQ_LOWSHELF, 300.0, -6.0, 0.7),
            (engine.EQ_PEAK, 3000.0, -9.0, 4.0)]
JOIN = {"lead_frames": 0, "trail_frames": 0, "fade_ms": 5.0}


def _paragraph(cfg, n):
    lens = [64 + (97 * u * u + 31 * u) % 193 for u in range(n)]               # 64 .. 256 phonemes
    return [sb.synthetic_ids(t, cfg.vocab, salt=u) for u, t in enumerate(lens)]


def _joined_stream(syn, ids, chunk):
    got = []
    t0 = time.perf_counter()
    chunks = syn.infer_joined_stream(ids, chunk, join=dict(JOIN, gap_frames=[8] * (len(ids) - 1)),
                                     on_chunk=lambda pcm, off, t: got.append(time.perf_counter() - t0) and False)
    return [got[0]], got[-1], sum(p.size for _, p in chunks), time.perf_counter() - t0


def _whole_joined(syn, ids, chunk):
    t0 = time.perf_counter()
    pcm = syn.infer_joined(ids, join=dict(JOIN, gap_frames=[8] * (len(ids) - 1)))
    t = time.perf_counter() - t0
    return [t], t, pcm.size, t


def _tables(cfg, n):
    """--plans: one request's tables of all three kinds -- a rate span, a -6 dB span with 5 ms ramps, and (a multi-speaker model) a blend
    of two table rows -- as Pool.submit_stream takes them"""
    rate = np.ones(n, np.float32)
    rate[n // 4:n // 2] = 1.1
    db = np.zeros(n, np.float32)
    db[n // 2:3 * n // 4] = -6.0
    t = {"plan": {"rate": rate}, "gain": {"gain_db": db, "ramp_ms": 5.0}}
    if cfg.is_ms:
        t["mix"] = {"sid": [0, int(cfg.spk_num) - 1], "weight": [0.7, 0.3]}
    return t


def _late_run(pool, ids, late_ids, chunk, with_late, tables=None):
    """one group of len(ids) streaming requests queued together behind a gate request, the late one submitted from client 0's second chunk.
    tables: the late client and every second member of the group carry them (sts_pool_submit_stream_ex)"""
    import threading
    gate_in, gate_go = threading.Event(), threading.Event()
    t0 = [0.0]
    first = [None] * len(ids)
    last = [0.0] * len(ids)
    late = {"submit": None, "first": None, "last": None, "ticket": None}
    seen0 = [0]

    def on_gate(pcm, off):          # holds the one worker until every client is queued, then stops: the group is what is queued
        gate_in.set()
        gate_go.wait(60.0)
        return True

    def on_late(pcm, off):
        t = time.perf_counter()
        if late["first"] is None:
            late["first"] = t
        late["last"] = t
        return False

    def client(i):
        def cb(pcm, off):
            t = time.perf_counter()
            if first[i] is None:
                first[i] = t
            last[i] = t
            if i == 0 and with_late:
                seen0[0] += 1
                if seen0[0] == 2:          # the group's second step has delivered
                    late["submit"] = time.perf_counter()
                    late["ticket"] = pool.submit_stream(late_ids, chunk, on_late, **(tables or {}))
            return False
        return cb
    tg = pool.submit_stream(ids[0][:8], chunk + 1, on_gate)
    gate_in.wait(60.0)
    tickets = [pool.submit_stream(x, chunk, client(i), **((tables or {}) if i % 2 else {})) for i, x in enumerate(ids)]
    t0[0] = time.perf_counter()
    gate_go.set()
    pool.wait(tg)
    for t in tickets:
        pool.wait(t)
    out = {"group_first_ms_min": (min(first) - t0[0]) * 1e3, "group_first_ms_max": (max(first) - t0[0]) * 1e3,
           "group_last_ms": (max(last) - t0[0]) * 1e3}
    if with_late:
        pool.wait(late["ticket"])
        out["late_first_ms"] = (late["first"] - late["submit"]) * 1e3
        out["late_last_ms"] = (late["last"] - late["submit"]) * 1e3
        out["late_first_before_group_last"] = bool(late["first"] < max(last))
    return out


def _late(a) -> None:
    kind = a.models.split(",")[0]
    cfg = sb.full_cfg(kind)
    blob = sb.make_blob(cfg, 1234)
    chunk = int(a.chunks.split(",")[0])
    ids = [sb.synthetic_ids(a.phonemes, cfg.vocab, salt=u) for u in range(a.clients)]
    late_ids = sb.synthetic_ids(a.phonemes, cfg.vocab, salt=a.clients)
    tables = _tables(cfg, a.phonemes) if a.plans else None
    for admission in (False, True):
        pool = engine.Pool(blob, device=0, n_engines=1, max_batch=2 * a.clients)
        if a.eq:        # the audio profile on every leg, streamed: with admission on the group runs as an open stream with per-slot EQ state
            pool.set_eq(EQ_BANDS)
            pool.set_eq_streaming(True)
        if admission:
            if not hasattr(pool, "set_stream_admission"):
                pool.close()
                break
            pool.set_stream_admission(True)
        for with_late in (False, True):
            _late_run(pool, ids, late_ids, chunk, with_late, tables)          # warm-up of this shape
            runs = [_late_run(pool, ids, late_ids, chunk, with_late, tables) for _ in range(a.reps)]
            row = {"model": kind, "scenario": "late_arrival", "admission": admission, "late_client": with_late, "plans": bool(a.plans), "eq": bool(a.eq), "clients": a.clients,
                   "chunk_frames": chunk, "phonemes": a.phonemes, "reps": a.reps}
            for k in runs[0]:
                row[k] = float(np.median([r[k] for r in runs])) if not isinstance(runs[0][k], bool) else all(r[k] for r in runs)
            if with_late:
                row["late_first_ms_runs"] = [round(r["late_first_ms"], 3) for r in runs]
            if hasattr(pool, "stream_stats"):
                row["stream_groups"], row["admitted_midstream"] = pool.stream_stats()
            print(json.dumps(row), flush=True)
        pool.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="hifigan_sdp,mbb_fix")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--chunks", default="32,64")
    ap.add_argument("--phonemes", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--direct", type=int, default=0)
    ap.add_argument("--rate", type=int, default=0, help="output sample rate (0: the native 16 kHz)")
    ap.add_argument("--eq", type=int, nargs="?", const=1, default=0,
                    help="--eq or --eq 1: the 4-band EQ of DESIGN.md 9j on every call, streamed (sts_set_eq_streaming); --late: on every leg's pool "
                         "(sts_pool_set_eq, sts_pool_set_eq_streaming)")
    ap.add_argument("--loud", type=int, default=0, help="1: loudness mode 1 on every call, measured in the streams (sts_set_loudness_streaming)")
    ap.add_argument("--joined", action="store_true", help="a paragraph: joined stream against the whole joined call and single streams in turn")
    ap.add_argument("--sentences", type=int, default=32)
    ap.add_argument("--late", action="store_true", help="a late arrival at a pool of one engine, stream admission off and on (first model, first chunk size)")
    ap.add_argument("--clients", type=int, default=32)
    ap.add_argument("--plans", action="store_true", help="--late: the late client and half of the group carry a duration plan, a gain plan and (multi-speaker) a mix")
    a = ap.parse_args()
    if a.late:
        _late(a)
        return
    forms = {"batched_stream": _batched, "serial_streams": _serial, "one_batch": _batch}
    if a.joined:
        forms = {"joined_stream": _joined_stream, "serial_streams": _serial, "whole_joined": _whole_joined}
        a.batches = str(a.sentences)
    for kind in a.models.split(","):
        cfg = sb.full_cfg(kind)
        syn = engine.Synthesizer(sb.make_blob(cfg, 1234))
        syn.debug_set("launch_ahead", 0)
        syn.debug_set("stream_direct", a.direct)
        syn.set_output_rate(a.rate)
        rate = syn.output_rate()
        if a.eq:
            syn.set_eq(EQ_BANDS)
            syn.set_eq_streaming(True)
        if a.loud:
            syn.set_loudness(engine.LOUD_MEASURE)
            syn.set_loudness_streaming(True)
        for B in [int(v) for v in a.batches.split(",")]:
            ids = _paragraph(cfg, B) if a.joined else [sb.synthetic_ids(a.phonemes, cfg.vocab, salt=u) for u in range(B)]
            for chunk in [int(v) for v in a.chunks.split(",")]:
                for name, fn in forms.items():
                    if name in ("one_batch", "whole_joined") and chunk != int(a.chunks.split(",")[0]):
                        continue                                  # (does not depend on the chunk size)
                    fn(syn, ids, chunk)                           # warm-up of this shape
                    runs = [fn(syn, ids, chunk) for _ in range(a.reps)]
                    med = lambda v: float(np.median(v))            # noqa: E731
                    row = {"model": kind, "B": B, "chunk_frames": chunk if name not in ("one_batch", "whole_joined") else None, "form": name,
                           "first_ms_min": med([min(r[0]) * 1e3 for r in runs]),
                           "first_ms_p50": med([np.median(r[0]) * 1e3 for r in runs]),
                           "first_ms_max": med([max(r[0]) * 1e3 for r in runs]),
                           "last_ms": med([r[1] * 1e3 for r in runs]),
                           "audio_s_per_wall_s": med([r[2] / rate / r[3] for r in runs]),
                           "rate": rate, "direct": a.direct, "eq": a.eq, "loud": a.loud, "reps": a.reps}
                    print(json.dumps(row), flush=True)
        syn.close()


if __name__ == "__main__":
    main()
