"""Cost of a pitch plan in a stream (DESIGN.md 9l "Streamed"), by tools/stream_latency.py's protocol: full-size synthetic HiFi-GAN,
128-phoneme utterances (one distinct utterance per client), chunks of 32 frames, B = 1 (sts_infer_ids_stream) and B = 32
(sts_infer_ids_batch_stream); the launch-ahead memo off; the legs alternated in rounds after three warm-up rounds, medians:

  pitch     +200 cents on every phoneme, through the range warp (sts_set_pitch_streaming)
  plain     the same stream with no plan
  stretch   a stream under the duration plan alone, rate = ratio: the frames and steps of the pitch leg, without the warp and its halo

Per (B, leg): time to the first chunk (median over the utterances of a call, then over the rounds), time to the last chunk, steps,
samples, and the halo in frames.  --rate R: PCM at R Hz.  --once LEG: one call of that leg at B = 1 and nothing else (for a kernel trace).

    python tools/pitch_stream_cost.py [--rounds 20] [--rate 16000]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summertts_amd import engine, synth_blob as sb  # noqa: E402

CHUNK = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--once", default="")
    a = ap.parse_args()
    cfg = sb.full_cfg("hifigan_sdp")
    syn = engine.Synthesizer(sb.make_blob(cfg, 1234), device=0)
    syn.debug_set("launch_ahead", 0)
    syn.set_pitch_streaming(True)
    syn.set_output_rate(a.rate)

    def leg(name, ids):
        n = [len(x) for x in ids]
        cents = [np.full(k, 200, np.int32) for k in n]
        halo = syn.stream_halo_frames()
        if name == "pitch":
            syn.set_pitch_plan(n, cents)
            halo = syn.stream_halo_frames()
        if name == "stretch":
            syn.set_duration_plan(n, [{"rate": engine.pitch_design(c, k)[0]} for c, k in zip(cents, n)])
        if len(ids) == 1:
            chunks, times = syn.infer_ids_stream(ids[0], CHUNK)
            chunks, times = [chunks], [times]
        else:
            chunks, times = syn.infer_batch_stream(ids, CHUNK)
        return (float(np.median([t[0] for t in times])), max(t[-1] for t in times), max(len(t) for t in times),
                sum(sum(c.size for c in cs) for cs in chunks), halo)

    if a.once:
        print(json.dumps({"leg": a.once, "result": leg(a.once, [sb.synthetic_ids(128, cfg.vocab, salt=0)])}))
        syn.close()
        return
    legs = ("pitch", "plain", "stretch")
    for B in (1, 32):
        ids = [sb.synthetic_ids(128, cfg.vocab, salt=u) for u in range(B)]
        rows = {k: [] for k in legs}
        for r in range(3 + a.rounds):
            for k in legs:
                v = leg(k, ids)
                if r >= 3:
                    rows[k].append(v)
        for k in legs:
            v = rows[k]
            print(json.dumps({"B": B, "rate": a.rate, "leg": k, "first chunk, ms": round(float(np.median([x[0] for x in v])) * 1e3, 3),
                              "last chunk, ms": round(float(np.median([x[1] for x in v])) * 1e3, 3), "steps": v[0][2], "samples": v[0][3],
                              "halo frames": v[0][4]}), flush=True)
    syn.close()


if __name__ == "__main__":
    main()
