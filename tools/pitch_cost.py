"""Cost of a pitch plan on the benchmark's one-utterance shape: 128 phonemes, full-size synthetic HiFi-GAN.  Wall time of
synchronised calls with host PCM on one engine, the legs plain / +200 cents on every phoneme / the duration plan alone (rate = ratio: the
frames the pitch plan makes the decoder run) / 48 kHz without a plan, alternated in rounds, medians; then the warp kernel alone on the
call's own wave with the prototype in LDS and in global memory (sts_debug_pitch_bench), and the decoder stage's device time with and
without the plan.

    python tools/pitch_cost.py [--rounds 40]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summertts_amd import engine, synth_blob as sb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    a = ap.parse_args()
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    syn = engine.Synthesizer(blob, device=0)
    ids = sb.synthetic_ids(128, cfg.vocab, salt=0)
    n = len(ids)
    cents = np.full(n, 200, np.int32)
    ratio = engine.pitch_design(cents, n)[0]
    hop = syn.info.samples_per_frame

    def leg(name):
        syn.set_output_rate(48000 if name == "48k" else 16000)
        if name == "pitch":
            syn.set_pitch_plan([n], [cents])
        if name == "stretch":
            syn.set_duration_plan([n], [{"rate": ratio}])
        t0 = time.perf_counter()
        pcm = syn.infer_ids(ids)
        return time.perf_counter() - t0, pcm.size

    legs = ("plain", "pitch", "stretch", "48k")
    t = {k: [] for k in legs}
    size = {}
    for r in range(3 + a.rounds):
        for k in legs:
            dt, size[k] = leg(k)
            if r >= 3:
                t[k].append(dt)
    out = {"call, ms (median)": {k: round(float(np.median(v)) * 1e3, 4) for k, v in t.items()}, "samples": size}
    c = out["call, ms (median)"]
    out["pitch - plain, us"] = round((c["pitch"] - c["plain"]) * 1e3, 1)
    out["pitch - stretch (the warp and its layout), us"] = round((c["pitch"] - c["stretch"]) * 1e3, 1)
    out["stretch - plain (1.12 x the frames), us"] = round((c["stretch"] - c["plain"]) * 1e3, 1)
    out["48k - plain (the resampler), us"] = round((c["48k"] - c["plain"]) * 1e3, 1)
    # device time of the decoder stage (the output chain is part of it)
    syn.set_output_rate(16000)
    syn.set_profiling(True)
    dec = {}
    for k in ("plain", "pitch", "stretch", "48k"):
        v = []
        for r in range(12):
            leg(k)
            v.append(syn.profile()["ms_decoder"])
        dec[k] = round(float(np.median(v[2:])), 4)
    syn.set_profiling(False)
    syn.set_output_rate(16000)
    out["decoder stage on the device, ms"] = dec
    # the warp kernel alone, on the stretched call's own wave
    syn.set_record_taps(True)
    syn.set_duration_plan([n], [{"rate": ratio}])
    syn.infer_ids(ids)
    wave, dur = syn.tap("wave")[0], syn.durations(n)
    syn.set_record_taps(False)
    ya, ms_global = engine.pitch_bench(wave, dur, cents, hop, False, 200)
    yb, ms_lds = engine.pitch_bench(wave, dur, cents, hop, True, 200)
    assert ya.tobytes() == yb.tobytes()
    out["warp kernel alone, us"] = {"prototype in global memory": round(ms_global * 1e3, 2), "prototype in LDS": round(ms_lds * 1e3, 2),
                                    "input samples": int(wave.size)}
    print(json.dumps(out, indent=1))
    syn.close()


if __name__ == "__main__":
    main()
