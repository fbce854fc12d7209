"""Cost of the look-ahead limiter: wall time of synchronised sts_run_batch calls with host PCM on one engine, the legs
off / limiter on / loudness mode 2 / mode 2 + limiter alternated in rounds, medians; then the first-chunk latency of a 32-frame stream with
the limiter off and on (the decode halo grows by the look-ahead).

    python tools/limiter_cost.py [--rounds1 60] [--rounds32 12]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summertts_amd import engine, synth_blob as sb  # noqa: E402

LEGS = (("off", 0, 0), ("limiter", 0, 1), ("loud2", 2, 0), ("loud2+limiter", 2, 1))


def measure(syn, batch, rounds, warmup=3):
    t = {name: [] for name, _, _ in LEGS}
    for r in range(warmup + rounds):
        for name, loud, lim in LEGS:
            syn.set_loudness(loud, -16.0, -1.0)
            syn.set_limiter(lim, 6.0, -1.0, 5.0)
            t0 = time.perf_counter()
            syn.run_batch(batch)
            dt = time.perf_counter() - t0
            if r >= warmup:
                t[name].append(dt)
    return {k: float(np.median(v)) * 1e3 for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds1", type=int, default=60)
    ap.add_argument("--rounds32", type=int, default=12)
    a = ap.parse_args()
    cfg = sb.full_cfg("hifigan_sdp")
    blob = sb.make_blob(cfg, 1234)
    syn = engine.Synthesizer(blob, device=0)
    out = {}
    one = syn.prepare([sb.synthetic_ids(128, cfg.vocab, salt=0)], [0], [1.0])
    out["configs[1] B=1 128 phonemes, ms"] = measure(syn, one, a.rounds1)
    lens = np.random.default_rng(1234).integers(64, 257, size=32).tolist()
    many = syn.prepare([sb.synthetic_ids(int(n), cfg.vocab, salt=u) for u, n in enumerate(lens)], [0] * 32, [1.0] * 32)
    out["configs[2]-shaped B=32 64-256 phonemes, ms"] = measure(syn, many, a.rounds32)
    ids = sb.synthetic_ids(128, cfg.vocab, salt=0)
    syn.set_loudness(0)
    first = {"off": [], "limiter": []}
    halo = {}
    for r in range(14):
        for name, lim in (("off", 0), ("limiter", 1)):
            syn.set_limiter(lim, 6.0, -1.0, 5.0)
            halo[name] = syn.stream_halo_frames()
            chunks, times = syn.infer_ids_stream(ids, 32)
            if r >= 2:
                first[name].append(times[0])
    out["first chunk of a 32-frame stream, ms"] = {k: float(np.median(v)) * 1e3 for k, v in first.items()}
    out["stream halo frames"] = halo
    syn.set_limiter(0)
    for k, v in out.items():
        if isinstance(v, dict) and "loud2" in v:
            v["limiter overhead us"] = round((v["limiter"] - v["off"]) * 1e3, 1)
            v["loud2 overhead us"] = round((v["loud2"] - v["off"]) * 1e3, 1)
            v["loud2+limiter overhead us"] = round((v["loud2+limiter"] - v["off"]) * 1e3, 1)
    print(json.dumps(out, indent=1))
    syn.close()


if __name__ == "__main__":
    main()
