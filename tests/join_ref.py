"""numpy restatement of the paragraph join (include/summertts_hip.h sts_infer_ids_joined, steps 1-4): integer layout, a float64 envelope
rounded once to float32, one fp32 multiply.  `join` is None (all zeros) or a mapping with any of gap_frames (B - 1 ints or None),
lead_frames, trail_frames and fade_ms, as summertts_amd.engine takes it."""
import numpy as np

from resample_ref import pcm_cast

MAX_FRAMES = 100000


def _fields(B, join):
    join = join or {}
    gaps = join.get("gap_frames")
    gaps = [0] * max(B - 1, 0) if gaps is None else [int(g) for g in gaps]
    assert len(gaps) == max(B - 1, 0)
    return gaps, int(join.get("lead_frames", 0)), int(join.get("trail_frames", 0)), float(join.get("fade_ms", 0.0))


def design(fade_ms):
    """step 1: h = floor(fade_ms * 16 + 0.5), fade_ms as the float32 the C ABI receives, the arithmetic in float64"""
    return int(np.floor(float(np.float32(fade_ms)) * 16.0 + 0.5))


def layout(frames, hop, join=None):
    """step 2 in Python integers: -> (start [B] int64 native samples, N_J, h)"""
    frames = [int(f) for f in frames]
    gaps, lead, trail, fade = _fields(len(frames), join)
    start, pos = [], lead * hop
    for b, f in enumerate(frames):
        start.append(pos)
        pos += f * hop + (gaps[b] * hop if b + 1 < len(frames) else 0)
    return np.asarray(start, np.int64), pos + trail * hop, design(fade)


def envelope(n, h):
    """step 3: e[t] = float32(float64(min(t + 1, n - t, h + 1)) / float64(h + 1)) for t in [0, n)"""
    t = np.arange(n, dtype=np.int64)
    m = np.minimum(np.minimum(t + 1, n - t), h + 1)
    return (m.astype(np.float64) / np.float64(h + 1)).astype(np.float32)


def join(signals, frames, hop, join=None):
    """steps 2-4: the sentences' float32 signals (frames[b] * hop samples each) -> (J float32 [N_J], its cast int16 [N_J])"""
    start, total, h = layout(frames, hop, join)
    J = np.zeros(total, np.float32)
    for b, x in enumerate(signals):
        x = np.ascontiguousarray(x, np.float32).ravel()
        assert x.size == int(frames[b]) * hop, (b, x.size)
        with np.errstate(invalid="ignore", over="ignore"):
            J[start[b]:start[b] + x.size] = x * envelope(x.size, h)
    return J, pcm_cast(J)
