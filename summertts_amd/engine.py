"""ctypes binding of ``libsummertts_hip.so`` (C ABI: ``include/summertts_hip.h``).

This is host-side plumbing only: every call goes straight to the HIP engine; there is NO CPU
fallback -- if the shared library or a GPU is missing the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SUMMERTTS_HIP_LIB") or os.path.join(_HERE, "lib", "libsummertts_hip.so")   # override: kernel timing experiments
CSRC = os.path.join(_HERE, "csrc")


def build_library(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into ``summertts_amd/lib/libsummertts_hip.so`` (in-tree)."""
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


class ModelInfo(C.Structure):
    _fields_ = [("is_multi_speaker", C.c_int32), ("lang_type", C.c_int32), ("dur_pred_type", C.c_int32),
                ("dec_type", C.c_int32), ("vocab", C.c_int32), ("hidden", C.c_int32), ("inter_channels", C.c_int32),
                ("speaker_num", C.c_int32), ("gin_channels", C.c_int32), ("samples_per_frame", C.c_int32),
                ("sample_rate", C.c_int32), ("blob_floats_consumed", C.c_int64)]


class Profile(C.Structure):
    _fields_ = [("ms_text_encoder", C.c_float), ("ms_duration", C.c_float), ("ms_flow", C.c_float),
                ("ms_decoder", C.c_float), ("ms_total_device", C.c_float), ("ms_decoder_mfma", C.c_float),
                ("decoder_mfma_launches", C.c_int32), ("flops_text_encoder", C.c_double),
                ("flops_duration", C.c_double), ("flops_flow", C.c_double), ("flops_decoder", C.c_double),
                ("flops_decoder_mfma", C.c_double), ("bytes_decoder_min", C.c_double), ("frames", C.c_int64),
                ("samples", C.c_int64), ("phonemes", C.c_int64), ("flops_decoder_mfma_executed", C.c_double),
                ("bytes_text_encoder", C.c_double), ("bytes_duration", C.c_double), ("bytes_flow", C.c_double),
                ("ms_sync_wait_host", C.c_float), ("flops_decoder_bf16_issued", C.c_double),
                ("conv_math_fallbacks", C.c_int64), ("conv_math_pinned", C.c_int32), ("launch_ahead", C.c_int32), ("launch_ahead_misses", C.c_int64),
                ("us_host_setup", C.c_float), ("us_host_enqueue", C.c_float), ("us_host_tail", C.c_float),
                ("poison_bytes", C.c_int64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class DurPlan(C.Structure):
    """``sts_dur_plan``: one utterance's duration plan (include/summertts_hip.h sts_set_duration_plan)."""
    _fields_ = [("rate", C.c_void_p), ("fixed", C.c_void_p), ("target_frames", C.c_int32)]


def _dur_plans(n: Sequence[int], plans):
    """-> (n as int32 array, ctypes array of DurPlan, the numpy arrays it points into).  ``plans[b]``: None or a mapping with any of
    ``rate`` (float per phoneme), ``fixed`` (int per phoneme, -1 = predicted), ``target_frames``."""
    n = np.ascontiguousarray(n, dtype=np.int32)
    if len(plans) != n.size:
        raise ValueError("one plan (or None) per utterance")
    arr, keep = (DurPlan * max(n.size, 1))(), []
    for b, p in enumerate(plans):
        p = p or {}
        for key, dt in (("rate", np.float32), ("fixed", np.int32)):
            v = p.get(key)
            if v is not None:
                v = np.ascontiguousarray(v, dtype=dt)
                if v.size != n[b]:
                    raise ValueError(f"plan {b}: {key} needs one entry per phoneme")
                keep.append(v)
                setattr(arr[b], key, v.ctypes.data)
        arr[b].target_frames = int(p.get("target_frames") or 0)
    return n, arr, keep


class SpeakerMix(C.Structure):
    """``sts_speaker_mix``: one utterance's speaker mix (include/summertts_hip.h sts_set_speaker_mix)."""
    _fields_ = [("k", C.c_int32), ("sid", C.c_void_p), ("weight", C.c_void_p), ("vector", C.c_void_p), ("vector_weight", C.c_float)]


def _speaker_mixes(mixes, gin: Optional[int] = None):
    """-> (ctypes array of SpeakerMix, the numpy arrays it points into).  ``mixes[b]``: None (the plain sid) or a mapping with any of
    ``sid`` + ``weight`` (table rows and their weights, equally many), ``vector`` (a caller's embedding, ``gin`` floats) and
    ``vector_weight`` (default 1)."""
    arr, keep = (SpeakerMix * max(len(mixes), 1))(), []
    for b, m in enumerate(mixes):
        m = m or {}
        sid, w = m.get("sid"), m.get("weight")
        if (sid is None) != (w is None):
            raise ValueError(f"mix {b}: sid and weight come together")
        if sid is not None:
            sid = np.ascontiguousarray(sid, dtype=np.int32).ravel()
            w = np.ascontiguousarray(w, dtype=np.float32).ravel()
            if sid.size != w.size:
                raise ValueError(f"mix {b}: one weight per sid")
            keep += [sid, w]
            arr[b].k = sid.size
            if sid.size:
                arr[b].sid, arr[b].weight = sid.ctypes.data, w.ctypes.data
        v = m.get("vector")
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.float32).ravel()
            if gin and v.size != gin:
                raise ValueError(f"mix {b}: vector needs gin_channels = {gin} entries")
            keep.append(v)
            arr[b].vector = v.ctypes.data
            arr[b].vector_weight = float(m.get("vector_weight", 1.0))
    return arr, keep


class GainPlan(C.Structure):
    """``sts_gain_plan``: one utterance's gain plan (include/summertts_hip.h sts_set_gain_plan)."""
    _fields_ = [("gain_db", C.c_void_p), ("ramp_ms", C.c_float)]


def _gain_plans(n: Sequence[int], plans):
    """-> (n as int32 array, ctypes array of GainPlan, the numpy arrays it points into).  ``plans[b]``: None (no plan) or a mapping with
    ``gain_db`` (float per phoneme, ``-inf`` = mute; None = no gains) and ``ramp_ms`` (default 0)."""
    n = np.ascontiguousarray(n, dtype=np.int32)
    if len(plans) != n.size:
        raise ValueError("one plan (or None) per utterance")
    arr, keep = (GainPlan * max(n.size, 1))(), []
    for b, p in enumerate(plans):
        p = p or {}
        v = p.get("gain_db")
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.float32).ravel()
            if v.size != n[b]:
                raise ValueError(f"plan {b}: gain_db needs one entry per phoneme")
            keep.append(v)
            arr[b].gain_db = v.ctypes.data
        arr[b].ramp_ms = float(p.get("ramp_ms", 0.0))
    return n, arr, keep


class PitchPlan(C.Structure):
    """``sts_pitch_plan``: one utterance's pitch plan (include/summertts_hip.h sts_set_pitch_plan)."""
    _fields_ = [("cents", C.c_void_p)]


def _pitch_plans(n: Sequence[int], plans):
    """-> (n as int32 array, ctypes array of PitchPlan, the numpy arrays it points into).  ``plans[b]``: None (no plan) or a mapping with
    ``cents`` (int per phoneme), or the sequence of cents itself."""
    n = np.ascontiguousarray(n, dtype=np.int32)
    if len(plans) != n.size:
        raise ValueError("one plan (or None) per utterance")
    arr, keep = (PitchPlan * max(n.size, 1))(), []
    for b, p in enumerate(plans):
        v = p.get("cents") if isinstance(p, dict) else p
        if v is not None:
            v = np.asarray(v)
            if v.dtype.kind not in "iu":
                raise ValueError(f"plan {b}: cents are integers")
            v = np.ascontiguousarray(v, dtype=np.int32).ravel()
            if v.size != n[b]:
                raise ValueError(f"plan {b}: cents needs one entry per phoneme")
            keep.append(v)
            arr[b].cents = v.ctypes.data
    return n, arr, keep


class Join(C.Structure):
    """``sts_join``: how the sentences of a paragraph are joined (include/summertts_hip.h sts_infer_ids_joined)."""
    _fields_ = [("gap_frames", C.c_void_p), ("lead_frames", C.c_int32), ("trail_frames", C.c_int32), ("fade_ms", C.c_float)]


def _join(B: int, join):
    """-> (ctypes pointer to a Join or None, what it points into).  ``join``: None (all zeros) or a mapping with any of ``gap_frames``
    (B - 1 ints, silence between sentence b and b + 1, in frames; None = all 0), ``lead_frames``, ``trail_frames`` (default 0) and
    ``fade_ms`` (edge fade of every sentence, default 0)."""
    if join is None:
        return None, None
    j = Join()
    g = join.get("gap_frames")
    if g is not None:
        g = np.ascontiguousarray(g, dtype=np.int32).ravel()
        if g.size != max(int(B) - 1, 0):
            raise ValueError("gap_frames needs B - 1 entries")
        j.gap_frames = g.ctypes.data if g.size else None
    j.lead_frames = int(join.get("lead_frames", 0))
    j.trail_frames = int(join.get("trail_frames", 0))
    j.fade_ms = float(join.get("fade_ms", 0.0))
    return C.pointer(j), (j, g)


class EqBand(C.Structure):
    """``sts_eq_band``: one section of the parametric equaliser (include/summertts_hip.h sts_set_eq)."""
    _fields_ = [("type", C.c_int32), ("freq_hz", C.c_float), ("gain_db", C.c_float), ("q", C.c_float)]


EQ_MAX_BANDS = 4
EQ_PEAK, EQ_LOWSHELF, EQ_HIGHSHELF, EQ_HIGHPASS, EQ_LOWPASS = 1, 2, 3, 4, 5


def _eq_bands(bands):
    """-> (n, ctypes array of EqBand or None).  ``bands``: None / empty (the stage off) or a sequence of ``(type, freq_hz, gain_db, q)``
    tuples or mappings with those keys (``gain_db`` defaults to 0, ``q`` to 1 / sqrt(2))."""
    bands = list(bands) if bands is not None else []
    if not bands:
        return 0, None
    arr = (EqBand * len(bands))()
    for i, b in enumerate(bands):
        if isinstance(b, dict):
            b = (b["type"], b["freq_hz"], b.get("gain_db", 0.0), b.get("q", 0.7071067811865476))
        arr[i].type, arr[i].freq_hz, arr[i].gain_db, arr[i].q = int(b[0]), float(b[1]), float(b[2]), float(b[3])
    return len(bands), arr


class PreparedBatch:
    """run_batch's argument arrays, built once (Synthesizer.prepare)."""

    def __init__(self, ids, sid=None, length_scale=None):
        B = self.B = len(ids)
        self.arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in ids]
        self.ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in self.arrs])
        self.n = np.asarray([a.size for a in self.arrs], dtype=np.int32)
        self.sid = np.zeros(B, np.int32) if sid is None else np.ascontiguousarray(sid, dtype=np.int32)
        self.ls = np.ones(B, np.float32) if length_scale is None else np.ascontiguousarray(length_scale, dtype=np.float32)
        self.n_out = np.zeros(B, np.int32)
        self.total = C.c_int64()
        self.n_p, self.sid_p, self.ls_p, self.n_out_p = self.n.ctypes.data, self.sid.ctypes.data, self.ls.ctypes.data, self.n_out.ctypes.data
        self.total_ref = C.byref(self.total)

    def __len__(self):
        return self.B


_lib = None


# the streaming callbacks of the C ABI (include/summertts_hip.h sts_chunk_cb, sts_batch_chunk_cb)
CHUNK_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int16), C.c_int32, C.c_int32)
BATCH_CHUNK_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int16), C.c_int32, C.c_int32)


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.sts_last_error.restype = C.c_char_p
    lib.sts_create.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]
    lib.sts_destroy.argtypes = [C.c_void_p]
    lib.sts_speaker_num.argtypes = [C.c_void_p]
    lib.sts_get_info.argtypes = [C.c_void_p, C.POINTER(ModelInfo)]
    lib.sts_infer_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                  C.POINTER(C.POINTER(C.c_int16)), C.POINTER(C.c_int32)]
    lib.sts_run_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(C.c_int64)]
    lib.sts_copy_pcm_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_copy_pcm_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_pcm_host_view.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(C.c_int64)]
    lib.sts_set_forced_durations.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_set_record_taps.argtypes = [C.c_void_p, C.c_int]
    lib.sts_set_conv_mode.argtypes = [C.c_void_p, C.c_int]
    lib.sts_set_conv_math.argtypes = [C.c_void_p, C.c_int]
    lib.sts_debug_set.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.sts_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.sts_set_host_pcm.argtypes = [C.c_void_p, C.c_int]
    lib.sts_get_profile.argtypes = [C.c_void_p, C.POINTER(Profile)]
    lib.sts_get_profile_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_get_tap.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int64)]
    lib.sts_get_durations.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_set_noise.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint64]
    lib.sts_get_noise.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    lib.sts_set_output_rate.argtypes = [C.c_void_p, C.c_int32]
    lib.sts_get_output_rate.argtypes = [C.c_void_p]
    lib.sts_resample_table.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.c_void_p, C.c_int64]
    lib.sts_pool_set_output_rate.argtypes = [C.c_void_p, C.c_int32]
    lib.sts_set_loudness.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    lib.sts_get_loudness_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.sts_get_loudness.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_pool_set_loudness.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    lib.sts_multi_set_loudness.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    lib.sts_kweight_coeffs.argtypes = [C.c_int32, C.c_void_p]
    lib.sts_loudness_measure.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p]
    lib.sts_set_loudness_streaming.argtypes = [C.c_void_p, C.c_int]
    lib.sts_get_loudness_streaming.argtypes = [C.c_void_p]
    lib.sts_loudness_measure_chunked.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_set_limiter.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    lib.sts_get_limiter_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.sts_get_limiter.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_pool_set_limiter.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    lib.sts_multi_set_limiter.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    lib.sts_limiter_design.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]
    lib.sts_limiter_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_multi_set_output_rate.argtypes = [C.c_void_p, C.c_int32]
    lib.sts_set_duration_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_multi_set_duration_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_get_phoneme_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_duration_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.sts_duration_plan_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_pool_submit_plan.restype = C.c_int64
    lib.sts_pool_submit_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_int32]
    lib.sts_set_speaker_mix.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sts_multi_set_speaker_mix.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sts_speaker_mix_check.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.sts_get_speaker_embedding.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    lib.sts_speaker_blend.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_pool_submit_mix.restype = C.c_int64
    lib.sts_pool_submit_mix.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_void_p]
    lib.sts_set_gain_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_multi_set_gain_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_gain_plan_check.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_gain_design.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.POINTER(C.c_int32)]
    lib.sts_gain_plan_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_debug_spline_step.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_debug_attention.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sts_debug_layer_norm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_int32]
    lib.sts_debug_resblock_layer.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                             C.c_int32, C.POINTER(C.c_uint32)]
    lib.sts_debug_col_layer.argtypes = ([C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 5 + [C.c_int32] * 3 +
                                        [C.c_void_p] * 7 + [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_float] + [C.c_void_p] * 2 + [C.c_int32] +
                                        [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
    lib.sts_set_pitch_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_multi_set_pitch_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_pool_submit_pitch.restype = C.c_int64
    lib.sts_pool_submit_pitch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_void_p]
    lib.sts_pitch_plan_check.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_pitch_design.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_pitch_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_pitch_table.argtypes = [C.c_void_p, C.c_int64]
    lib.sts_pitch_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64]
    lib.sts_set_pitch_streaming.argtypes = [C.c_void_p, C.c_int]
    lib.sts_pitch_chunk_starts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
    lib.sts_pitch_apply_range.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_debug_pitch_bench.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int32, C.c_int32, C.POINTER(C.c_float)]
    lib.sts_pool_submit_gain.restype = C.c_int64
    lib.sts_pool_submit_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_void_p]
    lib.sts_join_check.argtypes = [C.c_int32, C.c_void_p]
    lib.sts_join_layout.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.sts_join_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_join_apply_range.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_void_p]
    lib.sts_infer_ids_joined_stream.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                CHUNK_CB, C.c_void_p, C.c_void_p]
    lib.sts_infer_ids_joined.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.POINTER(C.c_int16)), C.POINTER(C.c_int32)]
    lib.sts_get_join_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_pool_submit_joined.restype = C.c_int64
    lib.sts_pool_submit_joined.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                           C.c_uint64, C.c_void_p]
    lib.sts_set_eq.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sts_get_eq.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int32]
    lib.sts_eq_check.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    lib.sts_eq_design.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sts_eq_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_pool_set_eq.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sts_set_eq_streaming.argtypes = [C.c_void_p, C.c_int]
    lib.sts_get_eq_streaming.argtypes = [C.c_void_p]
    lib.sts_pool_set_eq_streaming.argtypes = [C.c_void_p, C.c_int]
    lib.sts_eq_apply_chunked.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sts_multi_set_eq.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sts_infer_ids_batch_stream.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                               BATCH_CHUNK_CB, C.c_void_p, C.c_void_p]
    lib.sts_pool_submit_stream.restype = C.c_int64
    lib.sts_pool_submit_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64,
                                           C.c_int32, CHUNK_CB, C.c_void_p]
    lib.sts_stream_open.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64]
    lib.sts_stream_open_ex.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    lib.sts_stream_tables_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "sts_stream_get_loudness"):       # (added without a new ABI revision: an older library of revision 18 lacks it)
        lib.sts_stream_get_loudness.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sts_debug_adopt_tables.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_pool_submit_stream_ex.restype = C.c_int64
    lib.sts_pool_submit_stream_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64,
                                              C.c_int32, CHUNK_CB, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_stream_admit.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    lib.sts_stream_step.argtypes = [C.c_void_p, BATCH_CHUNK_CB, C.c_void_p, C.c_void_p]
    lib.sts_stream_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_stream_close.argtypes = [C.c_void_p]
    lib.sts_debug_adopt_z.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int32]
    lib.sts_para_open.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float]
    lib.sts_para_append.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
    lib.sts_para_finish.argtypes = [C.c_void_p, C.c_int32]
    lib.sts_para_step.argtypes = [C.c_void_p, CHUNK_CB, C.c_void_p, C.c_void_p]
    lib.sts_para_info.argtypes = [C.c_void_p] + [C.c_void_p] * 9
    lib.sts_para_close.argtypes = [C.c_void_p]
    lib.sts_pool_set_stream_admission.argtypes = [C.c_void_p, C.c_int]
    lib.sts_pool_get_stream_admission.argtypes = [C.c_void_p]
    lib.sts_pool_stream_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_free.argtypes = [C.c_void_p]
    lib.sts_debug_conv1d.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                     C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32)]
    lib.sts_debug_conv1d_bench.argtypes = lib.sts_debug_conv1d.argtypes + [C.c_int32, C.POINTER(C.c_float)]
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "sts_create", "sts_destroy", "sts_speaker_num", "sts_get_info", "sts_infer_ids", "sts_infer_ids_batch",
    "sts_run_batch", "sts_copy_pcm_device", "sts_copy_pcm_host", "sts_pcm_host_view", "sts_set_forced_durations",
    "sts_set_record_taps", "sts_get_tap", "sts_get_durations", "sts_set_conv_mode", "sts_set_conv_math", "sts_set_profiling",
    "sts_get_profile", "sts_set_host_pcm", "sts_debug_conv1d", "sts_debug_conv1d_bench", "sts_debug_conv1d_packed", "sts_debug_conv1d_epi", "sts_debug_conv_h2p", "sts_debug_conv_h2p_packed", "sts_debug_conv_h2w", "sts_free", "sts_last_error",
    "sts_infer_ids_stream", "sts_stream_halo_frames", "sts_debug_wino_pack", "sts_debug_set", "sts_multi_create_ex", "sts_multi_gather_mode", "sts_multi_gather_layout",
    "sts_pool_create", "sts_pool_destroy", "sts_pool_submit", "sts_pool_wait", "sts_pool_stats", "sts_pool_last_error",
    "sts_multi_create", "sts_multi_destroy", "sts_multi_device_count", "sts_multi_speaker_num", "sts_multi_infer_ids_batch",
    "sts_multi_shard_of", "sts_multi_last_error", "sts_multi_set_rccl_library", "sts_multi_rccl_ranks", "sts_multi_last_gather_ms", "sts_multi_set_conv_math", "sts_get_profile_ex", "sts_abi_version", "sts_build_flags",
    "sts_set_noise", "sts_get_noise", "sts_pool_submit_ex", "sts_multi_set_noise",
    "sts_set_output_rate", "sts_get_output_rate", "sts_resample_table", "sts_pool_set_output_rate", "sts_multi_set_output_rate",
    "sts_infer_ids_batch_stream", "sts_pool_submit_stream",
    "sts_set_loudness", "sts_get_loudness_mode", "sts_get_loudness", "sts_pool_set_loudness", "sts_multi_set_loudness",
    "sts_kweight_coeffs", "sts_loudness_measure",
    "sts_set_limiter", "sts_get_limiter_mode", "sts_get_limiter", "sts_pool_set_limiter", "sts_multi_set_limiter",
    "sts_limiter_design", "sts_limiter_apply",
    "sts_set_duration_plan", "sts_get_phoneme_offsets", "sts_duration_fit", "sts_duration_plan_apply", "sts_pool_submit_plan",
    "sts_multi_set_duration_plan",
    "sts_set_speaker_mix", "sts_speaker_mix_check", "sts_get_speaker_embedding", "sts_speaker_blend", "sts_pool_submit_mix",
    "sts_multi_set_speaker_mix",
    "sts_set_gain_plan", "sts_gain_plan_check", "sts_gain_design", "sts_gain_plan_apply", "sts_pool_submit_gain",
    "sts_multi_set_gain_plan",
    "sts_set_pitch_plan", "sts_pool_submit_pitch", "sts_multi_set_pitch_plan",
    "sts_debug_pitch_bench", "sts_pitch_plan_check", "sts_pitch_design", "sts_pitch_layout", "sts_pitch_table", "sts_pitch_apply",
    "sts_set_pitch_streaming", "sts_pitch_chunk_starts", "sts_pitch_apply_range",
    "sts_debug_spline_step", "sts_debug_attention", "sts_debug_layer_norm", "sts_debug_resblock_layer", "sts_debug_col_layer",
    "sts_join_check", "sts_join_layout", "sts_join_apply", "sts_infer_ids_joined", "sts_get_join_offsets", "sts_pool_submit_joined",
    "sts_infer_ids_joined_stream", "sts_join_apply_range",
    "sts_set_eq", "sts_get_eq", "sts_eq_check", "sts_eq_design", "sts_eq_apply", "sts_pool_set_eq", "sts_multi_set_eq",
    "sts_set_eq_streaming", "sts_get_eq_streaming", "sts_pool_set_eq_streaming", "sts_eq_apply_chunked",
    "sts_set_loudness_streaming", "sts_get_loudness_streaming", "sts_loudness_measure_chunked",
    "sts_stream_open", "sts_stream_admit", "sts_stream_step", "sts_stream_info", "sts_stream_close", "sts_debug_adopt_z",
    "sts_pool_set_stream_admission", "sts_pool_get_stream_admission", "sts_pool_stream_stats",
    "sts_para_open", "sts_para_append", "sts_para_finish", "sts_para_step", "sts_para_info", "sts_para_close",
    "sts_stream_open_ex", "sts_stream_tables_info", "sts_pool_submit_stream_ex", "sts_debug_adopt_tables",
    "sts_stream_get_loudness",
]


class StreamNoise(C.Structure):
    """``sts_stream_noise``: the sampling noise of one utterance of an admission (Synthesizer.stream_admit)"""
    _fields_ = [("noise_scale", C.c_float), ("noise_scale_w", C.c_float), ("seed", C.c_uint64)]


def debug_adopt_z(src, dst, src_off, dst_off, lengths, device: int = 0) -> np.ndarray:
    """The kernel that moves an admission's latents into an open stream's pool (sts_debug_adopt_z), on caller data: columns
    ``[src_off[b], src_off[b] + lengths[b])`` of every row of ``src`` [C][ld_src] go to ``[dst_off[b], ...)`` of a copy of ``dst``
    [C][ld_dst], which is returned; everything outside the destination ranges is what ``dst`` held."""
    lib = load_library()
    a = np.ascontiguousarray(src, dtype=np.float32)
    out = np.array(dst, dtype=np.float32, order="C", copy=True)
    if a.ndim != 2 or out.ndim != 2 or a.shape[0] != out.shape[0]:
        raise ValueError("src [C][ld_src] and dst [C][ld_dst] with the same C are required")
    so = np.ascontiguousarray(src_off, dtype=np.int64)
    do = np.ascontiguousarray(dst_off, dtype=np.int64)
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    if not (so.size == do.size == ln.size):
        raise ValueError("one source offset, destination offset and length per segment")
    _check(lib, lib.sts_debug_adopt_z(device, a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data, out.shape[1], so.ctypes.data,
                                      do.ctypes.data, ln.ctypes.data, ln.size))
    return out


def debug_adopt_tables(g, gpool, cum, q, pool, slot_words, slot, src_off, n, dst_off, h, device: int = 0):
    """The kernel that moves an admission's tables into a planned open stream's pools (sts_debug_adopt_tables), on caller data.  For
    newcomer b with ``slot[b] >= 0``: column b of ``g`` [gin][B] goes to column ``slot[b]`` of ``gpool`` [gin][max_live] (both None: no
    conditioning vectors); ``n[b] > 0``: ``cum`` / ``q`` ``[src_off[b], + n[b])`` go to rows 0 / 1 of ``pool`` [2][capacity + 1] at column
    ``dst_off[b]`` and its column of ``slot_words`` [3][max_live] becomes ``(dst_off[b], n[b], h[b])``; ``n[b] == 0``: ``(capacity, 1, 0)``.
    Returns copies ``(gpool, pool, slot_words)``; everything outside the destinations is what the arguments held."""
    lib = load_library()
    sl = np.ascontiguousarray(slot, dtype=np.int32)
    so, nn, do, hh = (np.ascontiguousarray(v, dtype=np.int32) for v in (src_off, n, dst_off, h))
    if not (sl.size == so.size == nn.size == do.size == hh.size):
        raise ValueError("one slot, source offset, count, destination offset and h per newcomer")
    po = np.array(pool, dtype=np.int32, order="C", copy=True)
    sw = np.array(slot_words, dtype=np.int32, order="C", copy=True)
    if po.ndim != 2 or po.shape[0] != 2 or po.shape[1] < 2 or sw.ndim != 2 or sw.shape[0] != 3:
        raise ValueError("pool [2][capacity + 1] and slot_words [3][max_live] are required")
    cu = None if cum is None else np.ascontiguousarray(cum, dtype=np.int32).ravel()
    qq = None if q is None else np.ascontiguousarray(q, dtype=np.int32).ravel()
    if (cu is None) != (qq is None) or (cu is not None and cu.size != qq.size):
        raise ValueError("cum and q come together, equally long")
    ga = gp = None
    gin = 0
    if g is not None:
        ga = np.ascontiguousarray(g, dtype=np.float32)
        gp = np.array(gpool, dtype=np.float32, order="C", copy=True)
        if ga.ndim != 2 or gp.ndim != 2 or ga.shape[0] != gp.shape[0] or ga.shape[1] != sl.size or gp.shape[1] != sw.shape[1]:
            raise ValueError("g [gin][B] and gpool [gin][max_live] are required")
        gin = ga.shape[0]
    _check(lib, lib.sts_debug_adopt_tables(device, None if ga is None else ga.ctypes.data, gin, sl.size, None if gp is None else gp.ctypes.data,
                                           sw.shape[1], None if cu is None else cu.ctypes.data, None if qq is None else qq.ctypes.data,
                                           0 if cu is None else cu.size, po.ctypes.data, po.shape[1] - 1, sw.ctypes.data, sl.ctypes.data,
                                           so.ctypes.data, nn.ctypes.data, do.ctypes.data, hh.ctypes.data))
    return gp, po, sw


def speaker_mix_check(speaker_num: int, gin: int, mixes) -> None:
    """The validity rules of a speaker mix (include/summertts_hip.h sts_speaker_mix_check; host only, no GPU) for ``mixes`` (as
    ``Synthesizer.set_speaker_mix`` takes them) against a table of ``speaker_num`` rows of ``gin`` floats; ``speaker_num`` 0 = a
    single-speaker model.  Raises StsError for an invalid mix.  (A vector is read as ``gin`` floats: it must hold at least that many.)"""
    lib = load_library()
    arr, keep = _speaker_mixes(mixes)
    for b, m in enumerate(mixes):
        if m and m.get("vector") is not None and np.size(m["vector"]) < gin:
            raise ValueError(f"mix {b}: vector needs gin = {gin} entries")
    _check(lib, lib.sts_speaker_mix_check(int(speaker_num), int(gin), len(mixes), C.cast(arr, C.c_void_p)))


def speaker_blend(table, mixes, sid=None, device: int = 0) -> np.ndarray:
    """The speaker-blend kernel on a caller's table (sts_speaker_blend): ``table`` float32 [gin][speaker_num] (the blob's layout),
    ``mixes`` as ``Synthesizer.set_speaker_mix`` takes them, ``sid`` None or one row per utterance (what an empty entry takes) ->
    float32 [B][gin]."""
    lib = load_library()
    t = np.ascontiguousarray(table, dtype=np.float32)
    if t.ndim != 2:
        raise ValueError("table is [gin][speaker_num]")
    gin, spk = t.shape
    arr, keep = _speaker_mixes(mixes, gin)
    B = len(mixes)
    s = None if sid is None else np.ascontiguousarray(sid, dtype=np.int32)
    if s is not None and s.size != B:
        raise ValueError("one sid per utterance")
    out = np.zeros((max(B, 1), gin), np.float32)
    _check(lib, lib.sts_speaker_blend(int(device), t.ctypes.data, spk, gin, B, None if s is None else s.ctypes.data,
                                      C.cast(arr, C.c_void_p), out.ctypes.data))
    return out[:B]


def gain_plan_check(n: Sequence[int], plans) -> None:
    """The validity rules of a gain plan (include/summertts_hip.h sts_gain_plan_check; host only, no GPU) for ``plans`` (as
    ``Synthesizer.set_gain_plan`` takes them) of ``n[b]`` phonemes each.  Raises StsError for an invalid plan."""
    lib = load_library()
    nn, arr, keep = _gain_plans(n, plans)
    _check(lib, lib.sts_gain_plan_check(nn.size, nn.ctypes.data, C.cast(arr, C.c_void_p)))


def gain_design(gain_db, n: int, ramp_ms: float = 0.0):
    """Step 1 of the gain-plan definition (include/summertts_hip.h sts_gain_design; host only, no GPU): ``gain_db`` None or ``n`` floats
    -> (q, h): the int32 fixed-point gains and the half ramp width in native samples."""
    lib = load_library()
    g = None if gain_db is None else np.ascontiguousarray(gain_db, dtype=np.float32).ravel()
    if g is not None and g.size != n:
        raise ValueError("gain_db needs one entry per phoneme")
    q = np.zeros(max(int(n), 1), np.int32)
    h = C.c_int32()
    _check(lib, lib.sts_gain_design(None if g is None else g.ctypes.data, int(n), float(ramp_ms), q.ctypes.data, C.byref(h)))
    return q[:int(n)], h.value


def _pack_signals(signals):
    """Float signals as the stage entries take them -> (sig, x, lens, total): each signal as a flat float32 array, their concatenation (one
    zero where there is no sample at all), their lengths (int64) and the lengths' sum."""
    sig = [np.ascontiguousarray(s, dtype=np.float32).ravel() for s in signals]
    lens = np.asarray([s.size for s in sig], np.int64)
    total = int(lens.sum())
    return sig, (np.concatenate(sig) if sig and total > 0 else np.zeros(1, np.float32)), lens, total


def _split(packed, lens):
    """A packed output buffer cut back into one copy per signal."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [packed[off[b]:off[b + 1]].copy() for b in range(len(lens))]


def gain_plan_apply(signals, durations, plans, samples_per_frame: int, device: int = 0):
    """The gain-plan kernel on caller signals (sts_gain_plan_apply): ``durations`` a list of int arrays (frames per phoneme), one per
    utterance; ``signals[b]`` its float signal of ``max(1, sum d) * samples_per_frame`` samples; ``plans`` as
    ``Synthesizer.set_gain_plan`` takes them -> (y, pcm): lists of the gained float32 signals and their int16 casts."""
    lib = load_library()
    ds = [np.ascontiguousarray(d, dtype=np.int32).ravel() for d in durations]
    sig, x, _, _ = _pack_signals(signals)
    if len(sig) != len(ds):
        raise ValueError("one signal per utterance")
    lens = np.asarray([max(1, int(d.sum())) * int(samples_per_frame) for d in ds], np.int64)
    for b, v in enumerate(sig):
        if v.size != lens[b]:
            raise ValueError(f"signal {b} needs max(1, sum d) * samples_per_frame = {lens[b]} samples")
    nn, arr, keep = _gain_plans([d.size for d in ds], plans)
    total = int(lens.sum())
    d = np.concatenate(ds) if ds and sum(v.size for v in ds) else np.zeros(1, np.int32)
    y = np.zeros(max(total, 1), np.float32)
    pcm = np.zeros(max(total, 1), np.int16)
    _check(lib, lib.sts_gain_plan_apply(int(device), x.ctypes.data, d.ctypes.data, nn.ctypes.data, len(ds), int(samples_per_frame),
                                        C.cast(arr, C.c_void_p), y.ctypes.data, pcm.ctypes.data))
    return _split(y, lens), _split(pcm, lens)


PITCH_TABLE_FLOATS = 16386


def pitch_plan_check(n: Sequence[int], plans) -> None:
    """The validity rules of a pitch plan (include/summertts_hip.h sts_pitch_plan_check; host only, no GPU) for ``plans`` (as
    ``Synthesizer.set_pitch_plan`` takes them) of ``n[b]`` phonemes each.  Raises StsError for an invalid plan."""
    lib = load_library()
    nn, arr, keep = _pitch_plans(n, plans)
    _check(lib, lib.sts_pitch_plan_check(nn.size, nn.ctypes.data, C.cast(arr, C.c_void_p)))


def pitch_design(cents, n: int):
    """Step 1 of the pitch-plan definition (sts_pitch_design; host only): ``cents`` None or ``n`` ints -> (ratio float32 [n], step int64
    [n]): the duration ratios and the Q32 input samples per output sample."""
    lib = load_library()
    _, arr, keep = _pitch_plans([n], [cents])
    ratio, step = np.zeros(max(int(n), 1), np.float32), np.zeros(max(int(n), 1), np.int64)
    _check(lib, lib.sts_pitch_design(arr[0].cents, int(n), ratio.ctypes.data, step.ctypes.data))
    return ratio[:int(n)], step[:int(n)]


def pitch_layout(durations, step, samples_per_frame: int):
    """Step 3 of the pitch-plan definition (sts_pitch_layout; host only): frames and Q32 steps per phoneme -> (o, e), int64 [n + 1] each:
    the first output of every phoneme (o[n]: the warped length) and the Q32 offset of that output behind the phoneme's first sample."""
    lib = load_library()
    d = np.ascontiguousarray(durations, dtype=np.int32).ravel()
    s = np.ascontiguousarray(step, dtype=np.int64).ravel()
    if s.size != d.size:
        raise ValueError("one step per phoneme")
    o, e = np.zeros(d.size + 1, np.int64), np.zeros(d.size + 1, np.int64)
    _check(lib, lib.sts_pitch_layout(d.ctypes.data, s.ctypes.data, d.size, int(samples_per_frame), o.ctypes.data, e.ctypes.data))
    return o, e


def pitch_table() -> np.ndarray:
    """The interpolator's prototype h0 (sts_pitch_table; host only): 16386 float32."""
    lib = load_library()
    t = np.zeros(PITCH_TABLE_FLOATS, np.float32)
    _check(lib, lib.sts_pitch_table(t.ctypes.data, t.size))
    return t


def pitch_apply(signals, durations, plans, samples_per_frame: int, device: int = 0):
    """The pitch-plan kernel on caller signals (sts_pitch_apply): ``durations`` a list of int arrays (frames per phoneme), one per
    utterance; ``signals[b]`` its float signal of ``max(1, sum d) * samples_per_frame`` samples; ``plans`` as
    ``Synthesizer.set_pitch_plan`` takes them -> (y, pcm): lists of the warped float32 signals and their int16 casts, ``len(y[b])`` the
    warped length."""
    lib = load_library()
    ds = [np.ascontiguousarray(d, dtype=np.int32).ravel() for d in durations]
    sig, x, _, _ = _pack_signals(signals)
    if len(sig) != len(ds):
        raise ValueError("one signal per utterance")
    for b, v in enumerate(sig):
        if v.size != max(1, int(ds[b].sum())) * int(samples_per_frame):
            raise ValueError(f"signal {b} needs max(1, sum d) * samples_per_frame samples")
    nn, arr, keep = _pitch_plans([d.size for d in ds], plans)
    d = np.concatenate(ds) if ds and sum(v.size for v in ds) else np.zeros(1, np.int32)
    lens = np.zeros(max(len(ds), 1), np.int64)
    args = (int(device), x.ctypes.data, d.ctypes.data, nn.ctypes.data, len(ds), int(samples_per_frame), C.cast(arr, C.c_void_p))
    _check(lib, lib.sts_pitch_apply(*args, lens.ctypes.data, None, None, 0))
    lens = lens[:len(ds)]
    total = int(lens.sum())
    y = np.zeros(max(total, 1), np.float32)
    pcm = np.zeros(max(total, 1), np.int16)
    _check(lib, lib.sts_pitch_apply(*args, lens.ctypes.data, y.ctypes.data, pcm.ctypes.data, total))
    return _split(y, lens), _split(pcm, lens)


class PitchRange(C.Structure):
    """``sts_pitch_range``: one window of ``sts_pitch_apply_range``."""
    _fields_ = [("utt", C.c_int32), ("xbase", C.c_int64), ("u0", C.c_int64), ("xlen", C.c_int64), ("y0", C.c_int64), ("y1", C.c_int64)]


def pitch_chunk_starts(durations, step, samples_per_frame: int, chunk_frames: int) -> np.ndarray:
    """Which warped outputs every chunk of a stream through the pitch warp starts at (sts_pitch_chunk_starts; host only): frames per
    phoneme, the Q32 steps of ``pitch_design`` (None: an utterance without a plan) -> int64 [chunks + 1]: Y(k C) for every chunk of
    ``chunk_frames`` frames, then the warped length N'."""
    lib = load_library()
    d = np.ascontiguousarray(durations, dtype=np.int32).ravel()
    s = None if step is None else np.ascontiguousarray(step, dtype=np.int64).ravel()
    if s is not None and s.size != d.size:
        raise ValueError("one step per phoneme")
    args = (d.ctypes.data, None if s is None else s.ctypes.data, d.size, int(samples_per_frame), int(chunk_frames))
    n = int(lib.sts_pitch_chunk_starts(*args, None, 0))
    _check(lib, min(n, 0))
    out = np.zeros(n + 1, np.int64)
    _check(lib, min(int(lib.sts_pitch_chunk_starts(*args, out.ctypes.data, out.size)), 0))
    return out


def pitch_apply_range(x, durations, plans, samples_per_frame: int, windows, device: int = 0):
    """The range form of the pitch-plan kernel on caller data (sts_pitch_apply_range): ``x`` one float buffer; ``durations`` and
    ``plans`` the batch as ``pitch_apply`` takes it; ``windows`` a list of ``(utt, xbase, u0, xlen, y0, y1)`` -- the native samples
    ``[u0, u0 + xlen)`` of utterance ``utt`` stand at ``x[xbase:xbase + xlen]``, and the warped outputs ``[y0, y1)`` are asked for ->
    (y, pcm): lists with one float32 / int16 array per window.  Raises StsError when a window does not cover what its outputs read."""
    lib = load_library()
    ds = [np.ascontiguousarray(d, dtype=np.int32).ravel() for d in durations]
    xx = np.ascontiguousarray(x, dtype=np.float32).ravel()
    nn, arr, keep = _pitch_plans([d.size for d in ds], plans)
    d = np.concatenate(ds) if ds and sum(v.size for v in ds) else np.zeros(1, np.int32)
    win = (PitchRange * max(len(windows), 1))()
    for i, w in enumerate(windows):
        win[i] = PitchRange(*[int(v) for v in w])
    lens = np.asarray([max(0, int(w[5]) - int(w[4])) for w in windows], np.int64)
    total = int(lens.sum())
    y = np.zeros(max(total, 1), np.float32)
    pcm = np.zeros(max(total, 1), np.int16)
    _check(lib, lib.sts_pitch_apply_range(int(device), xx.ctypes.data, xx.size, d.ctypes.data, nn.ctypes.data, len(ds), int(samples_per_frame),
                                          C.cast(arr, C.c_void_p), C.cast(win, C.c_void_p), len(windows), y.ctypes.data, pcm.ctypes.data, total))
    return _split(y, lens), _split(pcm, lens)


def pitch_bench(signal, durations, cents, samples_per_frame: int, table_in_lds: bool, iters: int = 50, device: int = 0):
    """Lab (sts_debug_pitch_bench): the warp of one utterance with the prototype in LDS or in global memory -> (y, mean milliseconds of
    ``iters`` launches)."""
    lib = load_library()
    d = np.ascontiguousarray(durations, dtype=np.int32).ravel()
    x = np.ascontiguousarray(signal, dtype=np.float32).ravel()
    nn, arr, keep = _pitch_plans([d.size], [cents])
    cap = 2 * x.size + 64
    y = np.zeros(cap, np.float32)
    ms = C.c_float()
    _check(lib, lib.sts_debug_pitch_bench(int(device), x.ctypes.data, d.ctypes.data, nn.ctypes.data, 1, int(samples_per_frame),
                                          C.cast(arr, C.c_void_p), y.ctypes.data, cap, int(bool(table_in_lds)), int(iters), C.byref(ms)))
    return y, float(ms.value)


def join_check(B: int, join) -> None:
    """The validity rules of a join (include/summertts_hip.h sts_join_check; host only, no GPU) for ``B`` sentences; ``join`` as
    ``Synthesizer.infer_joined`` takes it.  Raises StsError for an invalid join."""
    lib = load_library()
    jp, keep = _join(B, join)
    _check(lib, lib.sts_join_check(int(B), jp))


def join_layout(frames: Sequence[int], samples_per_frame: int, join=None):
    """Steps 1-2 of the join definition (include/summertts_hip.h sts_join_layout; host only, no GPU): sentences of ``frames[b]`` frames ->
    (start, total, h): each sentence's first sample in the joined signal (int64, native samples), the joined length N_J and the fade
    length in samples."""
    lib = load_library()
    f = np.ascontiguousarray(frames, dtype=np.int32).ravel()
    jp, keep = _join(f.size, join)
    start = np.zeros(max(f.size, 1), np.int64)
    total, h = C.c_int64(), C.c_int32()
    _check(lib, lib.sts_join_layout(f.size, f.ctypes.data, int(samples_per_frame), jp, start.ctypes.data, C.byref(total), C.byref(h)))
    return start[:f.size], int(total.value), int(h.value)


def join_apply(signals, frames: Sequence[int], samples_per_frame: int, join=None, device: int = 0):
    """The join kernel on caller signals (sts_join_apply): ``signals[b]`` a float signal of ``frames[b] * samples_per_frame`` samples ->
    (J, pcm): the joined float32 signal and its int16 cast."""
    lib = load_library()
    f = np.ascontiguousarray(frames, dtype=np.int32).ravel()
    sig, x, _, _ = _pack_signals(signals)
    if len(sig) != f.size:
        raise ValueError("one signal per sentence")
    for b, v in enumerate(sig):
        if v.size != int(f[b]) * int(samples_per_frame):
            raise ValueError(f"signal {b} needs frames * samples_per_frame = {int(f[b]) * int(samples_per_frame)} samples")
    _, total, _ = join_layout(f, samples_per_frame, join)
    jp, keep = _join(f.size, join)
    y = np.zeros(max(total, 1), np.float32)
    pcm = np.zeros(max(total, 1), np.int16)
    _check(lib, lib.sts_join_apply(int(device), x.ctypes.data, f.ctypes.data, f.size, int(samples_per_frame), jp, y.ctypes.data,
                                   pcm.ctypes.data))
    return y[:total], pcm[:total]


def join_apply_range(signals, frames: Sequence[int], samples_per_frame: int, first_frame: int, n_frames: int, join=None, device: int = 0):
    """The windowed join kernel of a joined stream on caller signals (sts_join_apply_range): the frames ``[first_frame, first_frame +
    n_frames)`` of the joined signal -> (J part, pcm part).  ``signals`` / ``frames`` / ``join`` as ``join_apply`` takes them."""
    lib = load_library()
    f = np.ascontiguousarray(frames, dtype=np.int32).ravel()
    sig, x, _, _ = _pack_signals(signals)
    if len(sig) != f.size:
        raise ValueError("one signal per sentence")
    for b, v in enumerate(sig):
        if v.size != int(f[b]) * int(samples_per_frame):
            raise ValueError(f"signal {b} needs frames * samples_per_frame = {int(f[b]) * int(samples_per_frame)} samples")
    jp, keep = _join(f.size, join)
    count = max(int(n_frames), 0) * int(samples_per_frame)
    y = np.zeros(max(count, 1), np.float32)
    pcm = np.zeros(max(count, 1), np.int16)
    _check(lib, lib.sts_join_apply_range(int(device), x.ctypes.data, f.ctypes.data, f.size, int(samples_per_frame), jp, int(first_frame),
                                         int(n_frames), y.ctypes.data, pcm.ctypes.data))
    return y[:count], pcm[:count]


def debug_spline_step(h, filter_sqrt: float, r0=None, r1=None, device: int = 0, o0=None, o1=None):
    """One reverse ConvFlow step on caller data (sts_debug_spline_step, the engine's spline_step launch): ``h`` float32 [29][n], ``r0`` /
    ``r1`` None (= zeros) or n floats -> (o0, o1) = (inverse spline of r1, r0).  ``o0`` / ``o1``: optional contiguous float32 arrays of at
    least n entries to write into (the first n are written, the rest must stay as they were)."""
    lib = load_library()
    h = np.ascontiguousarray(h, dtype=np.float32)
    if h.ndim != 2 or h.shape[0] != 29:
        raise ValueError("h is [29][n]")
    n = h.shape[1]
    r = [None if v is None else np.ascontiguousarray(v, dtype=np.float32).ravel() for v in (r0, r1)]
    if any(v is not None and v.size != n for v in r):
        raise ValueError("r0 and r1 hold n entries")
    o = [np.zeros(max(n, 1), np.float32) if v is None else v for v in (o0, o1)]
    if any(v.dtype != np.float32 or not v.flags.c_contiguous or v.size < n for v in o):
        raise ValueError("o0 and o1 are contiguous float32 arrays of at least n entries")
    _check(lib, lib.sts_debug_spline_step(int(device), h.ctypes.data, n, float(filter_sqrt), None if r[0] is None else r[0].ctypes.data,
                                          None if r[1] is None else r[1].ctypes.data, o[0].ctypes.data, o[1].ctypes.data))
    return o[0][:n], o[1][:n]


ATTN_VARIANTS = {0: "engine's choice", 1: "generic", 2: "register", 3: "mfma"}


def _f32(x, shape, what):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape != tuple(shape):
        raise ValueError(f"{what} is {list(shape)}, got {list(x.shape)}")
    return x


def debug_attention(q, k, v, relk, relv, nheads: int, win: int, lengths, variant: int = 0, device: int = 0, extra_rows: int = 0):
    """The text encoder's attention on caller data (sts_debug_attention): ``q``, ``k``, ``v`` float32 [nheads * kc][L] with L =
    sum(lengths), utterances packed back to back; ``relk`` / ``relv`` [kc][2 win + 1], None when ``win`` is 0.  ``variant``: 0 = the
    engine's choice, 1 = generic, 2 = register, 3 = matrix-core kernel; a forced variant outside its limits raises StsError (STS_EINVAL).
    -> (o [nheads * kc + extra_rows][L], variant launched, keys per lane of the register kernel or 0).  The output starts out as the word
    0xFFFFFFFF on the device and comes back whole: ``extra_rows`` > 0 adds rows no kernel may write."""
    lib = load_library()
    q = np.ascontiguousarray(q, dtype=np.float32)
    lens = np.ascontiguousarray(lengths, dtype=np.int32).ravel()
    if q.ndim != 2 or nheads < 1 or q.shape[0] % nheads or lens.size < 1 or int(lens.sum()) != q.shape[1]:
        raise ValueError("q is [nheads * kc][sum(lengths)]")
    rows, L = q.shape
    kc = rows // nheads
    k, v = _f32(k, q.shape, "k"), _f32(v, q.shape, "v")
    if win > 0:
        relk, relv = _f32(relk, (kc, 2 * win + 1), "relk"), _f32(relv, (kc, 2 * win + 1), "relv")
    elif relk is not None or relv is not None:
        raise ValueError("relk and relv are None when win is 0")
    o = np.zeros((rows + int(extra_rows), L), np.float32)
    var, jpl = C.c_int32(), C.c_int32()
    _check(lib, lib.sts_debug_attention(int(device), q.ctypes.data, k.ctypes.data, v.ctypes.data, None if win <= 0 else relk.ctypes.data,
                                        None if win <= 0 else relv.ctypes.data, int(nheads), kc, int(win), lens.ctypes.data, lens.size,
                                        int(variant), o.ctypes.data, o.shape[0], C.byref(var), C.byref(jpl)))
    return o, var.value, jpl.value


def debug_layer_norm(a, gamma, beta, lengths, b=None, res=None, pre_relu: bool = False, post_gelu: bool = False, dw_w=None, dw_b=None,
                     dw_dil: int = 1, dw_pad: int = 0, device: int = 0, extra_rows: int = 0):
    """The LayerNorm launch on caller data (sts_debug_layer_norm): ``a`` float32 [C][L], L = sum(lengths); ``b`` None or [nb][C][L]
    split-K partials (nb <= 8); ``res`` None or [C][L]; ``dw_w`` None or [k][C] (fused depthwise conv, ``dw_b`` None or [C]).
    -> y [C + extra_rows][L], whole, from a device buffer that started out as the word 0xFFFFFFFF."""
    lib = load_library()
    a = np.ascontiguousarray(a, dtype=np.float32)
    lens = np.ascontiguousarray(lengths, dtype=np.int32).ravel()
    if a.ndim != 2 or lens.size < 1 or int(lens.sum()) != a.shape[1]:
        raise ValueError("a is [C][sum(lengths)]")
    Cc, L = a.shape
    gamma, beta = _f32(gamma, (Cc,), "gamma"), _f32(beta, (Cc,), "beta")
    nb = 0
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        if b.ndim != 3 or b.shape[1:] != a.shape or not 1 <= b.shape[0] <= 8:
            raise ValueError("b is [nb][C][L] with 1 <= nb <= 8")
        nb = b.shape[0]
    if res is not None:
        res = _f32(res, a.shape, "res")
    kk = 0
    if dw_w is not None:
        dw_w = np.ascontiguousarray(dw_w, dtype=np.float32)
        if dw_w.ndim != 2 or dw_w.shape[1] != Cc:
            raise ValueError("dw_w is [k][C]")
        kk = dw_w.shape[0]
        if dw_b is not None:
            dw_b = _f32(dw_b, (Cc,), "dw_b")
    elif dw_b is not None:
        raise ValueError("dw_b goes with dw_w")
    y = np.zeros((Cc + int(extra_rows), L), np.float32)
    ptr = lambda x: None if x is None else x.ctypes.data
    _check(lib, lib.sts_debug_layer_norm(int(device), a.ctypes.data, ptr(b), nb, Cc * L, ptr(res), gamma.ctypes.data, beta.ctypes.data, Cc,
                                         int(bool(pre_relu)), int(bool(post_gelu)), ptr(dw_w), ptr(dw_b), kk, int(dw_dil), int(dw_pad),
                                         lens.ctypes.data, lens.size, y.ctypes.data, y.shape[0]))
    return y


RESBLOCK_KINDS = {1: "resblock_layer", 2: "resblock_wino", 3: "resblock_bf3 bf16x3", 4: "resblock_bf3 f16x2"}


def debug_resblock_layer(x, lengths, members, slope: float, kind: int, variant: int = -1, device: int = 0, extra_rows: int = 0):
    """One fused ResBlock layer launch on caller data (sts_debug_resblock_layer): ``x`` float32 [C][ld], the utterances of ``lengths``
    packed back to back from column 0 (sum(lengths) <= ld); ``members``: 1 to 4 tuples (w1 [C][k1][C], b1 [C] or None, dil1, w2 [C][k2][C],
    b2 [C] or None), every member reads ``x``.  ``kind``: 1 = resblock_layer, 2 = resblock_wino, 3 = resblock_bf3 on three bf16 terms, 4 =
    on two fp16 terms; ``variant`` -1 / 0 / 1 goes to resblock_bf3.  A shape the kind's eligibility function refuses raises StsError
    (STS_EINVAL).  -> (y [n][C + extra_rows][ld] whole, from device buffers that started out as the word 0xFFFFFFFF; the overflow word)."""
    lib = load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    lens = np.ascontiguousarray(lengths, dtype=np.int32).ravel()
    if x.ndim != 2 or lens.size < 1 or int(lens.sum()) > x.shape[1]:
        raise ValueError("x is [C][ld] with sum(lengths) <= ld")
    Cc, ld = x.shape
    n = len(members)
    if n < 1:
        raise ValueError("at least one member")
    keep, w1p, b1p, w2p, b2p = [], (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    k1, k2, dil = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for j, (w1, b1, d1, w2, b2) in enumerate(members):
        w1, w2 = np.ascontiguousarray(w1, dtype=np.float32), np.ascontiguousarray(w2, dtype=np.float32)
        if w1.ndim != 3 or w2.ndim != 3 or (w1.shape[0], w1.shape[2]) != (Cc, Cc) or (w2.shape[0], w2.shape[2]) != (Cc, Cc):
            raise ValueError("w1 is [C][k1][C] and w2 is [C][k2][C]")
        b1 = None if b1 is None else _f32(b1, (Cc,), "b1")
        b2 = None if b2 is None else _f32(b2, (Cc,), "b2")
        keep += [w1, w2, b1, b2]
        w1p[j], w2p[j] = w1.ctypes.data, w2.ctypes.data
        b1p[j], b2p[j] = (None if b1 is None else b1.ctypes.data), (None if b2 is None else b2.ctypes.data)
        k1[j], k2[j], dil[j] = w1.shape[1], w2.shape[1], int(d1)
    y = np.zeros((n, Cc + int(extra_rows), ld), np.float32)
    ovf = C.c_uint32()
    _check(lib, lib.sts_debug_resblock_layer(int(device), x.ctypes.data, Cc, lens.ctypes.data, lens.size, ld, n, w1p, b1p, k1.ctypes.data,
                                             dil.ctypes.data, w2p, b2p, k2.ctypes.data, float(slope), int(kind), int(variant), y.ctypes.data,
                                             y.shape[1], C.byref(ovf)))
    del keep
    return y, ovf.value


COL_LAYER_ALIASES = {0: "none", 1: "y = x", 2: "o0 = r0", 3: "o0 = r1", 4: "o1 = r1", 5: "o1 = r0"}


def debug_col_layer(x, lengths, w, g2, b2, bias=None, add=None, post_gelu: bool = False, use_res: bool = False, xs_w=None, xs_b=None, xr=None,
                    dw_w=None, dw_b=None, dw_dil: int = 1, dw_pad: int = 0, dw_k=None, g1=None, b1=None, tp_w=None, tp_b=None,
                    tp_fs: float = 1.0, tp_r0=None, tp_r1=None, alias: int = 0, device: int = 0, extra_rows: int = 0, out=None):
    """One launch of the fused column-block layer on caller data (sts_debug_col_layer; include/summertts_hip.h states the forms): ``x``
    float32 [C][ld], the utterances of ``lengths`` packed back to back from column 0 (sum(lengths) <= ld); ``w`` [C][C] in [out][in] order;
    ``add`` None or [C][ld]; ``xs_w`` / ``xs_b`` [C] and ``xr`` [ld] the folded rank-1 input; ``dw_w`` [k][C] (``dw_k`` overrides the tap
    count handed to the entry: the refusal tests); ``tp_w`` [29][C], ``tp_b`` [29], ``tp_r0`` / ``tp_r1`` [ld] the tail.  What
    col_layer_eligible refuses raises StsError (STS_EINVAL).  ``out``: None, or (y, o0, o1) float32 arrays [C + extra_rows][ld], [ld], [ld]
    to write into (a refused call leaves them as they were).
    -> (y [C + extra_rows][ld], o0 [ld] or None, o1 [ld] or None), whole, from device buffers that started out as the word 0xFFFFFFFF."""
    lib = load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    lens = np.ascontiguousarray(lengths, dtype=np.int32).ravel()
    if x.ndim != 2 or lens.size < 1 or int(lens.sum()) > x.shape[1]:
        raise ValueError("x is [C][ld] with sum(lengths) <= ld")
    Cc, ld = x.shape
    opt = lambda v, shape, what: None if v is None else _f32(v, shape, what)
    w = _f32(w, (Cc, Cc), "w")
    g1, b1, g2, b2 = opt(g1, (Cc,), "g1"), opt(b1, (Cc,), "b1"), opt(g2, (Cc,), "g2"), opt(b2, (Cc,), "b2")
    bias, add = opt(bias, (Cc,), "bias"), opt(add, (Cc, ld), "add")
    xs_w, xs_b, xr = opt(xs_w, (Cc,), "xs_w"), opt(xs_b, (Cc,), "xs_b"), opt(xr, (ld,), "xr")
    kk = 0
    if dw_w is not None:
        dw_w = np.ascontiguousarray(dw_w, dtype=np.float32)
        if dw_w.ndim != 2 or dw_w.shape[1] != Cc:
            raise ValueError("dw_w is [k][C]")
        kk = dw_w.shape[0] if dw_k is None else int(dw_k)
        if kk > dw_w.shape[0]:
            raise ValueError("dw_k counts rows of dw_w")
    dw_b = opt(dw_b, (Cc,), "dw_b")
    tp_w, tp_b = opt(tp_w, (29, Cc), "tp_w"), opt(tp_b, (29,), "tp_b")
    tp_r0, tp_r1 = opt(tp_r0, (ld,), "tp_r0"), opt(tp_r1, (ld,), "tp_r1")
    if out is None:
        y, o0, o1 = np.zeros((Cc + int(extra_rows), ld), np.float32), np.zeros(ld, np.float32), np.zeros(ld, np.float32)
    else:
        y, o0, o1 = out
        if (y.dtype, o0.dtype, o1.dtype) != (np.float32,) * 3 or not (y.flags.c_contiguous and o0.flags.c_contiguous and o1.flags.c_contiguous) \
                or y.shape != (Cc + int(extra_rows), ld) or o0.shape != (ld,) or o1.shape != (ld,):
            raise ValueError("out is (y [C + extra_rows][ld], o0 [ld], o1 [ld]), contiguous float32")
    ptr = lambda v: None if v is None else v.ctypes.data
    _check(lib, lib.sts_debug_col_layer(int(device), x.ctypes.data, Cc, lens.ctypes.data, lens.size, ld, ptr(xs_w), ptr(xs_b), ptr(xr), ptr(dw_w),
                                        ptr(dw_b), kk, int(dw_dil), int(dw_pad), ptr(g1), ptr(b1), w.ctypes.data, ptr(bias), ptr(add), ptr(g2),
                                        ptr(b2), int(bool(post_gelu)), int(bool(use_res)), ptr(tp_w), ptr(tp_b), float(tp_fs), ptr(tp_r0),
                                        ptr(tp_r1), int(alias), y.ctypes.data, y.shape[0], o0.ctypes.data, o1.ctypes.data))
    return (y, o0, o1) if tp_w is not None else (y, None, None)


def duration_fit(w, fixed=None, target_frames: int = 0) -> np.ndarray:
    """Steps 3-4 of the duration-plan definition on caller weights (include/summertts_hip.h sts_duration_fit; host only, no GPU): -> int32
    durations.  An invalid or infeasible plan raises."""
    lib = load_library()
    w = np.ascontiguousarray(w, dtype=np.float32).ravel()
    f = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32).ravel()
    if f is not None and f.size != w.size:
        raise ValueError("fixed needs one entry per weight")
    out = np.zeros(max(w.size, 1), np.int32)
    _check(lib, lib.sts_duration_fit(w.ctypes.data if w.size else None, None if f is None else f.ctypes.data, w.size, int(target_frames),
                                     out.ctypes.data))
    return out[:w.size]


def duration_plan_apply(weights, fixed=None, target_frames=None, device: int = 0) -> List[np.ndarray]:
    """The duration-plan kernel on caller weights (sts_duration_plan_apply): ``weights`` a list of float arrays, one per utterance;
    ``fixed`` None or a list of int arrays (an entry may be None = all predicted); ``target_frames`` None or one int per utterance ->
    list of int32 duration arrays."""
    lib = load_library()
    ws = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in weights]
    lens = np.asarray([x.size for x in ws], np.int32)
    w = np.concatenate(ws) if ws and lens.sum() > 0 else np.zeros(1, np.float32)
    f = None
    if fixed is not None:
        f = np.concatenate([np.full(ws[b].size, -1, np.int32) if fx is None else np.ascontiguousarray(fx, dtype=np.int32).ravel()
                            for b, fx in enumerate(fixed)])
        if f.size != int(lens.sum()):
            raise ValueError("fixed needs one entry per weight")
    t = None if target_frames is None else np.ascontiguousarray(target_frames, dtype=np.int32)
    out = np.zeros(max(int(lens.sum()), 1), np.int32)
    _check(lib, lib.sts_duration_plan_apply(int(device), w.ctypes.data, None if f is None else f.ctypes.data, lens.ctypes.data, len(ws),
                                            None if t is None else t.ctypes.data, out.ctypes.data))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [out[off[b]:off[b + 1]].copy() for b in range(len(ws))]

LOUD_OFF, LOUD_MEASURE, LOUD_NORMALIZE = 0, 1, 2
# sts_loudness: lufs (-inf when unmeasured), peak, gain, blocks
LOUDNESS_DTYPE = np.dtype([("lufs", np.float32), ("peak", np.float32), ("gain", np.float32), ("blocks", np.int32)])


def kweight_coeffs(rate: int) -> np.ndarray:
    """The library's K-weighting for ``rate`` (include/summertts_hip.h sts_kweight_coeffs; host only, no GPU): float64 [2][5], each row
    {b0, b1, b2, a1, a2} -- the shelf, then the high-pass."""
    lib = load_library()
    c = np.zeros(10, np.float64)
    _check(lib, lib.sts_kweight_coeffs(int(rate), c.ctypes.data))
    return c.reshape(2, 5)


def loudness_measure(signals, rate: int, target_lufs: float = -16.0, peak_dbfs: float = -1.0, device: int = 0) -> np.ndarray:
    """Integrated loudness, sample peak and normalising gain of each float signal in ``signals`` at ``rate`` on the GPU (the engine's
    kernels, sts_loudness_measure) -> structured array of LOUDNESS_DTYPE, one entry per signal."""
    lib = load_library()
    sig, x, lens, _ = _pack_signals(signals)
    out = np.zeros(len(sig), LOUDNESS_DTYPE)
    _check(lib, lib.sts_loudness_measure(int(device), x.ctypes.data, lens.ctypes.data, len(sig), int(rate), float(target_lufs),
                                         float(peak_dbfs), out.ctypes.data))
    return out


def loudness_measure_chunked(signals, rate: int, bounds, back: int = 0, target_lufs: float = -16.0, peak_dbfs: float = -1.0,
                             device: int = 0, want_partial: bool = True):
    """Loudness's STREAM-mode kernels on each float signal in ``signals`` (sts_loudness_measure_chunked): step k consumes
    [bounds[k], bounds[k + 1]) of every signal that reaches it (the last step: to the end) and presents the window widened by ``back``
    samples on either side -> (out, partial): structured arrays of LOUDNESS_DTYPE, ``out[b]`` the final result and ``partial[k][b]`` the
    result as if the call had stopped behind step k (None unless ``want_partial``).  Both buffers carry a sentinel entry behind their
    end, which the library must leave alone."""
    lib = load_library()
    sig, x, lens, _ = _pack_signals(signals)
    bnd = np.ascontiguousarray(bounds, dtype=np.int64).ravel()
    K, B = int(bnd.size), len(sig)
    sentinel = np.array([(-1234.5, -7.0, -9.0, -77)], LOUDNESS_DTYPE)
    out = np.repeat(sentinel, B + 1)
    part = np.repeat(sentinel, K * B + 1)
    _check(lib, lib.sts_loudness_measure_chunked(int(device), x.ctypes.data, lens.ctypes.data, B, int(rate), float(target_lufs), float(peak_dbfs),
                                                 bnd.ctypes.data, K, int(back), out.ctypes.data, part.ctypes.data if want_partial else None))
    if out[B:].tobytes() != sentinel.tobytes() or part[K * B:].tobytes() != sentinel.tobytes():
        raise StsError("sts_loudness_measure_chunked wrote behind its results")
    if not want_partial and part.tobytes() != np.repeat(sentinel, K * B + 1).tobytes():
        raise StsError("sts_loudness_measure_chunked wrote partial results nobody asked for")
    return out[:B].copy(), (part[:K * B].reshape(K, B).copy() if want_partial else None)


LIMITER_OFF, LIMITER_ON = 0, 1
# sts_limiter_stats: gain (g0), min_gain (min s, 1.0 when untouched), peak_out (max |y|), limited (samples with s < 1 before rounding)
LIMITER_DTYPE = np.dtype([("gain", np.float32), ("min_gain", np.float32), ("peak_out", np.float32), ("limited", np.int32)])


def limiter_design(rate: int, gain_db: float = 0.0, ceiling_dbfs: float = -1.0, lookahead_ms: float = 5.0):
    """The library's limiter design for ``rate`` (include/summertts_hip.h sts_limiter_design; host only, no GPU) -> (H, c, G): the half
    window in samples, the ceiling and the make-up gain as float64."""
    lib = load_library()
    H, c, G = C.c_int32(), C.c_double(), C.c_double()
    _check(lib, lib.sts_limiter_design(int(rate), float(gain_db), float(ceiling_dbfs), float(lookahead_ms), C.byref(H), C.byref(c),
                                       C.byref(G)))
    return H.value, c.value, G.value


def limiter_apply(signals, rate: int, gain_db: float = 0.0, ceiling_dbfs: float = -1.0, lookahead_ms: float = 5.0, device: int = 0):
    """The look-ahead limiter on each float signal in ``signals`` at ``rate`` on the GPU (the engine's kernel, sts_limiter_apply) ->
    (y, pcm, stats): lists of the limited float32 signals and their int16 casts, and a structured array of LIMITER_DTYPE."""
    lib = load_library()
    sig, x, lens, total = _pack_signals(signals)
    y = np.zeros(max(total, 1), np.float32)
    pcm = np.zeros(max(total, 1), np.int16)
    stats = np.zeros(len(sig), LIMITER_DTYPE)
    _check(lib, lib.sts_limiter_apply(int(device), x.ctypes.data, lens.ctypes.data, len(sig), int(rate), float(gain_db), float(ceiling_dbfs),
                                      float(lookahead_ms), y.ctypes.data, pcm.ctypes.data, stats.ctypes.data))
    return _split(y, lens), _split(pcm, lens), stats


def eq_check(rate: int, bands) -> None:
    """The validity rules of the equaliser at output rate ``rate`` (include/summertts_hip.h sts_eq_check; host only, no GPU); raises
    StsError with the reason."""
    lib = load_library()
    n, arr = _eq_bands(bands)
    _check(lib, lib.sts_eq_check(int(rate), n, arr))


def eq_design(rate: int, bands) -> np.ndarray:
    """The library's biquad coefficients of ``bands`` at ``rate`` (sts_eq_design; host only, no GPU) -> float64 [n][5],
    {b0, b1, b2, a1, a2} per band."""
    lib = load_library()
    n, arr = _eq_bands(bands)
    c = np.zeros((n, 5), np.float64)
    _check(lib, lib.sts_eq_design(int(rate), n, arr, c.ctypes.data))
    return c


def eq_apply(signals, rate: int, bands, device: int = 0, want_y: bool = True, want_pcm: bool = True):
    """The equaliser on each float signal in ``signals`` at ``rate`` on the GPU (the engine's kernels, sts_eq_apply) -> (y, pcm): lists of
    the float32 outputs and their int16 casts.  An output that is not wanted is not computed; its list then holds the sentinel the
    caller's buffer started with (NaN / 0x7FFF)."""
    lib = load_library()
    n, arr = _eq_bands(bands)
    sig, x, lens, total = _pack_signals(signals)
    y = np.full(max(total, 1), np.nan, np.float32)
    pcm = np.full(max(total, 1), 0x7FFF, np.int16)
    _check(lib, lib.sts_eq_apply(int(device), x.ctypes.data, lens.ctypes.data, len(sig), int(rate), n, arr,
                                 y.ctypes.data if want_y else None, pcm.ctypes.data if want_pcm else None))
    return _split(y, lens), _split(pcm, lens)


def eq_apply_chunked(signals, rate: int, bands, bounds, back: int = 0, device: int = 0):
    """The equaliser's STREAM-mode kernels on each float signal in ``signals`` (sts_eq_apply_chunked): step k covers
    [bounds[k], bounds[k + 1]) of every signal that reaches it (the last step: to the end) and presents the window widened by ``back``
    samples on either side -> (y, pcm, windows): the float32 outputs and int16 casts assembled from the steps, and ``windows[k][b]`` =
    (start, float32 output of step k's whole window of signal b), or None where signal b takes no part in step k.  Every output buffer
    starts as NaN / 0x7FFF."""
    lib = load_library()
    n, arr = _eq_bands(bands)
    sig, x, lens, total = _pack_signals(signals)
    bnd = np.ascontiguousarray(bounds, dtype=np.int64).ravel()
    K, B = int(bnd.size), len(sig)
    wins = []                    # (k, b, start, stop) in the library's order
    for k in range(K):
        c0 = int(bnd[k]); c1 = int(bnd[k + 1]) if k + 1 < K else None
        for b in range(B):
            N = int(lens[b])
            if N > c0:
                wins.append((k, b, max(0, c0 - int(back)), N if c1 is None else min(N, c1 + int(back))))
    wtotal = sum(w[3] - w[2] for w in wins)
    y = np.full(max(total, 1), np.nan, np.float32)
    pcm = np.full(max(total, 1), 0x7FFF, np.int16)
    wy = np.full(wtotal + 1, np.nan, np.float32)
    woff = np.full(max(K * B, 1), -2, np.int64)
    _check(lib, lib.sts_eq_apply_chunked(int(device), x.ctypes.data, lens.ctypes.data, B, int(rate), n, arr, bnd.ctypes.data, K, int(back),
                                         y.ctypes.data, pcm.ctypes.data, wy.ctypes.data, wtotal, woff.ctypes.data))
    windows = [[None] * B for _ in range(K)]
    for k, b, a0, a1 in wins:
        o = int(woff[k * B + b])
        if o < 0:
            raise StsError(f"sts_eq_apply_chunked: no window for step {k}, signal {b}")
        windows[k][b] = (a0, wy[o:o + a1 - a0].copy())
    if not np.isnan(wy[wtotal]):
        raise StsError("sts_eq_apply_chunked wrote behind its windows")
    return _split(y, lens), _split(pcm, lens), windows


def resample_table(in_rate: int, out_rate: int):
    """The output-rate filter of the library (include/summertts_hip.h sts_resample_table; host only, no GPU): -> (P, Q, table), table the
    float32 [P][taps] coefficients the resampling kernel uses."""
    lib = load_library()
    P, Q, taps = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib, lib.sts_resample_table(int(in_rate), int(out_rate), C.byref(P), C.byref(Q), C.byref(taps), None, 0))
    t = np.zeros((P.value, taps.value), np.float32)
    _check(lib, lib.sts_resample_table(int(in_rate), int(out_rate), None, None, None, t.ctypes.data, t.size))
    return P.value, Q.value, t


def lab_build() -> bool:
    """True when the loaded library was built with -DSTS_EXPERIMENTS (`make -C summertts_amd/csrc exp`)."""
    return bool(load_library().sts_build_flags() & 1)


class StsError(RuntimeError):
    pass


def _check(lib, rc: int):
    if rc != 0:
        raise StsError(f"sts error {rc}: {lib.sts_last_error().decode(errors='replace')}")


class _TableSetters:
    """The table setters of ``Synthesizer`` and ``MultiDevice`` (``set_duration_plan``, ``set_speaker_mix``, ``set_gain_plan``,
    ``set_pitch_plan``) in one place.  A class names its C entries (``_TABLE_ENTRY % kind``), the gin a mix's vector is checked
    against here (``_mix_gin``, None: the library checks it) and how a failed entry raises (``_table_failed``)."""

    _TABLE_BUILDERS = {"duration_plan": _dur_plans, "gain_plan": _gain_plans, "pitch_plan": _pitch_plans}

    def _set_table(self, kind: str, n, tables):
        name = self._TABLE_ENTRY % kind
        fn = getattr(self.lib, name)
        if kind == "speaker_mix":
            if tables is None:
                rc = fn(self.h, 0, None)
            else:
                arr, keep = _speaker_mixes(tables, self._mix_gin())
                rc = fn(self.h, len(tables), C.cast(arr, C.c_void_p))
        elif n is None or tables is None:
            rc = fn(self.h, 0, None, None)
        else:
            nn, arr, keep = self._TABLE_BUILDERS[kind](n, tables)
            rc = fn(self.h, nn.size, nn.ctypes.data, C.cast(arr, C.c_void_p))
        if rc != 0:
            self._table_failed(name, rc)


class Synthesizer(_TableSetters):
    """Python mirror of the reference's ``SynthesizerTrn`` (include/SynthesizerTrn.h) at the phoneme-id
    boundary: construct from a model blob, ``infer_ids`` -> int16 PCM.  Adds the batched entry."""

    def __init__(self, blob: np.ndarray, device: int = 0):
        self.lib = load_library()
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self.h = C.c_void_p()
        _check(self.lib, self.lib.sts_create(blob.ctypes.data, blob.nbytes, device, C.byref(self.h)))
        self.info = ModelInfo()
        _check(self.lib, self.lib.sts_get_info(self.h, C.byref(self.info)))
        self.set_host_pcm(True)     # run_batch + pcm_host is the common pairing; a device-side gather switches it off

    def set_host_pcm(self, on: bool):
        """PCM download as part of the run (one stream sync per call); off = the PCM only stays on the device."""
        _check(self.lib, self.lib.sts_set_host_pcm(self.h, 1 if on else 0))

    # -- reference surface -------------------------------------------------------------------
    def get_speaker_num(self) -> int:
        return int(self.lib.sts_speaker_num(self.h))

    def infer_ids(self, ids: Sequence[int], sid: int = 0, length_scale: float = 1.0) -> np.ndarray:
        return self.infer_batch([ids], [sid], [length_scale])[0]

    # -- streaming (sts_infer_ids_stream) -----------------------------------------------------
    def infer_ids_stream(self, ids: Sequence[int], chunk_frames: int, sid: int = 0, length_scale: float = 1.0,
                         on_chunk=None):
        """Decodes chunk by chunk; ``on_chunk(pcm: np.int16[], sample_offset, t_seconds)`` is called per chunk
        (return True to stop).  Returns (list of chunks, list of arrival times since the call started)."""
        import time
        a = np.ascontiguousarray(ids, dtype=np.int32)
        chunks, times = [], []
        t0 = time.perf_counter()

        def _cb(user, pcm, n, off):
            arr = np.ctypeslib.as_array(pcm, shape=(n,)).copy()
            t = time.perf_counter() - t0
            chunks.append(arr); times.append(t)
            return 1 if (on_chunk and on_chunk(arr, off, t)) else 0
        CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int16), C.c_int32, C.c_int32)
        cb = CB(_cb)
        total = C.c_int32()
        self.lib.sts_infer_ids_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, CB,
                                                  C.c_void_p, C.POINTER(C.c_int32)]
        _check(self.lib, self.lib.sts_infer_ids_stream(self.h, a.ctypes.data, a.size, sid, length_scale, chunk_frames, cb, None,
                                                       C.byref(total)))
        return chunks, times

    # -- batched streaming (sts_infer_ids_batch_stream) ---------------------------------------
    def infer_batch_stream(self, ids, chunk_frames: int, sid: Optional[Sequence[int]] = None,
                           length_scale: Optional[Sequence[float]] = None, on_chunk=None, n_total: Optional[list] = None):
        """Streams B utterances together: step k decodes chunk k of every live utterance in one pass.  ``on_chunk(utt, pcm: np.int16[],
        sample_offset, t_seconds)`` is called per chunk, step by step and within a step in ascending ``utt`` (return True to stop that
        utterance only).  Returns (per-utterance lists of chunks, per-utterance lists of arrival times since the call started); with
        ``n_total`` a list, it receives the library's per-utterance sample counts."""
        import time
        B = len(ids)
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in ids]
        ptrs = (C.c_void_p * max(B, 1))(*[a.ctypes.data for a in arrs])
        n = np.array([a.size for a in arrs], dtype=np.int32)
        sid_a = None if sid is None else np.ascontiguousarray(sid, dtype=np.int32)
        ls_a = None if length_scale is None else np.ascontiguousarray(length_scale, dtype=np.float32)
        tot = np.zeros(max(B, 1), dtype=np.int32)
        chunks = [[] for _ in range(B)]
        times = [[] for _ in range(B)]
        t0 = time.perf_counter()

        def _cb(user, utt, pcm, ns, off):
            arr = np.ctypeslib.as_array(pcm, shape=(ns,)).copy() if ns else np.zeros(0, np.int16)
            t = time.perf_counter() - t0
            chunks[utt].append(arr); times[utt].append(t)
            return 1 if (on_chunk and on_chunk(utt, arr, off, t)) else 0
        cb = BATCH_CHUNK_CB(_cb)
        _check(self.lib, self.lib.sts_infer_ids_batch_stream(self.h, B, ptrs, n.ctypes.data,
                                                             None if sid_a is None else sid_a.ctypes.data,
                                                             None if ls_a is None else ls_a.ctypes.data, chunk_frames, cb, None,
                                                             tot.ctypes.data))
        if n_total is not None:
            n_total[:] = [int(v) for v in tot[:B]]
        return chunks, times

    def stream_halo_frames(self) -> int:
        return int(self.lib.sts_stream_halo_frames(self.h))

    # -- open streams (sts_stream_open .. sts_stream_close) -----------------------------------
    def stream_open(self, chunk_frames: int, max_live: int, capacity_frames: int, capacity_phonemes: int = 0):
        """Opens the engine's stream: utterances are admitted between its steps (``stream_admit``), every ``stream_step`` decodes the next
        chunk of each live one.  Fixes chunk size, output rate, limiter, conv mode and conv math until ``stream_close``.
        ``capacity_phonemes`` > 0 opens a planned stream (sts_stream_open_ex): ``set_duration_plan``, ``set_speaker_mix``,
        ``set_gain_plan`` and ``set_forced_durations`` then apply to the next ``stream_admit``; 0 is sts_stream_open."""
        if capacity_phonemes:
            _check(self.lib, self.lib.sts_stream_open_ex(self.h, int(chunk_frames), int(max_live), int(capacity_frames), int(capacity_phonemes)))
        else:
            _check(self.lib, self.lib.sts_stream_open(self.h, int(chunk_frames), int(max_live), int(capacity_frames)))

    def stream_tables_info(self) -> dict:
        """The phoneme pool of a planned open stream (sts_stream_tables_info); zeros when none is open."""
        pl, cap, fr = C.c_int32(), C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.sts_stream_tables_info(self.h, C.addressof(pl), C.addressof(cap), C.addressof(fr)))
        return {"planned": bool(pl.value), "capacity_phonemes": int(cap.value), "free_phonemes": int(fr.value)}

    def stream_admit(self, ids, sid: Optional[Sequence[int]] = None, length_scale: Optional[Sequence[float]] = None, noise=None):
        """Admits the utterances ``ids`` as one packed batch.  ``noise``: None (the engine's setting, utterance b with seed + b) or one
        ``(noise_scale, noise_scale_w, seed)`` per utterance.  Returns ``(slots, n_samples)`` -- per utterance its slot (the ``utt`` of its
        chunks) and its total output samples -- or None when slots or frames do not suffice now (nothing has changed)."""
        p = PreparedBatch(ids, sid, length_scale)
        B = len(p)
        nz = None
        if noise is not None:
            nz = (StreamNoise * B)(*[StreamNoise(float(a), float(b), int(c) & 0xFFFFFFFFFFFFFFFF) for a, b, c in noise])
        slots = np.full(B, -1, np.int32)
        tot = np.zeros(B, np.int32)
        adm = C.c_int32()
        _check(self.lib, self.lib.sts_stream_admit(self.h, B, p.ptrs, p.n_p, p.sid_p, p.ls_p, None if nz is None else C.cast(nz, C.c_void_p),
                                                   slots.ctypes.data, tot.ctypes.data, C.addressof(adm)))
        if adm.value == 0:
            return None
        return [int(v) for v in slots], [int(v) for v in tot]

    def stream_step(self, on_chunk=None):
        """One step: ``on_chunk(slot, pcm: np.int16[], sample_offset)`` per live slot in ascending slot order (return True to stop that
        slot).  Returns (list of ``(slot, pcm, sample_offset)`` of this step, slots still live)."""
        got = []

        def _cb(user, utt, pcm, ns, off):
            arr = np.ctypeslib.as_array(pcm, shape=(ns,)).copy() if ns else np.zeros(0, np.int16)
            got.append((int(utt), arr, int(off)))
            return 1 if (on_chunk and on_chunk(int(utt), arr, int(off))) else 0
        cb = BATCH_CHUNK_CB(_cb)
        live = C.c_int32()
        _check(self.lib, self.lib.sts_stream_step(self.h, cb, None, C.addressof(live)))
        return got, int(live.value)

    def stream_info(self) -> dict:
        o, l, fs, ff, st = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.sts_stream_info(self.h, C.addressof(o), C.addressof(l), C.addressof(fs), C.addressof(ff), C.addressof(st)))
        return {"open": bool(o.value), "live": int(l.value), "free_slots": int(fs.value), "free_frames": int(ff.value), "steps": int(st.value)}

    def stream_loudness(self):
        """A measuring open stream (LOUD_MEASURE with ``set_loudness_streaming``): the slots the most recent ``stream_step`` retired, ascending,
        and their results -- ``(slots int32 [n], results LOUDNESS_DTYPE [n])``, each result what ``loudness()`` reports after a closed
        stream of that utterance.  Empty after a step that retired nothing (sts_stream_get_loudness)."""
        if not hasattr(self.lib, "sts_stream_get_loudness"):
            raise StsError("sts_stream_get_loudness: this library lacks the entry (it was added without a new ABI revision)")
        n = self.lib.sts_stream_get_loudness(self.h, None, None, 0)
        if n < 0:
            _check(self.lib, n)
        slots, out = np.zeros(n, np.int32), np.zeros(n, LOUDNESS_DTYPE)
        if n:
            rc = self.lib.sts_stream_get_loudness(self.h, slots.ctypes.data, out.ctypes.data, n)
            if rc < 0:
                _check(self.lib, rc)
        return slots, out

    def stream_close(self):
        """Drops the live slots without delivering and frees the pool."""
        _check(self.lib, self.lib.sts_stream_close(self.h))

    # -- open paragraphs (sts_para_open .. sts_para_close) ------------------------------------
    def para_open(self, chunk_frames: int, max_resident: int, capacity_frames: int, lead_frames: int = 0, fade_ms: float = 0.0):
        """Opens the engine's paragraph: ONE joined stream whose sentences are appended between its steps (``para_append``); every
        ``para_step`` delivers the next chunk of the joined signal once it can no longer change.  Fixes chunk size, output rate, limiter,
        conv mode, conv math and the join's lead and fade until ``para_close``."""
        _check(self.lib, self.lib.sts_para_open(self.h, int(chunk_frames), int(max_resident), int(capacity_frames), int(lead_frames), float(fade_ms)))

    def para_append(self, ids, sid: Optional[Sequence[int]] = None, length_scale: Optional[Sequence[float]] = None,
                    gap_frames: Optional[Sequence[int]] = None):
        """Appends the sentences ``ids`` as one packed batch; ``gap_frames[b]`` is the silence in front of sentence b (the paragraph's first:
        0).  Returns ``(frames, starts)`` -- per sentence its frame count and its start in output samples -- or None when slots or frames
        do not suffice now (nothing has changed; step, then retry)."""
        p = PreparedBatch(ids, sid, length_scale)
        B = len(p)
        gap = None if gap_frames is None else np.ascontiguousarray(gap_frames, np.int32)
        if gap is not None and gap.shape != (B,):
            raise ValueError("gap_frames takes one entry per appended sentence")
        frames = np.zeros(B, np.int32)
        start = np.zeros(B, np.int64)
        app = C.c_int32()
        _check(self.lib, self.lib.sts_para_append(self.h, B, p.ptrs, p.n_p, p.sid_p, p.ls_p, None if gap is None else gap.ctypes.data,
                                                  frames.ctypes.data, start.ctypes.data, C.addressof(app)))
        if app.value == 0:
            return None
        return [int(v) for v in frames], [int(v) for v in start]

    def para_finish(self, trail_frames: int = 0):
        """No more sentences will come: the joined signal ends ``trail_frames`` behind the last one, and every remaining chunk may leave."""
        _check(self.lib, self.lib.sts_para_finish(self.h, int(trail_frames)))

    def para_step(self, on_chunk=None):
        """One step: the next chunk of the joined signal, if it is deliverable.  ``on_chunk(pcm: np.int16[], sample_offset)`` may return True
        to stop the paragraph.  Returns (``(sample_offset, pcm)`` or None when nothing was deliverable, chunks deliverable after it)."""
        got = []

        def _cb(user, pcm, ns, off):
            arr = np.ctypeslib.as_array(pcm, shape=(ns,)).copy() if ns else np.zeros(0, np.int16)
            got.append((int(off), arr))
            return 1 if (on_chunk and on_chunk(arr, int(off))) else 0
        cb = CHUNK_CB(_cb)
        ready = C.c_int32()
        _check(self.lib, self.lib.sts_para_step(self.h, cb, None, C.addressof(ready)))
        return (got[0] if got else None), int(ready.value)

    def para_info(self) -> dict:
        o, f, r, fs = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        n, ff, fk, fd, st = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.sts_para_info(self.h, C.addressof(o), C.addressof(f), C.addressof(n), C.addressof(r), C.addressof(fs),
                                                C.addressof(ff), C.addressof(fk), C.addressof(fd), C.addressof(st)))
        return {"open": bool(o.value), "finished": bool(f.value), "sentences": int(n.value), "resident": int(r.value),
                "free_slots": int(fs.value), "free_frames": int(ff.value), "frames_known": int(fk.value),
                "frames_delivered": int(fd.value), "steps": int(st.value)}

    def para_close(self):
        """Frees the pool and drops what was not delivered."""
        _check(self.lib, self.lib.sts_para_close(self.h))

    def stream_paragraph(self, sentences_iter, chunk_frames: int, max_resident: int = 8, capacity_frames: int = 8192, sid_iter=None,
                         gap_frames: int = 0, lead_frames: int = 0, trail_frames: int = 0, fade_ms: float = 0.0, length_scale: float = 1.0):
        """A generator over the chunks ``(sample_offset, pcm)`` of the paragraph whose sentences (id sequences) ``sentences_iter`` yields one
        by one -- a language model's output, say: each sentence is appended as it arrives, ``gap_frames`` behind the one before, and
        whatever has become deliverable is drained before the next one is asked for.  ``sid_iter``: an iterable of speaker ids, one per
        sentence (None: 0); one that ends before the sentences do raises ValueError.  An append that finds no room is tried again after
        a step; a lack of slots is seen before any work, but a lack of frames only once the sentence's length is known, so every such
        attempt runs its text encoder and duration predictor again (never the flow): a pool with room for the sentences in flight spares
        that work.  The paragraph is closed when the generator ends or is closed."""
        self.para_open(chunk_frames, max_resident, capacity_frames, lead_frames, fade_ms)
        try:
            sids = iter(sid_iter) if sid_iter is not None else None
            first = True
            for ids in sentences_iter:
                sid = None
                if sids is not None:
                    try:
                        sid = [int(next(sids))]
                    except StopIteration:
                        raise ValueError("stream_paragraph: sid_iter ran out of speaker ids before sentences_iter ran out of sentences") from None
                while self.para_append([ids], sid, [length_scale], [0 if first else gap_frames]) is None:
                    chunk, _ = self.para_step()      # no room now: deliver, which retires sentences
                    if chunk is None:
                        raise StsError("stream_paragraph: a sentence does not fit the pool (capacity_frames) and nothing is left to deliver")
                    yield chunk
                first = False
                while True:
                    chunk, ready = self.para_step()
                    if chunk is None:
                        break
                    yield chunk
                    if ready == 0:
                        break
            if not first:
                self.para_finish(trail_frames)
                while True:
                    chunk, ready = self.para_step()
                    if chunk is None:
                        break
                    yield chunk
        finally:
            self.para_close()

    # -- batched -----------------------------------------------------------------------------
    def prepare(self, ids: Sequence[Sequence[int]], sid: Optional[Sequence[int]] = None,
                length_scale: Optional[Sequence[float]] = None) -> "PreparedBatch":
        """The argument arrays of run_batch built once, for a caller that submits the same batch object repeatedly (a benchmark
        loop, a retry): run_batch(prepared) then costs one foreign call."""
        return PreparedBatch(ids, sid, length_scale)

    def run_batch(self, ids, sid: Optional[Sequence[int]] = None, length_scale: Optional[Sequence[float]] = None) -> np.ndarray:
        """Runs the batch (ids: a sequence of id sequences, or a PreparedBatch) and leaves the PCM on the device (and, with
        set_host_pcm, in the engine's pinned host buffer); returns per-utterance sample counts (a fresh array per call).  Views handed out by
        pcm_host(copy=False) alias the engine's pinned buffer: the next run on this engine rewrites them in place."""
        p = ids if isinstance(ids, PreparedBatch) else PreparedBatch(ids, sid, length_scale)
        _check(self.lib, self.lib.sts_run_batch(self.h, p.B, p.ptrs, p.n_p, p.sid_p, p.ls_p, p.n_out_p, p.total_ref))
        self._total = int(p.total.value)
        self._n_out = p.n_out.copy()       # (the prepared object's own array is overwritten by its next run: ADVICE r04)
        return self._n_out

    def pcm_host(self, copy: bool = True) -> np.ndarray:
        """PCM of the last run on the host.  copy=False: a read-only view of the engine's pinned download buffer (valid until the
        next run on this engine; needs set_host_pcm(True), the default of this class)."""
        if not copy:
            ptr, cnt = C.POINTER(C.c_int16)(), C.c_int64()
            _check(self.lib, self.lib.sts_pcm_host_view(self.h, C.byref(ptr), C.byref(cnt)))
            if cnt.value == 0:
                return np.empty(0, np.int16)
            v = np.ctypeslib.as_array(ptr, shape=(cnt.value,))
            v.flags.writeable = False
            return v
        out = np.empty(self._total, np.int16)
        _check(self.lib, self.lib.sts_copy_pcm_host(self.h, out.ctypes.data, out.size))
        return out

    def profile_struct(self) -> "Profile":
        """The raw profile record of the last run (no dict built: for a timed loop that converts afterwards)."""
        p = Profile()
        _check(self.lib, self.lib.sts_get_profile_ex(self.h, C.byref(p), C.sizeof(p)))
        return p

    def pcm_to_device_ptr(self, ptr: int, capacity: int) -> None:
        _check(self.lib, self.lib.sts_copy_pcm_device(self.h, C.c_void_p(ptr), capacity))

    def infer_batch(self, ids, sid=None, length_scale=None) -> List[np.ndarray]:
        n_out = self.run_batch(ids, sid, length_scale)
        flat = self.pcm_host()
        offs = np.concatenate([[0], np.cumsum(n_out)])
        return [flat[offs[b]:offs[b + 1]].copy() for b in range(len(n_out))]

    def infer_joined(self, ids, sid=None, length_scale=None, join=None) -> np.ndarray:
        """A paragraph (include/summertts_hip.h sts_infer_ids_joined): the sentences ``ids`` run as one packed batch and are joined on the
        device into ONE int16 signal, which the resampler, loudness and the limiter see as a single utterance.  ``join``: None (back to
        back, no fade) or a mapping with any of ``gap_frames`` (B - 1 ints), ``lead_frames``, ``trail_frames`` and ``fade_ms``.  Pending
        forced durations, duration plans, speaker mixes and gain plans apply per sentence.  An invalid join raises and changes nothing."""
        p = ids if isinstance(ids, PreparedBatch) else PreparedBatch(ids, sid, length_scale)
        jp, keep = _join(p.B, join)
        out, n = C.POINTER(C.c_int16)(), C.c_int32()
        _check(self.lib, self.lib.sts_infer_ids_joined(self.h, p.B, p.ptrs, p.n_p, p.sid_p, p.ls_p, jp, C.byref(out), C.byref(n)))
        pcm = np.ctypeslib.as_array(out, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int16)
        self.lib.sts_free(out)
        return pcm

    def infer_joined_stream(self, ids, chunk_frames: int, sid=None, length_scale=None, join=None, on_chunk=None):
        """A paragraph, streamed (include/summertts_hip.h sts_infer_ids_joined_stream): the joined signal of ``infer_joined`` in chunks of
        ``chunk_frames`` frames of the JOINED time axis, in order.  ``on_chunk(pcm: np.int16[], sample_offset, t_seconds)`` is called per
        chunk (return True to end the call).  Returns the list of ``(sample_offset, pcm)``; ``self.stream_total`` holds the library's count
        of delivered samples."""
        import time
        p = ids if isinstance(ids, PreparedBatch) else PreparedBatch(ids, sid, length_scale)
        jp, keep = _join(p.B, join)
        out = []
        t0 = time.perf_counter()

        def _cb(user, pcm, ns, off):
            arr = np.ctypeslib.as_array(pcm, shape=(ns,)).copy() if ns else np.zeros(0, np.int16)
            out.append((int(off), arr))
            return 1 if (on_chunk and on_chunk(arr, int(off), time.perf_counter() - t0)) else 0
        cb = CHUNK_CB(_cb)
        total = C.c_int32()
        _check(self.lib, self.lib.sts_infer_ids_joined_stream(self.h, p.B, p.ptrs, p.n_p, p.sid_p, p.ls_p, jp, int(chunk_frames), cb, None,
                                                              C.byref(total)))
        self.stream_total = int(total.value)
        return out

    def join_offsets(self, B: int) -> np.ndarray:
        """Start of every sentence of the last ``infer_joined`` in output samples at the current output rate (sts_get_join_offsets)."""
        s = np.zeros(max(int(B), 1), np.int64)
        _check(self.lib, self.lib.sts_get_join_offsets(self.h, s.ctypes.data, int(B)))
        return s[:int(B)]

    # -- parity / diagnostics ---------------------------------------------------------------
    def set_forced_durations(self, dur: Optional[Sequence[int]]):
        if dur is None:
            _check(self.lib, self.lib.sts_set_forced_durations(self.h, None, 0))
            return
        d = np.ascontiguousarray(dur, dtype=np.int32)
        _check(self.lib, self.lib.sts_set_forced_durations(self.h, d.ctypes.data, d.size))

    _TABLE_ENTRY = "sts_set_%s"

    def _mix_gin(self):
        return int(self.info.gin_channels)

    def _table_failed(self, name, rc):
        _check(self.lib, rc)

    def set_duration_plan(self, n: Optional[Sequence[int]], plans=None):
        """Duration plan of the NEXT call only (include/summertts_hip.h sts_set_duration_plan).  ``n``: phoneme count of every utterance
        of that call; ``plans``: per utterance None or a mapping with any of ``rate`` (float per phoneme, multiplies the length scale),
        ``fixed`` (frames per phoneme, -1 = predicted), ``target_frames`` (the utterance's exact length; 0 = none).  ``n`` or ``plans``
        None drops a pending plan.  An invalid plan raises and changes nothing."""
        self._set_table("duration_plan", n, plans)

    def set_speaker_mix(self, mixes=None):
        """Speaker mix of the NEXT call only (include/summertts_hip.h sts_set_speaker_mix).  ``mixes``: per utterance of that call None
        (its plain sid) or a mapping with any of ``sid`` + ``weight`` (rows of the model's table and their weights), ``vector`` (a caller's
        embedding, gin_channels floats) and ``vector_weight`` (default 1).  None drops a pending mix.  An invalid mix raises and changes
        nothing."""
        self._set_table("speaker_mix", None, mixes)

    def set_gain_plan(self, n: Optional[Sequence[int]], plans=None):
        """Gain plan of the NEXT call only (include/summertts_hip.h sts_set_gain_plan).  ``n``: phoneme count of every utterance of that
        call; ``plans``: per utterance None or a mapping with ``gain_db`` (dB per phoneme, ``-inf`` = mute) and ``ramp_ms`` (width of the
        transition across a phoneme boundary, default 0).  ``n`` or ``plans`` None drops a pending plan.  An invalid plan raises and
        changes nothing."""
        self._set_table("gain_plan", n, plans)

    def set_pitch_plan(self, n: Optional[Sequence[int]], plans=None):
        """Pitch plan of the NEXT call only (include/summertts_hip.h sts_set_pitch_plan).  ``n``: phoneme count of every utterance of that
        call; ``plans``: per utterance None, a sequence of cents per phoneme (integers in [-600, 600]) or a mapping with ``cents``.  The
        formants move with the pitch.  ``n`` or ``plans`` None drops a pending plan.  An invalid plan raises and changes nothing."""
        self._set_table("pitch_plan", n, plans)

    def speaker_embedding(self, sid: int) -> np.ndarray:
        """Row ``sid`` of the model's speaker table: float32 [gin_channels] (sts_get_speaker_embedding)."""
        out = np.zeros(max(int(self.info.gin_channels), 1), np.float32)
        _check(self.lib, self.lib.sts_get_speaker_embedding(self.h, int(sid), out.ctypes.data, int(self.info.gin_channels)))
        return out[:int(self.info.gin_channels)]

    def phoneme_offsets(self, total_phonemes: int) -> np.ndarray:
        """Start of every phoneme of the last run in output samples at the current output rate, packed like ``durations``."""
        s = np.zeros(total_phonemes, np.int64)
        _check(self.lib, self.lib.sts_get_phoneme_offsets(self.h, s.ctypes.data, s.size))
        return s

    def set_record_taps(self, on: bool):
        _check(self.lib, self.lib.sts_set_record_taps(self.h, 1 if on else 0))

    def set_noise(self, noise_scale: float = 0.0, noise_scale_w: float = 0.0, seed: int = 0):
        """Sampling noise of every later call (include/summertts_hip.h sts_set_noise): ``noise_scale`` scales the prior sample
        (z_p = m + eps * logs * noise_scale, the reference's expression), ``noise_scale_w`` the stochastic duration predictor's
        latent; utterance b of a batch samples with ``seed + b``.  All zero (the default) = the reference's noise-free ``infer``."""
        _check(self.lib, self.lib.sts_set_noise(self.h, float(noise_scale), float(noise_scale_w), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def noise(self):
        """(noise_scale, noise_scale_w, seed) as set by ``set_noise``."""
        ns, nsw, seed = C.c_float(), C.c_float(), C.c_uint64()
        _check(self.lib, self.lib.sts_get_noise(self.h, C.byref(ns), C.byref(nsw), C.byref(seed)))
        return ns.value, nsw.value, seed.value

    def set_output_rate(self, rate: int):
        """PCM sample rate of every later call (include/summertts_hip.h sts_set_output_rate): 0 or 16000 = the model's native rate, else an
        integer in [8000, 48000], resampled on the device.  An invalid rate raises and leaves the setting unchanged."""
        _check(self.lib, self.lib.sts_set_output_rate(self.h, int(rate)))

    def output_rate(self) -> int:
        return int(self.lib.sts_get_output_rate(self.h))

    def set_loudness(self, mode: int, target_lufs: float = -16.0, peak_dbfs: float = -1.0):
        """Loudness of every later whole-utterance call (include/summertts_hip.h sts_set_loudness): LOUD_OFF, LOUD_MEASURE (PCM unchanged,
        results in ``loudness()``) or LOUD_NORMALIZE (each utterance cast with its own gain towards ``target_lufs``, peak at most
        ``peak_dbfs``).  Invalid arguments raise and leave the setting unchanged."""
        _check(self.lib, self.lib.sts_set_loudness(self.h, int(mode), float(target_lufs), float(peak_dbfs)))

    def loudness_mode(self):
        """(mode, target_lufs, peak_dbfs) as set by ``set_loudness``."""
        m, t, p = C.c_int(), C.c_float(), C.c_float()
        _check(self.lib, self.lib.sts_get_loudness_mode(self.h, C.byref(m), C.byref(t), C.byref(p)))
        return m.value, t.value, p.value

    def loudness(self) -> np.ndarray:
        """Results of the last whole-utterance call, or of the last stream that measured (``set_loudness_streaming``), one per utterance
        in call order (LOUDNESS_DTYPE; empty in mode LOUD_OFF)."""
        n = self.lib.sts_get_loudness(self.h, None, 0)
        if n < 0:
            _check(self.lib, n)
        out = np.zeros(n, LOUDNESS_DTYPE)
        if n:
            rc = self.lib.sts_get_loudness(self.h, out.ctypes.data, n)
            if rc < 0:
                _check(self.lib, rc)
        return out

    def set_loudness_streaming(self, enable: bool = True):
        """Let streaming calls run under LOUD_MEASURE (sts_set_loudness_streaming): each step measures the samples it delivers from a state
        carried per utterance, the chunks are those of a stream without loudness, and ``loudness()`` afterwards returns the whole call's
        entries for every chunk size (of a stopped utterance: the measurement of what was delivered).  LOUD_NORMALIZE stays refused in a
        stream.  Off by default; persists."""
        _check(self.lib, self.lib.sts_set_loudness_streaming(self.h, 1 if enable else 0))

    def loudness_streaming(self) -> bool:
        """The switch set by ``set_loudness_streaming``."""
        return bool(self.lib.sts_get_loudness_streaming(self.h))

    def set_limiter(self, mode: int, gain_db: float = 0.0, ceiling_dbfs: float = -1.0, lookahead_ms: float = 5.0):
        """Look-ahead peak limiter of every later whole-utterance call (include/summertts_hip.h sts_set_limiter): LIMITER_OFF or
        LIMITER_ON (make-up gain ``gain_db``, then no sample above ``ceiling_dbfs``; results in ``limiter()``).  Invalid arguments raise
        and leave the setting unchanged."""
        _check(self.lib, self.lib.sts_set_limiter(self.h, int(mode), float(gain_db), float(ceiling_dbfs), float(lookahead_ms)))

    def set_eq(self, bands=None):
        """Parametric equaliser of every later whole-utterance call (include/summertts_hip.h sts_set_eq): up to 4 bands
        ``(type, freq_hz, gain_db, q)`` (EQ_PEAK, EQ_LOWSHELF, EQ_HIGHSHELF, EQ_HIGHPASS, EQ_LOWPASS) in front of loudness and the
        limiter; None or an empty list switches it off.  Invalid bands raise and change nothing; streaming calls are refused while
        bands are set, unless ``set_eq_streaming(True)``."""
        n, arr = _eq_bands(bands)
        _check(self.lib, self.lib.sts_set_eq(self.h, n, arr))

    def set_eq_streaming(self, enable: bool = True):
        """Let streaming calls run while an equaliser is set (sts_set_eq_streaming): each step continues the filter from a state carried per
        utterance, and the concatenated chunks are the whole call's PCM for every chunk size.  Off by default; persists until changed."""
        _check(self.lib, self.lib.sts_set_eq_streaming(self.h, 1 if enable else 0))

    def set_pitch_streaming(self, enable: bool = True):
        """Let ``infer_ids_stream`` and ``infer_batch_stream`` run with a pitch plan pending (sts_set_pitch_streaming): every step warps its
        decode windows, and the concatenated chunks are the whole call's PCM with the same plan for every chunk size.  Off by default;
        persists until changed.  Open streams, joined runs, paragraphs and the pool's streams still refuse a plan."""
        _check(self.lib, self.lib.sts_set_pitch_streaming(self.h, 1 if enable else 0))

    def get_eq_streaming(self) -> bool:
        """The switch set by ``set_eq_streaming``."""
        return bool(self.lib.sts_get_eq_streaming(self.h))

    def get_eq(self):
        """The bands set by ``set_eq``: a list of ``(type, freq_hz, gain_db, q)``."""
        n = C.c_int32()
        arr = (EqBand * EQ_MAX_BANDS)()
        _check(self.lib, self.lib.sts_get_eq(self.h, C.byref(n), arr, EQ_MAX_BANDS))
        return [(int(arr[i].type), float(arr[i].freq_hz), float(arr[i].gain_db), float(arr[i].q)) for i in range(n.value)]

    def limiter_mode(self):
        """(mode, gain_db, ceiling_dbfs, lookahead_ms) as set by ``set_limiter``."""
        m, g, c, l = C.c_int(), C.c_float(), C.c_float(), C.c_float()
        _check(self.lib, self.lib.sts_get_limiter_mode(self.h, C.byref(m), C.byref(g), C.byref(c), C.byref(l)))
        return m.value, g.value, c.value, l.value

    def limiter(self) -> np.ndarray:
        """Results of the last whole-utterance call, one per utterance in call order (LIMITER_DTYPE; empty with the limiter off)."""
        n = self.lib.sts_get_limiter(self.h, None, 0)
        if n < 0:
            _check(self.lib, n)
        out = np.zeros(n, LIMITER_DTYPE)
        if n:
            rc = self.lib.sts_get_limiter(self.h, out.ctypes.data, n)
            if rc < 0:
                _check(self.lib, rc)
        return out

    def set_conv_math(self, mode):
        """Arithmetic of the decoder trunk convs: 0 / 'bf16x3' = fp32 operands as three bf16 terms on the bf16 matrix cores,
        1 / 'f32' = the exact-fp32 MFMA instruction, 3 / 'f16x2' = two fp16 terms, three products (default; a call whose
        activations leave fp16's range is repeated as 'bf16x3'; Profile.conv_math_fallbacks counts them)."""
        m = {"bf16x3": 0, "f32": 1, "bf16x3_all": 2, "f16x2": 3}.get(mode, mode)
        _check(self.lib, self.lib.sts_set_conv_math(self.h, int(m)))

    def set_conv_mode(self, mode: int):
        _check(self.lib, self.lib.sts_set_conv_mode(self.h, mode))

    def debug_set(self, key: str, value: int):
        """Test hooks (include/summertts_hip.h sts_debug_set): 'attn_block_min_wgs' | 'flow_fused' | 'launch_ahead' | ..."""
        _check(self.lib, self.lib.sts_debug_set(self.h, {"attn_block_min_wgs": 1, "flow_fused": 5, "launch_ahead": 6, "attn_reg": 7, "dds_tail": 8, "pcm_direct": 9, "memo_clear": 10, "h2p": 11, "h2p_tile": 12, "chain_streams": 13, "tail_fused": 14, "ups_rowph": 15, "stream_retry_step": 16, "stream_direct": 17, "poison": 18, "col_proj": 19, "sdp_pre_ride": 20}[key], int(value)))

    def set_profiling(self, on):
        """False / True: no / all eight stage events per run; 2: only the two events around the decoder's matrix-core region (the
        per-stage times of Profile then read 0; every event is a barrier packet between two kernels, so the timed headline step uses 2)."""
        _check(self.lib, self.lib.sts_set_profiling(self.h, 2 if on == 2 else (1 if on else 0)))

    def profile(self) -> dict:
        p = Profile()
        _check(self.lib, self.lib.sts_get_profile_ex(self.h, C.byref(p), C.sizeof(p)))
        return p.as_dict()

    def tap(self, name: str) -> np.ndarray:
        ptr = C.POINTER(C.c_float)()
        ch, ln = C.c_int32(), C.c_int64()
        _check(self.lib, self.lib.sts_get_tap(self.h, name.encode(), C.byref(ptr), C.byref(ch), C.byref(ln)))
        a = np.ctypeslib.as_array(ptr, shape=(ch.value, ln.value)).copy()
        self.lib.sts_free(ptr)
        return a

    def durations(self, total_phonemes: int) -> np.ndarray:
        d = np.zeros(total_phonemes, np.int32)
        _check(self.lib, self.lib.sts_get_durations(self.h, d.ctypes.data, d.size))
        return d

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.sts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_conv1d(x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], pad: int, dil: int = 1,
                 stride_transposed: int = 0, depthwise: bool = False, in_slope: float = 0.0, in_act: int = 0,
                 mode: int = 0, device: int = 0, iters: int = 0):
    """One conv through the engine's kernels.  x: [Cin, L]; w: [Cout, k, Cin] (reference layout).
    With iters > 0 returns (y, mean milliseconds per launch)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    cout, k = w.shape[0], w.shape[1]
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    y = C.POINTER(C.c_float)()
    lout = C.c_int32()
    ms = C.c_float(0.0)
    _check(lib, lib.sts_debug_conv1d_bench(device, x.ctypes.data, x.shape[0], x.shape[1], w.ctypes.data,
                                           None if b is None else b.ctypes.data, cout, k, pad, dil, stride_transposed,
                                           1 if depthwise else 0, in_slope, in_act, mode, C.byref(y), C.byref(lout),
                                           iters, C.byref(ms)))
    out = np.ctypeslib.as_array(y, shape=(cout, lout.value)).copy()
    lib.sts_free(y)
    return (out, float(ms.value)) if iters > 0 else out


def debug_conv_h2p(x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], dil: int = 1, res: Optional[np.ndarray] = None,
                   in_slope: float = 0.1, out_slope: float = 0.1, tile: int = -1, members: int = 1, device: int = 0, iters: int = 0):
    """One 'same'-padded conv through the pre-split path (conv_h2p.hip).  x: [Cin, L]; w: [Cout, k, Cin].  Returns the three output
    forms decoded to fp32 [Cout, L]: (y, y16, yp) -- yp = lrelu(out, out_slope) to the two-term precision -- and ms per launch."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    cout, k = w.shape[0], w.shape[1]
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = None if res is None else np.ascontiguousarray(res, np.float32)
    L = x.shape[1]
    y = np.zeros((cout, L), np.float32); y16 = np.zeros((cout, L), np.float32); yp = np.zeros((cout, L), np.float32)
    ms = C.c_float(0.0)
    lib.sts_debug_conv_h2p.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.POINTER(C.c_float)]
    _check(lib, lib.sts_debug_conv_h2p(device, x.ctypes.data, x.shape[0], L, w.ctypes.data, None if b is None else b.ctypes.data, cout, k, dil,
                                       None if r is None else r.ctypes.data, in_slope, out_slope, tile, members, y.ctypes.data,
                                       y16.ctypes.data, yp.ctypes.data, iters, C.byref(ms)))
    return y, y16, yp, float(ms.value)     # (iters < 0: |iters| timed launches WITHOUT the fp32 [C][L] output: a layer's second conv as the engine runs it)


def debug_conv1d_packed(x: np.ndarray, lengths, w: np.ndarray, bias: Optional[np.ndarray], dil: int = 1, stride_transposed: int = 0,
                        depthwise: bool = False, in_slope: float = 0.0, in_act: int = 0, mode: int = 0, device: int = 0, return_ovf: bool = False):
    """One conv on utterances packed back to back along the time axis (sts_debug_conv1d_packed).  x: [Cin, sum(lengths)]; w: [Cout, k, Cin].
    'Same' padding (odd k), or a transposed conv with pad = (k - stride) / 2: the output holds the segments in the same order, each
    stride times as long.  return_ovf: also the overflow word of the two-term fp16 kernels."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    ln = np.ascontiguousarray(lengths, np.int32)
    cout, k = w.shape[0], w.shape[1]
    pad = (k - stride_transposed) // 2 if stride_transposed else dil * (k - 1) // 2
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    y = C.POINTER(C.c_float)()
    lout = C.c_int32()
    ovf = C.c_uint32(0)
    lib.sts_debug_conv1d_packed.argtypes = lib.sts_debug_conv1d.argtypes + [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)]
    _check(lib, lib.sts_debug_conv1d_packed(device, x.ctypes.data, x.shape[0], x.shape[1], w.ctypes.data, None if b is None else b.ctypes.data,
                                            cout, k, pad, dil, stride_transposed, 1 if depthwise else 0, in_slope, in_act, mode,
                                            C.byref(y), C.byref(lout), ln.ctypes.data, ln.size, C.byref(ovf)))
    out = np.ctypeslib.as_array(y, shape=(cout, lout.value)).copy()
    lib.sts_free(y)
    return (out, int(ovf.value)) if return_ovf else out


class ConvEpiOpts(C.Structure):
    """sts_conv_epi_opts (include/summertts_hip.h)."""
    _fields_ = [("size_bytes", C.c_int32), ("epi", C.c_int32), ("epi_flag", C.c_int32), ("H", C.c_int32), ("gate_perm", C.c_int32),
                ("in_reflect", C.c_int32), ("nsum", C.c_int32), ("kslices", C.c_int32),
                ("ubias", C.c_void_p), ("res", C.c_void_p), ("y_init", C.c_void_p), ("aux_init", C.c_void_p), ("xs1", C.c_void_p),
                ("xs2", C.c_void_p), ("aux_out", C.c_void_p), ("pcm_out", C.c_void_p)]


EPI_STORE, EPI_RESADD, EPI_SUB, EPI_GATE, EPI_RESSKIP, EPI_TANH_PCM = 0, 1, 3, 4, 5, 6      # kernels.hpp Epilogue
CONV_EPI_SENTINEL = 0xFFFFFFFF          # what the columns outside the output segments hold (pcm: 0x7FFF) ...
CONV_EPI_SENTINEL_RMW = 0x2F5A5A5A      # ... and in a tensor that was given initial values: finite, so that old + v changes its bits


def debug_conv1d_epi(x: np.ndarray, lengths, w: np.ndarray, bias: Optional[np.ndarray], dil: int = 1, stride_transposed: int = 0,
                     in_slope: float = 0.0, in_act: int = 0, mode: int = 0, gap: int = 0, epi: int = EPI_STORE, epi_flag: int = 0, H: int = 0,
                     gate_perm: int = 0, in_reflect: int = 0, nsum: int = 0, kslices: int = 1, ubias=None, res=None, y_init=None,
                     aux_init=None, xs1=None, xs2=None, device: int = 0, size_bytes: Optional[int] = None, want_aux: Optional[bool] = None,
                     want_pcm: Optional[bool] = None):
    """One packed conv with an engine epilogue and operand form (sts_debug_conv1d_epi).  x: [Cin, sum(lengths) + B gap], every segment followed
    by `gap` unused columns; the other operands have the shape of the tensor they belong to, ubias is [Cout, B] in source row order.  Returns a
    dict: y [rows, Lout] (kslices > 1: [kslices, Cout, Lout]), ovf, and aux [H or 1, Lout] / pcm [Lout] for RESSKIP / TANH_PCM."""
    lib = load_library()
    f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
    ptr = lambda v: None if v is None else v.ctypes.data
    x, w, b = f32(x), f32(w), f32(bias)
    ln = np.ascontiguousarray(lengths, np.int32)
    cout, k = w.shape[0], w.shape[1]
    scale = max(stride_transposed, 1)
    lout_want = x.shape[1] * scale + (ln.size if in_reflect else 0)
    pad = (k - stride_transposed) // 2 if stride_transposed else dil * (k - 1) // 2
    keep = [f32(v) for v in (ubias, res, y_init, aux_init, xs1, xs2)]
    if want_aux is None:
        want_aux = epi in (EPI_RESSKIP, EPI_TANH_PCM)
    if want_pcm is None:
        want_pcm = epi == EPI_TANH_PCM
    aux = np.zeros((H if epi == EPI_RESSKIP else 1, lout_want), np.float32) if want_aux else None
    pcm = np.zeros(lout_want, np.int16) if want_pcm else None
    o = ConvEpiOpts(C.sizeof(ConvEpiOpts) if size_bytes is None else size_bytes, epi, epi_flag, H, gate_perm, in_reflect, nsum, kslices,
                    *[ptr(v) for v in keep], ptr(aux), ptr(pcm))
    y = C.POINTER(C.c_float)()
    lout = C.c_int32()
    ovf = C.c_uint32(0)
    lib.sts_debug_conv1d_epi.argtypes = lib.sts_debug_conv1d.argtypes + [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(ConvEpiOpts), C.c_int32]
    _check(lib, lib.sts_debug_conv1d_epi(device, x.ctypes.data, x.shape[0], x.shape[1], w.ctypes.data, ptr(b), cout, k, pad, dil, stride_transposed,
                                         0, in_slope, in_act, mode, C.byref(y), C.byref(lout), ln.ctypes.data, ln.size, C.byref(ovf),
                                         C.byref(o), gap))
    assert lout.value == lout_want, (lout.value, lout_want)
    rows = H if epi in (EPI_GATE, EPI_RESSKIP) else cout
    out = np.ctypeslib.as_array(y, shape=(kslices * rows, lout.value)).copy()
    lib.sts_free(y)
    if kslices > 1:
        out = out.reshape(kslices, rows, lout.value)
    return {"y": out, "ovf": int(ovf.value), "aux": aux, "pcm": pcm}


def debug_conv_h2p_packed(x: np.ndarray, lengths, w: np.ndarray, bias: Optional[np.ndarray], dil: int = 1, res: Optional[np.ndarray] = None,
                          in_slope: float = 0.1, out_slope: float = 0.1, tile: int = -1, members: int = 1, device: int = 0):
    """debug_conv_h2p on utterances packed back to back (sts_debug_conv_h2p_packed).  x, res: [C, sum(lengths)].  Returns (y, y16, yp, ovf)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    ln = np.ascontiguousarray(lengths, np.int32)
    cout, k = w.shape[0], w.shape[1]
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = None if res is None else np.ascontiguousarray(res, np.float32)
    L = x.shape[1]
    y = np.zeros((cout, L), np.float32); y16 = np.zeros((cout, L), np.float32); yp = np.zeros((cout, L), np.float32)
    ovf = C.c_uint32(0)
    lib.sts_debug_conv_h2p_packed.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)]
    _check(lib, lib.sts_debug_conv_h2p_packed(device, x.ctypes.data, x.shape[0], L, w.ctypes.data, None if b is None else b.ctypes.data, cout, k, dil,
                                              None if r is None else r.ctypes.data, in_slope, out_slope, tile, members, y.ctypes.data,
                                              y16.ctypes.data, yp.ctypes.data, ln.ctypes.data, ln.size, C.byref(ovf)))
    return y, y16, yp, int(ovf.value)


def debug_conv_h2w(x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], dil: int = 1, res: Optional[np.ndarray] = None,
                   in_slope: float = 0.1, out_slope: float = 1.0, members: int = 1, device: int = 0, iters: int = 0):
    """One 'same'-padded conv through the Winograd-domain lab kernel (conv_h2w.hip).  x: [C, L]; w: [C, k, C].  Returns (y, y16, ms)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    c, k = w.shape[0], w.shape[1]
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = None if res is None else np.ascontiguousarray(res, np.float32)
    L = x.shape[1]
    y = np.zeros((c, L), np.float32); y16 = np.zeros((c, L), np.float32)
    ms = C.c_float(0.0)
    lib.sts_debug_conv_h2w.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
    _check(lib, lib.sts_debug_conv_h2w(device, x.ctypes.data, c, L, w.ctypes.data, None if b is None else b.ctypes.data, k, dil,
                                       None if r is None else r.ctypes.data, in_slope, out_slope, members, y.ctypes.data, y16.ctypes.data, iters, C.byref(ms)))
    return y, y16, float(ms.value)


def debug_wino_pack(w: np.ndarray) -> np.ndarray:
    """Winograd-domain transform of conv weights w[Cout][k][Cin] -> U[seg][4][Cin_pad][Cout_pad] (host only)."""
    lib = load_library()
    w = np.ascontiguousarray(w, dtype=np.float32)
    co, k, ci = w.shape
    cip, cop = (ci + 15) // 16 * 16, (co + 31) // 32 * 32
    nseg = {0: k // 3, 2: (k - 2) // 3 + 1, 1: (k - 4) // 3 + 2}[k % 3]
    out = np.zeros((nseg, 4, cip, cop), np.float32)
    rc = lib.sts_debug_wino_pack(w.ctypes.data_as(C.c_void_p), co, k, ci, out.ctypes.data_as(C.c_void_p), C.c_int64(out.size))
    if rc != nseg:
        raise StsError(f"sts_debug_wino_pack: {rc}")
    return out


class Pool:
    """``sts_pool``: N engines on one GPU behind one request queue (dynamic packed batching)."""

    def __init__(self, blob: np.ndarray, device: int = 0, n_engines: int = 2, max_batch: int = 8):
        self.lib = load_library()
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self.h = C.c_void_p()
        self.lib.sts_pool_last_error.restype = C.c_char_p
        self.lib.sts_pool_submit.restype = C.c_int64
        self.lib.sts_pool_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float]
        self.lib.sts_pool_submit_ex.restype = C.c_int64
        self.lib.sts_pool_submit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64]
        self.lib.sts_pool_wait.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(C.c_int32)]
        self.lib.sts_pool_create.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.sts_pool_destroy.argtypes = [C.c_void_p]
        self.lib.sts_pool_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self._streams: Dict[int, object] = {}      # ticket -> the ctypes callback of a streaming request (kept alive until it is waited)
        rc = self.lib.sts_pool_create(blob.ctypes.data, blob.nbytes, device, n_engines, max_batch, C.byref(self.h))
        if rc != 0:
            raise StsError(f"sts_pool_create: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def submit_stream(self, ids: Sequence[int], chunk_frames: int, on_chunk, sid: int = 0, length_scale: float = 1.0,
                      noise_scale: float = 0.0, noise_scale_w: float = 0.0, seed: int = 0, plan=None, mix=None, gain=None) -> int:
        """Queue one streaming request (sts_pool_submit_stream).  ``on_chunk(pcm: np.int16[], sample_offset)`` runs on the pool's worker
        thread (return True to stop this request); it must not wait on a ticket of this pool.  ``wait(ticket)`` then returns the number of
        samples delivered.  ``plan``, ``mix``, ``gain``: this request's own duration plan, speaker mix and gain plan, each None or a mapping
        as the ``Synthesizer.set_*`` of its kind takes per utterance (sts_pool_submit_stream_ex; any combination)."""
        a = np.ascontiguousarray(ids, dtype=np.int32)

        def _cb(user, pcm, ns, off):
            arr = np.ctypeslib.as_array(pcm, shape=(ns,)).copy() if ns else np.zeros(0, np.int16)
            return 1 if on_chunk(arr, off) else 0
        cb = CHUNK_CB(_cb)
        if plan is None and mix is None and gain is None:
            t = int(self.lib.sts_pool_submit_stream(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale), float(noise_scale_w),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(chunk_frames), cb, None))
        else:
            keep, ptr = [], [None, None, None]
            if plan is not None:
                _, arr, k = _dur_plans([a.size], [plan]); keep += [arr, k]; ptr[0] = C.cast(arr, C.c_void_p)
            if mix is not None:
                arr, k = _speaker_mixes([mix]); keep += [arr, k]; ptr[1] = C.cast(arr, C.c_void_p)
            if gain is not None:
                _, arr, k = _gain_plans([a.size], [gain]); keep += [arr, k]; ptr[2] = C.cast(arr, C.c_void_p)
            t = int(self.lib.sts_pool_submit_stream_ex(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale), float(noise_scale_w),
                                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(chunk_frames), cb, None, ptr[0], ptr[1], ptr[2]))
        if t <= 0:
            raise StsError(f"sts_pool_submit_stream: {t}: {self.lib.sts_pool_last_error().decode()}")
        self._streams[t] = cb
        return t

    def submit(self, ids: Sequence[int], sid: int = 0, length_scale: float = 1.0, noise_scale: float = 0.0,
               noise_scale_w: float = 0.0, seed: int = 0, plan=None, mix=None, gain=None, pitch=None) -> int:
        """Queue one request; the noise arguments are this request's own (``Synthesizer.set_noise``; ``seed`` is used as given), and so
        is ``plan``: None or a mapping as ``Synthesizer.set_duration_plan`` takes per utterance (sts_pool_submit_plan), or ``mix``: None
        or a mapping as ``Synthesizer.set_speaker_mix`` takes per utterance (sts_pool_submit_mix).  One request carries a plan or a mix,
        not both.  ``gain``: None or a mapping as ``Synthesizer.set_gain_plan`` takes per utterance (sts_pool_submit_gain); a request with
        a gain plan carries neither of the other two.  ``pitch``: None or the cents per phoneme as ``Synthesizer.set_pitch_plan`` takes
        them per utterance (sts_pool_submit_pitch); a request with a pitch plan carries none of the other three."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        if pitch is not None:
            if plan is not None or mix is not None or gain is not None:
                raise ValueError("a request with a pitch plan carries no duration plan, no mix and no gain plan")
            _, arr, keep = _pitch_plans([a.size], [pitch])
            t = int(self.lib.sts_pool_submit_pitch(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale), float(noise_scale_w),
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, C.cast(arr, C.c_void_p)))
            if t <= 0:
                raise StsError(f"sts_pool_submit: {t}: {self.lib.sts_pool_last_error().decode()}")
            return t
        if plan is not None and mix is not None:
            raise ValueError("a request carries a plan or a mix, not both")
        if gain is not None and (plan is not None or mix is not None):
            raise ValueError("a request with a gain plan carries no duration plan and no mix")
        if gain is not None:
            _, arr, keep = _gain_plans([a.size], [gain])
            t = int(self.lib.sts_pool_submit_gain(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale), float(noise_scale_w),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, C.cast(arr, C.c_void_p)))
        elif mix is not None:
            arr, keep = _speaker_mixes([mix])
            t = int(self.lib.sts_pool_submit_mix(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale), float(noise_scale_w),
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, C.cast(arr, C.c_void_p)))
        elif plan is not None:
            _, arr, keep = _dur_plans([a.size], [plan])
            t = int(self.lib.sts_pool_submit_plan(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale), float(noise_scale_w),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, arr[0].rate, arr[0].fixed, arr[0].target_frames))
        elif noise_scale == 0.0 and noise_scale_w == 0.0 and seed == 0:
            t = int(self.lib.sts_pool_submit(self.h, a.ctypes.data, a.size, sid, length_scale))
        else:
            t = int(self.lib.sts_pool_submit_ex(self.h, a.ctypes.data, a.size, sid, length_scale, float(noise_scale),
                                                float(noise_scale_w), int(seed) & 0xFFFFFFFFFFFFFFFF))
        if t <= 0:
            raise StsError(f"sts_pool_submit: {t}: {self.lib.sts_pool_last_error().decode()}")
        return t

    def submit_joined(self, ids, sid=None, length_scale=None, noise_scale: float = 0.0, noise_scale_w: float = 0.0, seed: int = 0,
                      join=None) -> int:
        """Queue one paragraph (sts_pool_submit_joined): the sentences ``ids`` with ``join`` as ``Synthesizer.infer_joined`` takes it.  One
        ticket, one PCM; it runs as its own packed batch, whatever ``max_batch`` is.  Sentence b samples with ``seed + b``."""
        p = PreparedBatch(ids, sid, length_scale)
        jp, keep = _join(p.B, join)
        t = int(self.lib.sts_pool_submit_joined(self.h, p.B, p.ptrs, p.n_p, p.sid_p, p.ls_p, float(noise_scale), float(noise_scale_w),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, jp))
        if t <= 0:
            raise StsError(f"sts_pool_submit_joined: {t}: {self.lib.sts_pool_last_error().decode()}")
        return t

    def wait(self, ticket: int) -> np.ndarray:
        """The PCM of a whole-utterance or joined request; for a streaming request (submit_stream) the number of samples delivered."""
        p = C.POINTER(C.c_int16)()
        n = C.c_int32()
        rc = self.lib.sts_pool_wait(self.h, ticket, C.byref(p), C.byref(n))
        if ticket in self._streams:
            self._streams.pop(ticket)
            if rc != 0:
                raise StsError(f"sts_pool_wait: {rc}: {self.lib.sts_pool_last_error().decode()}")
            return int(n.value)
        if rc != 0:
            raise StsError(f"sts_pool_wait: {rc}: {self.lib.sts_pool_last_error().decode()}")
        out = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int16)
        self.lib.sts_free(p)
        return out

    def set_output_rate(self, rate: int):
        """``Synthesizer.set_output_rate`` for every engine of the pool; raises while any request is outstanding (STS_ESTATE)."""
        rc = self.lib.sts_pool_set_output_rate(self.h, int(rate))
        if rc != 0:
            raise StsError(f"sts_pool_set_output_rate: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def set_loudness(self, mode: int, target_lufs: float = -16.0, peak_dbfs: float = -1.0):
        """``Synthesizer.set_loudness`` for every engine of the pool (LOUD_OFF or LOUD_NORMALIZE); raises while any request is outstanding
        (STS_ESTATE)."""
        rc = self.lib.sts_pool_set_loudness(self.h, int(mode), float(target_lufs), float(peak_dbfs))
        if rc != 0:
            raise StsError(f"sts_pool_set_loudness: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def set_limiter(self, mode: int, gain_db: float = 0.0, ceiling_dbfs: float = -1.0, lookahead_ms: float = 5.0):
        """``Synthesizer.set_limiter`` for every engine of the pool; raises while any request is outstanding (STS_ESTATE)."""
        rc = self.lib.sts_pool_set_limiter(self.h, int(mode), float(gain_db), float(ceiling_dbfs), float(lookahead_ms))
        if rc != 0:
            raise StsError(f"sts_pool_set_limiter: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def set_eq(self, bands=None):
        """``Synthesizer.set_eq`` for every engine of the pool (one setting for every request); raises while any request is outstanding
        (STS_ESTATE).  Streamed requests are refused while bands are set, unless ``set_eq_streaming``."""
        n, arr = _eq_bands(bands)
        rc = self.lib.sts_pool_set_eq(self.h, n, arr)
        if rc != 0:
            raise StsError(f"sts_pool_set_eq: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def set_eq_streaming(self, enable: bool = True):
        """``Synthesizer.set_eq_streaming`` for every engine of the pool: streamed requests run while bands are set.  Raises while any
        request is outstanding (STS_ESTATE)."""
        rc = self.lib.sts_pool_set_eq_streaming(self.h, 1 if enable else 0)
        if rc != 0:
            raise StsError(f"sts_pool_set_eq_streaming: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def set_stream_admission(self, enable: bool = True):
        """Streamed groups run as open streams: a worker admits queued streaming requests of its group's chunk size between the steps of
        the running stream (sts_pool_set_stream_admission).  Raises while any request is outstanding (STS_ESTATE)."""
        rc = self.lib.sts_pool_set_stream_admission(self.h, 1 if enable else 0)
        if rc != 0:
            raise StsError(f"sts_pool_set_stream_admission: {rc}: {self.lib.sts_pool_last_error().decode()}")

    def stream_admission(self) -> bool:
        return bool(self.lib.sts_pool_get_stream_admission(self.h))

    def stream_stats(self):
        """(streamed groups run as open streams, requests admitted into a running one)"""
        g, a = C.c_int64(), C.c_int64()
        self.lib.sts_pool_stream_stats(self.h, C.addressof(g), C.addressof(a))
        return int(g.value), int(a.value)

    def stats(self):
        b, r = C.c_int64(), C.c_int64()
        self.lib.sts_pool_stats(self.h, C.byref(b), C.byref(r))
        return int(b.value), int(r.value)

    def close(self):
        if self.h:
            self.lib.sts_pool_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_gather_layout(counts: Sequence[int]):
    """Host arithmetic of the RCCL gather buffer (sts_multi_gather_layout): -> (offsets per rank, extent), in samples."""
    lib = load_library()
    lib.sts_multi_gather_layout.restype = C.c_int64
    lib.sts_multi_gather_layout.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    c = np.ascontiguousarray(counts, dtype=np.int64)
    off = np.zeros(c.size, np.int64)
    total = int(lib.sts_multi_gather_layout(c.ctypes.data, c.size, off.ctypes.data))
    return off, total


class MultiDevice(_TableSetters):
    """``sts_multi``: one process, one engine per listed HIP device; batches are sharded by utterance."""

    MODES = {"auto": 0, "rccl": 1, "download": 2}

    def __init__(self, blob: np.ndarray, devices: Sequence[int], gather: str = "auto"):
        """gather: 'auto' / 'download' (every device downloads its own shard) | 'rccl' (opt-in: RCCL gather to devices[0];
        distinct devices, one is allowed)."""
        self.lib = load_library()
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self.h = C.c_void_p()
        self.lib.sts_multi_last_error.restype = C.c_char_p
        self.lib.sts_multi_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        self.lib.sts_multi_destroy.argtypes = [C.c_void_p]
        self.lib.sts_multi_device_count.argtypes = [C.c_void_p]
        self.lib.sts_multi_speaker_num.argtypes = [C.c_void_p]
        self.lib.sts_multi_infer_ids_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
        self.lib.sts_multi_shard_of.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.lib.sts_multi_create_ex.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        self.lib.sts_multi_gather_mode.argtypes = [C.c_void_p]
        rc = self.lib.sts_multi_create_ex(blob.ctypes.data, blob.nbytes, dev.ctypes.data, dev.size, self.MODES[gather], C.byref(self.h))
        if rc != 0:
            raise StsError(f"sts_multi_create_ex: {rc}: {self.lib.sts_multi_last_error().decode()}")

    def gather_mode(self) -> str:
        return "rccl" if int(self.lib.sts_multi_gather_mode(self.h)) == 1 else "download"

    def rccl_ranks(self) -> int:
        """Size of the handle's communicator as RCCL reports it (ncclCommCount); 0 without an RCCL gather."""
        self.lib.sts_multi_rccl_ranks.argtypes = [C.c_void_p]
        return int(self.lib.sts_multi_rccl_ranks(self.h))

    def last_gather_ms(self) -> float:
        self.lib.sts_multi_last_gather_ms.argtypes = [C.c_void_p]
        self.lib.sts_multi_last_gather_ms.restype = C.c_double
        return float(self.lib.sts_multi_last_gather_ms(self.h))

    def set_noise(self, noise_scale: float = 0.0, noise_scale_w: float = 0.0, seed: int = 0):
        """``Synthesizer.set_noise`` for every device; utterance b of a batch samples with ``seed + b`` whatever its device."""
        self.lib.sts_multi_set_noise.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint64]
        if self.lib.sts_multi_set_noise(self.h, float(noise_scale), float(noise_scale_w), int(seed) & 0xFFFFFFFFFFFFFFFF) != 0:
            raise StsError(f"sts_multi_set_noise: {self.lib.sts_multi_last_error().decode()}")

    def set_output_rate(self, rate: int):
        """``Synthesizer.set_output_rate`` for every device; the gathers then count output samples."""
        rc = self.lib.sts_multi_set_output_rate(self.h, int(rate))
        if rc != 0:
            raise StsError(f"sts_multi_set_output_rate: {rc}: {self.lib.sts_multi_last_error().decode()}")

    def set_loudness(self, mode: int, target_lufs: float = -16.0, peak_dbfs: float = -1.0):
        """``Synthesizer.set_loudness`` for every device (LOUD_OFF or LOUD_NORMALIZE)."""
        rc = self.lib.sts_multi_set_loudness(self.h, int(mode), float(target_lufs), float(peak_dbfs))
        if rc != 0:
            raise StsError(f"sts_multi_set_loudness: {rc}: {self.lib.sts_multi_last_error().decode()}")

    def set_limiter(self, mode: int, gain_db: float = 0.0, ceiling_dbfs: float = -1.0, lookahead_ms: float = 5.0):
        """``Synthesizer.set_limiter`` for every device."""
        rc = self.lib.sts_multi_set_limiter(self.h, int(mode), float(gain_db), float(ceiling_dbfs), float(lookahead_ms))
        if rc != 0:
            raise StsError(f"sts_multi_set_limiter: {rc}: {self.lib.sts_multi_last_error().decode()}")

    def set_eq(self, bands=None):
        """``Synthesizer.set_eq`` for every device."""
        n, arr = _eq_bands(bands)
        rc = self.lib.sts_multi_set_eq(self.h, n, arr)
        if rc != 0:
            raise StsError(f"sts_multi_set_eq: {rc}: {self.lib.sts_multi_last_error().decode()}")

    _TABLE_ENTRY = "sts_multi_set_%s"

    def _mix_gin(self):
        return None

    def _table_failed(self, name, rc):
        raise StsError(f"{name}: {rc}: {self.lib.sts_multi_last_error().decode()}")

    def set_duration_plan(self, n: Optional[Sequence[int]], plans=None):
        """``Synthesizer.set_duration_plan`` for the next ``infer_batch``: ``plans[b]`` belongs to utterance b of that batch, whatever its
        device."""
        self._set_table("duration_plan", n, plans)

    def set_speaker_mix(self, mixes=None):
        """``Synthesizer.set_speaker_mix`` for the next ``infer_batch``: ``mixes[b]`` belongs to utterance b of that batch, whatever its
        device."""
        self._set_table("speaker_mix", None, mixes)

    def set_gain_plan(self, n: Optional[Sequence[int]], plans=None):
        """``Synthesizer.set_gain_plan`` for the next ``infer_batch``: ``plans[b]`` belongs to utterance b of that batch, whatever its
        device."""
        self._set_table("gain_plan", n, plans)

    def set_pitch_plan(self, n: Optional[Sequence[int]], plans=None):
        """``Synthesizer.set_pitch_plan`` for the next ``infer_batch``: ``plans[b]`` belongs to utterance b of that batch, whatever its
        device."""
        self._set_table("pitch_plan", n, plans)

    def set_conv_math(self, mode):
        m = {"bf16x3": 0, "f32": 1, "bf16x3_all": 2, "f16x2": 3}.get(mode, mode)
        self.lib.sts_multi_set_conv_math.argtypes = [C.c_void_p, C.c_int]
        if self.lib.sts_multi_set_conv_math(self.h, int(m)) != 0:
            raise StsError(f"sts_multi_set_conv_math: {self.lib.sts_multi_last_error().decode()}")

    @staticmethod
    def set_rccl_library(path: Optional[str], allow_repeated_devices: bool = False):
        """Test hook (sts_multi_set_rccl_library): which shared library provides the nccl* entry points; only before the first
        'rccl' handle of the process."""
        lib = load_library()
        lib.sts_multi_set_rccl_library.argtypes = [C.c_char_p, C.c_int]
        lib.sts_multi_last_error.restype = C.c_char_p
        rc = lib.sts_multi_set_rccl_library(path.encode() if path else None, 1 if allow_repeated_devices else 0)
        if rc != 0:
            raise StsError(f"sts_multi_set_rccl_library: {rc}: {lib.sts_multi_last_error().decode()}")

    def device_count(self) -> int:
        return int(self.lib.sts_multi_device_count(self.h))

    def shard_of(self, lengths: Sequence[int]) -> np.ndarray:
        n = np.ascontiguousarray(lengths, dtype=np.int32)
        out = np.zeros(n.size, np.int32)
        rc = self.lib.sts_multi_shard_of(self.h, n.size, n.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise StsError(f"sts_multi_shard_of: {rc}: {self.lib.sts_multi_last_error().decode()}")
        return out

    def infer_batch(self, ids, sid=None, length_scale=None) -> List[np.ndarray]:
        B = len(ids)
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in ids]
        ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in arrs])
        n = np.asarray([a.size for a in arrs], dtype=np.int32)
        sidv = np.zeros(B, np.int32) if sid is None else np.ascontiguousarray(sid, dtype=np.int32)
        lsv = np.ones(B, np.float32) if length_scale is None else np.ascontiguousarray(length_scale, dtype=np.float32)
        outp = (C.POINTER(C.c_int16) * B)()
        n_out = np.zeros(B, np.int32)
        rc = self.lib.sts_multi_infer_ids_batch(self.h, B, ptrs, n.ctypes.data, sidv.ctypes.data, lsv.ctypes.data,
                                                C.cast(outp, C.c_void_p), n_out.ctypes.data)
        if rc != 0:
            raise StsError(f"sts_multi_infer_ids_batch: {rc}: {self.lib.sts_multi_last_error().decode()}")
        res = []
        for b in range(B):
            res.append(np.ctypeslib.as_array(outp[b], shape=(int(n_out[b]),)).copy() if n_out[b] else np.zeros(0, np.int16))
            self.lib.sts_free(C.cast(outp[b], C.c_void_p))
        return res

    def close(self):
        if self.h:
            self.lib.sts_multi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
