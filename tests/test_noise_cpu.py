"""Sampling noise, host side: the Philox streams, the float64 SDP checker pinned to the oracle at noise 0, the new C ABI."""
import ctypes as C

import numpy as np
import pytest

import noise_ref as nr
from oracle import pyref
from summertts_amd import engine, synth_blob as sb


def test_philox_known_answers():
    # Random123 known answers of Philox4x64-10: zero counter and key; all-ones counter and key
    g = np.random.Philox(key=np.array([0, 0], dtype=np.uint64), counter=(1 << 256) - 1)
    assert [int(v) for v in g.random_raw(4)] == [0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b]
    # the stream helpers address block c of stream s as counter (c, s, 0, 0)
    assert [int(v) for v in nr.philox_block(0, 0, 0)] == [0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b]
    w = nr.noise_words(12345, 1, 4 * 7 + 2)
    for blk in (0, 3, 7):
        assert np.array_equal(w[4 * blk:4 * blk + 4][: len(w) - 4 * blk], nr.philox_block(12345, 1, blk)[: len(w) - 4 * blk])
    assert not np.array_equal(nr.noise_words(12345, 0, 8), nr.noise_words(12345, 1, 8))
    assert not np.array_equal(nr.noise_words(12345, 0, 8), nr.noise_words(12346, 0, 8))


def test_box_muller_is_standard_normal():
    e = nr.normals(7, 1, 200000)
    assert e.dtype == np.float32 and np.isfinite(e).all()
    assert abs(e.mean()) < 0.01 and abs(e.std() - 1.0) < 0.01


def test_sdp_latent_order_and_flip():
    T = 9
    e = nr.normals(3, nr.STREAM_SDP, 2 * T)
    r0, r1 = nr.sdp_latent(3, 0.5, T)
    # rand_gen(2, T) is column-major (j = t * 2 + ch); nn_flip(z, 0) swaps the two rows
    assert np.allclose(r0, e[1::2] * np.float32(0.5)) and np.allclose(r1, e[0::2] * np.float32(0.5))


@pytest.mark.parametrize("kind", ["hifigan_sdp", "ms_hifigan_sdp", "ms_sdp"])
def test_sdp_checker_reproduces_the_oracle_at_noise_zero(kind):
    cfg = sb.tiny_cfg(kind)
    blob = sb.make_blob(cfg, 1234)
    sec = nr.SdpSection(blob, cfg, 1234)
    for T, sid in ((13, 0), (21, 2 if cfg.is_ms else 0)):
        ids = sb.synthetic_ids(T, cfg.vocab)
        o = pyref.PortModel(blob).infer_ids(ids, sid, 1.0, taps=True)
        z = np.zeros(T)
        logw = nr.sdp_logw(sec, o["x_enc"], z, z, sid)
        assert np.abs(logw - o["logw"][0]).max() <= 1e-4
        assert np.array_equal(nr.durations(logw), o["durations"])


def test_prior_checker_matches_its_definition():
    rng = np.random.default_rng(0)
    m, logs = rng.standard_normal((4, 5)), rng.standard_normal((4, 5))
    dur = np.array([1, 0, 3, 2, 1])
    zp, eps = nr.prior(m, logs, dur, 0.0, 1)
    assert np.array_equal(zp, m[:, np.repeat(np.arange(5), dur)])
    zp, eps = nr.prior(m, logs, dur, 0.667, 1)
    F = int(dur.sum())
    assert np.allclose(eps.ravel(), nr.normals(1, nr.STREAM_PRIOR, 4 * F))      # j = c * F + f
    idx = np.repeat(np.arange(5), dur)
    assert np.allclose(zp, m[:, idx] + eps * logs[:, idx] * 0.667)


def test_noise_symbols_are_exported():
    lib = engine.load_library()
    for s in ("sts_set_noise", "sts_get_noise", "sts_pool_submit_ex", "sts_multi_set_noise"):
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.sts_abi_version() >= 8


def test_noise_setters_validate_without_a_gpu():
    lib = engine.load_library()
    lib.sts_set_noise.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint64]
    lib.sts_get_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sts_multi_set_noise.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint64]
    lib.sts_pool_submit_ex.restype = C.c_int64
    lib.sts_pool_submit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64]
    assert lib.sts_set_noise(None, 0.5, 0.5, 1) < 0
    assert lib.sts_get_noise(None, None, None, None) < 0
    assert lib.sts_multi_set_noise(None, 0.5, 0.5, 1) < 0
    ids = np.arange(3, dtype=np.int32)
    assert lib.sts_pool_submit_ex(None, ids.ctypes.data, 3, 0, 1.0, 0.5, 0.5, 1) < 0
