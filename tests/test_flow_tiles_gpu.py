"""GPU suite (MI355X): the two tile widths of flow_layer_kernel (wn_flow.hip), 32 and 16 output frames per workgroup, through the engine.
`flow_fused` 2 forces 32-frame tiles, 3 forces 16-frame tiles (1 chooses).  The two widths run the same arithmetic in the same order, so the
latent z and the PCM must be equal bit for bit between them; both are also held against the oracle.  Frame counts F sit on and around both tile
widths (forced durations give an exact F), small models cover the kernel's shape limits: the narrowest and the widest WaveNet (one channel group
and eight), the flagship's 192 channels (six groups: two spill classes in the block mapping), a 1-tap gate conv (no halo, `pre` on one column
tile at either width) and 5 taps."""
import dataclasses

import numpy as np
import pytest

from conftest import TAP_MAXABS_TOL, assert_pcm_close
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

SHAPES = [(32, 5, 32), (192, 5, 96), (256, 3, 64), (64, 1, 32)]      # (H, gate taps, half = inter / 2)
FRAMES = [1, 15, 16, 17, 31, 32, 33, 48, 49]
BATCH = [33, 1, 17]                                                    # a ragged batch: tiles of 16 that end inside, on and past a member
POISON = 0x7FC00000                                                    # a quiet NaN in every float of the workspace


def _spread(F):
    """F frames over 5-7 phonemes: phoneme 1 has none, phoneme 2 is the long one (tests/test_packed_edges_gpu.py)."""
    T = 5 + F % 3
    d = [0] * T
    rest = F
    for j in (0, 3, 4, T - 1):
        if rest > 1:
            d[j] += 1
            rest -= 1
    d[2] += rest
    assert sum(d) == F
    return d


_models = {}       # shape -> (cfg, blob, ids per F, oracle result per F): computed once, read by every test


def _model(shape):
    if shape not in _models:
        H, k, half = shape
        cfg = dataclasses.replace(sb.tiny_cfg("hifigan_sdp"), flow_hidden=H, flow_k=k, inter=2 * half, flow_layers=3)
        blob = sb.make_blob(cfg, 23)
        port = pyref.PortModel(blob)
        ids, ref = {}, {}
        for F in sorted(set(FRAMES + BATCH)):
            ids[F] = sb.synthetic_ids(len(_spread(F)), cfg.vocab, salt=F)
            ref[F] = port.infer_ids(ids[F], 0, 1.0, forced_dur=_spread(F), taps=True)
            assert ref[F]["z"].shape[1] == F
        _models[shape] = (cfg, blob, ids, ref)
    return _models[shape]


def _engine(blob):
    syn = engine.Synthesizer(blob)
    syn.set_profiling(True)
    syn.set_record_taps(True)
    return syn


def _run(syn, mode, ids, fs):
    """One call under flow_fused = mode with forced frame counts fs -> (z, pcm, sample counts); no call may have been repeated in split-bf16."""
    syn.debug_set("flow_fused", mode)
    syn.set_forced_durations(sum((_spread(F) for F in fs), []))
    n = syn.run_batch([ids[F] for F in fs])
    p = syn.profile()
    assert p["conv_math_fallbacks"] == 0, (mode, fs, "the call was repeated in the split-bf16 form")
    return syn.tap("z").copy(), syn.pcm_host().copy(), n.copy()


def _check_oracle(what, z, pcm, o):
    ez = float(np.abs(z - o["z"]).max())
    assert ez <= TAP_MAXABS_TOL * max(1.0, float(np.abs(o["z"]).max())), (what, "z", ez)
    assert_pcm_close(pcm, o["pcm"], what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d_k%d_half%d" % s)
def test_one_utterance_at_both_tile_widths(shape):
    cfg, blob, ids, ref = _model(shape)
    syn = _engine(blob)
    for F in FRAMES:
        z32, pcm32, n32 = _run(syn, 2, ids, [F])
        z16, pcm16, n16 = _run(syn, 3, ids, [F])
        what = f"{shape}, F = {F}"
        assert n32.tolist() == n16.tolist() == [F * cfg.hop_total], what
        assert np.array_equal(z32.view(np.uint32), z16.view(np.uint32)), (what, "z differs between 32- and 16-frame tiles")
        assert np.array_equal(pcm32, pcm16), (what, "PCM differs between 32- and 16-frame tiles")
        _check_oracle(what + ", 16-frame tiles", z16, pcm16, ref[F])
        _check_oracle(what + ", 32-frame tiles", z32, pcm32, ref[F])
    # the automatic choice returns the same bits, and the per-conv launches do not (other arithmetic: the forced kernel engaged)
    z1, pcm1, _ = _run(syn, 1, ids, [49])
    z0, _, _ = _run(syn, 0, ids, [49])
    assert np.array_equal(z1.view(np.uint32), z16.view(np.uint32)) and np.array_equal(pcm1, pcm16), (shape, "automatic choice")
    assert not np.array_equal(z0, z16), (shape, "the one-launch-per-layer kernel did not engage under flow_fused = 3")
    syn.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d_k%d_half%d" % s)
def test_ragged_batch_on_16_frame_tiles(shape):
    cfg, blob, ids, ref = _model(shape)
    syn = _engine(blob)
    z16, pcm16, n16 = _run(syn, 3, ids, BATCH)
    z32, pcm32, n32 = _run(syn, 2, ids, BATCH)
    assert n16.tolist() == n32.tolist() == [F * cfg.hop_total for F in BATCH], shape
    assert np.array_equal(z16.view(np.uint32), z32.view(np.uint32)) and np.array_equal(pcm16, pcm32), (shape, "batch differs between the tile widths")
    off = 0
    for F in BATCH:
        _check_oracle(f"{shape}, batch member F = {F}", z16[:, off:off + F], pcm16[off * cfg.hop_total:(off + F) * cfg.hop_total], ref[F])
        off += F
    syn.close()


def test_16_frame_tiles_do_not_read_stale_memory():
    """STS_DBG_POISON fills the workspace with NaN patterns before every call: the 16-frame tiles (whose dead accumulator columns do see
    whatever lies past their window) return the bits of an engine that was never poisoned."""
    shape = SHAPES[1]
    cfg, blob, ids, ref = _model(shape)
    out = {}
    for poisoned in (False, True):
        syn = _engine(blob)
        if poisoned:
            syn.debug_set("poison", POISON)
        out[poisoned] = [_run(syn, 3, ids, fs) for fs in ([17], BATCH, [49])]
        assert (syn.profile()["poison_bytes"] > 0) == poisoned
        syn.close()
    for (za, pa, na), (zb, pb, nb) in zip(out[False], out[True]):
        assert na.tolist() == nb.tolist()
        assert np.array_equal(za.view(np.uint32), zb.view(np.uint32)) and np.array_equal(pa, pb), "poisoned workspace changed the result"
