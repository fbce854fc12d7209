"""GPU suite (MI355X): frame counts on and around the kernels' tile widths, through the engine.  Forced durations give every utterance an exact
frame count F from {1, 2, 31 .. 33, 63 .. 65, 127 .. 129, 255 .. 257}: 32 frames is flow_layer_kernel's tile, 32 / 64 / 128 columns the conv tiles,
128 the pre-split kernel's, 256 expand_frames', 64 the frame bucket of a one-utterance call.  One packed batch holds all of them (two orderings), and
every member is compared with the oracle run on that utterance alone -- latents, waveform, PCM, sample count."""
import dataclasses

import numpy as np
import pytest

from conftest import TAP_MAXABS_TOL, assert_pcm_close, assert_wave_close
from oracle import pyref
from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

FRAMES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
ONE_UTT = [1, 63, 64, 65, 128]          # around the 64-frame bucket of the batch-1 path
ORDERS = {"ascending": list(range(len(FRAMES))),
          "interleaved": [0, 13, 1, 12, 2, 11, 3, 10, 4, 9, 5, 8, 6, 7]}     # short, long, short, long, ...


def _spread(F):
    """F frames over 5-7 phonemes: phoneme 1 has none, phoneme 2 is the long one, the others one frame each while frames last."""
    T = 5 + F % 3
    d = [0] * T
    rest = F
    for j in (0, 3, 4, T - 1):
        if rest > 1:
            d[j] += 1
            rest -= 1
    d[2] += rest
    assert sum(d) == F and min(d) == 0
    return d


WIDE = dict(up_init=256, res_k=(5, 9), res_d=((1, 2, 4), (3, 1, 5)))      # the small pre-split model of tests/test_poison_gpu.py

# (label, tiny config, overrides, conv math or None, ((debug key, value), ...))
VARIANTS = [
    ("hifigan_sdp flow_fused=1", "hifigan_sdp", {}, None, (("flow_fused", 1),)),
    ("hifigan_sdp flow_fused=0", "hifigan_sdp", {}, None, (("flow_fused", 0),)),
    ("mbb_fix tail_fused=1", "mbb_fix", {}, None, (("tail_fused", 1),)),
    ("mbb_fix tail_fused=0", "mbb_fix", {}, None, (("tail_fused", 0),)),
    ("istft_fix tail_fused=1", "istft_fix", {}, None, (("tail_fused", 1),)),
    ("istft_fix tail_fused=0", "istft_fix", {}, None, (("tail_fused", 0),)),
    ("ms_sdp tail_fused=1", "ms_sdp", {}, None, (("tail_fused", 1),)),
    ("ms_sdp tail_fused=0", "ms_sdp", {}, None, (("tail_fused", 0),)),
    ("ms_hifigan_fix mixed speakers", "ms_hifigan_fix", {}, None, ()),
    ("wide hifigan_fix f16x2 pre-split", "hifigan_fix", WIDE, "f16x2", (("h2p", 2),)),
    ("wide hifigan_fix bf16x3", "hifigan_fix", WIDE, "bf16x3", ()),
    ("wide hifigan_fix f32", "hifigan_fix", WIDE, "f32", ()),
    ("hifigan_fix ups_rowph=1", "hifigan_fix", {}, None, (("ups_rowph", 1),)),
    ("hifigan_fix ups_rowph=0", "hifigan_fix", {}, None, (("ups_rowph", 0),)),
]

_models = {}       # (kind, overrides) -> (cfg, blob, ids per F, speaker per F, oracle result per F): computed once, read by every variant


def _model(kind, over):
    key = (kind, repr(sorted(over.items())))
    if key not in _models:
        cfg = dataclasses.replace(sb.tiny_cfg(kind), **over)
        blob = sb.make_blob(cfg, 77 + (256 if over else 0))
        port = pyref.PortModel(blob)
        ids, sid, ref = {}, {}, {}
        for i, F in enumerate(FRAMES):
            ids[F] = sb.synthetic_ids(len(_spread(F)), cfg.vocab, salt=F)
            sid[F] = i % cfg.spk_num if cfg.is_ms else 0
            ref[F] = port.infer_ids(ids[F], sid[F], 1.0, forced_dur=_spread(F), taps=True)
            assert ref[F]["z_p"].shape[1] == F
        _models[key] = (cfg, blob, ids, sid, ref)
    return _models[key]


def _check_member(label, F, o, hop, m, z_p, z, wave, pcm):
    """m: the engine's own prior mean of this utterance [C, phonemes].  The noise-free regulator only copies: z_p must be exactly m's columns
    repeated by the forced durations (the oracle's z_p is ITS m repeated, and the two text encoders differ by fp32 summation order, so
    equality with the oracle's z_p holds to the tap tolerance only -- asserted as well)."""
    what = f"{label}: F = {F}"
    assert pcm.size == F * hop and o["pcm"].size == F * hop, (what, pcm.size)
    assert z_p.shape == o["z_p"].shape and np.array_equal(z_p, np.repeat(m, _spread(F), axis=1)), (what, "z_p is not a copy of m's columns")
    ep = float(np.abs(z_p - o["z_p"]).max())
    assert ep <= TAP_MAXABS_TOL * max(1.0, float(np.abs(o["z_p"]).max())), (what, "z_p", ep)
    ez = float(np.abs(z - o["z"]).max())
    assert ez <= TAP_MAXABS_TOL * max(1.0, float(np.abs(o["z"]).max())), (what, "z", ez)
    assert_wave_close(wave, o["wave"], what)
    assert_pcm_close(pcm, o["pcm"], what)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0].replace(" ", "_"))
def test_frame_counts_on_tile_edges_match_the_oracle(variant):
    label, kind, over, math, knobs = variant
    cfg, blob, ids, sid, ref = _model(kind, over)
    hop = cfg.hop_total
    syn = engine.Synthesizer(blob)
    if math is not None:
        syn.set_conv_math(math)
    for key, value in knobs:
        syn.debug_set(key, value)
    syn.set_record_taps(True)
    for name, order in ORDERS.items():
        fs = [FRAMES[i] for i in order]
        syn.set_forced_durations(sum((_spread(F) for F in fs), []))
        n = syn.run_batch([ids[F] for F in fs], [sid[F] for F in fs])
        assert n.tolist() == [F * hop for F in fs], (label, name)
        m, z_p, z, wave, pcm = syn.tap("m"), syn.tap("z_p"), syn.tap("z"), syn.tap("wave")[0], syn.pcm_host()
        assert z_p.shape[1] == sum(fs) and wave.size == sum(fs) * hop
        off = toff = 0
        for F in fs:
            T = len(_spread(F))
            _check_member(f"{label}, batch {name}", F, ref[F], hop, m[:, toff:toff + T], z_p[:, off:off + F], z[:, off:off + F],
                          wave[off * hop:(off + F) * hop], pcm[off * hop:(off + F) * hop])
            off += F
            toff += T
    for F in ONE_UTT:
        syn.set_forced_durations(_spread(F))
        syn.run_batch([ids[F]], [sid[F]])
        _check_member(f"{label}, one utterance", F, ref[F], hop, syn.tap("m"), syn.tap("z_p"), syn.tap("z"), syn.tap("wave")[0], syn.pcm_host())
    # with the kernel variant pinned, an utterance's samples do not depend on what it is batched with
    syn.set_record_taps(False)
    syn.set_conv_mode(6)
    fs = [FRAMES[i] for i in ORDERS["interleaved"]]
    syn.set_forced_durations(sum((_spread(F) for F in fs), []))
    batch = syn.infer_batch([ids[F] for F in fs], [sid[F] for F in fs])
    for F, got in zip(fs, batch):
        syn.set_forced_durations(_spread(F))
        one = syn.infer_ids(ids[F], sid[F], 1.0)
        assert np.array_equal(got, one), (label, "pinned kernels: batch member differs from its own one-utterance call, F =", F)
    syn.close()
