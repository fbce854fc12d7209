"""Every section of a step's table in one step, on the MI355X (summertts_amd/csrc/stream_step.hpp): a gain plan, 48 kHz, the streamed
4-band EQ, streamed loudness and the limiter together, in a batched stream and in a joined one.  The conv mode is pinned, and every
comparison is of bits."""
import numpy as np
import pytest

from summertts_amd import engine, synth_blob as sb

pytestmark = pytest.mark.gpu

P, LS, HP = 1, 2, 4
BANDS4 = [(HP, 100.0, 0.0, 0.707), (P, 1000.0, 6.0, 2.0), (LS, 300.0, -6.0, 0.7), (P, 3000.0, -9.0, 4.0)]     # (tests/test_eq_stream_gpu.py's)
PHONEMES = (20, 2, 12)                    # 104, 11 and 68 frames: the second is shorter than two chunks of 7
CHUNKS = (1, 7)


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def model():
    cfg = sb.tiny_cfg("mbb_fix")
    blob = sb.make_blob(cfg, 7)
    ids = [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in PHONEMES]
    rng = np.random.default_rng(5)
    plans = []
    for n in PHONEMES:                    # every phoneme its own gain, one of them muted
        db = rng.uniform(-12.0, 6.0, n).astype(np.float32)
        db[n // 2] = -np.inf
        plans.append({"gain_db": db, "ramp_ms": 2.0})
    return blob, ids, plans


def _syn(blob):
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    syn.set_output_rate(48000)
    syn.set_eq(BANDS4)
    syn.set_eq_streaming(True)
    syn.set_loudness(engine.LOUD_MEASURE, -23.0, -2.0)
    syn.set_loudness_streaming(True)
    syn.set_limiter(engine.LIMITER_ON, 20.0, -3.0, 5.0)
    return syn


def _cat(chunks):
    return np.concatenate(chunks) if len(chunks) else np.zeros(0, np.int16)


def _bits(res):
    return np.frombuffer(res.tobytes(), np.uint8)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_a_batched_stream_with_every_stage_equals_its_single_streams(model, chunk):
    blob, ids, plans = model
    syn = _syn(blob)
    single = []
    for b, n in enumerate(PHONEMES):
        syn.set_gain_plan([n], [plans[b]])
        chunks, _ = syn.infer_ids_stream(ids[b], chunk)
        single.append((_cat(chunks), syn.loudness()))
        assert single[b][0].size > 0 and len(single[b][1]) == 1
    assert int(syn.durations(PHONEMES[2]).sum()) > 2 * max(CHUNKS)
    syn.set_gain_plan(list(PHONEMES), plans)
    got, _ = syn.infer_batch_stream(ids, chunk)
    res = syn.loudness()
    assert len(res) == 3
    for b in range(3):
        assert np.array_equal(_cat(got[b]), single[b][0]), (chunk, b)
        assert np.array_equal(_bits(res[b:b + 1]), _bits(single[b][1])), (chunk, b, res[b], single[b][1])
    # the short utterance leaves the step's tables while the others go on
    assert len(got[1]) < len(got[2]) < len(got[0]) and (chunk != 7 or len(got[1]) == 2)
    syn.close()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_a_joined_stream_with_every_stage_equals_the_whole_call(model, chunk):
    blob, ids, plans = model
    syn = _syn(blob)
    gap = max(CHUNKS) + 2 * syn.stream_halo_frames() + 3              # a step whose window of J meets no sentence
    join = {"gap_frames": [gap, 2], "lead_frames": 3, "trail_frames": 4, "fade_ms": 2.0}
    syn.set_gain_plan(list(PHONEMES), plans)
    whole = syn.infer_joined(ids, join=join)
    want = syn.loudness()
    assert len(want) == 1 and whole.size > 0
    syn.set_gain_plan(list(PHONEMES), plans)
    got = syn.infer_joined_stream(ids, chunk, join=join)
    assert np.array_equal(_cat([p for _, p in got]), whole), chunk
    assert np.array_equal(_bits(syn.loudness()), _bits(want)), (chunk, syn.loudness(), want)
    syn.close()
