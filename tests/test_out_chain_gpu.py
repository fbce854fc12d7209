"""The output chain on the MI355X (summertts_amd/csrc/out_chain.hpp): the wiring between the stages behind the decoder's
tail, not the stages' kernels -- their tile edges are their own test files' -- so every case runs the tiniest models.  For every
combination of gain plan, join, output rate, EQ, loudness mode and limiter: the call with and without taps returns the same bytes, the
PCM is the cast of the last running stage's float tap, and every stage's tap is its reference applied to the tap of the stage the
planner's table names as its source (bit for bit where the reference is exact, else by the comparison of the stage's own test file).
Then the streaming forms against the whole-utterance PCM, the three tail forms, and poisoned workspaces."""
import itertools

import numpy as np
import pytest

import eq_ref
import gain_ref as gr
import join_ref as jr
import limiter_ref as lm
import loudness_ref as lr
import resample_ref as rr
from summertts_amd import engine, synth_blob as sb
from test_eq_gpu import _check as eq_check                  # y within 2^-24 |ref| + 2^-26 max |ref| of the float64 definition
from test_join_gpu import RESAMPLE_WAVE_TOL                 # 1e-5: tests/test_resample_gpu.py _check_against_checker
from test_loudness_gpu import _close as loud_close          # lufs 0.01, peak exact, gain 1e-4

pytestmark = pytest.mark.gpu

LENS = (17, 9, 30)
EQ = [(eq_ref.LOWSHELF, 300.0, -6.0, 0.7)]
JOIN = {"lead_frames": 3, "gap_frames": [0, 6], "trail_frames": 2, "fade_ms": 2.0}
LIM = dict(gain_db=30.0, ceiling_dbfs=-6.0, lookahead_ms=2.0)
TARGET, CEILING = -23.0, -1.0
RAMP = 2.0


@pytest.fixture(scope="module", autouse=True)
def _torch_device_first():
    import torch
    torch.cuda.init()


def _model(kind):
    cfg = sb.tiny_cfg(kind)
    return sb.make_blob(cfg, 21), [sb.synthetic_ids(n, cfg.vocab, salt=n) for n in LENS]


def _engine(blob, poison=None):
    syn = engine.Synthesizer(blob)
    syn.set_conv_mode(6)
    if poison is not None:
        syn.debug_set("poison", poison)
    return syn


def _gain_db():
    db = np.zeros(LENS[1], np.float32)
    db[2] = 6.0; db[4] = -np.inf; db[7] = -9.0
    return db


GAINS = [None, {"gain_db": _gain_db(), "ramp_ms": RAMP}, None]


@pytest.fixture(scope="module")
def hifigan():
    blob, ids = _model("hifigan_sdp")
    syn = _engine(blob)
    plain = _engine(blob)
    want = plain.infer_batch(ids)                           # an engine that never had a stage set
    plain.close()
    yield syn, ids, want
    syn.close()


def _set(syn, rate, eq, loud, lim):
    syn.set_output_rate(rate)
    syn.set_eq(EQ if eq else None)
    syn.set_loudness(loud, TARGET, CEILING)
    syn.set_limiter(engine.LIMITER_ON if lim else engine.LIMITER_OFF, **LIM)


def _whole(syn, ids, gain, join, members=None):
    """one whole-utterance call -> the list of returned signals (a joined call: one)"""
    members = list(range(len(ids))) if members is None else members
    if gain:
        syn.set_gain_plan([LENS[b] for b in members], [GAINS[b] for b in members])
    sel = [ids[b] for b in members]
    return [syn.infer_joined(sel, join=JOIN)] if join else syn.infer_batch(sel)


def _split(flat, counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert flat.size == off[-1], (flat.size, int(off[-1]))
    return [flat[off[b]:off[b + 1]] for b in range(len(counts))]


_memo = {}


def _ref(name, fn, *arrays):
    """a stage's reference on these very inputs, computed once: the cases of the matrix share most of their stage inputs"""
    key = (name,) + tuple(np.ascontiguousarray(a).tobytes() for a in arrays)
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _check_case(syn, ids, plain, gain, join, rate, eq, loud, lim, tail_only=False):
    what = f"gain {gain} join {join} rate {rate} eq {eq} loud {loud} lim {lim}"
    _set(syn, rate, eq, loud, lim)
    hop = syn.info.samples_per_frame
    syn.set_record_taps(True)
    pcm = _whole(syn, ids, gain, join)
    taps = {}
    for name in ("wave", "wave_gain", "wave_join", "wave_out", "wave_eq", "wave_lim"):
        try:
            taps[name] = syn.tap(name)[0]
        except engine.StsError:
            pass
    dur = syn.durations(sum(LENS))
    loud_res, lim_res = syn.loudness(), syn.limiter()
    syn.set_record_taps(False)
    # (a) the same call without taps: the launch-ahead memo may serve it, and one utterance's PCM goes straight into pinned host memory
    again = _whole(syn, ids, gain, join)
    assert len(again) == len(pcm) and all(a.tobytes() == b.tobytes() for a, b in zip(again, pcm)), what
    assert syn.loudness().tobytes() == loud_res.tobytes() and syn.limiter().tobytes() == lim_res.tobytes(), what
    # exactly the stages of this case left a tap
    on = {"wave": True, "wave_gain": gain, "wave_join": join, "wave_out": rate != 16000, "wave_eq": eq, "wave_lim": lim}
    assert sorted(taps) == sorted(k for k, v in on.items() if v), (what, sorted(taps))
    assert len(loud_res) == (len(pcm) if loud else 0) and len(lim_res) == (len(pcm) if lim else 0), what
    off = np.concatenate([[0], np.cumsum(LENS)])
    durs = [dur[off[b]:off[b + 1]] for b in range(len(LENS))]
    frames = [max(1, int(d.sum())) for d in durs]
    # the chain, stage by stage: `cur` is the list of per-utterance float signals the table names as the next stage's source
    cur = _split(taps["wave"], [f * hop for f in frames])
    cast = None                                             # the writer's cast of its own float output
    if gain:
        want = [_ref("gain", lambda b=b: gr.apply(cur[b], durs[b], hop, None if GAINS[b] is None else GAINS[b]["gain_db"], RAMP), cur[b], durs[b])
                for b in range(len(LENS))]
        assert taps["wave_gain"].tobytes() == np.concatenate(want).tobytes(), what
        assert want[1].tobytes() != cur[1].tobytes() and want[0].tobytes() == cur[0].tobytes(), what
        cur = _split(taps["wave_gain"], [f * hop for f in frames]); cast = gr.pcm_cast
    if join:
        want = _ref("join", lambda: jr.join(cur, frames, hop, JOIN)[0], *cur)
        assert taps["wave_join"].tobytes() == want.tobytes(), what
        cur = [taps["wave_join"]]; cast = jr.pcm_cast
    counts = [p.size for p in pcm]
    assert counts == [rr.out_len(x.size, rate) if rate != 16000 else x.size for x in cur], what
    if rate != 16000:
        got = _split(taps["wave_out"], counts)
        for b, x in enumerate(cur):
            want = _ref("resample", lambda: rr.resample(x, rate), x)
            err = float(np.abs(got[b] - want).max())
            print(f"{what} utterance {b}: max |wave_out - checker| = {err:.3e} (cap {RESAMPLE_WAVE_TOL:.0e})")
            assert err <= RESAMPLE_WAVE_TOL, (what, b, err)
        cur = got; cast = rr.pcm_cast
    if eq:
        got = _split(taps["wave_eq"], counts)
        for b, x in enumerate(cur):
            eq_check(got[b], None, x, rate, EQ, f"{what} utterance {b}")
        cur = got; cast = eq_ref.pcm_cast
    gl = [1.0] * len(cur)
    if loud:
        for b, x in enumerate(cur):
            want = dict(_ref("loud", lambda: lr.loudness(x, rate, TARGET, CEILING), x))
            if lim:         # the limiter holds the peak: the gain is the loudness rule alone (loudness_ref.gain without a peak)
                want["gain"] = lr.gain(want["lufs"], 0.0, np.float32(TARGET), np.float32(CEILING))
            loud_close(loud_res[b], want, f"{what} utterance {b}")
        if loud == 2:
            gl = [r["gain"] for r in loud_res]
            cast = None
    if lim:
        H, c, G = engine.limiter_design(rate, **LIM)
        got = _split(taps["wave_lim"], counts)
        for b, x in enumerate(cur):
            want = _ref("limit", lambda: lm.limit(x, lm.static_gain(G, gl[b]), H, c)[0], x, np.float32(gl[b]))
            assert got[b].tobytes() == want.tobytes(), (what, b)
        assert (lim_res["limited"] > 0).any(), what         # it limits
        cur = got; cast = lm.pcm_cast
    # (b) the PCM is the cast of the last running stage's float output
    for b, x in enumerate(cur):
        if loud == 2 and not lim:
            want = lr.normalize(x, loud_res[b]["gain"])
        elif cast is None:  # the tail wrote it: no stage (or loudness measuring alone) -- an engine that never had a stage set
            want = plain[b]
        else:
            want = cast(x)
        assert np.array_equal(pcm[b], want), (what, b)
    if tail_only:
        return
    # (e) the writer's path into pinned host memory: one utterance alone is that member of the batch
    if not join:
        one = _whole(syn, ids, gain, False, members=[2])
        assert one[0].tobytes() == pcm[2].tobytes(), what


MATRIX = list(itertools.product((0, 1), (0, 1), (16000, 8000), (0, 1), (0, 1, 2), (0, 1)))
assert len(MATRIX) == 96


@pytest.mark.parametrize("gain,join,rate,eq,loud,lim", MATRIX)
def test_whole_utterance_chain(hifigan, gain, join, rate, eq, loud, lim):
    syn, ids, plain = hifigan
    _check_case(syn, ids, plain, gain, join, rate, eq, loud, lim)


def _cat(chunks):
    return np.concatenate(chunks) if chunks else np.zeros(0, np.int16)


def _stream(syn, ids, gain, batch):
    """-> the PCM of every streamed utterance, chunks concatenated: utterance 0 alone at 7 frames per chunk, or the three at 5"""
    members = [0, 1, 2] if batch else [0]
    if gain:
        syn.set_gain_plan([LENS[b] for b in members], [GAINS[b] for b in members])
    if batch:
        return [_cat(c) for c in syn.infer_batch_stream(ids, 5)[0]]
    return [_cat(syn.infer_ids_stream(ids[0], 7)[0])]


STREAMS = [(g, r, m, b, 0) for g, r, m, b in itertools.product((0, 1), (16000, 8000), (0, 1), (0, 1))] + \
          [(g, 16000, 0, b, 1) for g, b in itertools.product((0, 1), (0, 1))]


@pytest.mark.parametrize("gain,rate,lim,batch,direct", STREAMS)
def test_streams_concatenate_to_the_whole_utterance(hifigan, gain, rate, lim, batch, direct):
    syn, ids, plain = hifigan
    _set(syn, rate, 0, 0, lim)
    whole = _whole(syn, ids, gain, False)
    syn.debug_set("stream_direct", direct)
    try:
        got = _stream(syn, ids, gain, batch)
    finally:
        syn.debug_set("stream_direct", 0)
    for b, p in enumerate(got):
        assert p.tobytes() == whole[b].tobytes(), (gain, rate, lim, batch, direct, b)


@pytest.mark.parametrize("kind", ["mbb_fix", "istft_fix"])
@pytest.mark.parametrize("rate,lim", [(16000, 0), (16000, 1), (8000, 0)], ids=["plain", "limiter", "rate8000"])
def test_tail_forms(kind, rate, lim):
    """the fused iSTFT tail, the synthesis filter and the plain overlap-add each write (or skip) their float wave their own way"""
    blob, ids = _model(kind)
    plain = _engine(blob)
    want = plain.infer_batch(ids)
    plain.close()
    syn = _engine(blob)
    _check_case(syn, ids, want, 0, 0, rate, 0, 0, lim, tail_only=True)
    syn.close()


POISONED = [(0, 0, 16000, 0, 0, 0), (1, 0, 16000, 0, 0, 0), (0, 1, 16000, 0, 1, 0), (0, 0, 8000, 0, 0, 0), (1, 1, 8000, 1, 2, 1), (0, 0, 16000, 1, 2, 0),
            (1, 0, 8000, 0, 1, 1), (0, 1, 8000, 1, 0, 0)]
POISONED_STREAMS = [(0, 16000, 0, 1, 0), (1, 8000, 1, 1, 0), (1, 16000, 0, 0, 1), (0, 8000, 0, 0, 0)]


def test_a_poisoned_workspace_changes_nothing():
    blob, ids = _model("hifigan_sdp")

    def scenario(pattern):
        syn = _engine(blob, pattern)
        out = []
        for gain, join, rate, eq, loud, lim in POISONED:
            _set(syn, rate, eq, loud, lim)
            for taps in (True, False):
                syn.set_record_taps(taps)
                out.append(b"".join(p.tobytes() for p in _whole(syn, ids, gain, join)) + syn.loudness().tobytes() + syn.limiter().tobytes())
            if not join:
                out.append(_whole(syn, ids, gain, False, members=[2])[0].tobytes())
        for gain, rate, lim, batch, direct in POISONED_STREAMS:
            _set(syn, rate, 0, 0, lim)
            syn.debug_set("stream_direct", direct)
            out.append(b"".join(p.tobytes() for p in _stream(syn, ids, gain, batch)))
            syn.debug_set("stream_direct", 0)
        if pattern is not None:
            assert syn.profile()["poison_bytes"] > 0
        syn.close()
        return out

    assert scenario(0x7FC00000) == scenario(None)
