"""Float64 checker of the sampling-noise feature (test helper, not a test module).

* ``philox_block`` / ``noise_words`` / ``normals``: the noise streams of include/summertts_hip.h sts_set_noise, drawn through
  ``numpy.random.Philox`` (Philox4x64-10; numpy increments its counter before each block, so block ``c`` of stream ``s`` comes
  from counter ``c - 1 + s * 2**64``).
* ``sdp_latent``: the flipped SDP latent the first reverse ConvFlow reads.
* ``prior``: z_p = m_expand + eps * logs_expand * ns (the reference's expression: logs, not exp(logs)).
* ``SdpSection`` / ``sdp_logw``: the stochastic duration predictor's inference path in float64 with an injected latent, from the
  encoder output ``x`` (the ``x_enc`` tap) and the weights read out of the model blob.
"""
from __future__ import annotations

import math

import numpy as np

from spline_ref import rq_inverse
from summertts_amd import synth_blob as sb

STREAM_SDP, STREAM_PRIOR = 0, 1
_U64 = (1 << 64) - 1


def philox_block(seed: int, stream: int, block: int) -> np.ndarray:
    """The four 64-bit words of Philox4x64-10 with key (seed, 0) and counter (block, stream, 0, 0)."""
    g = np.random.Philox(key=np.array([seed & _U64, 0], dtype=np.uint64),
                         counter=((stream << 64) + block - 1) % (1 << 256))
    return g.random_raw(4).astype(np.uint64)


def noise_words(seed: int, stream: int, n: int) -> np.ndarray:
    """Words j = 0 .. n-1 of a stream (word j = word j % 4 of block j // 4)."""
    nb = (n + 3) // 4
    g = np.random.Philox(key=np.array([seed & _U64, 0], dtype=np.uint64), counter=((stream << 64) - 1) % (1 << 256))
    return g.random_raw(4 * nb).astype(np.uint64)[:n]


def box_muller(w: np.ndarray) -> np.ndarray:
    """Cosine-branch Box-Muller in fp32, as the device computes it."""
    w = np.asarray(w, dtype=np.uint64)
    u1 = ((w >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = ((w >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
    return (np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(2.0 * math.pi) * u2)).astype(np.float32)


def normals(seed: int, stream: int, n: int) -> np.ndarray:
    return box_muller(noise_words(seed, stream, n))


def sdp_latent(seed: int, nsw: float, T: int):
    """(r0, r1): rand_gen(2, T) * nsw (column-major: j = t * 2 + ch) after nn_flip(z, 0): r0 = z[1], r1 = z[0]."""
    e = normals(seed, STREAM_SDP, 2 * T).reshape(T, 2).astype(np.float64) * np.float32(nsw)
    return e[:, 1].copy(), e[:, 0].copy()


def prior(m: np.ndarray, logs: np.ndarray, dur: np.ndarray, ns: float, seed: int) -> np.ndarray:
    """z_p [C, F] of one utterance: m_expand + eps * logs_expand * ns, eps[c, f] = element c * F + f of the prior stream."""
    idx = np.repeat(np.arange(m.shape[1]), np.asarray(dur, dtype=np.int64))
    me, le = m[:, idx].astype(np.float64), logs[:, idx].astype(np.float64)
    C, F = me.shape
    eps = normals(seed, STREAM_PRIOR, C * F).reshape(C, F).astype(np.float64)
    return me + eps * le * ns, eps


# ---------------------------------------------------------------------------------------------------------------------------
# the SDP section of a blob (synth_blob._dur order)

class _Reader:
    def __init__(self, blob: np.ndarray, pos: int):
        self.b, self.p = blob, pos

    def ints(self, n):
        v = [int(x) for x in self.b[self.p:self.p + n]]
        self.p += n
        return v

    def arr(self, n):
        a = self.b[self.p:self.p + n].astype(np.float64)
        assert a.size == n, "blob ends early"
        self.p += n
        return a

    def conv(self):
        out_ch, in_ch, k, pad, dil, has_b = self.ints(6)
        w = self.arr(out_ch * k * in_ch).reshape(out_ch, k, in_ch)
        b = self.arr(out_ch) if has_b else np.zeros(out_ch)
        return dict(w=w, b=b, k=k, pad=pad, dil=dil)

    def ln(self):
        (n,) = self.ints(1)
        return dict(g=self.arr(n), b=self.arr(n))

    def dds(self):
        n, k = self.ints(2)
        sep = [self.conv() for _ in range(n)]
        for i, c in enumerate(sep):             # dilation k**i, "same" padding (DDSConv.cpp)
            c["dil"] = k ** i
            c["pad"] = (k * c["dil"] - c["dil"]) // 2
        pw = [self.conv() for _ in range(n)]
        n1 = [self.ln() for _ in range(n)]
        n2 = [self.ln() for _ in range(n)]
        return dict(sep=sep, pw=pw, n1=n1, n2=n2)

    def convflow(self):
        return dict(pre=self.conv(), dds=self.dds(), proj=self.conv())


def _sdp_offset(cfg: sb.ModelCfg, seed: int) -> int:
    """Floats in front of the duration predictor: the writer replayed up to that section."""
    w = sb._W(seed, cfg.stats)
    w.ints(cfg.is_ms, cfg.lang, cfg.dur_type, cfg.dec_type)
    sb._text_encoder(w, cfg)
    sb._decoder(w, cfg)
    sb._flow(w, cfg)
    return w.n


class SdpSection:
    """Weights of the stochastic duration predictor (and the speaker table of a multi-speaker model)."""

    def __init__(self, blob: np.ndarray, cfg: sb.ModelCfg, seed: int):
        assert cfg.dur_type == sb.DUR_STOCHASTIC
        r = _Reader(np.asarray(blob, dtype=np.float32), _sdp_offset(cfg, seed))
        (self.n_flows,) = r.ints(1)
        self.ea_m, self.ea_logs = r.arr(2), r.arr(2)
        self.flows = [r.convflow() for _ in range(self.n_flows)]
        r.conv(); r.conv(); r.dds(); r.arr(4)                 # posterior side: loaded, never run at inference
        for _ in range(4):
            r.convflow()
        self.pre, self.proj, self.dds = r.conv(), r.conv(), r.dds()
        self.cond = r.conv() if cfg.is_ms else None
        self.emb_g = None
        if cfg.is_ms:
            spk, gin = r.ints(2)
            self.emb_g = r.arr(gin * spk).reshape(gin, spk)
        assert r.p == r.b.size, f"blob walker consumed {r.p} of {r.b.size} floats"


def _conv(c, x):
    """x [Cin, T] -> [Cout, T]; W [out][k][in], zero padding c['pad'] on both sides, dilation c['dil']."""
    w, k, pad, dil = c["w"], c["k"], c["pad"], c["dil"]
    T = x.shape[1]
    xp = np.pad(x, ((0, 0), (pad, pad)))
    Tout = xp.shape[1] - dil * (k - 1)
    y = np.zeros((w.shape[0], Tout))
    for t in range(k):
        y += w[:, t, :] @ xp[:, t * dil:t * dil + Tout]
    assert Tout == T
    return y + c["b"][:, None]


def _dwconv(c, x):
    w, k, pad, dil = c["w"][:, :, 0], c["k"], c["pad"], c["dil"]
    xp = np.pad(x, ((0, 0), (pad, pad)))
    T = x.shape[1]
    return sum(w[:, t:t + 1] * xp[:, t * dil:t * dil + T] for t in range(k)) + c["b"][:, None]


def _ln(p, x):
    mu = x.mean(0, keepdims=True)
    var = (x * x).mean(0, keepdims=True) - mu * mu
    return (x - mu) / np.sqrt(var + 1e-5) * p["g"][:, None] + p["b"][:, None]


def _gelu(x):
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _dds(d, x):
    for sep, pw, n1, n2 in zip(d["sep"], d["pw"], d["n1"], d["n2"]):
        y = _gelu(_ln(n1, _dwconv(sep, x)))
        y = _gelu(_ln(n2, _conv(pw, y)))
        x = x + y
    return x


def sdp_logw(sec: SdpSection, x: np.ndarray, r0: np.ndarray, r1: np.ndarray, sid: int = 0, spline=rq_inverse, trace=None) -> np.ndarray:
    """logw [T] of one utterance: x = the encoder output [H, T], (r0, r1) = the flipped latent (sdp_latent).  ``spline``: the inverse
    spline to use (spline_ref.rq_inverse, or rq_inverse_f32 to measure what fp32 costs in it); ``trace``: a list that receives
    (input, parameters, fs, selected bins) of every spline step."""
    x = np.asarray(x, dtype=np.float64)
    h = _conv(sec.pre, x)
    if sec.cond is not None:
        h = h + _conv(sec.cond, sec.emb_g[:, sid:sid + 1])
    g = _conv(sec.proj, _dds(sec.dds, h))
    z0, z1 = np.asarray(r0, np.float64), np.asarray(r1, np.float64)
    for i in range(sec.n_flows - 1, 0, -1):          # flow 0 stays skipped, as in the reference
        f = sec.flows[i]
        hh = _conv(f["pre"], z0[None]) + g
        p = _conv(f["proj"], _dds(f["dds"], hh))
        fs = math.sqrt(f["pre"]["w"].shape[0])
        if spline is rq_inverse:
            out, bins, _ = spline(z1, p, fs)
        else:                                         # a float32 spline: its inputs rounded once, everything else stays float64
            out, bins, _ = spline(z1.astype(np.float32), p.astype(np.float32), np.float32(fs))
        if trace is not None:
            trace.append((z1.copy(), p, fs, bins))
        z0, z1 = out.astype(np.float64), z0           # the spline step, then the channel flip
    return (z0 - sec.ea_m[0]) * np.exp(-sec.ea_logs[0])


def durations(logw: np.ndarray, length_scale: float = 1.0) -> np.ndarray:
    return np.ceil(np.exp(logw) * length_scale).astype(np.int64)
