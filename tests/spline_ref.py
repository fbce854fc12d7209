"""References of the duration predictor's rational-quadratic spline (test helper, not a test module; plain numpy, no GPU).

The spline of one position has 10 bins on [-5, 5] x [-5, 5] and is the identity outside (-5, 5).  Its 29 parameters ``h[:, t]`` are 10
unnormalised widths, 10 unnormalised heights (both divided by ``fs`` = sqrt(filter channels), then softmax, floor 1e-3) and the 9 inner
knot derivatives (softplus + 1e-3; the two boundary derivatives come from a padding constant chosen so that they equal 1).

* ``rq_inverse``      float64, the checker the GPU results are held against: value, selected bin, discriminant.
* ``rq_forward``      float64, the forward spline straight from the VITS formulas; ``rq_forward(rq_inverse(x)) == x`` is what makes the
                      checker trusted on its own account (tests/test_spline_cpu.py).
* ``rq_inverse_f32``  float32, step by step in the reference implementation's order of operations (exp without a max shift, sum, then the
                      divisions; the cumulative sums; the quadratic as written there).  It restates the reference, not the HIP kernel: it
                      measures what fp32 costs in this formula, and that cost sets the bars of tests/test_spline_gpu.py.
* ``knots_f32``       the eleven cumulative-height edges in float32, formed like ``rq_inverse_f32`` forms them; the tests place inputs on and
                      next to them.

Bins are numbered 0..9; -1 / 10 stand for the lower / upper tail.
"""
from __future__ import annotations

import numpy as np

NB, TAIL = 10, 5.0
_X = np.longdouble          # the float64 references work in x87 extended precision inside and round once at the end: near a knot with a
                            # small derivative the spline's slope reaches 10^3 either way, which would cost plain float64 three digits
PAD_DERIVATIVE = 0.5397424172369522          # log(e^(1 - 1e-3) - 1): pads the derivatives, softplus(.) + 1e-3 = 1 at both ends


def _softplus(x):
    return np.log1p(np.exp(x))


def tables(h, fs):
    """(cw, ch, der), each [11, n] in extended precision: cumulative widths, cumulative heights, knot derivatives."""
    h = np.asarray(h, _X)
    fs = _X(fs)
    n = h.shape[1]

    def cum(u):
        e = np.exp(u - u.max(0, keepdims=True))
        v = e / e.sum(0, keepdims=True) * (1 - _X(1e-3) * NB) + _X(1e-3)
        c = np.concatenate([np.zeros((1, n), _X), np.cumsum(v, 0)]) * 2 * TAIL - TAIL
        c[0], c[-1] = -TAIL, TAIL
        return c
    dend = np.full((1, n), _softplus(_X(PAD_DERIVATIVE)) + _X(1e-3))
    return cum(h[:NB] / fs), cum(h[NB:2 * NB] / fs), np.concatenate([dend, _softplus(h[2 * NB:]) + _X(1e-3), dend])


def _pick(tab, b):
    return np.take_along_axis(tab, b[None], 0)[0]


def _search(edges, x):
    """The reference's searchsorted: count of edges <= x (the last edge raised by 1e-6) minus one, clamped to a bin."""
    e = edges.copy()
    e[-1] += e.dtype.type(1e-6)
    return np.clip((x[None] >= e).sum(0) - 1, 0, NB - 1)


def _tail_bins(x, inside, b):
    return np.where(inside, b, np.where(x >= TAIL, NB, -1))


def rq_inverse(x, h, fs, bins=None, exact=False):
    """Inverse spline with linear tails: x [n], h [29, n] -> (value, bin, discriminant), float64.  ``bins`` (optional, [n]) forces the bin
    of every inside position instead of searching for it (continuity checks at the knots).  The discriminant of a tail position is 1.
    ``exact``: the value and the discriminant stay in extended precision (and x may come in it)."""
    x = np.asarray(x, _X)
    cw, ch, der = tables(h, fs)
    inside = (x < TAIL) & (x > -TAIL)
    b = _search(ch, x) if bins is None else np.asarray(bins, np.int64)
    w_, h_ = _pick(cw, b + 1) - _pick(cw, b), _pick(ch, b + 1) - _pick(ch, b)
    d0, d1, delta = _pick(der, b), _pick(der, b + 1), h_ / w_
    xm = x - _pick(ch, b)
    a = xm * (d0 + d1 - 2 * delta) + h_ * (delta - d0)
    bq = h_ * d0 - xm * (d0 + d1 - 2 * delta)
    c = -delta * xm
    disc = bq * bq - 4 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        root = 2 * c / (-bq - np.sqrt(disc))
    out, disc = np.where(inside, root * w_ + _pick(cw, b), x), np.where(inside, disc, _X(1))
    return (out, _tail_bins(x, inside, b), disc) if exact else (out.astype(np.float64), _tail_bins(x, inside, b), disc.astype(np.float64))


def rq_forward(y, h, fs, bins=None, exact=False):
    """Forward spline (VITS rational_quadratic_spline, inverse=False) with linear tails: y [n] -> (value, bin), float64."""
    y = np.asarray(y, _X)
    cw, ch, der = tables(h, fs)
    inside = (y < TAIL) & (y > -TAIL)
    b = _search(cw, y) if bins is None else np.asarray(bins, np.int64)
    w_, h_ = _pick(cw, b + 1) - _pick(cw, b), _pick(ch, b + 1) - _pick(ch, b)
    d0, d1, delta = _pick(der, b), _pick(der, b + 1), h_ / w_
    th = (y - _pick(cw, b)) / w_
    t1 = th * (1 - th)
    num = h_ * (delta * th * th + d0 * t1)
    den = delta + (d0 + d1 - 2 * delta) * t1
    out = np.where(inside, _pick(ch, b) + num / den, y)
    return (out if exact else out.astype(np.float64)), _tail_bins(y, inside, b)


# ---------------------------------------------------------------------------------------------------------------------------
# float32, in the reference implementation's order of operations

_F = np.float32


def _cum_f32(u):
    """Eleven float32 edges [11, n] from unnormalised float32 logits u [10, n]: exp, sequential sum, division, * 0.99 + 1e-3, running
    sum, * 10 - 5, then the two end edges set to -5 / 5."""
    e = np.exp(u).astype(_F)
    s = np.zeros(u.shape[1], _F)
    for i in range(NB):
        s = s + e[i]
    v = (e / s) * _F(1 - 1e-3 * NB) + _F(1e-3)
    c = np.zeros((NB + 1, u.shape[1]), _F)
    acc = np.zeros(u.shape[1], _F)
    for i in range(NB):
        acc = v[i] if i == 0 else acc + v[i]
        c[i + 1] = acc
    c = c * _F(2 * TAIL) + _F(-TAIL)
    c[0], c[-1] = _F(-TAIL), _F(TAIL)
    return c


def knots_f32(h, fs):
    """The cumulative-height edges [11, n] as float32."""
    h = np.asarray(h, _F)
    return _cum_f32(h[NB:2 * NB] / _F(fs))


def rq_inverse_f32(x, h, fs, guarded=False):
    """The inverse spline in float32 -> (value float32, bin, discriminant float32).  ``guarded``: with the two guards of the HIP kernel
    (devmath.hpp) that the reference does not have -- the root of max(disc, 0) where rounding drives the discriminant below 0, and
    softplus(h) = h where e^h overflows (a derivative logit above ~88.7); the reference is NaN in both places."""
    x, h = np.asarray(x, _F), np.asarray(h, _F)
    assert x.dtype == _F and h.dtype == _F
    n = x.size
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        cw, ch = _cum_f32(h[:NB] / _F(fs)), knots_f32(h, fs)
        pad = np.full((1, n), PAD_DERIVATIVE, _F)
        ud = np.concatenate([pad, h[2 * NB:], pad])
        der = np.log(np.exp(ud) + _F(1))
        if guarded:
            der = np.where(np.isinf(np.exp(ud)), ud, der)
        der = der + _F(1e-3)
        wsub, hsub = cw[1:] - cw[:-1], ch[1:] - ch[:-1]
        inside = (x < _F(TAIL)) & (x > _F(-TAIL))
        b = _search(ch, x)
        in_cw, in_w, in_ch, in_h = _pick(cw, b), _pick(wsub, b), _pick(ch, b), _pick(hsub, b)
        delta, d0, d1 = _pick(hsub / wsub, b), _pick(der, b), _pick(der, b + 1)
        xm = x - in_ch
        a = xm * (d0 + d1 - delta * _F(2)) + in_h * (delta - d0)
        bq = in_h * d0 - xm * (d0 + d1 - _F(2) * delta)
        c = -(delta * xm)
        disc = bq * bq - a * c * _F(4)
        root = (c * _F(2)) / (-bq - np.sqrt(np.maximum(disc, _F(0)) if guarded else disc))
        out = root * in_w + in_cw
    for v in (cw, der, a, bq, c, disc, out):
        assert v.dtype == _F
    return np.where(inside, out, x), _tail_bins(x, inside, b), np.where(inside, disc, _F(1))


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs of the kernel-level tests (tests/test_spline_cpu.py audits them, tests/test_spline_gpu.py runs them)

KERNEL_CASES = [(sigma, filt) for sigma in (0.5, 2.0) for filt in (24, 192)]
KERNEL_SEED = 20261018
N_COLS, N_KNOT_COLS, N_MONO = 4096, 256, 64


def kernel_inputs(sigma, filt):
    """One case: 4096 parameter columns, rows 0-19 ~ N(0, sigma^2) * sqrt(filt), rows 20-28 ~ N(0, 2^2), from
    default_rng([KERNEL_SEED, round(10 sigma), filt]).  Every evaluated position is a (column, x) pair:

      sweep   column i at x = -6 + 12 (i + 0.5) / 4096, i = 0..4095
      bound   columns 0..5 at -5, 5 and their float32 neighbours on both sides
      knots   columns 0..255, each at its eleven float32 knots and the float32 numbers just below and above each (33 per column)
      zero    columns 0..255 at 0
      past    columns 0..255 at the last knot + 1e-6 (float32)
      mono    columns 0..63, each at 64 sorted draws of U(-6, 6)

    -> dict: h float32 [29, n] (the columns gathered per position), x float32 [n], fs float32, col [n], and one slice per group."""
    rng = np.random.default_rng([KERNEL_SEED, int(round(10 * sigma)), filt])
    hc = np.empty((29, N_COLS), _F)
    hc[:2 * NB] = rng.standard_normal((2 * NB, N_COLS)) * sigma * np.sqrt(filt)
    hc[2 * NB:] = rng.standard_normal((29 - 2 * NB, N_COLS)) * 2.0
    fs = _F(np.sqrt(_F(filt)))
    k = knots_f32(hc[:, :N_KNOT_COLS], fs)                                   # [11, 256]
    five = _F(TAIL)
    groups = {
        "sweep": (np.arange(N_COLS), (-6.0 + 12.0 * (np.arange(N_COLS) + 0.5) / N_COLS).astype(_F)),
        "bound": (np.arange(6), np.array([-five, np.nextafter(-five, _F(-9)), np.nextafter(-five, _F(9)),
                                          five, np.nextafter(five, _F(-9)), np.nextafter(five, _F(9))], _F)),
        "knots": (np.repeat(np.arange(N_KNOT_COLS), 33),
                  np.stack([np.nextafter(k, _F(-9)), k, np.nextafter(k, _F(9))], 0).transpose(2, 1, 0).reshape(-1).astype(_F)),
        "zero": (np.arange(N_KNOT_COLS), np.zeros(N_KNOT_COLS, _F)),
        "past": (np.arange(N_KNOT_COLS), k[-1] + _F(1e-6)),
        "mono": (np.repeat(np.arange(N_MONO), N_MONO), np.sort(rng.uniform(-6.0, 6.0, (N_MONO, N_MONO)), 1).reshape(-1).astype(_F)),
    }
    out, cols, xs, at = {"fs": fs}, [], [], 0
    for name, (c, x) in groups.items():
        assert c.size == x.size and x.dtype == _F
        out[name] = slice(at, at + c.size)
        cols.append(c); xs.append(x); at += c.size
    out["col"], out["x"] = np.concatenate(cols), np.concatenate(xs)
    out["h"] = np.ascontiguousarray(hc[:, out["col"]])
    return out


def fp32_cost():
    """(E_max, E_rms, n_negative, per-case E_rms): max and root-mean-square of |rq_inverse_f32 - rq_inverse| over every position of every
    kernel case where the restatement is finite, the number of positions where it is not (its discriminant came out negative), and the
    same root-mean-square of each case alone, {(sigma, filter): rms}."""
    if not _COST:
        err, bad, each = [], 0, {}
        for sigma, filt in KERNEL_CASES:
            c = kernel_inputs(sigma, filt)
            want = rq_inverse(c["x"], c["h"], c["fs"])[0]
            got = rq_inverse_f32(c["x"], c["h"], c["fs"])[0]
            ok = np.isfinite(got)
            bad += int((~ok).sum())
            err.append((got[ok] - want[ok]))
            each[sigma, filt] = float(np.sqrt((err[-1] * err[-1]).mean()))
        err = np.concatenate(err)
        _COST.extend([float(np.abs(err).max()), float(np.sqrt((err * err).mean())), bad, each])
    return tuple(_COST)


_COST = []

# ---------------------------------------------------------------------------------------------------------------------------
# the engine-level cases: tiny models under a wide duration latent

ENGINE_NSW, ENGINE_T, ENGINE_LENS, ENGINE_BLOB_SEED = 3.0, 256, (37, 16, 1, 49, 130), 1234
ENGINE_KINDS = ("hifigan_sdp", "ms_hifigan_sdp")
ENGINE_MODELS = ("base", "f48", "f64", "w32")


def engine_cfg(kind, model):
    """The tiny configuration of ``kind`` (sdp_filter 32, the 2-wave fused tail) or a variant: ``f48`` a filter width the column kernel is
    not instantiated for (every DDSConv layer unfused, spline_step_kernel), ``f64`` the 4-wave fused tail, ``w32`` text encoder and
    predictor both 32 wide (the model of test_parity_gpu.py test_fused_column_layers_at_every_instantiated_width)."""
    import dataclasses
    from summertts_amd import synth_blob as sb
    if model == "full":          # the upstream-sized model: sdp_filter 192, the 12-wave fused tail of every production call (GPU test only)
        return sb.full_cfg(kind)
    cfg = sb.tiny_cfg(kind)
    return {"base": cfg, "f48": dataclasses.replace(cfg, sdp_filter=48), "f64": dataclasses.replace(cfg, sdp_filter=64),
            "w32": dataclasses.replace(cfg, hidden=32, sdp_filter=32, n_layers=1, ffn=64)}[model]


def engine_ids(cfg):
    """(ids of the T = 256 utterance, its sid, ids of the ragged batch, their sids)."""
    from summertts_amd import synth_blob as sb
    spk = max(cfg.spk_num, 1)
    return (sb.synthetic_ids(ENGINE_T, cfg.vocab, salt=3), 1 % spk,
            [sb.synthetic_ids(t, cfg.vocab, salt=10 + i) for i, t in enumerate(ENGINE_LENS)], [i % spk for i in range(len(ENGINE_LENS))])


# noise seed of each model: the first seed >= 1 at which, by the CPU audit of tests/test_spline_cpu.py (the oracle's encoder output, the
# float64 checker), every one of the sdp_flows - 1 spline steps of the T = 256 utterance selects every bin and both tails at least twice
ENGINE_SEEDS = {("hifigan_sdp", "base"): 23, ("hifigan_sdp", "f48"): 4, ("hifigan_sdp", "f64"): 1, ("hifigan_sdp", "w32"): 1,
                ("ms_hifigan_sdp", "base"): 8, ("ms_hifigan_sdp", "f48"): 4, ("ms_hifigan_sdp", "f64"): 76, ("ms_hifigan_sdp", "w32"): 76}


def bins_hit(trace):
    """The smallest count over the 10 bins and 2 tails, over the spline steps of a noise_ref.sdp_logw trace."""
    return min(int(np.bincount(b + 1, minlength=NB + 2).min()) for (_, _, _, b) in trace)


def logw_fp32_cost(sec, x, r0, r1, sid=0):
    """(max, n_nan) of |sdp_logw with rq_inverse_f32 - sdp_logw with rq_inverse| over one utterance's phonemes; n_nan counts those the
    float32 restatement has no value for (a negative discriminant at one phoneme reaches its neighbours through the later flows'
    dilated convs), which the max leaves out."""
    import noise_ref as nr
    d = np.abs(nr.sdp_logw(sec, x, r0, r1, sid, spline=rq_inverse_f32) - nr.sdp_logw(sec, x, r0, r1, sid))
    return (float(np.nanmax(d)) if np.isfinite(d).any() else 0.0), int(np.isnan(d).sum())


# The figures of record (tests/test_spline_cpu.py holds them against what it measures; tests/test_spline_gpu.py and DESIGN.md quote them):
# max and rms of |rq_inverse_f32 - rq_inverse| over the kernel cases, the positions there without a float32 root, and the largest
# float32 cost of logw over the eight models' utterances (T = 256 and the ragged batch).  The engine bar follows from the last.
# E_RMS_CASE: E_rms of each kernel case alone (the pooled figure is nearly all one position of the third case).  LOGW_NAN: the phonemes
# per model that the cost of logw leaves out because the float32 restatement has no value there.
E_MAX, E_RMS, N_NEGATIVE, LOGW_COST = 5.27e-3, 2.14e-5, 2, 1.42e-4
E_RMS_CASE = {(0.5, 24): 5.86e-6, (0.5, 192): 5.68e-6, (2.0, 24): 4.15e-5, (2.0, 192): 6.55e-6}
LOGW_NAN = {("ms_hifigan_sdp", "f48"): 22}          # (every other model: 0)
LOGW_BAR = min(4 * LOGW_COST, 1e-3)
