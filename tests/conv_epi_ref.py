"""Float64 definition of every epilogue and operand form a conv kernel of the engine has (kernels.hpp ConvArgs), for sts_debug_conv1d_epi.

A batch is a list of segments (one utterance each); every segment is convolved on its own with packed_conv_ref64.  Per segment b

    v = conv64(in') + bias + ubias[:, b],   in' = lrelu(reflect_view(mean(x, xs1, xs2)))

and the epilogue forms follow the table of include/summertts_hip.h.  The module also holds the layout helpers of the entry's `gap` packing,
the float32 restatement of the project's tanh / sigmoid / PCM cast, the error bounds and the table of what each kernel family takes."""
import functools

import numpy as np

from packed_conv_ref import packed_conv_ref64

STORE, RESADD, SUB, GATE, RESSKIP, TANH_PCM = 0, 1, 3, 4, 5, 6          # kernels.hpp Epilogue
EINVAL, EDEVICE = "sts error -1:", "sts error -3:"                     # how engine.StsError starts
BAR = 2e-5                                                              # the project's conv bar against float64 (test_packed_conv_gpu.py)
SENTINEL = np.array([0xFFFFFFFF], np.uint32).view(np.float32)[0]        # columns outside the output segments (pcm: 0x7FFF)
PCM_SENTINEL = np.int16(0x7FFF)
# ... and in a tensor that was given initial values (the target of a read-modify-write epilogue) a finite, tiny pattern: an update that runs
# into such a column gives old + v, other bits; on the NaN sentinel it would give the same NaN back and go unseen
PLAIN_BITS, RMW_BITS = 0xFFFFFFFF, 0x2F5A5A5A
RMW_SENTINEL = np.array([RMW_BITS], np.uint32).view(np.float32)[0]


# ---- layout of the entry's tensors: segment b at off[b] = sum_{i < b} (len_i + gap); outputs x scale, + b (and one longer) with `extra`
def spans(lengths, gap=0, scale=1, extra=0):
    out, off = [], 0
    for b, n in enumerate(lengths):
        lo = off * scale + b * extra
        out.append((lo, lo + int(n) * scale + extra))
        off += int(n) + gap
    return out


def row_len(lengths, gap=0, scale=1, extra=0):
    return (int(np.sum(lengths)) + len(lengths) * gap) * scale + len(lengths) * extra


def pack(segs, gap=0, fill=np.nan, scale=1, extra=0):
    """A list of [C, n_b] arrays -> [C, row] with `fill` in every column outside the segments.  The segments' lengths are the OUTPUT lengths
    n_b = len_b * scale + extra; the base lengths follow from them."""
    base = [(s.shape[1] - extra) // scale for s in segs]
    out = np.full((segs[0].shape[0], row_len(base, gap, scale, extra)), fill, segs[0].dtype)
    for s, (lo, hi) in zip(segs, spans(base, gap, scale, extra)):
        out[:, lo:hi] = s
    return out


def gap_mask(lengths, gap=0, scale=1, extra=0):
    m = np.ones(row_len(lengths, gap, scale, extra), bool)
    for lo, hi in spans(lengths, gap, scale, extra):
        m[lo:hi] = False
    return m


# ---- the operand forms
def mean32(x, xs1=None, xs2=None, nsum=0):
    """((x + xs1) + xs2) / nsum, every step rounded to float32 in this order (sum_scale's order, which the folding kernels promise)."""
    if nsum < 2:
        return np.asarray(x)
    t = np.asarray(x, np.float32) + np.asarray(xs1, np.float32)
    if nsum > 2:
        t = t + np.asarray(xs2, np.float32)
    assert t.dtype == np.float32
    return t / np.float32(nsum)


def reflect_view(x):
    """[C, L] -> [C, L + 1]: position p reads x[p - 1], p = 0 reads x[1]; a 1-long segment reads 0 at p = 0."""
    first = x[:, 1:2] if x.shape[1] > 1 else np.zeros((x.shape[0], 1), x.dtype)
    return np.concatenate([first, x], axis=1)


# ---- the project's float32 formulas (devmath.hpp), restated in numpy float32, and their float64 meaning
def tanh32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        e, n = np.exp(x), np.exp(-x)
    e = np.where(np.isinf(e), np.float32(1e10), e)
    n = np.where(np.isinf(n), np.float32(1e10), n)
    m0, m1 = e - n, e + n
    m1 = np.where(m1 < np.float32(1e-8), np.float32(1e-8), m1)
    out = m0 / m1
    assert out.dtype == np.float32
    return out


def sigmoid32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        out = np.float32(1.0) / (np.float32(1.0) + np.exp(-x))
    assert out.dtype == np.float32
    return out


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def pcm_cast(wave):
    """devmath.hpp pcm_cast: one float32 multiply, truncation to int32, the low 16 bits."""
    v = np.asarray(wave, np.float32) * np.float32(32737.0)
    assert v.dtype == np.float32
    q = np.where(np.abs(v) < np.float32(2147483648.0), v, np.float32(-2147483648.0)).astype(np.int64)     # (astype truncates toward zero)
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)


@functools.lru_cache(maxsize=None)
def grid_activation_error():
    """(E_tanh, E_gate) on a dense grid: max |float32 restatement - float64| of tanh_ref on [-100, 100] (step 5e-4) and of
    tanh_ref(a) sigmoid_ref(b) on [-100, 100]^2 (1601 x 1601 points, denser around 0)."""
    a = np.linspace(-100.0, 100.0, 400001).astype(np.float32)
    e_t = float(np.abs(tanh32(a).astype(np.float64) - np.tanh(a.astype(np.float64))).max())
    g = np.concatenate([np.linspace(-100.0, 100.0, 801), np.linspace(-8.0, 8.0, 800)]).astype(np.float32)
    t32, s32 = tanh32(g), sigmoid32(g)
    p32 = t32[:, None] * s32[None, :]
    assert p32.dtype == np.float32
    p64 = np.tanh(g.astype(np.float64))[:, None] * sigmoid64(g)[None, :]
    return e_t, float(np.abs(p32.astype(np.float64) - p64).max())


def activation_error(vt=None, vs=None):
    """The grid's errors, raised by those at a test's own pre-activations: vt alone (TANH_PCM) or the (vt, vs) pairs of a gate."""
    e_t, e_g = grid_activation_error()
    if vt is not None:
        vt32 = np.asarray(vt, np.float32)
        e_t = max(e_t, float(np.abs(tanh32(vt32).astype(np.float64) - np.tanh(vt32.astype(np.float64))).max()))
        if vs is not None:
            vs32 = np.asarray(vs, np.float32)
            p = tanh32(vt32) * sigmoid32(vs32)
            e_g = max(e_g, float(np.abs(p.astype(np.float64) - np.tanh(vt32.astype(np.float64)) * sigmoid64(vs32)).max()))
    return e_t, e_g


# ---- the reference
def epi_ref64(xs, w, bias, dil=1, stride=0, in_slope=None, epi=STORE, epi_flag=0, H=0, in_reflect=0, nsum=0, xs1=None, xs2=None, ubias=None,
              res=None, y_init=None, aux_init=None):
    """xs (xs1, xs2): one [Cin, len_b] float32 array per segment; w [Cout, k, Cin]; ubias [Cout, B]; res / y_init / aux_init: one array per
    segment, of the tensor's shape.  Returns one dict per segment: v (the pre-activation), y, aux (None where the form has none), and mag_y /
    mag_aux = |v| + |bias| + |ubias| + |res or old|, the magnitudes the extra float32 additions of the epilogue round at."""
    w = np.asarray(w, np.float32)
    co = w.shape[0]
    ins = []
    for b, x in enumerate(xs):
        t = mean32(x, None if xs1 is None else xs1[b], None if xs2 is None else xs2[b], nsum)
        ins.append(reflect_view(t) if in_reflect else t)
    conv = packed_conv_ref64(np.concatenate(ins, axis=1), [t.shape[1] for t in ins], w, None, dil, stride, False, in_slope)
    out, off = [], 0
    b64 = np.zeros(co) if bias is None else np.asarray(bias, np.float64)
    for b, t in enumerate(ins):
        n = t.shape[1] * max(stride, 1)
        u64 = np.zeros(co) if ubias is None else np.asarray(ubias, np.float64)[:, b]
        v = conv[:, off:off + n] + b64[:, None] + u64[:, None]
        off += n
        mag = np.abs(v) + np.abs(b64)[:, None] + np.abs(u64)[:, None]
        d = {"v": v, "y": None, "aux": None, "mag_y": mag, "mag_aux": None}
        if epi == STORE:
            d["y"] = v
        elif epi == RESADD:
            r = np.asarray(res[b], np.float64)
            d["y"], d["mag_y"] = v + r, mag + np.abs(r)
        elif epi == SUB:
            old = np.asarray(y_init[b], np.float64)
            d["y"], d["mag_y"] = old - v, mag + np.abs(old)
        elif epi == GATE:
            assert co == 2 * H
            d["y"], d["mag_y"] = np.tanh(v[:H]) * sigmoid64(v[H:]), None          # source row order whatever the packing
        elif epi == RESSKIP:
            assert co in (H, 2 * H)
            old_aux = np.zeros((H, n)) if (epi_flag & 1) else np.asarray(aux_init[b], np.float64)
            if co == 2 * H:
                old = np.asarray(y_init[b], np.float64)
                d["y"], d["mag_y"] = old + v[:H], mag[:H] + np.abs(old)
                d["aux"], d["mag_aux"] = old_aux + v[H:], mag[H:] + np.abs(old_aux)
            else:                                                              # every row goes to aux, y is untouched
                d["y"], d["mag_y"] = None, None
                d["aux"], d["mag_aux"] = old_aux + v, mag + np.abs(old_aux)
        elif epi == TANH_PCM:
            assert co == 1
            d["aux"], d["mag_aux"], d["mag_y"] = np.tanh(v), None, None
        else:
            raise ValueError(epi)
        out.append(d)
    return out


def bound(epi, g, mag=None, e_act=0.0):
    """Per-element bound of a kernel's result against epi_ref64.  g: 64 for a loud segment, 1 for a quiet one.  The linear forms pay the conv
    bar plus at most three more float32 additions (bias, ubias, res / old value), each within 2^-24 of the magnitudes involved.  The gate's
    derivatives are <= 1 in v_t and <= 1/4 in v_s, so the conv bar enters 1.25 times; e_act is the float32 evaluation error of the
    activation formulas themselves (4 x activation_error() on the device: its expf may differ from numpy's by an ulp or two in each of up
    to three calls)."""
    if epi == GATE:
        return 1.25 * BAR * g + e_act
    if epi == TANH_PCM:
        return BAR * g + e_act
    return BAR * g + 3.0 * 2.0 ** -24 * mag


# ---- the operands of a test case, drawn once and shared by the CPU and the GPU file
LOUD = 64.0


def make_case(ci, co, k, lengths, seed, stride=0, H=0, in_reflect=0):
    """Per segment and loudness (0 quiet / 1 loud = the same values x 64): x, xs1, xs2 [ci, len] (the generator of test_packed_conv_gpu.py:
    a gain per channel in [0.05, 3]), res / y_init [rows, out_len] and aux_init [H, out_len] at the scale of the segment; w, b; a random
    ubias [co, B] and the ramp 100 b + row / 8, under which a wrong segment or row index is an error of order 100."""
    rng = np.random.default_rng(seed)
    scale, B = max(stride, 1), len(lengths)
    gain = rng.uniform(0.05, 3.0, (ci, 1))
    both = lambda q: (q, (q * np.float32(LOUD)).astype(np.float32))
    c = {"x": [], "xs1": [], "xs2": [], "res": [], "y_init": [], "aux_init": [], "lengths": list(lengths)}
    for n in lengths:
        for name in ("x", "xs1", "xs2"):
            c[name].append(both((rng.standard_normal((ci, n)) * gain).astype(np.float32)))
        on = n * scale + in_reflect
        c["res"].append(both(rng.standard_normal((co, on)).astype(np.float32)))
        c["y_init"].append(both(rng.standard_normal((co, on)).astype(np.float32)))
        c["aux_init"].append(both(rng.standard_normal((max(H, 1), on)).astype(np.float32)))
    c["w"] = (rng.standard_normal((co, k, ci)) / np.sqrt(k * ci / scale)).astype(np.float32)
    c["b"] = rng.standard_normal(co).astype(np.float32)
    c["ubias_random"] = rng.standard_normal((co, B)).astype(np.float32)
    c["ubias_ramp"] = (100.0 * np.arange(B)[None, :] + np.arange(co)[:, None] / 8.0).astype(np.float32)
    return c


def pick(case, name, order, rows=None):
    """The per-segment list of operand `name` in `order` = [(segment, loud)], cut to the first `rows` rows."""
    return [case[name][i][1 if loud else 0][:rows] for i, loud in order]


# ---- what each kernel family takes, from the eligibility functions as they read today (conv_mfma_eligible, conv_wino_eligible,
# conv_bf3_eligible, conv_bf3_takes_sum's tiles, conv_cout1_takes) and the launchers: True = a combination the engine may use, it must
# run; False = no kernel of the family takes it, the entry must answer STS_EINVAL.  Families by a pinned mode of sts_debug_conv1d.
FAMILIES = {"generic": 1, "mfma tile": 5, "split-K": 8, "Winograd": 12, "split-bf16": 20, "two-term fp16": 60}
TAKES = {
    #                  generic  mfma   split-K Winograd bf3    h2
    "RESADD":         (True,    True,  True,   True,    True,  True),
    "SUB":            (True,    True,  True,   True,    True,  True),
    "RESSKIP":        (True,    True,  True,   True,    True,  True),
    "GATE permuted":  (True,    True,  True,   False,   True,  True),
    "GATE plain":     (True,    False, False,  False,   False, False),
    "TANH_PCM":       (True,    False, False,  False,   False, False),
    "ubias":          (True,    True,  True,   True,    True,  True),
    "in_reflect":     (True,    True,  True,   False,   True,  True),
    "kslices":        (False,   False, True,   False,   False, False),
    "nsum":           (False,   False, False,  False,   False, False),      # a 'same' conv with Cout > 1: no family folds the mean
}
