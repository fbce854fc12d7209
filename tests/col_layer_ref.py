"""float64 restatement of the fused column-block layer (col_layer.hip col_layer_kernel; oracle/vits_oracle.c dds_layer, convflow_inverse,
text_encoder) in its four forms, the case grid and the length sets of the kernel-level tests (test helper, not a test module; numpy only).

    h = x                                        or, with the folded rank-1 input,  h[c][t] = xs_w[c] xr[t] + xs_b[c] + x[c][t]
    u = gelu(LN(dw_b + dwconv_{k,dil,pad}(h)) g1 + b1)      (taps outside the UTTERANCE read as zero)      or u = h without the conv
    v = add + W u + bias ;  y = LN(v) g2 + b2 ;  gelu(y) if post_gelu ;  y = h + y if use_res
    tail:  p = TP y + tp_b (29 rows) ;  o0[t] = rq_inverse(r1[t] | p[:, t], fs) ;  o1 = r0

Forms: A = a DDSConv layer (conv, both LayerNorms, both GELUs, residual); B = A on the folded input; C = the attention output projection
(no conv, add, no GELU, no residual); D = A or B with the tail.  Tensors are [C][L], utterances packed back to back along L."""
import functools

import numpy as np

import layer_norm_ref as lr
import spline_ref as sr

WIDTHS = (32, 64, 192, 256)           # 256: the only width with the two-half B read (KQ = 64 > 48)
TAIL_WIDTHS = (32, 64, 192)
PREDICTOR = ((3, 1, 1), (3, 3, 3), (3, 9, 9))                    # (k, dil, pad) of the stochastic duration predictor's three layers
GEOMS = PREDICTOR + ((1, 1, 0), (2, 1, 0), (2, 1, 1), (3, 2, 0), (3, 16, 16), (3, 17, 17))     # last two: every tap leaves the 16-column block
BLOCK_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 49)
PAD, ILL = 37, 8.0                    # ld = L + 37; mean = 8 std of the ill-conditioned cases


def dilation_edges(dil):
    return (dil, dil + 1, 2 * dil, 2 * dil + 1)


ASCENDING = tuple(sorted(set(BLOCK_EDGES) | set(dilation_edges(9)) | set(dilation_edges(17))))


def interleaved(lens):
    """short, long, short, long, ...: workgroups past a short utterance's end exit beside live ones of its neighbours"""
    lens = sorted(lens)
    out = []
    while lens:
        out.append(lens.pop(0))
        if lens:
            out.append(lens.pop())
    return tuple(out)


INTERLEAVED = interleaved(ASCENDING)


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def params(C, k):
    """The weights of width C with a k-tap depthwise conv: every operand of every form, float32, left unchanged."""
    rng = np.random.default_rng([20261020, C, k])
    f = np.float32
    tp_w = rng.standard_normal((29, C))
    tp_w[:20] *= 0.5                                  # widths / heights: p / sqrt(C) ~ N(0, (0.5 rms y)^2)
    tp_w[20:] *= 2.0 / np.sqrt(C)                     # derivative logits ~ N(0, (2 rms y)^2)
    return _ro(dict(dw_w=(rng.standard_normal((k, C)) / np.sqrt(k)).astype(f), dw_b=(0.1 * rng.standard_normal(C)).astype(f),
                    g1=rng.uniform(0.5, 1.5, C).astype(f), b1=rng.uniform(-0.5, 0.5, C).astype(f),
                    w=(rng.standard_normal((C, C)) / np.sqrt(C)).astype(f), bias=(0.1 * rng.standard_normal(C)).astype(f),
                    g2=rng.uniform(0.5, 1.5, C).astype(f), b2=rng.uniform(-0.5, 0.5, C).astype(f),
                    xs_w=rng.standard_normal(C).astype(f), xs_b=(0.1 * rng.standard_normal(C)).astype(f),
                    tp_w=tp_w.astype(f), tp_b=(0.1 * rng.standard_normal(29)).astype(f)))


LATENT_EDGES = np.array([5.0, -5.0, 5.5, -5.5, 4.999, -4.999, 0.0, 7.0], np.float32)


@functools.lru_cache(maxsize=None)
def segment(C, n):
    """One utterance of n columns: x, add [C][n]; xr, r0, r1 [n] (latents ~ N(0, 3^2) with values on and beyond +-5, the identity tails,
    planted at the front)."""
    rng = np.random.default_rng([20261021, C, n])
    f = np.float32
    std = rng.uniform(0.5, 2.0, (1, n))
    d = dict(x=(rng.standard_normal((C, n)) * std + std * rng.uniform(-1, 1, (1, n))).astype(f), add=rng.standard_normal((C, n)).astype(f),
             xr=(3 * rng.standard_normal(n)).astype(f), r0=(3 * rng.standard_normal(n)).astype(f), r1=(3 * rng.standard_normal(n)).astype(f))
    m = min(n, LATENT_EDGES.size)
    d["r1"][:m] = np.roll(LATENT_EDGES, n)[:m]
    return _ro(d)


def packed(C, lens):
    segs = [segment(C, int(n)) for n in lens]
    return {key: np.concatenate([s[key] for s in segs], axis=-1) for key in ("x", "add", "xr", "r0", "r1")}


def fold32(x, xs_w, xs_b, xr):
    """The folded input as the kernel and the oracle form it: fl(fl(fl(w r) + b) + g) in numpy float32; xr / xs_b None: zeros."""
    f = np.float32
    x = np.asarray(x, f)
    r = np.zeros(x.shape[1], f) if xr is None else np.asarray(xr, f)
    b = np.zeros(x.shape[0], f) if xs_b is None else np.asarray(xs_b, f)
    h = ((np.asarray(xs_w, f)[:, None] * r[None, :]).astype(f) + b[:, None]).astype(f) + x
    assert h.dtype == f
    return h


def pre_ln(x, lengths, dw_w=None, dw_b=None, dil=1, pad=0, xs_w=None, xs_b=None, xr=None, w=None, bias=None, add=None, g1=None, b1=None):
    """float64 (h, v1, v2): the input, what LayerNorm 1 sees (None without the conv) and what LayerNorm 2 sees."""
    d = np.float64
    h = np.asarray(x, d)
    if xs_w is not None:
        r = np.zeros(h.shape[1], d) if xr is None else np.asarray(xr, d)
        h = np.asarray(xs_w, d)[:, None] * r[None, :] + (0.0 if xs_b is None else np.asarray(xs_b, d)[:, None]) + h
    v1, u = None, h
    if dw_w is not None:
        v1 = lr.ln_input(h, lengths, dw_w=dw_w, dw_b=dw_b, dil=dil, pad=pad)
        u = lr.layer_norm(v1, g1, b1, post_gelu=True)
    v2 = np.asarray(w, d) @ u
    if bias is not None:
        v2 = v2 + np.asarray(bias, d)[:, None]
    if add is not None:
        v2 = np.asarray(add, d) + v2
    return h, v1, v2


def ref64(x, lengths, w, g2, b2, bias=None, add=None, post_gelu=False, use_res=False, xs_w=None, xs_b=None, xr=None, dw_w=None, dw_b=None,
          dil=1, pad=0, g1=None, b1=None, tp_w=None, tp_b=None, tp_fs=1.0, r0=None, r1=None):
    """float64 all the way, from the float32 operands -> (y [C][L], o0 [L] or None, o1 [L] or None)."""
    h, _, v2 = pre_ln(x, lengths, dw_w, dw_b, dil, pad, xs_w, xs_b, xr, w, bias, add, g1, b1)
    y = lr.layer_norm(v2, g2, b2, post_gelu=post_gelu, res=h if use_res else None)
    if tp_w is None:
        return y, None, None
    L = y.shape[1]
    p = np.asarray(tp_w, np.float64) @ y + np.asarray(tp_b, np.float64)[:, None]
    z1 = np.zeros(L) if r1 is None else np.asarray(r1, np.float64)
    z0 = np.zeros(L) if r0 is None else np.asarray(r0, np.float64)
    return y, sr.rq_inverse(z1, p, tp_fs)[0], z0


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
def grid():
    """-> list of case dicts: id, form, C, geom (k, dil, pad) or None, lens, and the flags no_bias / no_dw_b / no_add / xr_null / xs_b_null /
    fold (form D on the folded input) / ill ('ln1' | 'ln2')."""
    out = []

    def case(form, C, geom, lens, **flags):
        tag = "-".join([form, f"C{C}"] + (["k%dd%dp%d" % geom] if geom else []) + ["asc" if lens == ASCENDING else "mix" if lens == INTERLEAVED else "n%d" % lens[0]]
                       + [k if v is True else f"{k}={v}" for k, v in flags.items() if v])
        out.append(dict(id=tag, form=form, C=C, geom=geom, lens=tuple(lens), **flags))
    for C in WIDTHS:
        for i, geom in enumerate(GEOMS):
            case("A", C, geom, ASCENDING if i % 2 == 0 else INTERLEAVED, no_bias=(i == 3), no_dw_b=(i == 5))
        for n in ASCENDING:                                   # one-utterance calls; the isolation test holds the batch against them
            case("A", C, PREDICTOR[2], (n,))
        case("B", C, PREDICTOR[0], ASCENDING)
        case("B", C, PREDICTOR[1], INTERLEAVED, xr_null=True)
        case("B", C, PREDICTOR[2], ASCENDING, xs_b_null=True)
        case("C", C, None, ASCENDING)
        case("C", C, None, INTERLEAVED, no_bias=True)
        case("C", C, None, ASCENDING, no_add=True)
        case("A", C, PREDICTOR[1], ASCENDING, ill="ln1")
        case("C", C, None, ASCENDING, ill="ln2")
    for C in TAIL_WIDTHS:
        case("D", C, PREDICTOR[2], ASCENDING)
        case("D", C, PREDICTOR[0], INTERLEAVED, fold=True)
        case("D", C, GEOMS[8], ASCENDING, fold=True, xr_null=True)
        case("D", C, GEOMS[4], INTERLEAVED)
    return out


def _col_stats(v):
    return v.mean(axis=0), v.std(axis=0)


@functools.lru_cache(maxsize=None)
def _build(idx):
    c = grid()[idx]
    C, form = c["C"], c["form"]
    k, dil, pad = c["geom"] if c["geom"] else (1, 1, 0)
    p, t = params(C, k), packed(C, c["lens"])
    lens = list(c["lens"])
    a = dict(x=t["x"], lengths=lens, w=p["w"], g2=p["g2"], b2=p["b2"], bias=None if c.get("no_bias") else p["bias"])
    if form == "C":
        a.update(add=None if c.get("no_add") else t["add"], post_gelu=False, use_res=False)
    else:
        a.update(dw_w=p["dw_w"], dw_b=None if c.get("no_dw_b") else p["dw_b"], dil=dil, pad=pad, g1=p["g1"], b1=p["b1"], post_gelu=True, use_res=True)
    if form == "B" or c.get("fold"):
        a.update(xs_w=p["xs_w"], xs_b=None if c.get("xs_b_null") else p["xs_b"], xr=None if c.get("xr_null") else t["xr"])
    if form == "D":
        # as in the flow: the conv's input row IS the kept latent half (x0); with the all-zero latent both are absent
        r0 = None if c.get("xr_null") else t["r0"]
        a.update(tp_w=p["tp_w"], tp_b=p["tp_b"], tp_fs=float(np.float32(np.sqrt(np.float32(C)))), r0=r0, r1=t["r1"])
        if c.get("fold"):
            a.update(xr=r0)
    keys = ("dw_w", "dw_b", "dil", "pad", "xs_w", "xs_b", "xr", "w", "bias", "add", "g1", "b1")
    if c.get("ill") == "ln1":          # through dw_b: every channel's conv output is lifted by 8 times the median column's spread
        a["x"] = (a["x"] / a["x"].std(axis=0, keepdims=True)).astype(np.float32)      # (columns of one spread: one shift fits them all)
        _, v1, _ = pre_ln(a["x"], lens, **{q: a.get(q) for q in keys})
        mean, std = _col_stats(v1)
        a["dw_b"] = (a["dw_b"] + np.float32(ILL * np.median(std) - np.median(mean))).astype(np.float32)
    if c.get("ill") == "ln2":          # through bias and add, half each: per column for add, so every column sits at 8 std
        _, _, v2 = pre_ln(a["x"], lens, **{q: a.get(q) for q in keys})
        mean, std = _col_stats(v2)
        shift = ILL * std - mean
        a["bias"] = (a["bias"] + np.float32(0.5 * np.median(shift))).astype(np.float32)
        a["add"] = (a["add"] + (shift - 0.5 * np.median(shift))[None, :]).astype(np.float32)
    return _ro(a)


def make(idx):
    """The ref64 keyword arguments of grid case idx (shared, read-only arrays)."""
    return dict(_build(idx))


def oracle(pyref, a):
    """The same case through the oracle's ports -> (y, o0, o1) float32 (o0 / o1 None without a tail)."""
    if a.get("dw_w") is None:
        return pyref.port_oproj_ln(a["x"], a["w"], a.get("bias"), a.get("add"), a["g2"], a["b2"]), None, None
    common = (a["dw_w"], a.get("dw_b"), a["dil"], a["pad"], a["g1"], a["b1"], a["w"], a.get("bias"), a["g2"], a["b2"])
    if a.get("xs_w") is None and a.get("tp_w") is None:
        return pyref.port_dds_layer(a["x"], a["lengths"], *common), None, None
    C = a["x"].shape[0]
    # (without the folded input the composite runs with a zero pre conv: h = fl(fl(0 r) + 0) + g = g exactly)
    xs_w = np.zeros(C, np.float32) if a.get("xs_w") is None else a["xs_w"]
    folded, tail = a.get("xs_w") is not None, a.get("tp_w") is not None
    assert not (folded and tail) or a.get("xr") is a.get("r0"), "the composite has ONE x0: the pre conv's input and the kept half"
    x0 = a.get("xr") if folded else a.get("r0")
    return pyref.port_convflow_step(a["x"], a["lengths"], xs_w, a.get("xs_b"), x0, a.get("r1"), *common, proj_w=a.get("tp_w"),
                                    proj_b=a.get("tp_b"), filter_sqrt=a.get("tp_fs", 1.0))
