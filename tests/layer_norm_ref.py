"""float64 restatement of the LayerNorm launch (misc_kernels.hip layer_norm_kernel with ln_input; oracle/vits_oracle.c layer_norm, act_gelu)
and the float32 "oracle route" of its fused forms.

    v[c][t] = dw_b[c] + sum_j dw_w[j][c] a[c][t + j dil - pad]     (depthwise conv; taps outside the UTTERANCE read as zero) or a[c][t]
            + b_0[c][t] + ... + b_{nb-1}[c][t]                        (split-K partials)
    v       = max(v, 0)                                              if pre_relu
    mean = sum_c v / C ;  var = sum_c v^2 / C - mean^2 ;  den = sqrt(var + 1e-5)
    y    = (v - mean) / den * gamma + beta
    y    = gelu(y) = (tanh(u) + 1) y / 2,  u = (y + 0.044715 y^3) sqrt(2 / pi),  tanh(u) = (e^u - e^-u) / (e^u + e^-u)      if post_gelu
    y    = res + y                                                   if res
Tensors are [C][L], utterances packed back to back along L."""
import numpy as np

GELU_K = float(np.float32(0.7978845608028654))
GELU_A = float(np.float32(0.044715))


def ln_input(a, lengths, b=None, pre_relu=False, dw_w=None, dw_b=None, dil=1, pad=0, dtype=np.float64):
    """The input chain in ``dtype``: float64 for the restatement; float32 gives what the oracle's own conv1d / add_inplace / relu produce
    (one multiply-add per tap in tap order, partials added one after another)."""
    a = np.asarray(a, dtype)
    C, L = a.shape
    if dw_w is None:
        v = a.copy()
    else:
        w = np.asarray(dw_w, dtype)
        v = np.zeros((C, L), dtype)
        if dw_b is not None:
            v += np.asarray(dw_b, dtype)[:, None]
        off = 0
        for n in lengths:
            n = int(n)
            seg = a[:, off:off + n]
            for j in range(w.shape[0]):
                sh = j * dil - pad                          # output t reads seg[t + sh]
                lo, hi = max(0, -sh), min(n, n - sh)
                if lo < hi:
                    v[:, off + lo:off + hi] += (w[j][:, None] * seg[:, lo + sh:hi + sh]).astype(dtype)
            off += n
    if b is not None:
        bs = np.asarray(b, dtype)
        s = bs[0].copy()
        for p in range(1, bs.shape[0]):
            s += bs[p]
        v = v + s
    if pre_relu:
        v = np.maximum(v, 0)
    return v.astype(dtype)


def gelu(y):
    y = np.asarray(y, np.float64)
    u = (y + y * y * y * GELU_A) * GELU_K
    e, n = np.exp(u), np.exp(-u)
    return ((e - n) / (e + n) + 1.0) * y * 0.5


def layer_norm(v, gamma, beta, post_gelu=False, res=None):
    v = np.asarray(v, np.float64)
    C = v.shape[0]
    mean = v.sum(axis=0) / C
    var = (v * v).sum(axis=0) / C - mean * mean
    den = np.sqrt(var + 1e-05)
    y = (v - mean) / den * np.asarray(gamma, np.float64)[:, None] + np.asarray(beta, np.float64)[:, None]
    if post_gelu:
        y = gelu(y)
    if res is not None:
        y = np.asarray(res, np.float64) + y
    return y


def reference(a, gamma, beta, lengths, b=None, res=None, pre_relu=False, post_gelu=False, dw_w=None, dw_b=None, dil=1, pad=0):
    """float64 all the way, from the float32 inputs."""
    return layer_norm(ln_input(a, lengths, b, pre_relu, dw_w, dw_b, dil, pad), gamma, beta, post_gelu, res)


def oracle_route(port_layer_norm, a, gamma, beta, lengths, b=None, res=None, pre_relu=False, post_gelu=False, dw_w=None, dw_b=None,
                 dil=1, pad=0):
    """The same launch as the plain-C oracle computes it: float32 input chain, then ``port_layer_norm`` (oracle.pyref: layer_norm and
    act_gelu of vits_oracle.c), then the float32 residual add."""
    v = ln_input(a, lengths, b, pre_relu, dw_w, dw_b, dil, pad, dtype=np.float32)
    y = port_layer_norm(v, gamma, beta, post_gelu)
    if res is not None:
        y = (np.asarray(res, np.float32) + y).astype(np.float32)
    return y


def random_case(seed, C, lengths, nb=0, res=False, conv=None, mean_over_std=None):
    """Columns with |mean| <= std (E[x^2] - mean^2 well conditioned); ``mean_over_std`` = 8 makes every column's mean 8 std instead.
    conv = (k, dil): a fused depthwise conv with "same" padding.  -> dict of the launch's arguments."""
    rng = np.random.default_rng(seed)
    L = int(np.sum(lengths))
    std = rng.uniform(0.5, 2.0, (1, L))
    mean = std * (rng.uniform(-1.0, 1.0, (1, L)) if mean_over_std is None else mean_over_std)
    x = rng.standard_normal((C, L)) * std + mean
    d = dict(lengths=list(lengths), gamma=rng.uniform(0.5, 1.5, C).astype(np.float32), beta=rng.uniform(-0.5, 0.5, C).astype(np.float32))
    if nb:
        parts = rng.standard_normal((nb, C, L)) * std                                   # a + b_0 + ... + b_{nb-1} = x
        d["a"], d["b"] = (x - parts.sum(axis=0)).astype(np.float32), parts.astype(np.float32)
    else:
        d["a"] = x.astype(np.float32)
    if res:
        d["res"] = rng.standard_normal((C, L)).astype(np.float32)
    if conv is not None:
        k, dil = conv
        d.update(dw_w=(rng.standard_normal((k, C)) / np.sqrt(k)).astype(np.float32), dw_b=(0.1 * rng.standard_normal(C)).astype(np.float32),
                 dil=dil, pad=dil * (k - 1) // 2)
    return d


# ---- the grid of the kernel-level tests ---------------------------------------------------------------------------------------------
C_GRID = (1, 24, 31, 32, 33, 192, 256, 257, 288, 300)      # 256 | 257: the last channel kept in registers | the first recomputed one
PACKED, SINGLE = [1, 31, 32, 33, 70], [33]
CONVS = ((1, 1), (3, 1), (3, 9), (5, 3), (7, 27))          # (k, dil); pad = dil (k - 1) / 2 exceeds the shortest utterances


def grid():
    """-> list of (id, kwargs of random_case, flags of the launch)"""
    out = []
    for C in C_GRID:
        for name, lens in (("packed", PACKED), ("single", SINGLE)):
            out.append((f"C{C}-{name}-plain", dict(C=C, lengths=lens), {}))
            out.append((f"C{C}-{name}-nb8-res-gelu", dict(C=C, lengths=lens, nb=8, res=True), dict(post_gelu=True)))
    for C in (33, 192, 300):
        for k, dil in CONVS:
            out.append((f"C{C}-conv{k}x{dil}", dict(C=C, lengths=PACKED, conv=(k, dil)), dict(post_gelu=True)))
            out.append((f"C{C}-conv{k}x{dil}-single-res", dict(C=C, lengths=SINGLE, conv=(k, dil), res=True), {}))
    for nb in (1, 2):
        out.append((f"C192-nb{nb}", dict(C=192, lengths=PACKED, nb=nb), {}))
        out.append((f"C300-nb{nb}-relu-res", dict(C=300, lengths=PACKED, nb=nb, res=True), dict(pre_relu=True)))
    out.append(("C192-relu", dict(C=192, lengths=PACKED), dict(pre_relu=True)))
    out.append(("C33-relu-gelu", dict(C=33, lengths=PACKED), dict(pre_relu=True, post_gelu=True)))
    for C in (192, 300):
        out.append((f"C{C}-mean8std", dict(C=C, lengths=PACKED, mean_over_std=8.0), {}))
    return out


def make(idx):
    name, kw, flags = grid()[idx]
    d = random_case(20261019 + idx, **kw)
    d.update(flags)
    return d
