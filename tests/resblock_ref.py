"""Float64 restatement of one fused ResBlock layer of the decoder's narrow stages, its running error bound, and the input families and
length sets tests/test_resblock_layer_cpu.py / _gpu.py share.

    y = x + conv2(lrelu(conv1_dil(lrelu(x)) + b1)) + b2          ResBlock1.cpp:55-69, one dilation

on a packed batch: every utterance is convolved on its own, zero-padded at ITS edges.  The intermediate is zero outside [0, len) even though
b1 != 0 -- conv2 pads the biased, activated intermediate with zeros, it does not see conv1 evaluated past the edge.

A member of a launch is the tuple (w1 [C][k1][C], b1 [C] | None, dil1, w2 [C][k2][C], b2 [C] | None)."""
import numpy as np

HIFIGAN = ((3, 1, 3), (7, 3, 7), (11, 5, 11))            # (k1, dil1, k2): HiFi-GAN's three chains, dil1 = 1, 3, 5 in turn
ONE = ((7, 3, 7),)
FOUR = ((3, 1, 11), (11, 5, 3), (5, 2, 7), (7, 1, 5))     # kMaxGroup members of mixed shapes: the launchers re-sort them longest-first
MEMBER_SETS = {"hifigan": HIFIGAN, "one": ONE, "four": FOUR}
# which members of a set go without b1 / without b2 (by index): a set with several members carries bias-free ones
NO_B1 = {"hifigan": (1,), "one": (), "four": (1, 3)}
NO_B2 = {"hifigan": (2,), "one": (), "four": (2, 3)}


def _lrelu(a, slope):
    return np.where(a < 0, a * slope, a)


def _conv_same(a, w, dil):
    """a [C][n] float64, w [out][k][in] float64 -> [out][n], zero padding dil (k - 1) / 2 on both sides."""
    k = w.shape[1]
    h = dil * (k - 1) // 2
    n = a.shape[1]
    ap = np.zeros((a.shape[0], n + 2 * h))
    ap[:, h:h + n] = a
    y = np.zeros((w.shape[0], n))
    for j in range(k):
        y += w[:, j, :] @ ap[:, j * dil:j * dil + n]
    return y


def _layer(x, lengths, member, slope, absolute):
    w1, b1, dil1, w2, b2 = member
    x = np.asarray(x, dtype=np.float64)
    w1, w2 = np.asarray(w1, dtype=np.float64), np.asarray(w2, dtype=np.float64)
    assert w1.shape[1] % 2 == 1 and w2.shape[1] % 2 == 1 and int(np.sum(lengths)) == x.shape[1]
    b1 = np.zeros(x.shape[0]) if b1 is None else np.asarray(b1, dtype=np.float64)
    b2 = np.zeros(x.shape[0]) if b2 is None else np.asarray(b2, dtype=np.float64)
    s = float(np.float32(slope))                 # the slope the float32 kernels multiply by
    out = np.zeros(x.shape)
    off = 0
    for n in lengths:
        n = int(n)
        xs = x[:, off:off + n]
        if absolute:
            t = _conv_same(np.abs(_lrelu(xs, s)), np.abs(w1), dil1) + np.abs(b1)[:, None]          # B1 (>= |lrelu(intermediate)|)
            out[:, off:off + n] = _conv_same(t, np.abs(w2), 1) + np.abs(b2)[:, None] + np.abs(xs)
        else:
            t = _lrelu(_conv_same(_lrelu(xs, s), w1, dil1) + b1[:, None], s)
            out[:, off:off + n] = xs + _conv_same(t, w2, 1) + b2[:, None]
        off += n
    return out


def ref64(x, lengths, member, slope):
    """The layer in float64: x [C][sum(lengths)] -> [C][sum(lengths)]; position p of utterance b never sees utterance b +- 1."""
    return _layer(x, lengths, member, slope, False)


def bound(x, lengths, member, slope):
    """The same expression on absolute values, B1 = |W1| |lrelu x| + |b1|, B = |W2| B1 + |b2| + |x|: what a rounding error of any of the
    layer's sums is proportional to, per element.  Every tolerance of the layer tests is a multiple of it."""
    return _layer(x, lengths, member, slope, True)


# ---- input families ---------------------------------------------------------------------------------------------------------------------
def gaussian_members(seed, C, name):
    """w Gaussian / sqrt(k C), biases Gaussian of unit scale (a missing zero pad of the intermediate is then an error of order 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for j, (k1, d1, k2) in enumerate(MEMBER_SETS[name]):
        w1 = (rng.standard_normal((C, k1, C)) / np.sqrt(k1 * C)).astype(np.float32)
        w2 = (rng.standard_normal((C, k2, C)) / np.sqrt(k2 * C)).astype(np.float32)
        b1 = rng.standard_normal(C).astype(np.float32)
        b2 = rng.standard_normal(C).astype(np.float32)
        out.append((w1, None if j in NO_B1[name] else b1, d1, w2, None if j in NO_B2[name] else b2))
    return out


def gaussian_x(seed, C, n):
    """Gaussian with per-channel scales 0.05 ... 3."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((C, n)) * rng.uniform(0.05, 3.0, (C, 1))).astype(np.float32)


EXACT_SLOPE = 0.5


def exact_members(seed, C, shapes):
    """Every output row of w1 and w2 has at most 8 non-zero entries, from {+-2, +-4}; integer biases in [-3, 3].  With integer x in
    [-3, 3] and slope 0.5 every intermediate is a multiple of 0.5 below 2^12 (|conv1| <= 8 * 4 * 3 + 3 = 99, |conv2| <= 8 * 4 * 99 + 3,
    |y| <= 3174): every sum is exact in fp32, in two fp16 terms (99 / 0.5 < 2^11), in three bf16 terms and under the Winograd weight
    transform G = [1; 1/2 1/2 1/2; 1/2 -1/2 1/2; 1] (sums of even integers, halved)."""
    rng = np.random.default_rng(seed)
    out = []
    for (k1, d1, k2) in shapes:
        ws = []
        for k in (k1, k2):
            w = np.zeros((C, k * C), np.float32)
            for o in range(C):
                idx = rng.choice(k * C, size=8, replace=False)
                w[o, idx] = rng.choice(np.array([-4.0, -2.0, 2.0, 4.0], np.float32), size=8)
            ws.append(w.reshape(C, k, C))
        b1 = rng.integers(-3, 4, C).astype(np.float32)
        b2 = rng.integers(-3, 4, C).astype(np.float32)
        out.append((ws[0], b1, d1, ws[1], b2))
    return out


def exact_x(seed, C, n):
    return np.random.default_rng(seed).integers(-3, 4, (C, n)).astype(np.float32)


# ---- lengths on the kernels' real tiles ---------------------------------------------------------------------------------------------------
def tile_width(kind, C, variant=-1):
    """Intermediate columns W one workgroup produces; a tile covers NT = W - (k2 - 1) output columns.
    resblock_layer: 128.  resblock_wino: 60 per column group, 4 groups at C = 32, 2 at C = 64 / 128.  resblock_bf3: 32 NW WN = 128, except the
    shipped 32-channel shape (variant -1 / 0: 4 waves x 64 columns)."""
    if kind == 1:
        return 128
    if kind == 2:
        return 240 if C == 32 else 120
    return 256 if C == 32 and variant in (-1, 0) else 128


def tile_nts(W, shapes):
    return sorted({W - (k2 - 1) for (_, _, k2) in shapes})


def batch_lengths(W, shapes):
    """{1, 2, 3, h1 + h2 - 1, h1 + h2 + 1} of every member and {NT - 1, NT, NT + 1, 2 NT, 2 NT + 1} of every member's NT, ascending."""
    s = {1, 2, 3}
    for (k1, d1, k2) in shapes:
        h = d1 * (k1 - 1) // 2 + (k2 - 1) // 2
        s |= {h - 1, h + 1}
    for nt in tile_nts(W, shapes):
        s |= {nt - 1, nt, nt + 1, 2 * nt, 2 * nt + 1}
    return sorted(v for v in s if v >= 1)


def interleaved(lengths):
    """short, long, short, long ... of an ascending list"""
    a = list(lengths)
    out = []
    while a:
        out.append(a.pop(0))
        if a:
            out.append(a.pop())
    return out


def single_lengths(W, shapes):
    """the one-utterance calls: {1, NT, NT + 1} of every member's NT and 3 NT + 5 of the shortest tile"""
    nts = tile_nts(W, shapes)
    return sorted({1, 3 * nts[0] + 5} | {v for nt in nts for v in (nt, nt + 1)})


def oracle_gamma_limit(C, shapes):
    """What gamma_oracle = max(err_oracle / B) cannot exceed: the oracle adds the k C products of a conv and its bias one after another
    in float32, so each sum is off by at most (terms) u times the sum of its terms' magnitudes, u = 2^-24 (Higham, recursive summation,
    first order), the products and the two leaky relus add one rounding each, the residual one more."""
    return max(((k1 + k2) * C + 8) for (k1, _, k2) in shapes) * 2.0 ** -24
