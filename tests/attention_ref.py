"""float64 restatement of the text encoder's windowed relative-position attention (misc_kernels.hip attention_*_kernel, oracle/vits_oracle.c
attention_core), between the q / k / v convs and the output conv, plus the input constructions of the kernel-level tests.

Per head h (kc channels) and utterance of T positions, px = 2 win + 1:
    qs_i    = float32(q_i / sqrt(kc))                    (rounded to float32 first, as the oracle and every kernel do)
    S[i][j] = qs_i . k_j  +  [|j - i| <= win] qs_i . relK[:, j - i + win]
    P[i][j] = exp(S[i][j]) / sum_j exp(S[i][j])          (no max shift)
    O_i     = sum_j P[i][j] v_j  +  sum_{|j - i| <= win} P[i][j] relV[:, j - i + win]
Tensors are [nheads * kc][L], utterances packed back to back along L; relK / relV are [kc][px]."""
import numpy as np


def scaled_q(q, kc):
    return (np.asarray(q, np.float32) / np.sqrt(np.float32(kc))).astype(np.float32).astype(np.float64)


def banded_one(q, k, v, relk, relv, nheads, win):
    """One utterance, the banded form.  float32 inputs [nheads * kc][T] -> float64 [nheads * kc][T]."""
    rows, T = q.shape
    kc = rows // nheads
    qs = scaled_q(q, kc)
    k = np.asarray(k, np.float64)
    v = np.asarray(v, np.float64)
    out = np.zeros((rows, T))
    i = np.arange(T)[:, None]
    j = np.arange(T)[None, :]
    r = j - i + win
    band = (r >= 0) & (r <= 2 * win) & (win > 0)
    rc = np.clip(r, 0, max(2 * win, 0))
    for h in range(nheads):
        sl = slice(h * kc, (h + 1) * kc)
        S = qs[sl].T @ k[sl]                                   # [i][j]
        if win > 0:
            qrel = qs[sl].T @ np.asarray(relk, np.float64)     # [i][r]
            S = S + np.where(band, np.take_along_axis(qrel, rc, axis=1), 0.0)
        E = np.exp(S)
        P = E / E.sum(axis=1, keepdims=True)
        O = P @ v[sl].T                                        # [i][c]
        if win > 0:
            Pb = np.where(band, P, 0.0)
            W = np.zeros((T, 2 * win + 1))                     # W[i][r] = P[i][i + r - win]
            np.add.at(W, (np.broadcast_to(i, (T, T))[band], rc[band]), Pb[band])
            O = O + W @ np.asarray(relv, np.float64).T
        out[sl] = O.T
    return out


def banded(q, k, v, relk, relv, nheads, win, lengths):
    """A packed batch: every utterance on its own."""
    out = np.zeros(q.shape)
    off = 0
    for n in lengths:
        s = slice(off, off + int(n))
        out[:, s] = banded_one(q[:, s], k[:, s], v[:, s], relk, relv, nheads, win)
        off += int(n)
    return out


def _skew_rel_to_abs(x):
    """[T][2T - 1] relative logits -> [T][T] absolute: pad one column, flatten, pad T - 1, reshape [T + 1][2T - 1], slice."""
    T = x.shape[0]
    x = np.pad(x, ((0, 0), (0, 1)))
    x = np.pad(x.reshape(-1), (0, T - 1))
    return x.reshape(T + 1, 2 * T - 1)[:T, T - 1:]


def _skew_abs_to_rel(x):
    """[T][T] absolute weights -> [T][2T - 1] relative: pad T - 1 columns, flatten, pad T in front, reshape [T][2T], drop column 0."""
    T = x.shape[0]
    x = np.pad(x, ((0, 0), (0, T - 1)))
    x = np.pad(x.reshape(-1), (T, 0))
    return x.reshape(T, 2 * T)[:, 1:]


def _rel_embeddings(rel, win, T):
    """[kc][2 win + 1] -> [2T - 1][kc]: padded with zero rows when T > win + 1, sliced otherwise (VITS _get_relative_embeddings)."""
    e = np.asarray(rel, np.float64).T
    pad = max(T - (win + 1), 0)
    start = max((win + 1) - T, 0)
    e = np.pad(e, ((pad, pad), (0, 0)))
    return e[start:start + 2 * T - 1]


def skewed_one(q, k, v, relk, relv, nheads, win):
    """The same attention with DENSE relative logits through the published pad -> reshape -> slice skew (Shaw et al. relative positions as
    VITS applies them), for checking the banded form.  One utterance."""
    rows, T = q.shape
    kc = rows // nheads
    qs = scaled_q(q, kc)
    out = np.zeros((rows, T))
    for h in range(nheads):
        sl = slice(h * kc, (h + 1) * kc)
        S = qs[sl].T @ np.asarray(k[sl], np.float64)
        if win > 0:
            S = S + _skew_rel_to_abs(qs[sl].T @ _rel_embeddings(relk, win, T).T)
        E = np.exp(S)
        P = E / E.sum(axis=1, keepdims=True)
        O = P @ np.asarray(v[sl], np.float64).T
        if win > 0:
            O = O + _skew_abs_to_rel(P) @ _rel_embeddings(relv, win, T)
        out[sl] = O.T
    return out


# ---- inputs of the kernel-level tests -----------------------------------------------------------------------------------------------
def random_case(seed, nheads, kc, win, lengths):
    """q, k Gaussian with score standard deviation ~ 2 (|S| stays far from exp overflow, the band visibly changes P); relK, relV O(1);
    v O(1) plus an offset per key, so that a dropped or duplicated key moves the output by about 1 / T."""
    rng = np.random.default_rng(seed)
    L = int(np.sum(lengths))
    rows = nheads * kc
    q = rng.standard_normal((rows, L))
    k = rng.standard_normal((rows, L)) * 2.0            # S = q . k / sqrt(kc): variance 4
    v = rng.standard_normal((rows, L)) + (np.arange(L) % 7 - 3.0)[None, :]
    relk = relv = None
    if win > 0:
        relk = rng.standard_normal((kc, 2 * win + 1)).astype(np.float32)         # q . relK / sqrt(kc): standard deviation 1
        relv = rng.standard_normal((kc, 2 * win + 1)).astype(np.float32)
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32), relk, relv


def uniform_case(seed, nheads, kc, win, T):
    """q = 0 (k arbitrary): P = 1 / T exactly when T is a power of two; integer v and relV with |.| <= 64 -> every partial sum of
    P v is a multiple of 1 / T below 2^24 / T: exact in float32 in any order.  -> (q, k, v, relk, relv, expected float32)."""
    rng = np.random.default_rng(seed)
    rows = nheads * kc
    q = np.zeros((rows, T), np.float32)
    k = rng.standard_normal((rows, T)).astype(np.float32)
    v = rng.integers(-64, 65, (rows, T)).astype(np.float32)
    relk = relv = None
    want = np.repeat(v.astype(np.float64).mean(axis=1, keepdims=True), T, axis=1)
    if win > 0:
        relk = rng.standard_normal((kc, 2 * win + 1)).astype(np.float32)
        relv = rng.integers(-64, 65, (kc, 2 * win + 1)).astype(np.float32)
        for i in range(T):
            r = np.arange(2 * win + 1)
            ok = (i + r - win >= 0) & (i + r - win < T)
            want[:, i] += np.tile(relv[:, ok].astype(np.float64).sum(axis=1) / T, nheads)
    return q, k, v, relk, relv, want.astype(np.float32)


def onehot_jstar(T, win):
    """j*(i): the offset j* - i walks -win - 1 ... win + 1 (both band ends and one beyond) as i grows, clipped to the utterance."""
    i = np.arange(T)
    return np.clip(i + (i % (2 * win + 3)) - win - 1, 0, T - 1)


def onehot_case(seed, nheads, kc, win, T):
    """Every query attends to exactly one key: S[i][j] = -128 (j - j*(i))^2, an exact integer in float32 in any summation order (all
    terms are integers below 2^23), so S = 0 at j = j*(i) and S <= -128 elsewhere, where expf is exactly 0 with or without denormals
    (exp(-128) ~ 3e-56 < 2^-149).  Three channels per head carry it -- q_i = sqrt(kc) (1, y, y^2) with y = j*(i), k_j = 128 (-j^2, 2 j,
    -1) -- the others are zero; kc must be a power of 4 so that q / sqrt(kc) is exact.  relK = 0.  Then the row sum is exactly 1, P is
    exactly one-hot and O_i = v[:, j*] + relV[:, j* - i + win] inside the band, v[:, j*] outside: one float32 addition.
    -> (q, k, v, relk, relv, expected float32)"""
    root = int(round(np.sqrt(kc)))
    assert root * root == kc and root & (root - 1) == 0 and kc >= 4 and T <= 181
    rng = np.random.default_rng(seed)
    rows = nheads * kc
    js = onehot_jstar(T, win).astype(np.float64)
    j = np.arange(T, dtype=np.float64)
    q = np.zeros((rows, T))
    k = np.zeros((rows, T))
    for h in range(nheads):
        ch = h * kc + np.array([h % kc, (h + kc // 2) % kc, kc - 1 - (h % 2)])     # spread over the waves' channel ranges
        assert len(set(ch.tolist())) == 3
        q[ch[0]], q[ch[1]], q[ch[2]] = root, root * js, root * js * js
        k[ch[0]], k[ch[1]], k[ch[2]] = -128.0 * j * j, 256.0 * j, -128.0
    v = rng.standard_normal((rows, T)).astype(np.float32)
    relk = relv = None
    want = v[:, js.astype(int)].copy()
    if win > 0:
        relk = np.zeros((kc, 2 * win + 1), np.float32)
        relv = rng.standard_normal((kc, 2 * win + 1)).astype(np.float32)
        for i in range(T):
            r = int(js[i]) - i + win
            if 0 <= r <= 2 * win:
                want[:, i] = want[:, i] + np.tile(relv[:, r], nheads)
    return q.astype(np.float32), k.astype(np.float32), v, relk, relv, want.astype(np.float32)


# ---- the shape grid of the kernel-level tests (CPU: restatement <-> oracle; GPU: every kernel <-> restatement) ----------------------
KC_GRID = (5, 16, 18, 50, 96, 100, 128, 144)       # 5: the last wave owns no channel; 100: register refused, no multiple of 16; 128: the
WIN_GRID = (0, 1, 4, 7, 8, 15, 16)                 # matrix-core limit; 144: generic only.  px = 15 | 17: register limit, 31 | 33: matrix-core limit
SHAPES = ([(2, kc, 4) for kc in KC_GRID] + [(2, kc, win) for kc in (96, 16) for win in WIN_GRID if not (kc == 16 and win == 4)] +
          [(1, 32, 4), (3, 32, 4)])                # (nheads, kc, win)
LENGTH_SETS = ("edges", "b128", "b256", "one129", "one256", "one257", "one513")


def lengths_of(name, win):
    if name == "edges":
        return [n for n in (1, 2, win, win + 1, 15, 16, 17, 63, 64, 65) if n >= 1]
    return {"b128": [127, 128, 129], "b256": [255, 256, 257, 300], "one129": [129], "one256": [256], "one257": [257], "one513": [513]}[name]


def documented_route(nheads, kc, win, lengths, attn_reg=True, min_wgs=96):
    """What DESIGN.md says the dispatcher does -> (kernel, keys per lane): 3 = matrix-core from 96 workgroups of 16 queries on, when kc is a
    multiple of 16, kc <= 128 and px <= 32; else 2 = register when kc <= 96, px <= 16 and the longest utterance <= 256 (2 keys per lane
    up to 128, else 4); else 1 = generic."""
    px = 2 * win + 1 if win > 0 else 0
    longest = max(lengths)
    if -(-longest // 16) * nheads * len(lengths) >= min_wgs and mfma_admits(kc, win):
        return 3, 0
    if attn_reg and reg_admits(kc, win, longest):
        return 2, 2 if longest <= 128 else 4
    return 1, 0


def mfma_admits(kc, win):
    return kc % 16 == 0 and kc <= 128 and (2 * win + 1 if win > 0 else 0) <= 32


def reg_admits(kc, win, longest):
    return kc <= 96 and (2 * win + 1 if win > 0 else 0) <= 16 and longest <= 256


def admitted_variants(kc, win, lengths):
    return [1] + ([2] if reg_admits(kc, win, max(lengths)) else []) + ([3] if mfma_admits(kc, win) else [])


def case_seed(nheads, kc, win, name):
    return 20261019 + 1000003 * nheads + 1009 * kc + 31 * win + LENGTH_SETS.index(name)
