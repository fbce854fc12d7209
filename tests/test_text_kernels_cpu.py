"""CPU suite for the kernel-level text-encoder tests: the float64 restatements (tests/attention_ref.py, tests/layer_norm_ref.py) are vouched
for by the project's plain-C oracle (oracle/vits_oracle.c port_attention / port_layer_norm -- the very loops its model path runs, which
tests/test_oracle_cpu.py holds to the compiled reference), the banded attention by a dense pad -> reshape -> slice skew, and the two exact
constructions give their stated values.  The entries' argument checks run without a GPU."""
import os
import re

import numpy as np
import pytest

import attention_ref as ar
import layer_norm_ref as lr
from conftest import ROOT
from oracle import pyref
from summertts_amd import engine

EPS32 = 2.0 ** -24


@pytest.mark.parametrize("nheads,kc,win", ar.SHAPES)
def test_attention_restatement_agrees_with_the_oracle_on_the_grid(port_built, nheads, kc, win):
    """Bound on the oracle's own float32 rounding: a score is a sequential sum of kc (+ kc) products of magnitude |S| <~ 12, so its
    error is <= (2 kc + 2) eps |q|.|k| <~ 1e-4 at kc = 144, and exp turns an absolute score error into a relative error of P; the T-term
    sequential sums (row sum, P.V) add <= T eps.  With |v| <= 8: err <= 8 ((2 kc + 2) eps sum|q_c k_c| + 2 T eps) -- bounded here by
    the measured sum|q_c k_c| of the case.  (Measured: 1e-6 ... 8e-6 over the grid.)"""
    for name in ar.LENGTH_SETS:
        lens = ar.lengths_of(name, win)
        q, k, v, relk, relv = ar.random_case(ar.case_seed(nheads, kc, win, name), nheads, kc, win, lens)
        ref = ar.banded(q, k, v, relk, relv, nheads, win, lens)
        got = pyref.port_attention(q, k, v, relk, relv, nheads, win, lens)
        assert np.isfinite(got).all() and np.isfinite(ref).all(), (name, "the oracle must stay finite on every case of the grid")
        absdot = float(np.abs(q).max() * np.abs(k).max() * np.sqrt(kc))        # >= sum_c |qs_c k_c| (Cauchy-Schwarz would be tighter)
        bound = float(np.abs(v).max()) * ((2 * kc + 2) * EPS32 * absdot + 2 * max(lens) * EPS32)
        err = float(np.abs(got - ref).max())
        assert err <= bound, (name, err, bound)
        assert err <= 2e-5, (name, err)                       # and in absolute terms: a band or key error is >= 1e-3 here


@pytest.mark.parametrize("win,T", [(4, 1), (4, 3), (4, 4), (4, 5), (4, 6), (4, 64), (1, 1), (1, 2), (1, 40), (16, 9), (16, 17), (16, 18),
                                   (16, 150), (7, 8), (7, 100)])
def test_banded_attention_equals_the_dense_skew(win, T):
    """T < win + 1 (the relative table is sliced), T = win + 1 (used whole), T >> win (padded with zero rows): the band form
    S += q . relK[j - i + win], O += P[i][j] relV[j - i + win] is what the pad -> reshape -> slice skew of the dense relative logits means."""
    for nheads, kc in ((2, 6), (1, 16), (3, 5)):
        q, k, v, relk, relv = ar.random_case(100 * win + T, nheads, kc, win, [T])
        a = ar.banded_one(q, k, v, relk, relv, nheads, win)
        b = ar.skewed_one(q, k, v, relk, relv, nheads, win)
        assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(a).max())
        # and the band matters: without the relative terms the result moves by far more than any tolerance used on it
        assert np.abs(a - ar.banded_one(q, k, v, None, None, nheads, 0)).max() > 1e-2


@pytest.mark.parametrize("win", [0, 4])
def test_uniform_construction_is_exact_in_the_restatement_and_the_oracle(port_built, win):
    for T in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        q, k, v, relk, relv, want = ar.uniform_case(7 + T, 2, 5, win, T)
        ref = ar.banded_one(q, k, v, relk, relv, 2, win)
        assert (ref == want.astype(np.float64)).all()          # float64 gives exactly the float32-representable value
        got = pyref.port_attention(q, k, v, relk, relv, 2, win, [T])
        assert (got == want).all()


@pytest.mark.parametrize("T", [17, 65, 129])
def test_onehot_construction_is_exact_in_the_restatement_and_the_oracle(port_built, T):
    win = 4
    js = ar.onehot_jstar(T, win)
    d = js - np.arange(T)
    assert set(range(-win - 1, win + 2)) <= set(d.tolist())                 # both band ends and one beyond, in both directions
    assert js.min() == 0 and js.max() == T - 1                                # clipped at both utterance edges
    for nheads, kc in ((2, 16), (1, 64), (3, 16)):
        q, k, v, relk, relv, want = ar.onehot_case(11 + T, nheads, kc, win, T)
        ref = ar.banded_one(q, k, v, relk, relv, nheads, win)
        assert np.abs(ref - want).max() <= 2 * EPS32 * np.abs(want).max()    # want = float32(v + relV): one rounding away from float64
        got = pyref.port_attention(q, k, v, relk, relv, nheads, win, [T])
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # a band index off by one at either end changes the expected value by O(1)
    q, k, v, relk, relv, want = ar.onehot_case(11 + T, 2, 16, win, T)
    shifted = ar.banded_one(q, k, v, relk, np.roll(relv, 1, axis=1), 2, win)
    assert np.abs(shifted - want).max() > 0.1


@pytest.mark.parametrize("idx", range(len(lr.grid())), ids=[g[0] for g in lr.grid()])
def test_layer_norm_restatement_agrees_with_the_oracle_on_the_grid(port_built, idx):
    """Oracle rounding: var = sum(x^2) / C - mean^2 is formed in float32, so it carries an absolute error of about C eps E[x^2] / 2 (the
    sequential sums) and y = (x - mean) / sqrt(var) a relative error of half of that over var: |y| (C/4 + 4) eps (1 + mean^2 / var),
    plus a few eps for the affine map, GELU and the residual.  For |mean| <= std that is <= 2e-5 at C = 300; the mean = 8 std columns
    multiply it by 65 (measured there: 1.9e-4 ... 2.4e-4, against 1e-6 ... 5e-6 elsewhere)."""
    name, kw, flags = lr.grid()[idx]
    d = lr.make(idx)
    ref = lr.reference(**d)
    got = lr.oracle_route(pyref.port_layer_norm, **d)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    C = kw["C"]
    ratio = 1.0 + (kw.get("mean_over_std") or 1.0) ** 2
    bound = float(np.abs(ref).max() + 1.0) * ((C / 4.0 + 4.0) * EPS32 * ratio + 8 * EPS32)
    err = float(np.abs(got - ref).max())
    assert err <= bound, (name, err, bound)


def test_layer_norm_conv_padding_is_inside_the_utterance():
    """A tap that leaves its utterance reads zero, never the neighbour: the packed restatement equals every utterance on its own."""
    for k, dil in lr.CONVS:
        d = lr.random_case(5, 33, lr.PACKED, conv=(k, dil))
        whole = lr.reference(**d)
        off = 0
        for n in lr.PACKED:
            one = dict(d, a=d["a"][:, off:off + n], lengths=[n])
            assert np.abs(lr.reference(**one) - whole[:, off:off + n]).max() <= 1e-13        # (numpy's own summation blocking differs)
            off += n
        assert dil * (k - 1) // 2 >= 1 or k == 1
    d = lr.random_case(5, 33, lr.PACKED, conv=(3, 9))                # pad = 9: in the 1-position utterance only the centre tap lands inside
    assert (lr.ln_input(d["a"], d["lengths"], None, False, d["dw_w"], d["dw_b"], 9, 9)[:, 0] ==
            d["dw_b"].astype(np.float64) + d["dw_w"].astype(np.float64)[1] * d["a"][:, 0]).all()


def test_documented_routes_cover_every_limit():
    """The grid reaches every route of the dispatcher and both sides of every limit (what the GPU file then asserts kernel by kernel)."""
    seen = set()
    for nheads, kc, win in ar.SHAPES:
        for name in ar.LENGTH_SETS:
            lens = ar.lengths_of(name, win)
            seen.add(ar.documented_route(nheads, kc, win, lens))
    assert seen == {(1, 0), (2, 2), (2, 4), (3, 0)}
    assert ar.documented_route(2, 96, 4, [129]) == (2, 4) and ar.documented_route(2, 96, 4, [256]) == (2, 4)
    assert ar.documented_route(2, 96, 4, [257]) == (1, 0) and ar.documented_route(2, 16, 4, [513]) == (1, 0)
    assert ar.documented_route(2, 96, 7, [128]) == (2, 2) and ar.documented_route(2, 96, 8, [128]) == (1, 0)        # px 15 | 17
    assert ar.documented_route(2, 96, 15, [255, 256, 257, 300]) == (3, 0) and ar.documented_route(2, 96, 16, [255, 256, 257, 300]) == (1, 0)
    assert ar.documented_route(2, 128, 4, [127, 128, 129]) == (1, 0) and ar.documented_route(2, 128, 4, [255, 256, 257, 300]) == (3, 0)
    assert ar.documented_route(2, 100, 4, [255, 256, 257, 300]) == (1, 0) and ar.documented_route(2, 144, 4, [129]) == (1, 0)


def test_debug_entries_are_declared_bound_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    lib = engine.load_library()
    assert re.search(r"\bint sts_debug_attention\(int device, const float\* q, const float\* k, const float\* v, const float\* relk, "
                     r"const float\* relv, int32_t nheads,\s+int32_t kc, int32_t win, const int32_t\* lengths, int32_t B, int variant, "
                     r"float\* o, int32_t o_rows,\s+int32_t\* variant_out, int32_t\* jpl_out\);", hdr)
    assert re.search(r"\bint sts_debug_layer_norm\(int device, const float\* a, const float\* b, int32_t nb, int64_t b_stride, ", hdr)
    for name, nargs in (("sts_debug_attention", 16), ("sts_debug_layer_norm", 20)):
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS and len(getattr(lib, name).argtypes) == nargs
        assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18\n" in hdr
    z = np.zeros((10, 8), np.float32)
    with pytest.raises(ValueError):
        engine.debug_attention(z, z, z, None, None, 3, 0, [8])                 # 10 rows, 3 heads
    with pytest.raises(ValueError):
        engine.debug_attention(z, z, z, None, None, 2, 0, [7])                 # lengths do not add up
    with pytest.raises(ValueError):
        engine.debug_attention(z, z, z, np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), 2, 0, [8])
    with pytest.raises(ValueError):
        engine.debug_layer_norm(z, np.ones(9, np.float32), np.zeros(10, np.float32), [8])
    # limits checked by the library before any device is touched: STS_EINVAL (-1), nothing launched
    rel = np.zeros((5, 17), np.float32)
    for variant, args in ((2, (z, z, z, rel, rel, 2, 8, [8])),                  # px = 17 > 16: register kernel refused
                          (3, (z, z, z, None, None, 2, 0, [8])),                # kc = 5: no multiple of 16
                          (7, (z, z, z, None, None, 2, 0, [8]))):
        with pytest.raises(engine.StsError, match=r"sts error -1\b"):
            engine.debug_attention(*args, variant=variant)
    with pytest.raises(engine.StsError, match=r"sts error -1\b"):
        engine.debug_attention(z, z, z, None, None, 2, 0, [8, 0])              # an empty utterance
    long = np.zeros((2, 40000), np.float32)
    with pytest.raises(engine.StsError, match=r"sts error -1\b.*too long"):     # generic LDS row 5 T floats > 160 KiB: as the engine refuses it
        engine.debug_attention(long, long, long, None, None, 2, 0, [40000])
    with pytest.raises(engine.StsError, match=r"sts error -1\b"):
        engine.debug_attention(long, long, long, None, None, 2, 0, [40000], variant=1)
