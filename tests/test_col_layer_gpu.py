"""GPU suite: ONE launch of the fused column-block layer (col_layer.hip col_layer_kernel<NSUB, TAIL>, seven instantiations: widths 32, 64,
192, 256 and the tail at 32, 64, 192) on caller data through sts_debug_col_layer, against the float64 restatement of
tests/col_layer_ref.py (which tests/test_col_layer_cpu.py ties to the plain-C oracle).  Forms: A a DDSConv layer, B the same on the
folded rank-1 input, C the attention output projection with its residual and LayerNorm, D = A / B with the 29-row projection and the
reverse spline step behind it.

Bars, per case, in units of the oracle's own error (err_oracle = |port - ref64|, computed here on the CPU from the oracle's float32 loops):
    max|kernel - ref64| <= 4 max(err_oracle) + 2^-22 max|ref|          (the bar of tests/test_text_kernels_gpu.py)
    rms(kernel - ref64) <= 2 rms(err_oracle)                           (the RMS margin of tests/test_spline_gpu.py)
for y, and for form D's o0 against the oracle's composite (the spline's own sensitivity is in both sides); one-utterance calls carry
both bars each.  Every figure is printed before it
is asserted (pytest -s shows them); DESIGN.md section 3 records the largest per instantiation.

The bit-for-bit tests, the tail plumbing, the sentinels and the limits are conditions, not measurements.  Every launch runs with ld = L + 37
(NaN in the columns [L, ld) of every input) and one spare output row, and checks that no element of [C][L] stayed 0xFFFFFFFF and that
nothing outside it changed."""
import functools

import numpy as np
import pytest

import col_layer_ref as cr
from oracle import pyref
from summertts_amd import engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF
FLOOR = 2.0 ** -22
GRID = cr.grid()
BATCHES = [i for i, c in enumerate(GRID) if len(c["lens"]) > 1]
NAMES = dict(dil="dw_dil", pad="dw_pad", r0="tp_r0", r1="tp_r1")


def bits(v):
    return np.ascontiguousarray(v).view(np.uint32)


def padded(v, ld):
    if v is None:
        return None
    out = np.full(v.shape[:-1] + (ld,), np.nan, np.float32)
    out[..., :v.shape[-1]] = v
    return out


def launch(a, alias=0, **over):
    """One launch of the case `a` (keyword arguments of col_layer_ref.ref64), ld = L + 37 with NaN past L in x, add, xr, r0 and r1, one spare
    row of y.  Checks the sentinels, o1 == r0 and that a tail call leaves y alone.  -> (y [C][L] or None with a tail, o0 [L], o1 [L])"""
    a = dict(a, **over)
    C, L = a["x"].shape
    ld = L + cr.PAD
    kw = {NAMES.get(k, k): v for k, v in a.items() if k not in ("x", "lengths")}
    for k in ("add", "xr", "tp_r0", "tp_r1"):
        kw[k] = padded(kw.get(k), ld)
    y, o0, o1 = engine.debug_col_layer(padded(a["x"], ld), a["lengths"], alias=alias, extra_rows=1, **kw)
    assert y.shape == (C + 1, ld)
    yb = bits(y)
    if kw.get("tp_w") is None:
        assert o0 is None and o1 is None
        assert (yb[C:, :] == SENTINEL).all(), "a workgroup wrote a row past C"
        assert (yb[:, L:] == SENTINEL).all(), "a workgroup wrote a column in [L, ld)"
        assert not (yb[:C, :L] == SENTINEL).any(), "an element of [C][L] was left unwritten"
        return np.ascontiguousarray(y[:C, :L]), None, None
    assert (yb == SENTINEL).all(), "a tail call wrote y"
    assert o0.shape == (ld,) and o1.shape == (ld,)
    assert (bits(o0)[L:] == SENTINEL).all(), "o0 was written past L"
    assert not (bits(o0)[:L] == SENTINEL).any() and not (bits(o1)[:L] == SENTINEL).any(), "a column of o0 / o1 was left unwritten"
    if alias == 5:                  # o1 IS r0's buffer: its columns past L are r0's own
        assert np.array_equal(bits(o1)[L:], bits(kw["tp_r0"])[L:])
    else:
        assert (bits(o1)[L:] == SENTINEL).all(), "o1 was written past L"
    keep = np.zeros(L, np.float32) if a.get("r0") is None else a["r0"]
    assert np.array_equal(bits(o1[:L]), bits(keep)), "o1 is the kept half r0, bit for bit"
    return None, o0[:L].copy(), o1[:L].copy()


@functools.lru_cache(maxsize=None)
def reference(idx):
    """(ref64 y, o0; oracle y, o0) of grid case idx -- computed once, shared, left unchanged."""
    a = cr.make(idx)
    y, o0, _ = cr.ref64(a["x"], a["lengths"], **{k: v for k, v in a.items() if k not in ("x", "lengths")})
    py, p0, _ = cr.oracle(pyref, a)
    out = (y, o0, py, p0)
    for v in out:
        if v is not None:
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kernel(idx):
    out = launch(cr.make(idx))
    for v in out:
        if v is not None:
            v.setflags(write=False)
    return out


def judge(tag, what, got, ref, port, rms=True):
    """Both bars on one tensor; -> (err_kernel, err_oracle) arrays."""
    err, eo = np.abs(got - ref), np.abs(port - ref)
    tol = 4 * float(eo.max()) + FLOOR * float(np.abs(ref).max())
    rk, ro = float(np.sqrt(np.mean(err ** 2))), float(np.sqrt(np.mean(eo ** 2)))
    worst = np.unravel_index(np.argmax(err), err.shape)
    print(f"COL {tag} {what} err_kernel={err.max():.3e} err_oracle={eo.max():.3e} ratio={err.max() / eo.max():.3f} tol={tol:.3e} "
          f"rms_kernel={rk:.3e} rms_oracle={ro:.3e} rms_ratio={rk / ro:.3f} worst={tuple(int(v) for v in worst)}")
    assert np.isfinite(got).all(), (tag, what)
    assert err.max() <= tol, (tag, what, worst, float(err.max()), tol)
    if rms:
        assert rk <= 2 * ro, (tag, what, rk, ro)
    return err, eo


@pytest.mark.parametrize("idx", BATCHES, ids=[GRID[i]["id"] for i in BATCHES])
def test_packed_batch_against_float64(idx):
    """Every packed case of the grid: forms A - D, every instantiated width, the nine depthwise geometries, ascending and short-long
    interleaved batches on the block and dilation edges, absent bias / dw_b / add / xr / xs_b, and the two ill-conditioned LayerNorms.
    D-C32-k3d9p9-asc is the case that indicted the contracted arithmetic of rq_spline_inverse_t (devmath.hpp): o0 was 9.586e-05 from float64
    against the oracle's 1.647e-05 at column 163, where the discriminant is 3.0e-4; with contraction off there it is 1.647e-05."""
    c = GRID[idx]
    y, o0, py, p0 = reference(idx)
    ky, k0, _ = kernel(idx)
    if c["form"] == "D":
        judge(c["id"], "o0", k0, o0, p0)
        inside = np.abs(cr.make(idx)["r1"]) < 5
        assert np.array_equal(bits(k0[~inside]), bits(cr.make(idx)["r1"][~inside])), "outside (-5, 5) the spline is the identity"
    else:
        judge(c["id"], "y", ky, y, py)


@pytest.mark.parametrize("C", cr.WIDTHS)
def test_one_utterance_calls_against_float64(C):
    """Form A at dilation 9, every length of the batch as a call of its own: both bars on every call (a call of one column is C numbers),
    and the RMS of all fifteen pooled as one more figure."""
    errs, eos = [], []
    for idx in (i for i, c in enumerate(GRID) if c["C"] == C and len(c["lens"]) == 1):
        y, _, py, _ = reference(idx)
        err, eo = judge(GRID[idx]["id"], "y", kernel(idx)[0], y, py)
        errs.append(err.ravel())
        eos.append(eo.ravel())
    assert len(errs) == len(cr.ASCENDING)
    rk, ro = (float(np.sqrt(np.mean(np.concatenate(v) ** 2))) for v in (errs, eos))
    print(f"COL A-C{C}-alone-pooled y rms_kernel={rk:.3e} rms_oracle={ro:.3e} rms_ratio={rk / ro:.3f}")
    assert rk <= 2 * ro


def _case(form, C, geom=cr.PREDICTOR[2], lens=cr.ASCENDING, **flags):
    """The ref64 arguments of a case outside the grid, built as the grid builds its own."""
    k, dil, pad = geom
    p, t = cr.params(C, k), cr.packed(C, lens)
    a = dict(x=t["x"], lengths=list(lens), w=p["w"], g2=p["g2"], b2=p["b2"], bias=p["bias"])
    if form == "C":
        return dict(a, add=t["add"], post_gelu=False, use_res=False)
    a.update(dw_w=p["dw_w"], dw_b=p["dw_b"], dil=dil, pad=pad, g1=p["g1"], b1=p["b1"], post_gelu=True, use_res=True)
    if flags.get("fold"):
        a.update(xs_w=p["xs_w"], xs_b=p["xs_b"], xr=t["r0"] if flags.get("tail") else t["xr"])
    if flags.get("tail"):
        a.update(tp_w=p["tp_w"], tp_b=p["tp_b"], tp_fs=float(np.float32(np.sqrt(np.float32(C)))), r0=t["r0"], r1=t["r1"])
    return a


def same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert np.array_equal(bits(u), bits(v))


@pytest.mark.parametrize("C", cr.WIDTHS)
def test_folded_input_equals_the_materialised_one_bit_for_bit(C):
    """Form B == form A on h = fl(fl(fl(xs_w xr) + xs_b) + x) made in numpy float32 (the residual included); a null xr is a zero xr, a null
    xs_b a zero xs_b; with the tail too where the width has one."""
    b = _case("B", C, fold=True)
    zeros_r, zeros_b = np.zeros_like(b["xr"]), np.zeros_like(b["xs_b"])
    for xs_b, xr in ((b["xs_b"], b["xr"]), (None, b["xr"]), (b["xs_b"], None)):
        folded = launch(b, xs_b=xs_b, xr=xr)
        same(folded, launch(b, x=cr.fold32(b["x"], b["xs_w"], xs_b, xr), xs_w=None, xs_b=None, xr=None))
        if xs_b is None or xr is None:
            same(folded, launch(b, xs_b=zeros_b if xs_b is None else xs_b, xr=zeros_r if xr is None else xr))
    if C in cr.TAIL_WIDTHS:
        d = _case("D", C, geom=cr.PREDICTOR[0], lens=cr.INTERLEAVED, fold=True, tail=True)
        same(launch(d), launch(d, x=cr.fold32(d["x"], d["xs_w"], d["xs_b"], d["xr"]), xs_w=None, xs_b=None, xr=None))


@pytest.mark.parametrize("C", cr.WIDTHS)
def test_absent_operands_equal_zeros_bit_for_bit(C):
    z = np.zeros(C, np.float32)
    a = _case("A", C, geom=cr.GEOMS[6], lens=cr.INTERLEAVED)
    same(launch(a, bias=None, dw_b=None), launch(a, bias=z, dw_b=z))
    c = _case("C", C)
    same(launch(c, bias=None, add=None), launch(c, bias=z, add=np.zeros_like(c["add"])))
    same(launch(a, add=None), launch(a, add=np.zeros_like(a["x"])))


@pytest.mark.parametrize("C", cr.WIDTHS)
def test_every_utterance_alone_equals_its_columns_in_the_batch(C):
    """At any position: the ascending batch, the interleaved one, and each utterance as a call of its own."""
    alone = {GRID[i]["lens"][0]: kernel(i)[0] for i, c in enumerate(GRID) if c["C"] == C and len(c["lens"]) == 1}
    for lens in (cr.ASCENDING, cr.INTERLEAVED):
        y = launch(_case("A", C, lens=lens))[0]
        off = 0
        for n in lens:
            assert np.array_equal(bits(y[:, off:off + n]), bits(alone[n])), (lens[:2], n)
            off += n


@pytest.mark.parametrize("form,C", [(f, C) for C in cr.WIDTHS for f in ("B", "C")] + [("DB", C) for C in cr.TAIL_WIDTHS])
def test_every_utterance_alone_equals_its_columns_in_the_batch_in_the_other_forms(form, C):
    """The folded input, the output projection and the folded layer with the tail: every utterance of the interleaved batch as a call of
    its own returns the batch's columns (y, or o0 and o1), bit for bit."""
    flags = dict(fold=form in ("B", "DB"), tail=form == "DB")
    name = "D" if form == "DB" else form
    got = launch(_case(name, C, geom=cr.PREDICTOR[1], lens=cr.INTERLEAVED, **flags))
    off = 0
    for n in cr.INTERLEAVED:
        want = launch(_case(name, C, geom=cr.PREDICTOR[1], lens=(n,), **flags))
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert np.array_equal(bits(g[..., off:off + n]), bits(w)), (form, n)
        off += n


FORMS = [(f, C) for C in cr.WIDTHS for f in ("A", "B", "C")] + [(f, C) for C in cr.TAIL_WIDTHS for f in ("D", "DB")]


@pytest.mark.parametrize("form,C", FORMS)
def test_layer_never_reads_a_neighbouring_utterance(form, C):
    """Two middle utterances (17 columns: two blocks; 3 columns: every dilated tap reaches past both ends) between all-NaN neighbours -- x,
    add, xr, r0 and r1 alike -- equal themselves run alone, bit for bit."""
    flags = dict(fold=form in ("B", "DB"), tail=form in ("D", "DB"))
    lens, mids = (9, 17, 7, 3, 9), (1, 3)
    full = _case(form[0] if form != "DB" else "D", C, lens=lens, **flags)
    off = np.concatenate([[0], np.cumsum(lens)])
    poisoned = dict(full)
    for k in ("x", "add", "xr", "r0", "r1"):
        if full.get(k) is not None:
            v = full[k].copy()
            for b in (0, 2, 4):
                v[..., off[b]:off[b + 1]] = np.nan
            poisoned[k] = v
    got = launch(poisoned)
    for b in mids:
        sl = slice(off[b], off[b + 1])
        cut = {k: (np.ascontiguousarray(v[..., sl]) if k in ("x", "add", "xr", "r0", "r1") and v is not None else v) for k, v in full.items()}
        want = launch(dict(cut, lengths=[lens[b]]))
        for g, w in zip(got[:2], want[:2]):
            if g is not None:
                assert np.isfinite(g[..., sl]).all(), (form, lens[b])
                assert np.array_equal(bits(g[..., sl]), bits(w)), (form, lens[b])


@pytest.mark.parametrize("C", cr.TAIL_WIDTHS)
def test_tail_plumbing_is_exact(C):
    """Null r0 / r1 are zeros; with tp_w = 0 the spline sees tp_b alone; with a one-hot tp_w (row j picks channel c_j, tp_b = 0) it sees
    rows c_j of the same call's non-tail y -- the FMA chain is exact in both -- so o0 equals sts_debug_spline_step on that h, bit for bit.
    (o1 == r0 and an untouched y are checked on every tail launch of this file.)"""
    d = _case("D", C, tail=True)
    L = d["x"].shape[1]
    assert (np.abs(d["r1"]) > 5).any() and (np.abs(d["r1"]) < 5).any() and (d["r1"] == 5).any() and (d["r1"] == -5).any()
    z = np.zeros(L, np.float32)
    same(launch(d, r0=None, r1=None), launch(d, r0=z, r1=z))
    # tp_w = 0
    _, o0, _ = launch(d, tp_w=np.zeros((29, C), np.float32))
    h = np.repeat(d["tp_b"][:, None], L, axis=1)
    s0, s1 = engine.debug_spline_step(h, d["tp_fs"], d["r0"], d["r1"])
    assert np.array_equal(bits(o0), bits(s0)) and np.array_equal(bits(s1), bits(d["r0"]))
    # one-hot tp_w
    rng = np.random.default_rng(C)
    pick = rng.permutation(C)[:29]
    pick[0], pick[28] = 0, C - 1
    hot = np.zeros((29, C), np.float32)
    hot[np.arange(29), pick] = 1
    y = launch(d, tp_w=None, tp_b=None, r0=None, r1=None)[0]
    _, o0, _ = launch(d, tp_w=hot, tp_b=np.zeros(29, np.float32))
    s0, _ = engine.debug_spline_step(np.ascontiguousarray(y[pick]), d["tp_fs"], d["r0"], d["r1"])
    assert np.array_equal(bits(o0), bits(s0))
    assert np.abs(o0 - d["r1"])[np.abs(d["r1"]) < 5].max() > 1e-2            # (and the spline does move what is inside)


def refused(a, alias=0, **over):
    """STS_EINVAL, nothing launched: the outputs handed in are still the sentinel."""
    a = dict(a, **over)
    C, L = a["x"].shape
    ld = L + cr.PAD
    kw = {NAMES.get(k, k): v for k, v in a.items() if k not in ("x", "lengths")}
    for k in ("add", "xr", "tp_r0", "tp_r1"):
        kw[k] = padded(kw.get(k), ld)
    out = tuple(np.full(s, np.nan, np.float32).view(np.uint32) for s in ((C + 1, ld), (ld,), (ld,)))
    for o in out:
        o[...] = SENTINEL
    with pytest.raises(engine.StsError, match=r"sts error -1\b"):
        engine.debug_col_layer(padded(a["x"], ld), a["lengths"], alias=alias, extra_rows=1, out=tuple(o.view(np.float32) for o in out), **kw)
    assert all((o == SENTINEL).all() for o in out)


def test_shapes_outside_the_limits_are_refused():
    lens = (17, 5)
    for C in (48, 96, 128):                                                    # widths without an instantiation
        refused(_case("A", C, lens=lens))
        refused(_case("C", C, lens=lens))
    refused(_case("D", 256, lens=lens, tail=True))                             # a tail at 256
    a = _case("A", 64, lens=lens)
    refused(a, dw_k=0)
    refused(dict(a, dw_w=cr.params(64, 4)["dw_w"]))                            # four taps
    c = _case("C", 64, lens=lens)
    p = cr.params(64, 3)
    refused(c, xs_w=p["xs_w"])                                                 # the folded input without the conv
    refused(a, xs_w=p["xs_w"], use_res=False)                                  # ... and without the residual it is defined with
    refused(a, g1=None)
    refused(a, b1=None)
    refused(a, g1=None, b1=None)
    assert np.isfinite(launch(a)[0]).all() and np.isfinite(launch(c)[0]).all()     # and the entry does run what is inside them


def test_aliased_buffers_are_refused_except_o1_on_r0():
    lens = (17, 5)
    a = _case("A", 64, lens=lens)
    d = _case("D", 64, lens=lens, tail=True)
    refused(a, alias=1)                                                        # y = x
    refused(d, alias=1)
    for alias in (2, 3, 4):                                                    # o0 = r0, o0 = r1, o1 = r1
        refused(d, alias=alias)
    same(launch(d, alias=5), launch(d))                                        # o1 = r0: each thread reads its column before it writes it
