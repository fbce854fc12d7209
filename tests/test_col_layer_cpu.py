"""CPU suite for the column-block-layer kernel tests: the float64 restatement of tests/col_layer_ref.py is vouched for by the project's
plain-C oracle (oracle/vits_oracle.c port_dds_layer = the dds_layer function its dds_forward loops over; port_convflow_step = the body of
convflow_inverse with sdp_forward's channel flip; port_oproj_ln = text_encoder's LN(x + conv1x1(att)); tests/test_oracle_cpu.py holds all
three to the compiled reference through whole models).  The oracle's own distance from float64, err_oracle, is the unit of the GPU
file's bars.  The entry's argument checks run without a GPU."""
import os
import re

import numpy as np
import pytest

import col_layer_ref as cr
import spline_ref as sr
from conftest import ROOT
from oracle import pyref
from summertts_amd import engine

GRID = cr.grid()


def _ref(a):
    return cr.ref64(a["x"], a["lengths"], **{k: v for k, v in a.items() if k not in ("x", "lengths")})


@pytest.mark.parametrize("idx", range(len(GRID)), ids=[c["id"] for c in GRID])
def test_oracle_agrees_with_float64_at_float32_rounding_level(port_built, idx):
    """err_oracle = max|port - ref64| is finite and non-zero (the two are different computations) and at most
    C (1 + r^2) 2^-24 max|ref|: a float32 sum of C terms in sequence is off by at most C 2^-24 of its magnitude, and E[x^2] - mean^2 at
    mean = r std magnifies that by 1 + r^2 (r = 1 for the plain cases, 8 for the ill-conditioned ones).  A wrong tap, bias or gain is an
    error of order 1.  Form D's o0 goes through the spline, whose own float32 cost (spline_ref.E_MAX) bounds it; o1 is the kept half."""
    c, a = GRID[idx], cr.make(idx)
    y, o0, o1 = _ref(a)
    py, p0, p1 = cr.oracle(pyref, a)
    assert py.dtype == np.float32 and np.isfinite(py).all() and np.isfinite(y).all()
    eo = float(np.abs(py - y).max())
    r = cr.ILL if c.get("ill") else 1.0
    limit = c["C"] * (1 + r * r) * 2.0 ** -24 * float(np.abs(y).max())
    print(f"COL oracle {c['id']} err_oracle={eo:.3e} limit={limit:.3e}")
    assert 0.0 < eo <= limit, (eo, limit)
    if c["form"] == "D":
        e0 = float(np.abs(p0 - o0).max())
        print(f"COL oracle {c['id']} o0 err_oracle={e0:.3e}")
        assert np.isfinite(p0).all() and 0.0 < e0 <= sr.E_MAX
        assert np.array_equal(p1.astype(np.float64), o1)
        inside = np.abs(a["r1"]) < 5
        assert inside.any() and (~inside).any() and np.array_equal(p0[~inside], a["r1"][~inside]) and np.abs(p0 - a["r1"])[inside].max() > 1e-2
    else:
        assert o0 is None and p0 is None


@pytest.mark.parametrize("C", cr.WIDTHS)
def test_folded_input_restatement_is_the_oracles_bit_for_bit(port_built, C):
    """fl(fl(fl(w r) + b) + g) in numpy float32 == the oracle's conv1d(pre) + add_inplace; a null xr / xs_b is a zero one."""
    p, t = cr.params(C, 3), cr.packed(C, cr.ASCENDING)
    lens = list(cr.ASCENDING)
    layer = (p["dw_w"], p["dw_b"], 1, 1, p["g1"], p["b1"], p["w"], p["bias"], p["g2"], p["b2"])
    for xs_b, xr in ((p["xs_b"], t["xr"]), (None, t["xr"]), (p["xs_b"], None)):
        h = pyref.port_convflow_step(t["x"], lens, p["xs_w"], xs_b, xr, None, *layer, with_input=True)[0]
        mine = cr.fold32(t["x"], p["xs_w"], xs_b, xr)
        assert np.array_equal(h.view(np.uint32), mine.view(np.uint32))
        assert np.abs(h - t["x"]).max() > (1.0 if xr is not None else 0.05)        # and the fold contributes


@pytest.mark.parametrize("idx", [i for i, c in enumerate(GRID) if c.get("ill")], ids=[c["id"] for c in GRID if c.get("ill")])
def test_ill_conditioned_cases_have_the_ratio_they_claim(idx):
    """Per column mean / std of what the LayerNorm sees: ln1 (one dw_b shift for all columns) has median 8 and no column below 4 (the
    columns at an utterance's edge have fewer live taps, a smaller spread and so a larger ratio); ln2 (add shifts every column) is 8 in
    every column.  The plain twin of the same case stays below 2."""
    c, a = GRID[idx], cr.make(idx)
    keys = ("dw_w", "dw_b", "dil", "pad", "xs_w", "xs_b", "xr", "w", "bias", "add", "g1", "b1")
    _, v1, v2 = cr.pre_ln(a["x"], a["lengths"], **{q: a.get(q) for q in keys})
    v = v1 if c["ill"] == "ln1" else v2
    ratio = v.mean(axis=0) / v.std(axis=0)
    print(f"COL ill {c['id']} ratio min={ratio.min():.2f} median={np.median(ratio):.2f} max={ratio.max():.2f}")
    if c["ill"] == "ln1":
        assert abs(np.median(ratio) - cr.ILL) < 0.25 and ratio.min() > 4
        assert np.array_equal(a["bias"], cr.params(c["C"], 3)["bias"])
    else:
        assert np.abs(ratio - cr.ILL).max() < 1e-3
    p, t = cr.params(c["C"], 3), cr.packed(c["C"], c["lens"])
    b = dict(a, x=t["x"], dw_b=p["dw_b"]) if c["ill"] == "ln1" else dict(a, bias=p["bias"], add=t["add"])
    _, w1, w2 = cr.pre_ln(b["x"], b["lengths"], **{q: b.get(q) for q in keys})
    w = w1 if c["ill"] == "ln1" else w2
    assert np.median(np.abs(w.mean(axis=0) / w.std(axis=0))) < 2


def test_packed_equals_per_utterance_and_neighbours_would_matter(port_built):
    C, lens = 32, [1, 2, 9, 40, 3]
    p, t = cr.params(C, 3), cr.packed(C, lens)
    kw = dict(w=p["w"], g2=p["g2"], b2=p["b2"], bias=p["bias"], post_gelu=True, use_res=True, dw_w=p["dw_w"], dw_b=p["dw_b"], dil=9, pad=9,
              g1=p["g1"], b1=p["b1"])
    ref = cr.ref64(t["x"], lens, **kw)[0]
    off = 0
    for n in lens:
        assert np.allclose(cr.ref64(cr.segment(C, n)["x"], [n], **kw)[0], ref[:, off:off + n], rtol=1e-12, atol=1e-12)       # (BLAS blocks differ)
        off += n
    assert np.abs(cr.ref64(t["x"], [sum(lens)], **kw)[0] - ref).max() > 1e-2


def test_grid_covers_what_the_issue_lists():
    assert cr.ASCENDING == (1, 2, 9, 10, 15, 16, 17, 18, 19, 31, 32, 33, 34, 35, 49)
    assert sorted(cr.INTERLEAVED) == list(cr.ASCENDING) and cr.INTERLEAVED[:4] == (1, 49, 2, 35)
    forms = {(c["form"], c["C"]) for c in GRID}
    assert forms == {(f, C) for f in "ABC" for C in cr.WIDTHS} | {("D", C) for C in cr.TAIL_WIDTHS}
    for C in cr.WIDTHS:
        assert {c["geom"] for c in GRID if c["form"] == "A" and c["C"] == C} == set(cr.GEOMS)
        assert {c["lens"] for c in GRID if c["form"] == "A" and c["C"] == C and len(c["lens"]) == 1} == {(n,) for n in cr.ASCENDING}
        assert {c.get("ill") for c in GRID if c["C"] == C} == {None, "ln1", "ln2"}
    for flag in ("no_bias", "no_dw_b", "no_add", "xr_null", "xs_b_null", "fold"):
        assert any(c.get(flag) for c in GRID), flag
    assert len({c["id"] for c in GRID}) == len(GRID)


def test_entry_is_exported_declared_and_bound():
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    assert re.search(r"\bint sts_debug_col_layer\(int device, const float\* x, int32_t C, const int32_t\* lengths, int32_t B, int64_t ld, const float\* xs_w,", hdr)
    assert hasattr(lib, "sts_debug_col_layer") and "sts_debug_col_layer" in engine.EXPORTED_SYMBOLS
    assert len(lib.sts_debug_col_layer.argtypes) == 33
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18\n" in hdr
    assert "`sts_debug_col_layer`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_entry_argument_checks_need_no_gpu():
    """What the entry refuses before it touches a device: STS_EINVAL, whatever machine it runs on; the outputs stay as they were."""
    C = 32
    p = cr.params(C, 3)
    x = np.zeros((C, 20), np.float32)
    base = dict(w=p["w"], g2=p["g2"], b2=p["b2"])
    dds = dict(base, dw_w=p["dw_w"], dw_dil=1, dw_pad=1, g1=p["g1"], b1=p["b1"], post_gelu=True, use_res=True)
    tail = dict(dds, tp_w=p["tp_w"], tp_b=p["tp_b"], tp_fs=4.0)

    def refused(lens, **kw):
        out = (np.full((C, 20), 7, np.float32), np.full(20, 7, np.float32), np.full(20, 7, np.float32))
        with pytest.raises(engine.StsError, match=r"sts error -1\b"):
            engine.debug_col_layer(x, lens, out=out, **kw)
        assert all((o == 7).all() for o in out)

    refused([0, 20], **dds)                                 # a length below 1
    refused([20], **dict(base, g2=None))
    refused([20], **dict(dds, dw_k=0))
    refused([20], **dict(dds, dw_dil=0))
    refused([20], **dict(dds, dw_pad=-1))
    refused([20], **dict(base, dw_b=p["dw_b"]))             # dw_b without dw_w
    refused([20], **dict(dds, xs_b=p["xs_b"]))              # xs_b without xs_w
    refused([20], **dict(dds, xr=np.zeros(20, np.float32)))
    refused([20], **dict(tail, tp_fs=0.0))
    refused([20], **dict(dds, tp_b=p["tp_b"]))              # tp_b without tp_w
    refused([20], **dict(dds, alias=6))
    refused([20], **dict(dds, alias=2))                     # a latent alias without a tail
    refused([20], **dict(tail, alias=2))                    # ... and without that latent half
    refused([20], **dict(tail, alias=4, tp_r0=np.zeros(20, np.float32)))
    with pytest.raises(ValueError):
        engine.debug_col_layer(x, [21], **dds)              # sum(lengths) > ld
    with pytest.raises(ValueError):
        engine.debug_col_layer(x, [20], **dict(dds, w=p["w"][:, :16]))
