"""CPU suite: the float64 definition of the conv epilogues and operand forms (tests/conv_epi_ref.py) on hand-made cases with known answers
and against the plain-C oracle's WaveNet layer; the float32 evaluation error E_t of the project's tanh / sigmoid formulas, the unit of the GPU
file's activation bounds; the conditions that keep the GPU file discriminating; and sts_debug_conv1d_epi's declaration and argument checks,
every one of which answers before any device call."""
import os
import re

import numpy as np
import pytest

import conv_epi_ref as R
from conftest import ROOT
from conv_epi_ref import GATE, RESADD, RESSKIP, STORE, SUB, TANH_PCM
from oracle import pyref
from packed_conv_ref import packed_conv_ref64
from summertts_amd import engine
from test_packed_conv_gpu import LENGTHS, ORDERS

ONE = np.ones((1, 1, 1), np.float32)          # the identity conv on one channel


def _row(*v):
    return np.array([v], np.float32)


def test_reflect_view_on_lengths_1_2_5():
    assert R.reflect_view(_row(7)).tolist() == [[0, 7]]
    assert R.reflect_view(_row(7, 9)).tolist() == [[9, 7, 9]]
    assert R.reflect_view(_row(1, 2, 3, 4, 5)).tolist() == [[2, 1, 2, 3, 4, 5]]
    # through a 3-tap box filter: 'same' padding on the L + 1 positions of every segment
    out = R.epi_ref64([_row(7), _row(7, 9), _row(1, 2, 3, 4, 5)], np.ones((1, 3, 1), np.float32), None, in_reflect=1)
    assert [d["y"].tolist() for d in out] == [[[7, 7]], [[16, 25, 16]], [[3, 5, 6, 9, 12, 9]]]
    assert R.spans([1, 2, 5], gap=5, extra=1) == [(0, 2), (7, 10), (15, 21)] and R.row_len([1, 2, 5], 5, 1, 1) == 26
    assert R.spans([1, 2], gap=3, scale=4) == [(0, 4), (16, 24)]


def test_res_skip_routing():
    x = [np.array([[1, 2], [3, 4]], np.float32)]
    y0, a0 = [np.array([[10, 20], [30, 40]], np.float32)], [np.array([[100, 200], [300, 400]], np.float32)]
    w = np.zeros((4, 1, 2), np.float32)
    w[0, 0, 0] = w[1, 0, 1] = 1
    w[2, 0, 0] = w[3, 0, 1] = 2             # v = (x0, x1, 2 x0, 2 x1)
    for flag, aux in ((0, [[102, 204], [306, 408]]), (1, [[2, 4], [6, 8]])):
        d = R.epi_ref64(x, w, None, epi=RESSKIP, epi_flag=flag, H=2, y_init=y0, aux_init=a0)[0]
        assert d["y"].tolist() == [[11, 22], [33, 44]] and d["aux"].tolist() == aux
    for flag, aux in ((0, [[101, 202], [303, 404]]), (1, [[1, 2], [3, 4]])):           # Cout = H: every row goes to aux, y has no part
        d = R.epi_ref64(x, w[:2], None, epi=RESSKIP, epi_flag=flag, H=2, y_init=y0, aux_init=a0)[0]
        assert d["y"] is None and d["aux"].tolist() == aux
    assert R.epi_ref64(x, w[:2], np.array([1, 1], np.float32), epi=SUB, y_init=y0)[0]["y"].tolist() == [[8, 17], [26, 35]]
    assert R.epi_ref64(x, w[:2], None, epi=RESADD, res=y0, ubias=np.array([[5], [6]], np.float32))[0]["y"].tolist() == [[16, 27], [39, 50]]


def test_gate_pairs_source_rows_c_and_c_plus_H():
    """Rows (c, c + H) of the SOURCE order: a huge sigmoid pre-activation opens the gate of its own channel alone."""
    w = np.zeros((4, 1, 1), np.float32)
    b = np.array([0.5, -0.25, 100.0, -100.0], np.float32)      # channel 0: tanh(0.5) x 1; channel 1: tanh(-0.25) x 0
    y = R.epi_ref64([_row(0, 0)], w, b, epi=GATE, H=2)[0]["y"]
    assert np.allclose(y[0], np.tanh(0.5), rtol=0, atol=1e-15) and np.abs(y[1]).max() < 1e-40


def test_mean_is_formed_in_the_kernels_order():
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    left, right = ((a + b) + c) / np.float32(3), (a + (b + c)) / np.float32(3)
    assert left != right
    got = R.mean32(_row(a), _row(b), _row(c), 3)
    assert got.dtype == np.float32 and got[0, 0] == left
    assert R.mean32(_row(1, 3), _row(2, 4), None, 2).tolist() == [[1.5, 3.5]] and R.mean32(_row(5), None, None, 0).tolist() == [[5]]
    # first the mean, then the reflect view, then the activation
    out = R.epi_ref64([_row(-4, 6)], ONE, None, in_slope=0.5, in_reflect=1, nsum=2, xs1=[_row(-2, 2)])[0]["y"]
    assert out.tolist() == [[4, -1.5, 4]]


def test_pcm_cast_truncates_and_wraps():
    assert R.pcm_cast(np.array([0.0, 1.0, -1.0, 0.99999, 1.5, 1e30], np.float32)).tolist() == [0, 32737, -32737, 32736, int(np.int16(49105 - 65536)), 0]


def _oracle_bound(x, lens, in_w, in_b, g2, rs_w, rs_b, old, e_gate):
    """First-order bound of the oracle's float32 layer against float64: sequential sums of n terms are within n 2^-24 of the sum of the
    terms' magnitudes; the gate passes errors of v_t once and of v_s a quarter; e_gate is the activations' own evaluation error."""
    u, H = 2.0 ** -24, x.shape[0]
    k = in_w.shape[1]
    s1 = packed_conv_ref64(np.abs(x), lens, np.abs(in_w), np.abs(in_b)) + np.repeat(np.abs(g2).astype(np.float64), lens, axis=1)
    dv = (k * H + 3) * u * s1
    da = dv[:H] + 0.25 * dv[H:] + e_gate
    a64 = np.concatenate([d["y"] for d in R.epi_ref64(_split(x, lens), in_w, in_b, epi=GATE, H=H, ubias=g2)], axis=1)
    s2 = np.abs(rs_w[:, 0, :]).astype(np.float64) @ np.abs(a64) + np.abs(rs_b)[:, None]
    drs = np.abs(rs_w[:, 0, :]).astype(np.float64) @ da + (H + 2) * u * s2
    return drs + 2 * u * (np.abs(old) + s2)


def _split(t, lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    return [t[:, off[i]:off[i + 1]] for i in range(len(lens))]


@pytest.mark.parametrize("last", [0, 1])
def test_gate_then_res_skip_agrees_with_the_oracles_wavenet_layer(port_built, last):
    """GATE (with ubias = the layer's conditioning) followed by RESSKIP of the reference is the oracle's wn_layer, within the oracle's own
    float32 summation bound; a pairing or routing difference would be of order 1."""
    H, k, lens = 16, 5, [9, 1, 30, 4]
    rng = np.random.default_rng(5 + last)
    n = sum(lens)
    x, out0 = rng.standard_normal((H, n)).astype(np.float32), rng.standard_normal((H, n)).astype(np.float32)
    in_w = (rng.standard_normal((2 * H, k, H)) / np.sqrt(k * H)).astype(np.float32)
    rs_w = (rng.standard_normal(((1 if last else 2) * H, 1, H)) / np.sqrt(H)).astype(np.float32)
    in_b, rs_b = rng.standard_normal(2 * H).astype(np.float32), rng.standard_normal(rs_w.shape[0]).astype(np.float32)
    g2 = rng.standard_normal((2 * H, len(lens))).astype(np.float32)
    gx, gout = pyref.port_wn_layer(x, out0, lens, in_w, in_b, 1, rs_w, rs_b, g2)
    gate = R.epi_ref64(_split(x, lens), in_w, in_b, epi=GATE, H=H, ubias=g2)
    acts = [d["y"] for d in gate]
    # (the second conv of the reference runs on float64 activations: packed_conv_ref64 takes any float input)
    rs = R.epi_ref64(acts, rs_w, rs_b, epi=RESSKIP, H=H, y_init=_split(x, lens), aux_init=_split(out0, lens))
    e_gate = 4.0 * R.activation_error(np.concatenate([d["v"][:H].ravel() for d in gate]), np.concatenate([d["v"][H:].ravel() for d in gate]))[1]
    if last:
        want_x, want_out = x.astype(np.float64), np.concatenate([d["aux"] for d in rs], axis=1)
        lim_out = _oracle_bound(x, lens, in_w, in_b, g2, rs_w, rs_b, out0, e_gate)
        assert np.array_equal(gx, x)
    else:
        want_x, want_out = np.concatenate([d["y"] for d in rs], axis=1), np.concatenate([d["aux"] for d in rs], axis=1)
        lim = _oracle_bound(x, lens, in_w, in_b, g2, rs_w, rs_b, np.concatenate([x, out0]), e_gate)
        lim_x, lim_out = lim[:H], lim[H:]
        assert (np.abs(gx - want_x) <= lim_x).all(), float((np.abs(gx - want_x) / lim_x).max())
    assert (np.abs(gout - want_out) <= lim_out).all(), float((np.abs(gout - want_out) / lim_out).max())
    assert lim_out.max() < 1e-3          # (the worst-case bound still sits three orders below a pairing or routing error)
    print(f"WN_LAYER oracle last={last}: max err / bound = {float((np.abs(gout - want_out) / lim_out).max()):.3f}")


def test_activation_error_E_t():
    """E_t: max |float32 restatement - float64| of tanh_ref and of the gate tanh_ref x sigmoid_ref on a dense grid over [-100, 100] and
    at the GPU file's own pre-activations.  The GPU bounds use 4 x this.  It has to be a few float32 ulps of 1."""
    e_t, e_g = R.grid_activation_error()
    case = R.make_case(32, 64, 5, LENGTHS, 7 * 32, 0, 32)
    ref = R.epi_ref64(R.pick(case, "x", ORDERS["listed"]), case["w"], case["b"], epi=GATE, H=32)
    d_t, d_g = R.activation_error(np.concatenate([d["v"][:32].ravel() for d in ref]), np.concatenate([d["v"][32:].ravel() for d in ref]))
    print(f"E_T tanh_ref: grid {e_t:.3e}, with the gate case's pre-activations {d_t:.3e}; gate tanh_ref x sigmoid_ref: grid {e_g:.3e}, with them {d_g:.3e}")
    assert 0 < e_t <= d_t < 8 * 2.0 ** -24 and 0 < e_g <= d_g < 8 * 2.0 ** -24
    # the clamps: e^x overflows float32 from 88.8 on, where the formula must still give +-1
    assert R.tanh32(np.array([-100, -89, 89, 100], np.float32)).tolist() == [-1, -1, 1, 1]
    assert R.sigmoid32(np.array([-100, 100], np.float32)).tolist() == [0, 1]


def test_gpu_cases_discriminate():
    """On the reference alone: the quiet gate segments sit where tanh and sigmoid are steep, the tail's wave is neither silent nor saturated,
    and a conv across segment boundaries differs from the segmented one by far more than any bound."""
    for H in (32, 48):
        case = R.make_case(H, 2 * H, 5, LENGTHS, 7 * H, 0, H)
        order = ORDERS["listed"]
        ref = R.epi_ref64(R.pick(case, "x", order), case["w"], case["b"], epi=GATE, H=H)
        vt = np.concatenate([d["v"][:H].ravel() for d, (_, loud) in zip(ref, order) if not loud])
        vs = np.concatenate([d["v"][H:].ravel() for d, (_, loud) in zip(ref, order) if not loud])
        assert np.mean((np.abs(vt) < 2) & (np.abs(vs) < 4)) >= 0.5, (H, float(np.mean((np.abs(vt) < 2) & (np.abs(vs) < 4))))
    from test_conv_epi_gpu import TAIL_LONG, TAIL_SHORT
    for lengths in (TAIL_LONG, TAIL_SHORT):
        for nsum in (0, 3):
            case = R.make_case(32, 1, 7, lengths, 3217 + nsum + len(lengths))
            order = [(i, i % 2 == 1) for i in range(len(lengths))]
            ref = R.epi_ref64(R.pick(case, "x", order), case["w"], case["b"], in_slope=0.01, epi=TANH_PCM, nsum=nsum, xs1=R.pick(case, "xs1", order),
                              xs2=R.pick(case, "xs2", order))
            wave = np.abs(np.concatenate([d["aux"].ravel() for d in ref]))
            assert np.mean(wave > 0.5) >= 0.1 and np.mean(wave > 0.999) < 0.5, (lengths, nsum, float(np.mean(wave > 0.5)), float(np.mean(wave > 0.999)))
    case = R.make_case(64, 64, 3, LENGTHS, 131)
    order = ORDERS["listed"]
    xs = R.pick(case, "x", order)
    seg = np.concatenate([d["y"] for d in R.epi_ref64(xs, case["w"], case["b"])], axis=1)
    whole = R.epi_ref64([np.concatenate(xs, axis=1)], case["w"], case["b"])[0]["y"]
    edges = np.cumsum([LENGTHS[i] for i, _ in order])[:-1]
    for e in edges:
        assert np.abs(seg[:, e - 1:e + 1] - whole[:, e - 1:e + 1]).max() > 1e-2, int(e)


def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    assert re.search(r"int sts_debug_conv1d_epi\(", hdr) and "typedef struct sts_conv_epi_opts {" in hdr
    assert int(re.search(r"#define STS_ABI_VERSION (\d+)", hdr).group(1)) == 18
    lib = engine.load_library()
    assert hasattr(lib, "sts_debug_conv1d_epi") and "sts_debug_conv1d_epi" in engine.EXPORTED_SYMBOLS and lib.sts_abi_version() == 18
    fields = re.search(r"typedef struct sts_conv_epi_opts \{(.*?)\} sts_conv_epi_opts;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in engine.ConvEpiOpts._fields_] and names[0] == "size_bytes"
    assert (R.STORE, R.RESADD, R.SUB, R.GATE, R.RESSKIP, R.TANH_PCM) == (engine.EPI_STORE, engine.EPI_RESADD, engine.EPI_SUB, engine.EPI_GATE,
                                                                           engine.EPI_RESSKIP, engine.EPI_TANH_PCM)


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _epi(co=4, ci=4, k=3, n=(6, 3), gap=0, stride=0, mode=1, **kw):
    L = sum(n) + len(n) * gap
    lout = L * max(stride, 1) + (len(n) if kw.get("in_reflect") else 0)
    full = {"res": (co, lout), "y_init": (kw.get("H") or co, lout), "aux_init": (kw.get("H") or 1, lout), "xs1": (ci, L), "xs2": (ci, L),
            "ubias": (co, len(n))}
    for name in list(kw):
        if kw[name] is True and name in full:
            kw[name] = np.zeros(full[name], np.float32)
    return engine.debug_conv1d_epi(np.zeros((ci, L), np.float32), list(n), np.zeros((co, k, ci), np.float32), None, 1, stride, 0.0, 0, mode, gap, **kw)


BAD = {
    "unknown epi": dict(epi=2),
    "another unknown epi": dict(epi=7),
    "GATE without H": dict(epi=GATE),
    "GATE with Cout != 2 H": dict(epi=GATE, H=3),
    "gate_perm with H % 16 != 0": dict(co=16, epi=GATE, H=8, gate_perm=1),
    "gate_perm without GATE": dict(gate_perm=1),
    "RESSKIP with Cout not H or 2 H": dict(epi=RESSKIP, H=3, y_init=True, aux_init=True),
    "RESSKIP without H": dict(epi=RESSKIP, y_init=True, aux_init=True),
    "RESSKIP without aux_init": dict(epi=RESSKIP, H=2, y_init=True),
    "RESSKIP without y_init": dict(epi=RESSKIP, H=2, aux_init=True),
    "RESSKIP without aux_out": dict(epi=RESSKIP, H=2, y_init=True, aux_init=True, want_aux=False),
    "TANH_PCM with Cout != 1": dict(epi=TANH_PCM),
    "TANH_PCM without pcm_out": dict(co=1, epi=TANH_PCM, want_pcm=False),
    "RESADD without res": dict(epi=RESADD),
    "SUB without y_init": dict(epi=SUB),
    "nsum 1": dict(nsum=1),
    "nsum 4": dict(nsum=4, xs1=True, xs2=True),
    "nsum 2 without xs1": dict(nsum=2),
    "nsum 3 without xs2": dict(nsum=3, xs1=True),
    "kslices 0": dict(kslices=0),
    "kslices 3": dict(kslices=3),
    "kslices 16": dict(kslices=16),
    "kslices with RESADD": dict(kslices=2, epi=RESADD, res=True, mode=8, ci=32, co=32),
    "in_reflect on a transposed conv": dict(in_reflect=1, stride=2, k=4),
    "size_bytes too small": dict(size_bytes=8),
    "a negative gap": dict(gap=-1),
    "lengths that do not add up with the gap": dict(n=(6, 4), gap=0, xs1=np.zeros((4, 9), np.float32)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks_answer_einval(what):
    kw = dict(BAD[what])
    if what.startswith("lengths"):
        with pytest.raises(engine.StsError, match=R.EINVAL):
            engine.debug_conv1d_epi(np.zeros((4, 9), np.float32), [6, 4], np.zeros((4, 3, 4), np.float32), None)
        return
    with pytest.raises(engine.StsError, match=R.EINVAL):
        _epi(**kw)


@pytest.mark.skipif(_gpu_visible(), reason="this check is about machines without a GPU")
def test_argument_checks_need_no_device():
    """The complement of the table above on a machine without a GPU: a well-formed call of every form passes every check and only then fails
    for want of a device, and what a kernel family does not take is refused before that."""
    good = [dict(), dict(gap=5), dict(epi=RESADD, res=True), dict(epi=SUB, y_init=True), dict(epi=GATE, H=2), dict(co=32, epi=GATE, H=16, gate_perm=1),
            dict(epi=RESSKIP, H=2, y_init=True, aux_init=True), dict(epi=RESSKIP, H=4, aux_init=True), dict(epi=RESSKIP, H=4, epi_flag=1),
            dict(co=1, epi=TANH_PCM), dict(in_reflect=1), dict(ubias=True), dict(kslices=4, mode=9, ci=32, co=32),
            dict(nsum=3, xs1=True, xs2=True, stride=4, k=8, ci=32, co=32, mode=42), dict(nsum=2, xs1=True, stride=4, k=8, ci=32, co=32, mode=183)]
    for kw in good:
        with pytest.raises(engine.StsError, match=R.EDEVICE):
            _epi(**kw)
    import test_conv_epi_gpu as G
    for feature in sorted(R.TAKES):
        for (fam, mode), takes in zip(R.FAMILIES.items(), R.TAKES[feature]):
            with pytest.raises(engine.StsError, match=R.EDEVICE if takes else R.EINVAL):
                G._table_call(feature, mode)
    with pytest.raises(engine.StsError, match=R.EINVAL):            # the folded mean: short segments go to the generic kernel, which has none
        _epi(co=1, ci=32, k=7, n=(300, 255, 1), epi=TANH_PCM, nsum=3, xs1=True, xs2=True)
    with pytest.raises(engine.StsError, match=R.EDEVICE):
        _epi(co=1, ci=32, k=7, n=(4096, 1), epi=TANH_PCM, nsum=3, xs1=True, xs2=True)
    with pytest.raises(engine.StsError, match=R.EINVAL):            # row-interleaved phases: the plain epilogue only
        _epi(stride=4, k=8, ci=32, co=32, mode=142, ubias=True)
