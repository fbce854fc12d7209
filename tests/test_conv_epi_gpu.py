"""GPU suite (MI355X): what the conv kernels do on their way out, at the kernel.  sts_debug_conv1d_epi gives every kernel family the
epilogues (RESADD, SUB, GATE, RESSKIP, TANH_PCM, K slices) and operand forms (ubias, the reflect view, the folded mean) the engine gives
them, on the packed segments of test_packed_conv_gpu.py (boundaries on the tile widths, every second segment 64 x louder), once packed
back to back and once with 5 unused columns behind every segment, so that row starts lose their 16-byte alignment.  The unused columns
hold NaNs in every input and a sentinel in every output.  Everywhere: (a) no unused output column changed by a bit, (b) every output
inside a segment is finite and within its bound of float64 (tests/conv_epi_ref.py); for a pinned kernel also (c) every segment is
bit-identical to itself run alone and (d) the two-term kernels' overflow word is 0."""
import numpy as np
import pytest

import conv_epi_ref as R
from conv_epi_ref import GATE, RESADD, RESSKIP, STORE, SUB, TANH_PCM
from summertts_amd import engine
from test_packed_conv_gpu import AUTO, H2_MODES, LENGTHS, LOUD, ORDERS, _bf3_modes, _family

pytestmark = pytest.mark.gpu

GAPS = (0, 5)
MFMA = [2, 3, 4, 5, 6, 7]
SPLITK = [8, 9]
_WORST = {}


def _split_operand():
    return [13] + [m for m in _bf3_modes() if m != 13] + list(H2_MODES)


def _dense(wino=True):
    return [1, 0] + MFMA + SPLITK + ([12] if wino else []) + _split_operand()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _call(case, order, gap, mode, *, dil=1, stride=0, in_slope=None, epi=STORE, epi_flag=0, H=0, gate_perm=0, in_reflect=0, nsum=0, kslices=1,
          ubias=None, w=None, b="case", x=None, aux_init=None):
    """One launch on the segments of `order`; ubias: [co, len(order)] or None; x: a replacement of the per-segment inputs."""
    scale = max(stride, 1)
    co = case["w"].shape[0]
    rows = H if epi in (GATE, RESSKIP) else co
    inp = lambda name: R.pack(R.pick(case, name, order), gap, np.nan)
    outp = lambda name, r, fill: R.pack(R.pick(case, name, order, r), gap, fill, scale, in_reflect)
    kw = {}
    if nsum >= 2:
        kw["xs1"] = inp("xs1")
        if nsum == 3:
            kw["xs2"] = inp("xs2")
    if epi == RESADD:
        kw["res"] = outp("res", co, np.nan)
    if epi in (SUB, RESSKIP):           # (RESSKIP with Cout = H leaves y alone: it must come back as it went in)
        kw["y_init"] = outp("y_init", rows, R.SENTINEL)
    if epi == RESSKIP and not (epi_flag & 1):
        kw["aux_init"] = outp("aux_init", H, R.SENTINEL) if aux_init is None else R.pack(aux_init, gap, R.SENTINEL, scale, in_reflect)
    xin = inp("x") if x is None else R.pack(x, gap, np.nan)
    out = engine.debug_conv1d_epi(xin, [case["lengths"][i] for i, _ in order], case["w"] if w is None else w, case["b"] if isinstance(b, str) else b,
                                   dil, stride, 0.0 if in_slope is None else in_slope, 0 if in_slope is None else 1, mode, gap, epi=epi,
                                   epi_flag=epi_flag, H=H, gate_perm=gate_perm, in_reflect=in_reflect, nsum=nsum, kslices=kslices, ubias=ubias, **kw)
    # what the unused columns must still hold: the finite sentinel in a tensor that was given initial values, the NaN one elsewhere
    out["gap_bits"] = {"y": R.RMW_BITS if "y_init" in kw else R.PLAIN_BITS, "aux": R.RMW_BITS if "aux_init" in kw else R.PLAIN_BITS, "pcm": 0x7FFF}
    out["y_init"] = kw.get("y_init")
    return out


def _reference(case, order, *, dil=1, stride=0, in_slope=None, epi=STORE, epi_flag=0, H=0, in_reflect=0, nsum=0, ubias=None, w=None, b="case"):
    co = case["w"].shape[0]
    rows = H if epi in (GATE, RESSKIP) else co
    return R.epi_ref64(R.pick(case, "x", order), case["w"] if w is None else w, case["b"] if isinstance(b, str) else b, dil, stride, in_slope, epi, epi_flag,
                       H, in_reflect, nsum, R.pick(case, "xs1", order), R.pick(case, "xs2", order), ubias, R.pick(case, "res", order, co),
                       R.pick(case, "y_init", order, rows), R.pick(case, "aux_init", order, H if H else 1))


def _e_act(epi, ref):
    if epi == GATE:
        H = ref[0]["y"].shape[0]
        return 4.0 * R.activation_error(np.concatenate([d["v"][:H].ravel() for d in ref]), np.concatenate([d["v"][H:].ravel() for d in ref]))[1]
    if epi == TANH_PCM:
        return 4.0 * R.activation_error(np.concatenate([d["v"].ravel() for d in ref]))[0]
    return 0.0


def _assert_outputs(out, ref, order, lens, gap, where, *, epi, stride=0, in_reflect=0, e_act=0.0, tag=None):
    """(a), (b) and (d) on one launch's outputs.  Returns the tensors checked, for (c)."""
    scale = max(stride, 1)
    sp = R.spans(lens, gap, scale, in_reflect)
    mask = R.gap_mask(lens, gap, scale, in_reflect)
    tensors = {"y": out["y"]} if epi != TANH_PCM and not (epi == RESSKIP and ref[0]["y"] is None) else {}
    if epi in (RESSKIP, TANH_PCM):
        tensors["aux"] = out["aux"]
    assert out["ovf"] == 0, (where, "the two-term kernel's overflow word is up")                                         # d
    for name, t in list(tensors.items()) + ([("pcm", out["pcm"][None, :])] if epi == TANH_PCM else []):
        want = out["gap_bits"][name]
        assert t.shape[-1] == mask.size, (where, name, t.shape)
        assert (_bits(t)[..., mask] == want).all(), (where, name, "an unused column was written", int((_bits(t)[..., mask] != want).sum()))     # a
    if epi == RESSKIP and ref[0]["y"] is None:          # Cout = H: y keeps y_init bit for bit, and its unused columns their sentinel
        assert (_bits(out["y"])[:, mask] == R.RMW_BITS).all(), (where, "y", "an unused column was written")
        assert np.array_equal(_bits(out["y"])[:, ~mask], _bits(out["y_init"])[:, ~mask]), (where, "y was written though every row goes to aux")
    for name, t in tensors.items():
        for (lo, hi), (i, loud), d in zip(sp, order, ref):                                                               # b
            got = t[:, lo:hi]
            g = LOUD if loud else 1.0
            assert np.isfinite(got).all(), (where, name, "segment", i, "unwritten or non-finite positions", int((~np.isfinite(got)).sum()))
            err = np.abs(got - d[name])
            lim = R.bound(epi, g, d["mag_" + name], e_act)
            if tag:
                _WORST[tag] = max(_WORST.get(tag, 0.0), float(err.max()) / g)
            assert (err <= lim).all(), (where, name, "segment", i, "loud" if loud else "quiet", float(err.max()), float(np.min(lim)))
    return tensors


def _assert_alone(tensors, sp, order, alone, where, key, run):
    """(c) for a pinned kernel: every segment of `tensors` (name -> [.., columns]) is bit-identical to the same segment run alone through the
    same entry.  key(i, loud, b): what the lone run depends on (None: not compared); run(i, loud, b): the lone launch, made once per key."""
    for b, ((lo, hi), (i, loud)) in enumerate(zip(sp, order)):
        k = key(i, loud, b)
        if k is None:
            continue
        if k not in alone:
            alone[k] = run(i, loud, b)
        for name, t in tensors.items():
            assert np.array_equal(_bits(t[..., lo:hi]), _bits(alone[k][name])), (where, name, "segment", i, "differs from itself run alone")


def _check(ci, co, k, dil, stride, modes, seed, *, epi=STORE, epi_flag=0, H=0, gate_perm=0, in_reflect=0, in_slope=None, ubias=None, name=""):
    """Both orderings x both gaps x every mode: (a) (b) (d), and (c) for the pinned modes."""
    case = R.make_case(ci, co, k, LENGTHS, seed, stride, H, in_reflect)
    scale = max(stride, 1)
    fwd = dict(dil=dil, stride=stride, in_slope=in_slope, epi=epi, epi_flag=epi_flag, H=H, in_reflect=in_reflect)
    alone = {}
    for oname, order in ORDERS.items():
        ub = None if ubias is None else case["ubias_" + ubias]
        ref = _reference(case, order, ubias=ub, **fwd)
        e_act = _e_act(epi, ref)
        lens = [LENGTHS[i] for i, _ in order]
        for gap in GAPS:
            sp = R.spans(lens, gap, scale, in_reflect)
            for mode in modes:
                where = (name, ci, co, k, dil, stride, oname, "gap", gap, "mode", mode)
                out = _call(case, order, gap, mode, gate_perm=gate_perm, ubias=ub, **fwd)
                tensors = _assert_outputs(out, ref, order, lens, gap, where, epi=epi, stride=stride, in_reflect=in_reflect, e_act=e_act,
                                          tag=(name, _family(mode)))
                if mode in AUTO:
                    continue
                # (with ubias a segment's lone run depends on its place b: the second ordering repeats it for four lengths only)
                skip = lambda i: ub is not None and oname != "listed" and LENGTHS[i] not in (1, 33, 129, 256)
                _assert_alone(tensors, sp, order, alone, where,                                                           # c
                              lambda i, loud, b: None if skip(i) else (mode, i, loud, b if ub is not None else -1),
                              lambda i, loud, b: _call(case, [(i, loud)], 0, mode, gate_perm=gate_perm, ubias=None if ub is None else ub[:, b:b + 1], **fwd))
    for (nm, fam), e in sorted(_WORST.items()):
        if nm == name:
            print(f"EPI_ERR {nm} / {fam}: ci={ci} co={co} k={k} dil={dil} stride={stride} max|out - ref64| = {e:.3e} (loud segments / 64)")


@pytest.mark.parametrize("ci,co,k,dil", [(64, 64, 3, 1), (64, 40, 7, 3)], ids=str)
def test_residual_epilogue(ci, co, k, dil):
    """y = v + res in every family that has it, through the epilogue's own 16-byte residual loads.  (tile_res_prefetch, the residual requested
    ahead of the K loop, is a lab switch of the grouped launches -- STS_GROUP_RPF, off by default -- and is not reached from here.)"""
    _check(ci, co, k, dil, 0, _dense(), ci + co + k, epi=RESADD, name="RESADD")


@pytest.mark.parametrize("ubias", [None, "random"], ids=str)
@pytest.mark.parametrize("H", [32, 48])
def test_gate_with_the_loaders_row_packing(H, ubias):
    """tanh(v[c]) sigmoid(v[c + H]) on rows packed as (tanh16, sigmoid16) per 32-row tile: H = 32 is two row tiles, H = 48 three (the
    `ch < H` test); ubias goes through the same row permutation."""
    _check(H, 2 * H, 5, 1, 0, [1, 0] + MFMA + SPLITK + _split_operand(), 7 * H, epi=GATE, H=H, gate_perm=1, ubias=ubias, name="GATE")


@pytest.mark.parametrize("H", [32, 48])
def test_gate_pairing_by_zeroed_halves(H):
    """A pairing error shows directly: with the sigmoid half's weights and bias zero the gate is 0.5 tanh(v_t), within the bound; with the
    tanh half's zero it is exactly 0."""
    case = R.make_case(H, 2 * H, 5, LENGTHS, 11 * H, 0, H)
    order = ORDERS["listed"]
    lens = [LENGTHS[i] for i, _ in order]
    for half in ("sigmoid", "tanh"):
        w, b = case["w"].copy(), case["b"].copy()
        rows = slice(H, 2 * H) if half == "sigmoid" else slice(0, H)
        w[rows] = 0
        b[rows] = 0
        ref = _reference(case, order, epi=GATE, H=H, w=w, b=b)
        e_act = _e_act(GATE, ref)
        alone = {}
        for mode in [1] + MFMA + SPLITK + [20, 60]:
            for gap in GAPS:
                out = _call(case, order, gap, mode, epi=GATE, H=H, gate_perm=1, w=w, b=b)
                where = ("zero", half, H, mode, gap)
                tensors = _assert_outputs(out, ref, order, lens, gap, where, epi=GATE, e_act=e_act)
                _assert_alone(tensors, R.spans(lens, gap), order, alone, where, lambda i, loud, _: (mode, i, loud),
                              lambda i, loud, _: _call(case, [(i, loud)], 0, mode, epi=GATE, H=H, gate_perm=1, w=w, b=b))
                for (lo, hi), d in zip(R.spans(lens, gap), ref):
                    if half == "tanh":
                        assert not out["y"][:, lo:hi].any(), (where, "a zero tanh half must give exactly 0")
                    else:
                        assert np.allclose(d["y"], 0.5 * np.tanh(d["v"][:H]), rtol=0, atol=1e-15)


def test_gate_with_plain_rows():
    """Rows (c, c + H) without the tile permutation: the generic kernel's other gate form."""
    _check(8, 16, 5, 1, 0, [1], 808, epi=GATE, H=8, name="GATE plain rows")


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("H,co", [(32, 64), (48, 96), (32, 32), (48, 48)], ids=str)
def test_res_skip_routing(H, co, flag):
    """Cout = 2 H: rows < H add to y, rows >= H to aux (store, do not add, with epi_flag & 1); Cout = H: every row goes to aux."""
    _check(H, co, 1, 1, 0, _dense(wino=False), H + co + flag, epi=RESSKIP, epi_flag=flag, H=H, ubias="random" if (H, co, flag) == (48, 96, 0) else None,
           name="RESSKIP")


@pytest.mark.parametrize("H,co", [(32, 64), (48, 48)], ids=str)
def test_res_skip_leaves_alone_what_it_must(H, co):
    """epi_flag = 1: the result does not depend on aux_init (two runs with different aux_init, the second declared unused, bit-equal);
    Cout = H: y keeps y_init bit for bit."""
    case = R.make_case(H, co, 1, LENGTHS, 3 * H + co, 0, H)
    order = ORDERS["listed"]
    lens = [LENGTHS[i] for i, _ in order]
    for mode in [1, 5, 8, 20, 23, 60]:
        for gap in GAPS:
            a = _call(case, order, gap, mode, epi=RESSKIP, epi_flag=1, H=H)
            other = [np.full_like(t, 1e30) for t in R.pick(case, "aux_init", order, H)]
            o = dict(epi=RESSKIP, epi_flag=1, H=H)
            xin = R.pack(R.pick(case, "x", order), gap, np.nan)
            yin = R.pack(R.pick(case, "y_init", order, H), gap, R.RMW_SENTINEL)
            b = engine.debug_conv1d_epi(xin, lens, case["w"], case["b"], 1, 0, 0.0, 0, mode, gap, y_init=yin, aux_init=R.pack(other, gap, R.SENTINEL), **o)
            mask = R.gap_mask(lens, gap)          # (b's aux was given initial values, a's was not: their unused columns hold different sentinels)
            assert np.array_equal(_bits(a["aux"])[:, ~mask], _bits(b["aux"])[:, ~mask]), (H, co, mode, gap, "aux depends on aux_init")
            assert (_bits(b["aux"])[:, mask] == R.RMW_BITS).all() and (_bits(a["aux"])[:, mask] == R.PLAIN_BITS).all(), (H, co, mode, gap)
            assert np.array_equal(_bits(a["y"]), _bits(b["y"])), (H, co, mode, gap)
            if co == H:
                assert np.array_equal(_bits(b["y"]), _bits(yin)), (H, co, mode, gap, "y was written")


@pytest.mark.parametrize("ci,co,k", [(32, 40, 1), (64, 32, 3)], ids=str)
def test_subtracting_epilogue(ci, co, k):
    """y = y_init - v (the coupling's x1 -= m)."""
    _check(ci, co, k, 1, 0, _dense(wino=k > 1), ci + co + k + 1, epi=SUB, name="SUB")


def test_per_utterance_bias_same_padded():
    """ubias of segment b, row r = 100 b + r / 8: a wrong segment or row is an error of order 100."""
    _check(64, 40, 3, 1, 0, _dense(), 6440, ubias="ramp", name="STORE + ubias")


def test_per_utterance_bias_transposed():
    _check(64, 32, 8, 1, 4, _dense(wino=False), 6432, ubias="ramp", name="STORE + ubias, transposed")


def test_reflect_view_of_the_subband_conv():
    """Output segments one longer than their inputs at offset off + b; position 0 reads x[1], and 0 in a 1-long segment."""
    _check(32, 72, 7, 1, 0, [1, 0] + MFMA + SPLITK + _split_operand(), 3272, in_reflect=1, in_slope=0.01, name="in_reflect")


@pytest.mark.parametrize("ks", [2, 4, 8])
def test_k_slices_of_the_split_k_kernel(ks):
    """Partial planes whose sum is the conv; with all-zero weights plane 0 is bias + ubias exactly and every other plane exactly 0."""
    case = R.make_case(96, 64, 3, LENGTHS, 9664 + ks)
    alone = {}
    for oname, order in ORDERS.items():
        lens = [LENGTHS[i] for i, _ in order]
        ub = case["ubias_random"]
        ref = _reference(case, order, ubias=ub)
        for mode in SPLITK:
            for gap in GAPS:
                where = ("kslices", ks, oname, mode, gap)
                out = _call(case, order, gap, mode, kslices=ks, ubias=ub)
                assert out["y"].shape[0] == ks
                mask = R.gap_mask(lens, gap)
                assert (_bits(out["y"])[..., mask] == 0xFFFFFFFF).all(), (where, "an unused column was written")
                total = out["y"][:, :, ~mask].astype(np.float64).sum(axis=0)
                assert np.isfinite(total).all(), where
                summed = {"y": R.pack([total[:, lo:hi] for lo, hi in R.spans(lens)], gap, np.nan), "ovf": out["ovf"]}
                _assert_outputs_no_gaps(summed, ref, order, lens, gap, where)
                # (c) per plane: a pinned split-K launch takes its wave split from the conv's K alone, so every partial sum is the segment's own
                _assert_alone({"y": out["y"]}, R.spans(lens, gap), order, alone, where, lambda i, loud, b: (mode, i, loud, b),
                              lambda i, loud, b: _call(case, [(i, loud)], 0, mode, kslices=ks, ubias=ub[:, b:b + 1]))
                zero =_call(case, order, gap, mode, kslices=ks, ubias=ub, w=np.zeros_like(case["w"]))
                for (lo, hi), b in zip(R.spans(lens, gap), range(len(lens))):
                    want = np.broadcast_to((case["b"] + ub[:, b])[:, None], (64, hi - lo))
                    assert np.array_equal(zero["y"][0][:, lo:hi], want), (where, "plane 0 of zero weights is not bias + ubias")
                    assert not zero["y"][1:, :, lo:hi].any(), (where, "a later plane of zero weights is not 0")
    print(f"EPI_ERR kslices={ks} / {_family(8)}: ci=96 co=64 k=3 max|sum of planes - ref64| = {_WORST[('kslices', ks)]:.3e} (loud segments / 64)")


def _assert_outputs_no_gaps(out, ref, order, lens, gap, where):
    for (lo, hi), (i, loud), d in zip(R.spans(lens, gap), order, ref):
        g = LOUD if loud else 1.0
        err = np.abs(out["y"][:, lo:hi] - d["y"])
        _WORST[where[:2]] = max(_WORST.get(where[:2], 0.0), float(err.max()) / g)
        assert (err <= R.bound(STORE, g, d["mag_y"])).all(), (where, "segment", i, float(err.max()))


@pytest.mark.parametrize("nsum", [2, 3])
@pytest.mark.parametrize("ci,co,stride", [(64, 32, 4), (128, 32, 8)], ids=str)
def test_folded_mean_of_the_upsamplers(ci, co, stride, nsum):
    """((x + xs1) + xs2) / nsum formed while the phase-merged tiles stage their input: within the bound of float64, and bit-identical to the
    same launch on the mean the host materialised in float32."""
    case = R.make_case(ci, co, 2 * stride, LENGTHS, ci + stride + nsum, stride)
    alone = {}
    for oname, order in ORDERS.items():
        lens = [LENGTHS[i] for i, _ in order]
        ref = _reference(case, order, stride=stride, nsum=nsum)
        mean = [R.mean32(a, b, c, nsum) for a, b, c in zip(R.pick(case, "x", order), R.pick(case, "xs1", order), R.pick(case, "xs2", order))]
        for mode in (42, 43, 82, 83, 142, 143, 182, 183):
            for gap in GAPS:
                where = ("nsum", nsum, ci, co, stride, oname, mode, gap)
                out = _call(case, order, gap, mode, stride=stride, nsum=nsum)
                tensors = _assert_outputs(out, ref, order, lens, gap, where, epi=STORE, stride=stride, tag=("nsum", _family(mode)))
                _assert_alone(tensors, R.spans(lens, gap, stride), order, alone, where, lambda i, loud, _: (mode, i, loud),
                              lambda i, loud, _: _call(case, [(i, loud)], 0, mode, stride=stride, nsum=nsum))
                host = _call(case, order, gap, mode, stride=stride, x=mean)
                assert np.array_equal(_bits(out["y"]), _bits(host["y"])), (where, "the folded mean differs from the materialised one")
    for (nm, fam), e in sorted(_WORST.items()):
        if nm == "nsum":
            print(f"EPI_ERR nsum / {fam}: ci={ci} co={co} stride={stride} nsum={nsum} max|out - ref64| = {e:.3e} (loud segments / 64)")


TAIL_LONG = [4133, 1, 255, 256, 257, 300, 4096]       # max_n >= 4096: conv_cout1_kernel; vector-staged tiles, the straddling last tile, sub-tile segments, odd starts
TAIL_SHORT = [300, 255, 1]                            # the generic kernel's TANH_PCM


@pytest.mark.parametrize("lengths,nsum", [(TAIL_LONG, 0), (TAIL_LONG, 3), (TAIL_SHORT, 0)], ids=str)
def test_tanh_pcm_tail(lengths, nsum):
    """HiFi-GAN's output conv (32 -> 1, k 7, leaky-relu 0.01 in): the wave within its bound, the PCM exactly pcm_cast of the float32 wave the
    kernel returned, the folded mean bit-identical to the materialised one."""
    case = R.make_case(32, 1, 7, lengths, 3217 + nsum + len(lengths))
    order = [(i, i % 2 == 1) for i in range(len(lengths))]
    ref = _reference(case, order, in_slope=0.01, epi=TANH_PCM, nsum=nsum)
    e_act = _e_act(TANH_PCM, ref)
    mean = [R.mean32(a, b, c, nsum) for a, b, c in zip(R.pick(case, "x", order), R.pick(case, "xs1", order), R.pick(case, "xs2", order))]
    alone = {}
    for gap in GAPS:
        where = ("TANH_PCM", len(lengths), nsum, gap)
        out = _call(case, order, gap, 1, in_slope=0.01, epi=TANH_PCM, nsum=nsum)
        _assert_outputs(out, ref, order, lengths, gap, where, epi=TANH_PCM, e_act=e_act, tag=("TANH_PCM", _family(1)))
        mask = R.gap_mask(lengths, gap)
        assert np.array_equal(out["pcm"][~mask], R.pcm_cast(out["aux"][0, ~mask])), (where, "pcm is not pcm_cast(wave)")
        if nsum:
            host = _call(case, order, gap, 1, in_slope=0.01, epi=TANH_PCM, x=mean)
            assert np.array_equal(_bits(out["aux"]), _bits(host["aux"])) and np.array_equal(out["pcm"], host["pcm"]), (where, "folded mean")
        # (c): where the lone run takes the kernel the batch took -- every segment of the short batch (the generic kernel both times), the
        # segments >= 4096 of the long one (alone, a shorter segment goes to the generic kernel, which folds no mean)
        same_kernel = lambda i: max(lengths) < 4096 or lengths[i] >= 4096
        _assert_alone({"aux": out["aux"], "pcm": out["pcm"]}, R.spans(lengths, gap), order, alone, where,
                      lambda i, loud, _: (i, loud) if same_kernel(i) else None,
                      lambda i, loud, _: _call(case, [(i, loud)], 0, 1, in_slope=0.01, epi=TANH_PCM, nsum=nsum))
    if lengths is TAIL_SHORT:
        with pytest.raises(engine.StsError, match=R.EINVAL):
            _call(case, order, 0, 1, in_slope=0.01, epi=TANH_PCM, nsum=3)
    for (nm, fam), e in sorted(_WORST.items()):
        if nm == "TANH_PCM":
            print(f"EPI_ERR {nm} / {fam}: max|wave - ref64| = {e:.3e}; 4 x E_t = {e_act:.3e}")


def _table_call(feature, mode):
    H = 32
    if feature == "TANH_PCM":
        case, kw = R.make_case(32, 1, 3, [40, 9], 1), dict(epi=TANH_PCM)
    elif feature == "GATE plain":
        case, kw = R.make_case(32, 32, 3, [40, 9], 2, 0, 16), dict(epi=GATE, H=16)
    else:
        case = R.make_case(32, 64, 3, [40, 9], 3, 0, H)
        kw = {"RESADD": dict(epi=RESADD), "SUB": dict(epi=SUB), "RESSKIP": dict(epi=RESSKIP, H=H), "GATE permuted": dict(epi=GATE, H=H, gate_perm=1),
              "ubias": dict(ubias=case["ubias_ramp"]), "in_reflect": dict(in_reflect=1), "kslices": dict(kslices=2), "nsum": dict(nsum=2)}[feature]
        if feature == "in_reflect":
            case = R.make_case(32, 64, 3, [40, 9], 3, 0, H, 1)
    return _call(case, [(0, False), (1, True)], 0, mode, **kw)


@pytest.mark.parametrize("feature", sorted(R.TAKES))
def test_every_family_runs_what_it_takes_and_refuses_the_rest(feature):
    for (fam, mode), takes in zip(R.FAMILIES.items(), R.TAKES[feature]):
        if takes:
            _table_call(feature, mode)
        else:
            with pytest.raises(engine.StsError, match=R.EINVAL):
                _table_call(feature, mode)
