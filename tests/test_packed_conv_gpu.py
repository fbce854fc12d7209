"""GPU suite (MI355X): the conv kernels' plain epilogue (y = conv + bias; every other epilogue and operand form: tests/test_conv_epi_gpu.py)
on PACKED batches, at the kernel.  sts_debug_conv1d_packed / sts_debug_conv_h2p_packed hand every kernel
family a real B-entry segment table whose boundaries sit on the tile widths (32 / 64 / 128 columns), one position either side of them, and
around segments shorter than the conv's halo; the result is compared with a float64 convolution of every segment on its own
(tests/packed_conv_ref.py).  Every second segment is 64 x louder than its neighbours, so one halo tap read across a boundary lands orders of
magnitude above the bound of the quiet segment.  The output buffers start out as NaNs: a position no workgroup writes cannot pass."""
import numpy as np
import pytest

from packed_conv_ref import packed_conv_ref64, seg_bounds
from summertts_amd import engine

pytestmark = pytest.mark.gpu

BAR = 2e-5            # the project's conv bar against float64 (test_f16x2_conv_against_float64)
LOUD = 64.0
# boundaries on 128 / 64 / 32, one either side, segments of 1 / 2 / 3 / 5 (below the k = 11, dil = 5 halo of 25) between longer ones
LENGTHS = [129, 1, 128, 2, 127, 5, 64, 63, 65, 32, 31, 33, 256, 3]
# two orderings of the same segments (index into LENGTHS, loud?): as listed with every second one loud; the 1-long one first and the longest
# last (neighbours swapped pairwise, so quiet and loud still alternate)
ORDERS = {"listed": [(i, i % 2 == 1) for i in range(len(LENGTHS))],
          "short_first_longest_last": [(i ^ 1, (i ^ 1) % 2 == 1) for i in range(len(LENGTHS) - 2)] + [(13, True), (12, False)]}
KDIL = [(1, 1), (3, 1), (7, 3), (11, 5), (5, 2)]
H2_MODES = (50, 60, 63, 64, 80, 82, 83)          # as tests/test_parity_gpu.py
AUTO = (0, 13, 50, 113, 150)                     # automatic tile choice: the dispatcher may pick another tile for another grid


def _bf3_modes():      # as test_bf3_conv_is_as_accurate_as_the_fp32_matrix_core_kernel, plus the K-split tile (40)
    if engine.lab_build():
        return (13, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 40, 41, 42, 43)
    return (13, 20, 23, 24, 40, 42, 43)


def _family(mode, depthwise=False):
    m = mode % 100
    if depthwise:
        return "depthwise (generic)"
    rp = " row-interleaved" if mode >= 100 else ""
    if m == 0:
        return "automatic"
    if m == 1:
        return "generic VALU"
    if m in (8, 9):
        return "fp32 split-K"
    if m == 12:
        return "Winograd"
    if m < 12:
        return "fp32 matrix-core tiles"
    if m < 50:
        return "split-bf16" + rp
    return "two-term fp16" + rp


def _segments(ci, seed, depthwise=False):
    """Per segment of LENGTHS: (quiet input [ci, len], the same x 64).  The generator of the float64 conv tests, drawn once per case."""
    rng = np.random.default_rng(seed)
    gain = rng.uniform(0.05, 3.0, (ci, 1))
    segs = []
    for n in LENGTHS:
        q = (rng.standard_normal((ci, n)) * gain).astype(np.float32)
        segs.append((q, (q * np.float32(LOUD)).astype(np.float32)))
    return segs, rng


def _pack(segs, order):
    return np.concatenate([segs[i][1 if loud else 0] for i, loud in order], axis=1), [LENGTHS[i] for i, _ in order]


def _check_conv1d(ci, co, k, dil, stride, depthwise, modes, seed):
    scale = max(stride, 1)
    segs, rng = _segments(ci, seed, depthwise)
    w = (rng.standard_normal((co, k, 1 if depthwise else ci)) / np.sqrt(k * (1 if depthwise else ci) / scale)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32)
    pad = (k - stride) // 2 if stride else dil * (k - 1) // 2
    worst = {}
    alone = {}       # (mode, segment, loud) -> that segment through the same entry with B = 1
    for name, order in ORDERS.items():
        x, lens = _pack(segs, order)
        ref = packed_conv_ref64(x, lens, w, b, dil, stride, depthwise)
        bounds = seg_bounds(lens, scale)
        for mode in modes:
            y, ovf = engine.debug_conv1d_packed(x, lens, w, b, dil, stride, depthwise, mode=mode, return_ovf=True)
            where = (ci, co, k, dil, stride, name, mode)
            assert y.shape == ref.shape, where
            assert np.isfinite(y).all(), (where, "unwritten or non-finite positions", int((~np.isfinite(y)).sum()))      # 1
            assert ovf == 0, (where, "the two-term kernel's overflow word is up")
            err = np.abs(y - ref)
            for (lo, hi), (i, loud) in zip(bounds, order):                                                               # 2
                e = float(err[:, lo:hi].max())
                fam = _family(mode, depthwise)
                worst[fam] = max(worst.get(fam, 0.0), e / (LOUD if loud else 1.0))
                assert e <= BAR * (LOUD if loud else 1.0), (where, "segment", i, "loud" if loud else "quiet", e)
            if mode in AUTO:
                continue
            for (lo, hi), (i, loud) in zip(bounds, order):                                                               # 3
                key = (mode, i, loud)
                if key not in alone:
                    alone[key] = engine.debug_conv1d_packed(segs[i][1 if loud else 0], [LENGTHS[i]], w, b, dil, stride, depthwise, mode=mode)
                assert np.array_equal(y[:, lo:hi], alone[key]), (where, "segment", i, "differs from the same segment run alone",
                                                                 float(np.abs(y[:, lo:hi] - alone[key]).max()))
    for (mode, i, loud), y1 in alone.items():                                                                           # 4
        if LENGTHS[i] in (129, 1, 5, 64, 256) and not loud:
            old = engine.debug_conv1d(segs[i][0], w, b, pad, dil, stride, depthwise, mode=mode)
            assert np.array_equal(old, y1), (ci, co, k, dil, stride, mode, "table form differs from the single-segment entry, length", LENGTHS[i])
    for fam, e in sorted(worst.items()):
        print(f"PACKED_ERR {fam}: ci={ci} co={co} k={k} dil={dil} stride={stride} max|y - ref64| = {e:.3e} (loud segments / 64)")


@pytest.mark.parametrize("k,dil", KDIL, ids=lambda v: str(v))
@pytest.mark.parametrize("ci,co", [(32, 32), (64, 64), (128, 128), (64, 40)], ids=lambda v: str(v))
def test_packed_same_padded_convs_against_float64(ci, co, k, dil):
    """Every kernel family a "same"-padded conv is eligible for: generic VALU, the fp32 matrix-core tiles, split-K, Winograd, split-bf16 and
    two-term fp16 (automatic and pinned tiles).  1: no unwritten position; 2: within the conv bar of float64 per segment; 3: pinned tile ->
    every segment bit-identical to itself run alone; 4: table form == the single-segment entry."""
    modes = [1, 0, 2, 3, 4, 5, 6, 7, 8, 9] + ([12] if k >= 2 else []) + list(_bf3_modes()) + list(H2_MODES)
    _check_conv1d(ci, co, k, dil, 0, False, modes, seed=ci * 977 + co + k)


@pytest.mark.parametrize("ci,co,stride", [(64, 32, 2), (64, 32, 4), (128, 64, 8), (64, 40, 4)], ids=lambda v: str(v))
def test_packed_transposed_convs_against_float64(ci, co, stride):
    """The engine's upsamplers (k = 2 stride, pad = stride / 2; out_seg.scale = stride): phase-major packing, and the row-interleaved phases
    (+100) where Cout is a multiple of 32.  Same four assertions."""
    modes = [1, 0, 2, 3, 4, 5, 6, 7, 8, 9] + list(_bf3_modes()) + list(H2_MODES)
    if co % 32 == 0:
        modes += [113, 120, 123, 142, 143, 150, 160, 163, 182, 183]      # as test_upsampler_row_interleaved_phases_equal_the_phase_major_form
    _check_conv1d(ci, co, 2 * stride, 1, stride, False, modes, seed=ci * 31 + co + stride)


def test_packed_depthwise_conv_against_float64():
    """A depthwise conv (the duration predictor's DDSConv shape) goes to the generic kernel whatever the mode."""
    _check_conv1d(16, 16, 3, 9, 0, True, [1, 0], seed=16 * 131)


@pytest.mark.parametrize("C,k,dil", [(128, 1, 1), (128, 3, 1), (128, 7, 3), (128, 11, 5), (128, 5, 2), (256, 3, 1), (256, 11, 5)], ids=lambda v: str(v))
def test_packed_pre_split_conv_against_float64(C, k, dil):
    """split_planes + conv_h2p_group on the packed segments, every tile code and the automatic choice, all three output forms, with the bounds of
    test_pre_split_conv_against_float64 per segment class: y within 1.5 x the staged two-term kernel's own error (+ 1e-7), the channel-minor
    copy bit-equal to y, the planes within 5e-7 max(1, |lrelu(out)|max) of lrelu(y).  Pinned tile: every segment bit-identical to itself run
    alone; B = 1 in table form == the single-segment (by-value) entry."""
    segs, rng = _segments(C, C + k + dil)
    w = (rng.standard_normal((C, k, C)) / np.sqrt(k * C)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    rsegs = [rng.standard_normal((C, n)).astype(np.float32) for n in LENGTHS]
    pad = dil * (k - 1) // 2
    alone = {}
    worst = 0.0
    for name, order in ORDERS.items():
        x, lens = _pack(segs, order)
        res = np.concatenate([rsegs[i] for i, _ in order], axis=1)
        r64 = packed_conv_ref64(x, lens, w, b, dil, in_slope=0.1) + res
        bounds = seg_bounds(lens)
        staged, ovf = engine.debug_conv1d_packed(x, lens, w, b, dil, in_slope=0.1, in_act=1, mode=60, return_ovf=True)
        assert ovf == 0
        e_staged = np.abs(staged + res - r64)
        cls = {loud: np.concatenate([np.arange(lo, hi) for (lo, hi), (_, ld) in zip(bounds, order) if ld == loud]) for loud in (False, True)}
        for tile in list(range(11)) + [-1]:
            y, y16, yp, ovf = engine.debug_conv_h2p_packed(x, lens, w, b, dil, res, 0.1, 0.1, tile=tile, members=2 if tile % 2 else 1)
            where = (C, k, dil, name, tile)
            assert np.isfinite(y).all() and np.isfinite(y16).all() and np.isfinite(yp).all(), (where, "unwritten or non-finite positions")
            assert ovf == 0, (where, "the overflow word is up")
            assert np.array_equal(y16, y), where
            lre = np.where(y < 0, y * np.float32(0.1), y)
            err = np.abs(y - r64)
            for loud, idx in cls.items():
                e, es = float(err[:, idx].max()), float(e_staged[:, idx].max())
                worst = max(worst, e / (LOUD if loud else 1.0))
                assert e <= 1.5 * es + 1e-7, (where, "loud" if loud else "quiet", e, es)
                assert np.abs(yp[:, idx] - lre[:, idx]).max() <= 5e-7 * max(1.0, float(np.abs(lre[:, idx]).max())), (where, "planes", loud)
            # (a leak that the staged kernel shared would hide in the ratio above: the staged kernel's own error meets the plain conv bar)
            for (lo, hi), (i, loud) in zip(bounds, order):
                assert float(e_staged[:, lo:hi].max()) <= BAR * (LOUD if loud else 1.0), (where, "staged", i)
            if tile < 0:
                continue
            for (lo, hi), (i, loud) in zip(bounds, order):
                key = (tile, i, loud)
                if key not in alone:
                    alone[key] = engine.debug_conv_h2p_packed(segs[i][1 if loud else 0], [LENGTHS[i]], w, b, dil, rsegs[i], 0.1, 0.1, tile=tile,
                                                              members=2 if tile % 2 else 1)[:3]
                for got, want, form in zip((y, y16, yp), alone[key], ("y", "y16", "yp")):
                    assert np.array_equal(got[:, lo:hi], want), (where, "segment", i, form, "differs from the same segment run alone")
    for (tile, i, loud), forms in alone.items():
        if LENGTHS[i] in (129, 1, 5, 64, 256) and not loud:
            old = engine.debug_conv_h2p(segs[i][0], w, b, dil, rsegs[i], 0.1, 0.1, tile=tile, members=2 if tile % 2 else 1)[:3]
            for got, want, form in zip(forms, old, ("y", "y16", "yp")):
                assert np.array_equal(got, want), (C, k, dil, tile, form, "table form differs from the by-value entry, length", LENGTHS[i])
    print(f"PACKED_ERR pre-split two-term fp16: C={C} k={k} dil={dil} max|y - ref64| = {worst:.3e} (loud segments / 64)")


def test_packed_entries_validate_their_arguments():
    x = np.zeros((32, 10), np.float32)
    w = np.zeros((32, 3, 32), np.float32)
    for bad in ([10, 0], [11, -1], [4, 5]):            # an empty segment, a negative one, a sum that is not L
        with pytest.raises(engine.StsError):
            engine.debug_conv1d_packed(np.zeros((32, 10), np.float32), bad, w, None)
    with pytest.raises(engine.StsError):
        engine.debug_conv1d_packed(x, [10], np.zeros((32, 4, 32), np.float32), None)                     # even k, not transposed
    with pytest.raises(engine.StsError):
        engine.debug_conv1d_packed(x, [10], np.zeros((32, 5, 32), np.float32), None, stride_transposed=2)  # k - stride odd
    xw = np.zeros((128, 10), np.float32)
    ww = np.zeros((128, 3, 128), np.float32)
    for bad in ([10, 0], [4, 5]):
        with pytest.raises(engine.StsError):
            engine.debug_conv_h2p_packed(xw, bad, ww, None)
    y = engine.debug_conv1d_packed(x, [4, 6], w, np.ones(32, np.float32))
    assert y.shape == (32, 10) and np.array_equal(y, np.ones((32, 10), np.float32))
