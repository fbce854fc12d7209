"""GPU suite: the fused ResBlock layer kernels of the decoder's narrow stages (conv.hip resblock_layer_kernel, resblock_wino_kernel;
resblock_bf3.hip resblock_bf3_kernel in both arithmetics and both tile shapes per width) on caller data through sts_debug_resblock_layer,
against the float64 restatement of tests/resblock_ref.py (which tests/test_resblock_layer_cpu.py ties to the plain-C oracle).

Tolerance.  B = resblock_ref.bound is the layer evaluated on absolute values; gamma_oracle = max(err_oracle / B) of a run is computed here
on the CPU from the oracle's float32 loops.  Per element
    kinds 1 - 3:  |y - ref| <= 4 gamma_oracle B + 2^-22 max|ref|
    kind 4:       ... + 6 * 2^-22 B      (an operand kept as two fp16 terms: 2^-22; the dropped low x low product: 2^-22; per conv 3, two convs)
and per member rms(err) <= 1.5 rms(err_oracle) (kind 4: 2.0), the factors of the project's conv tests.  Every figure is printed before it is
asserted (pytest -s shows them); DESIGN.md section 3 records the largest per kernel family.

The exact family, the isolation test and the sentinel checks are conditions, not measurements: bit for bit."""
import functools

import numpy as np
import pytest

import resblock_ref as rr
from oracle import pyref
from summertts_amd import engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF
FLOOR = 2.0 ** -22
SLOPE = 0.1
PAD = 37                      # columns [L, ld) of x and of every y
LOUD = 7.0e4                  # beyond fp16: what the columns [L, ld) of x hold in every run
COMBOS = [(1, -1), (2, -1), (3, -1), (3, 1), (4, -1), (4, 1)]       # (kind, variant)
WIDTHS = [32, 64, 128]


def run_layer(xs, lens, members, slope, kind, variant=-1):
    """One launch on the segments xs packed back to back, ld = L + 37 with 7e4 in the columns past L, one spare row per y.  Checks the
    sentinels and, with finite data, the overflow word.  -> (y [n][C][L], ovf)"""
    C = xs[0].shape[0]
    L = int(sum(lens))
    x = np.full((C, L + PAD), LOUD, np.float32)
    x[:, :L] = np.concatenate(xs, axis=1)
    y, ovf = engine.debug_resblock_layer(x, lens, members, slope, kind, variant=variant, extra_rows=1)
    bits = y.view(np.uint32)
    assert y.shape == (len(members), C + 1, L + PAD)
    assert (bits[:, C:, :] == SENTINEL).all(), "a workgroup wrote a row past C"
    assert (bits[:, :, L:] == SENTINEL).all(), "a workgroup wrote a column in [L, ld)"
    assert not (bits[:, :C, :L] == SENTINEL).any(), "an element of [C][L] was left unwritten"
    if kind != 4:
        assert ovf == 0
    return np.ascontiguousarray(y[:, :C, :L]), ovf


def refused(*a, **kw):
    with pytest.raises(engine.StsError, match=r"sts error -1\b"):
        engine.debug_resblock_layer(*a, **kw)


@functools.lru_cache(maxsize=None)
def members_of(C, name):
    ms = rr.gaussian_members(9000 + C, C, name)
    for m in ms:
        for a in m:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return ms


@functools.lru_cache(maxsize=None)
def segment(C, name, n):
    """One utterance of n columns: x, and per member the float64 reference, the bound B and the oracle's error -- computed once per
    (C, member set, length), shared by every kind, variant, ordering and test, and left unchanged."""
    x = rr.gaussian_x(17 * C + 131 * n + len(name), C, n)
    ref, B, eo = [], [], []
    for m in members_of(C, name):
        r = rr.ref64(x, [n], m, SLOPE)
        ref.append(r)
        B.append(rr.bound(x, [n], m, SLOPE))
        eo.append(np.abs(pyref.port_resblock_layer(x, [n], m[0], m[1], m[2], m[3], m[4], SLOPE) - r))
    out = (x, np.stack(ref), np.stack(B), np.stack(eo))
    for a in out:
        a.setflags(write=False)
    return out


def check_run(tag, C, name, lens, kind, variant):
    """Launch on the cached segments of `lens`; per-element bar on every member; -> (err, err_oracle) [n][C][L] for the RMS bars."""
    segs = [segment(C, name, n) for n in lens]
    y, ovf = run_layer([s[0] for s in segs], lens, members_of(C, name), SLOPE, kind, variant)
    assert ovf == 0, "the overflow word on finite in-segment data"
    ref, B, eo = (np.concatenate([s[i] for s in segs], axis=2) for i in (1, 2, 3))
    err = np.abs(y - ref)
    gamma = float((eo / B).max())
    tol = 4 * gamma * B + FLOOR * float(np.abs(ref).max()) + (6 * FLOOR * B if kind == 4 else 0.0)
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    print(f"RESBLOCK {engine.RESBLOCK_KINDS[kind]} variant={variant} C={C} set={name} {tag} L={sum(lens)} err_kernel={err.max():.3e} "
          f"err_oracle={eo.max():.3e} ratio={err.max() / eo.max():.3f} err/B={float((err / B).max()):.3e} gamma_oracle={gamma:.3e} "
          f"worst(member,row,col)={tuple(int(v) for v in worst)} err={err[worst]:.3e} tol={tol[worst]:.3e}")
    assert (err <= tol).all(), (tag, worst, float(err[worst]), float(tol[worst]))
    return err, eo


def check_rms(tag, C, name, kind, variant, err, eo):
    factor = 2.0 if kind == 4 else 1.5
    for j in range(err.shape[0]):
        rk, ro = float(np.sqrt(np.mean(err[j] ** 2))), float(np.sqrt(np.mean(eo[j] ** 2)))
        print(f"RESBLOCK rms {engine.RESBLOCK_KINDS[kind]} variant={variant} C={C} set={name} {tag} member={j} rms_kernel={rk:.3e} "
              f"rms_oracle={ro:.3e} ratio={rk / ro:.3f} (bar {factor})")
        assert rk <= factor * ro, (tag, j, rk, ro)


@pytest.mark.parametrize("kind,variant", COMBOS)
@pytest.mark.parametrize("name", list(rr.MEMBER_SETS))
@pytest.mark.parametrize("C", WIDTHS)
def test_layer_against_float64(C, name, kind, variant):
    """Packed batches on the kernel's own tile edges in two orderings, then one-utterance calls; every member against ITS OWN reference
    (the launchers re-sort the members longest-first)."""
    shapes = rr.MEMBER_SETS[name]
    W = rr.tile_width(kind, C, variant)
    asc = rr.batch_lengths(W, shapes)
    for tag, lens in (("ascending", asc), ("interleaved", rr.interleaved(asc))):
        err, eo = check_run(tag, C, name, lens, kind, variant)
        check_rms(tag, C, name, kind, variant, err, eo)
    errs, eos = [], []
    for n in rr.single_lengths(W, shapes):
        err, eo = check_run(f"alone[{n}]", C, name, [n], kind, variant)
        errs.append(err)
        eos.append(eo)
    check_rms("alone-pooled", C, name, kind, variant, np.concatenate(errs, axis=2), np.concatenate(eos, axis=2))


@pytest.mark.parametrize("C", WIDTHS)
def test_variant_0_is_the_automatic_shape(C):
    for kind in (3, 4):
        lens = rr.batch_lengths(rr.tile_width(kind, C, -1), rr.HIFIGAN)
        xs = [segment(C, "hifigan", n)[0] for n in lens]
        a, _ = run_layer(xs, lens, members_of(C, "hifigan"), SLOPE, kind, -1)
        b, _ = run_layer(xs, lens, members_of(C, "hifigan"), SLOPE, kind, 0)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), kind


@pytest.mark.parametrize("kind,variant", COMBOS)
@pytest.mark.parametrize("C", WIDTHS)
def test_exact_family_bit_for_bit(C, kind, variant):
    """Integer x, sparse weights from {+-2, +-4}, integer biases, slope 0.5 (resblock_ref.exact_members): every sum is exact in all four
    arithmetics, so every kind and variant must give float64's value exactly -- at NT - 1, NT + 1 of every member's tile and at 5."""
    W = rr.tile_width(kind, C, variant)
    for shapes in (rr.HIFIGAN, rr.FOUR):
        members = rr.exact_members(700 + C + len(shapes), C, shapes)
        lens = sorted({5} | {v for nt in rr.tile_nts(W, shapes) for v in (nt - 1, nt + 1)})
        xs = [rr.exact_x(800 + C + n, C, n) for n in lens]
        y, ovf = run_layer(xs, lens, members, rr.EXACT_SLOPE, kind, variant)
        assert ovf == 0
        x = np.concatenate(xs, axis=1)
        for j, m in enumerate(members):
            ref = rr.ref64(x, lens, m, rr.EXACT_SLOPE)
            bad = np.argwhere(y[j].astype(np.float64) != ref)
            assert bad.size == 0, (len(shapes), j, bad[:4].tolist(), float(np.abs(y[j] - ref).max()))


@pytest.mark.parametrize("kind,variant", COMBOS)
@pytest.mark.parametrize("C", WIDTHS)
def test_layer_never_reads_a_neighbouring_utterance(C, kind, variant):
    """A middle utterance between two all-NaN neighbours is the same utterance run alone, bit for bit (two tiles: NT + 1 of the longest
    conv2, and a short one whose whole window reaches into both neighbours)."""
    W = rr.tile_width(kind, C, variant)
    members = members_of(C, "hifigan")
    for mid in (rr.tile_nts(W, rr.HIFIGAN)[0] + 1, 4):
        x = segment(C, "hifigan", mid)[0]
        nan_l, nan_r = np.full((C, 9), np.nan, np.float32), np.full((C, 7), np.nan, np.float32)
        alone, _ = run_layer([x], [mid], members, SLOPE, kind, variant)
        y, _ = engine.debug_resblock_layer(np.concatenate([nan_l, x, nan_r], axis=1), [9, mid, 7], members, SLOPE, kind, variant=variant)
        got = y[:, :, 9:9 + mid]
        assert np.isfinite(got).all(), mid
        assert (got.view(np.uint32) == alone.view(np.uint32)).all(), mid


@pytest.mark.parametrize("variant", [-1, 1])
@pytest.mark.parametrize("C", WIDTHS)
def test_overflow_word_of_the_two_term_form(C, variant):
    """0 on finite data with 7e4 only in the columns [L, ld) of x (every accuracy run of this file asserts that too); 1 when one in-segment x is
    7e4 (positive: the range check sees lrelu(x)) -- in the first or the second tile of the long utterance, or in a short neighbour."""
    W = rr.tile_width(4, C, variant)
    nt = rr.tile_nts(W, rr.ONE)[0]
    lens = [3, nt + 1, 6]
    members = members_of(C, "one")
    xs = [segment(C, "one", n)[0] for n in lens]
    _, ovf = run_layer(xs, lens, members, SLOPE, 4, variant)
    assert ovf == 0
    for seg, row, col in ((1, C - 1, nt // 2), (1, 0, nt), (2, 5, 0), (0, 1, 2)):
        loud = [a.copy() for a in xs]
        loud[seg][row, col] = LOUD
        _, ovf = run_layer(loud, lens, members, SLOPE, 4, variant)
        assert ovf == 1, (seg, row, col)
        _, ovf3 = run_layer(loud, lens, members, SLOPE, 3, variant)       # the three-term form has no range to leave
        assert ovf3 == 0


def _one(C, k1, d1, k2, seed=0):
    rng = np.random.default_rng(4000 + seed + C + 10 * k1 + 100 * d1 + 1000 * k2)
    w1 = (rng.standard_normal((C, k1, C)) / np.sqrt(k1 * C)).astype(np.float32)
    w2 = (rng.standard_normal((C, k2, C)) / np.sqrt(k2 * C)).astype(np.float32)
    return (w1, rng.standard_normal(C).astype(np.float32), d1, w2, rng.standard_normal(C).astype(np.float32))


def _accurate(C, member, lens, kind, variant=-1):
    x = rr.gaussian_x(77 + C + sum(lens), C, sum(lens))
    y, ovf = run_layer([x], lens, [member], SLOPE, kind, variant)
    assert ovf == 0
    ref, B = rr.ref64(x, lens, member, SLOPE), rr.bound(x, lens, member, SLOPE)
    eo = np.abs(pyref.port_resblock_layer(x, lens, member[0], member[1], member[2], member[3], member[4], SLOPE) - ref)
    err = np.abs(y[0] - ref)
    tol = 4 * float((eo / B).max()) * B + FLOOR * float(np.abs(ref).max()) + (6 * FLOOR * B if kind == 4 else 0.0)
    print(f"RESBLOCK limit {engine.RESBLOCK_KINDS[kind]} variant={variant} C={C} (k1,dil1,k2)={(member[0].shape[1], member[2], member[3].shape[1])} "
          f"err_kernel={err.max():.3e} err_oracle={eo.max():.3e} ratio={err.max() / eo.max():.3f} err/B={float((err / B).max()):.3e}")
    assert (err <= tol).all(), (kind, variant, float((err - tol).max()))


@pytest.mark.parametrize("C", WIDTHS)
def test_the_widest_admitted_geometry_is_accurate(C):
    """dil1 (k1 - 1) = 64 and k2 = 33, the edge the kernels admit: kinds 1, 3 and 4 (both variants); NT = W - 32."""
    m = _one(C, 3, 32, 33)
    for kind, variant in ((1, -1), (3, -1), (3, 1), (4, -1), (4, 1)):
        nt = rr.tile_width(kind, C, variant) - 32
        _accurate(C, m, [nt + 1, 1, 2 * nt, 47, nt - 1], kind, variant)


@pytest.mark.parametrize("C", WIDTHS)
def test_geometries_outside_the_limits_are_refused(C):
    x = rr.gaussian_x(3, C, 300 + PAD)
    ok = _one(C, 3, 1, 3)
    for kind in (1, 2, 3, 4):
        refused(x, [300], [_one(C, 3, 33, 3)], SLOPE, kind)          # dil1 (k1 - 1) = 66
        refused(x, [300], [_one(C, 3, 1, 35)], SLOPE, kind)          # k2 = 35
        refused(x, [300], [_one(C, 4, 1, 3)], SLOPE, kind)           # an even k1
        refused(x, [300], [_one(C, 3, 1, 4)], SLOPE, kind)           # an even k2
        refused(x, [300], [ok] * 5, SLOPE, kind)                     # n = 5
        y, _ = engine.debug_resblock_layer(x, [300], [ok], SLOPE, kind)          # and the entry does run what is inside them
        assert np.isfinite(y[0, :, :300]).all()
    # the Winograd form: dil1 must divide 30 (and be <= 6), 2 <= k2 <= 15
    refused(x, [300], [_one(C, 3, 4, 3)], SLOPE, 2)
    refused(x, [300], [_one(C, 3, 1, 17)], SLOPE, 2)
    refused(x, [300], [_one(C, 3, 32, 33)], SLOPE, 2)
    for d1 in (1, 2, 3, 5, 6):
        _accurate(C, _one(C, 11, d1, 7), [121, 9, 250], 2)


def test_a_width_no_kernel_has_is_refused():
    x = rr.gaussian_x(4, 96, 200)
    for kind in (1, 2, 3, 4):
        refused(x, [200], [_one(96, 3, 1, 3)], SLOPE, kind)
