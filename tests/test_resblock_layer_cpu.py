"""CPU suite for the fused-ResBlock-layer kernel tests: the float64 restatement of tests/resblock_ref.py is vouched for by the project's
plain-C oracle (oracle/vits_oracle.c port_resblock_layer = the resblock_layer function its resblock_forward loops over, which
tests/test_oracle_cpu.py holds to the compiled reference through whole models); the oracle's own distance from float64, gamma_oracle =
max(err_oracle / B) with B = resblock_ref.bound, is the unit of the GPU file's tolerances.  The entry's argument checks run without a GPU."""
import os
import re

import numpy as np
import pytest

import resblock_ref as rr
from conftest import ROOT
from oracle import pyref
from summertts_amd import engine

SLOPE = 0.1


def _gamma(x, lens, members, slope):
    g = 0.0
    for m in members:
        ref, B = rr.ref64(x, lens, m, slope), rr.bound(x, lens, m, slope)
        got = pyref.port_resblock_layer(x, lens, m[0], m[1], m[2], m[3], m[4], slope)
        assert np.isfinite(got).all() and (B > 0).all()
        g = max(g, float((np.abs(got - ref) / B).max()))
    return g


@pytest.mark.parametrize("name", list(rr.MEMBER_SETS))
@pytest.mark.parametrize("C", [32, 64])
def test_oracle_layer_agrees_with_float64_within_its_summation_bound(port_built, C, name):
    """gamma_oracle <= ((k1 + k2) C + 8) 2^-24 (resblock_ref.oracle_gamma_limit: sequential float32 sums), and far below what a wrong tap,
    a missing bias or a missing zero pad would give (those are errors of order 1 against B of order 10)."""
    shapes = rr.MEMBER_SETS[name]
    lens = rr.batch_lengths(128, shapes)[:12]
    members = rr.gaussian_members(1000 + C, C, name)
    x = rr.gaussian_x(2000 + C, C, sum(lens))
    g = _gamma(x, lens, members, SLOPE)
    limit = rr.oracle_gamma_limit(C, shapes)
    print(f"RESBLOCK oracle C={C} set={name} gamma_oracle={g:.3e} limit={limit:.3e}")
    assert 0.0 < g <= limit, (g, limit)
    assert g <= 1e-5


def test_packed_equals_per_utterance(port_built):
    """The packed wrapper convolves every utterance on its own, and so does ref64: position p of utterance b never sees b +- 1."""
    C, lens = 32, [1, 2, 9, 40, 3]
    m = rr.gaussian_members(5, C, "one")[0]
    x = rr.gaussian_x(6, C, sum(lens))
    packed = pyref.port_resblock_layer(x, lens, m[0], m[1], m[2], m[3], m[4], SLOPE)
    ref = rr.ref64(x, lens, m, SLOPE)
    off = 0
    for n in lens:
        seg = np.ascontiguousarray(x[:, off:off + n])
        alone = pyref.port_resblock_layer(seg, [n], m[0], m[1], m[2], m[3], m[4], SLOPE)
        assert np.array_equal(alone, packed[:, off:off + n])
        assert np.array_equal(rr.ref64(seg, [n], m, SLOPE), ref[:, off:off + n])
        off += n
    # and the neighbours matter to a conv that is NOT segmented: the whole row as one utterance differs at the inner edges
    whole = rr.ref64(x, [sum(lens)], m, SLOPE)
    assert np.abs(whole - ref).max() > 1e-2


def test_intermediate_is_zero_outside_the_utterance_although_b1_is_not():
    """One channel, x = 0, w1 = 0, b1 = 1, w2 = ones(3): the intermediate is lrelu(1) = 1 inside [0, n) and conv2 sums its 3 taps -- 2 at both
    edges, 3 inside.  A conv1 evaluated past the edge (bias included) would give 3 everywhere."""
    w1 = np.zeros((1, 3, 1), np.float32)
    w2 = np.ones((1, 3, 1), np.float32)
    one = np.ones(1, np.float32)
    y = rr.ref64(np.zeros((1, 9), np.float32), [5, 4], (w1, one, 1, w2, None), SLOPE)
    assert y.tolist() == [[2, 3, 3, 3, 2, 2, 3, 3, 2]]
    assert rr.bound(np.zeros((1, 9), np.float32), [5, 4], (w1, one, 1, w2, None), SLOPE).tolist() == [[2, 3, 3, 3, 2, 2, 3, 3, 2]]


@pytest.mark.parametrize("C", [32, 64])
def test_exact_family_is_exact_in_the_restatement_and_the_oracle(port_built, C):
    shapes = rr.HIFIGAN + rr.FOUR
    members = rr.exact_members(300 + C, C, shapes)
    lens = [117, 127, 5]
    x = rr.exact_x(400 + C, C, sum(lens))
    for m in members:
        ref = rr.ref64(x, lens, m, rr.EXACT_SLOPE)
        assert (ref * 2 == np.round(ref * 2)).all() and np.abs(ref).max() < 2 ** 12
        assert rr.bound(x, lens, m, rr.EXACT_SLOPE).max() < 2 ** 12
        assert np.count_nonzero(m[0].reshape(C, -1), axis=1).max() <= 8 and np.count_nonzero(m[3].reshape(C, -1), axis=1).max() <= 8
        got = pyref.port_resblock_layer(x, lens, m[0], m[1], m[2], m[3], m[4], rr.EXACT_SLOPE)
        assert (got.astype(np.float64) == ref).all()
        assert np.abs(ref - x).max() > 10           # and the family is no fixed point: the convs contribute


def test_lengths_sit_on_the_tiles():
    assert [rr.tile_width(1, c) for c in (32, 64, 128)] == [128] * 3
    assert [rr.tile_width(2, c) for c in (32, 64, 128)] == [240, 120, 120]
    assert [rr.tile_width(k, 32, v) for k in (3, 4) for v in (-1, 0, 1)] == [256, 256, 128] * 2
    assert [rr.tile_width(3, c, v) for c in (64, 128) for v in (-1, 0, 1)] == [128] * 6
    lens = rr.batch_lengths(128, rr.HIFIGAN)
    assert lens == sorted(set(lens)) and {1, 2, 3, 117, 118, 119, 236, 237, 121, 122, 123, 244, 245, 125, 126, 127, 252, 253} <= set(lens)
    assert {1, 3, 11, 13, 29, 31} <= set(lens)      # h1 + h2 -+ 1 of (3,1,3), (7,3,7), (11,5,11): h1 + h2 = 2, 12, 30
    il = rr.interleaved(lens)
    assert sorted(il) == lens and il[0] == lens[0] and il[1] == lens[-1] and il[2] == lens[1]
    assert rr.single_lengths(128, rr.FOUR) == sorted({1, 3 * 118 + 5, 118, 119, 122, 123, 124, 125, 126, 127})


def test_entry_is_exported_declared_and_bound():
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "summertts_hip.h")).read()
    assert re.search(r"\bint sts_debug_resblock_layer\(int device, const float\* x, int32_t C, const int32_t\* lengths, int32_t B, int64_t ld, int32_t n,", hdr)
    assert hasattr(lib, "sts_debug_resblock_layer") and "sts_debug_resblock_layer" in engine.EXPORTED_SYMBOLS
    assert len(lib.sts_debug_resblock_layer.argtypes) == 20
    assert lib.sts_abi_version() == 18 and "#define STS_ABI_VERSION 18\n" in hdr


def test_entry_argument_checks_need_no_gpu():
    """What the entry refuses before it touches a device: STS_EINVAL, whatever machine it runs on."""
    C = 32
    m = rr.gaussian_members(1, C, "one")[0]
    x = np.zeros((C, 20), np.float32)

    def refused(*a, **kw):
        with pytest.raises(engine.StsError, match=r"sts error -1\b"):
            engine.debug_resblock_layer(*a, **kw)

    refused(x, [20], [m] * 5, SLOPE, 1)                     # n = 5 > kMaxGroup
    refused(x, [20], [m], SLOPE, 0)
    refused(x, [20], [m], SLOPE, 5)
    refused(x, [20], [m], SLOPE, 3, variant=2)
    refused(x, [20], [m], SLOPE, 3, variant=-2)
    refused(x, [0, 20], [m], SLOPE, 1)                      # a length below 1
    refused(x, [10, 5], [(m[0], m[1], 0, m[3], m[4])], SLOPE, 1)      # dil1 = 0
    with pytest.raises(ValueError):
        engine.debug_resblock_layer(x, [21], [m], SLOPE, 1)           # sum(lengths) > ld
    with pytest.raises(ValueError):
        engine.debug_resblock_layer(x, [20], [(m[0][:, :, :16], m[1], 1, m[3], m[4])], SLOPE, 1)
