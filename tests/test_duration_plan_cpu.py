"""CPU suite of the duration plans (ABI 14): sts_duration_fit against the integer checker of tests/duration_ref.py bit for bit on random and
adversarial weights, the infeasibility rules, and the header / library surface.  Nothing here touches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import duration_ref as dr
from conftest import ROOT
from summertts_amd import engine

STS_EINVAL = -1
HEADER = os.path.join(ROOT, "include", "summertts_hip.h")
LENGTHS = (1, 2, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def check_properties(w, fixed, target, d):
    fx = [-1] * len(w) if fixed is None else list(fixed)
    assert int(d.astype(np.int64).sum()) == target
    share = dr.exact_share(w, fixed, target)
    for i, v in enumerate(fx):
        if v >= 0:
            assert d[i] == v, i
        else:
            assert d[i] >= 1, i
            num, K = share[i]
            assert abs((int(d[i]) - 1) * K - num) < K, (i, int(d[i]), num, K)      # |d - 1 - R' k / K| < 1, in integers


def test_reference_on_a_worked_example():
    # R' = 10 - 3 = 7, k = (1, 2, 4) 2^20: a = (1, 2, 4), r = (0, 0, 0): no frame left
    assert dr.fit([1.0, 2.0, 4.0], None, 10).tolist() == [2, 3, 5]
    # R' = 2 over three equal weights: a = 0, r equal, L = 2: the two lowest indices
    assert dr.fit([1.0, 1.0, 1.0], None, 5).tolist() == [2, 2, 1]
    # fixed entries stay; the free ones share the rest; all-zero weights count as equal
    assert dr.fit([0.0, 9.0, 0.0], [-1, 4, -1], 9).tolist() == [3, 4, 2]
    assert dr.fit([0.2, 1.5, 3.0, np.nan], [-1, -1, 0, -1], 0).tolist() == [1, 2, 0, 0]
    assert dr.fit([1e9, np.inf], None, 0).tolist() == [dr.MAX_DUR, dr.MAX_DUR]


@pytest.mark.parametrize("n", LENGTHS)
def test_fit_equals_the_reference_bit_for_bit(lib, n):
    for name, w in dr.weight_sets(n, 100 + n).items():
        for fixed in (None, [(-1 if i % 3 else (i % 7)) for i in range(n)]):
            fx = [-1] * n if fixed is None else fixed
            n_free = sum(1 for v in fx if v < 0); sfix = sum(v for v in fx if v >= 0)
            if n_free == 0:
                tg = [sfix] if sfix >= 1 else []
            else:
                tg = dr.targets([w[i] for i in range(n) if fx[i] < 0], n_free, sfix)
            for target in [0] + tg:
                got = engine.duration_fit(w, fixed, target)
                want = dr.fit(w, fixed, target)
                assert got.dtype == np.int32 and np.array_equal(got, want), (name, n, fixed is not None, target)
                if target:
                    check_properties(w, fixed, target, got)


def test_ties_go_by_index_and_the_outlier_takes_the_frames(lib):
    d = engine.duration_fit(np.full(65, 2.75, np.float32), None, 65 + 10)
    assert d.tolist() == [2] * 10 + [1] * 55
    w = np.full(257, 1e-3, np.float32); w[128] = 1e5
    d = engine.duration_fit(w, None, 257 + 1000)
    assert d[128] > 990 and d.sum() == 1257 and (d >= 1).all()
    z = engine.duration_fit(np.zeros(64, np.float32), None, 100)
    assert z.tolist() == [2] * 36 + [1] * 28
    assert np.array_equal(engine.duration_fit([np.nan, 1.0], None, 1 << 20), dr.fit([np.nan, 1.0], None, 1 << 20))


def test_infeasibility_rules(lib):
    rng = np.random.default_rng(5)
    out = np.zeros(8, np.int32)
    for trial in range(300):
        n = int(rng.integers(1, 9))
        w = rng.random(n).astype(np.float32)
        fixed = rng.integers(-1, 4, n).astype(np.int32)
        if trial % 5 == 0:
            fixed[:] = np.abs(fixed)                   # nobody free
        target = int(rng.integers(1, 16))
        sfix = int(fixed[fixed >= 0].sum()); n_free = int((fixed < 0).sum())
        bad = (target - sfix < n_free) if n_free else (sfix != target)
        assert bad == (not dr.feasible(fixed, n, target))
        rc = lib.sts_duration_fit(w.ctypes.data, fixed.ctypes.data, n, target, out.ctypes.data)
        assert rc == (STS_EINVAL if bad else 0), (fixed.tolist(), target)
    w = np.ones(3, np.float32)
    for fixed, target in (([-2, 1, 1], 0), ([100001, -1, -1], 0), (None, -1), (None, (1 << 20) + 1), (None, 2)):
        f = None if fixed is None else np.asarray(fixed, np.int32)
        assert lib.sts_duration_fit(w.ctypes.data, None if f is None else f.ctypes.data, 3, target, out.ctypes.data) == STS_EINVAL, (fixed, target)
    assert lib.sts_duration_fit(w.ctypes.data, None, 0, 0, out.ctypes.data) == STS_EINVAL
    assert lib.sts_duration_fit(w.ctypes.data, None, 3, 3, None) == STS_EINVAL
    assert lib.sts_duration_fit(w.ctypes.data, None, 3, 1 << 20, out.ctypes.data) == 0 and out[:3].sum() == 1 << 20
    with pytest.raises(engine.StsError, match="target"):
        engine.duration_fit(w, None, 2)


def _arg_count(name, src):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_says_15_and_the_library_agrees(lib, tmp_path):
    src = open(HEADER).read()
    assert re.search(r"#define STS_ABI_VERSION (\d+)", src).group(1) == "18" and lib.sts_abi_version() == 18
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("sts_set_duration_plan", 4), ("sts_duration_fit", 5), ("sts_duration_plan_apply", 7), ("sts_get_phoneme_offsets", 3),
                        ("sts_pool_submit_plan", 11), ("sts_multi_set_duration_plan", 4),
                        ("sts_debug_conv1d_packed", 20), ("sts_debug_conv_h2p_packed", 20)):       # ABI 15: the packed stand-alone conv entries
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS, name
        assert _arg_count(name, code) == nargs, name
    # the plan struct as the C compiler lays it out, its ctypes mirror, and sts_profile's pinned size
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "summertts_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu", '
                    'sizeof(sts_profile), sizeof(sts_dur_plan), offsetof(sts_dur_plan, rate), offsetof(sts_dur_plan, fixed), '
                    'offsetof(sts_dur_plan, target_frames)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    prof, plan, o_rate, o_fixed, o_target = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert prof == C.sizeof(engine.Profile) == 200          # (what ABI 13 had: the plan adds no profile field)
    assert plan == C.sizeof(engine.DurPlan) and (o_rate, o_fixed, o_target) == (engine.DurPlan.rate.offset, engine.DurPlan.fixed.offset,
                                                                              engine.DurPlan.target_frames.offset)
