"""oracle.undistort_image against an independent NumPy formulation of cv::remap(INTER_LINEAR,
BORDER_CONSTANT 0) (image_cases.remap_reference), on the calibrations that test_gpu_image_paths.py
runs on the device: pins the reference those GPU cases lean on, checks that each case really holds
the tile kinds and map entries it exists for, and that its inputs can tell the right rule from the
wrong ones.  CPU only."""
import time

import numpy as np
import pytest

import image_cases as ic


@pytest.mark.parametrize("name", ic.ALL_CASES)
def test_oracle_remap_equals_reference(oracle, name):
    c = ic.CASES[name]
    src = ic.source(name)[0]
    out, mx, my, _ = oracle.undistort_image(src, c["kd"], np.float32(c["dist"]))
    ref = ic.remap_reference(src, mx, my)
    assert np.array_equal(out, ref), (name, np.argwhere(out != ref)[:8].tolist())
    if name in ic.POLE_CASES:  # a non-finite entry is an outlier: 0, not the pixel at (0, 0)
        assert src[0, 0] == 255 and [int(ref[p]) for p in ic.POLE_PIXELS] == [0, 0, 0, 0]


def test_case_conditions(oracle):
    kinds = {}
    for name in ic.ALL_CASES:
        c = ic.CASES[name]
        mx, my = ic.oracle_maps(oracle, name)
        k = ic.tile_kinds(mx, my, c["w"], c["h"])
        assert k.shape == (-(-c["h"] // 16), -(-c["w"] // 64))
        kinds[name] = [int((k == v).sum()) for v in (ic.EMPTY, ic.STAGED, ic.FALLBACK)]
        if name not in ic.POLE_CASES:
            assert np.isfinite(mx).all() and np.isfinite(my).all(), name
    assert min(kinds["zoom"]) >= 1, kinds["zoom"]
    assert kinds["fold"][1] >= 1 and kinds["fold"][2] >= 1, kinds["fold"]
    assert ic.half_way_fraction(*ic.oracle_maps(oracle, "ties")) >= 0.9
    mx, my = ic.oracle_maps(oracle, "pole_inf")
    assert (np.isinf(mx) | np.isinf(my)).sum() >= 1
    mx, my = ic.oracle_maps(oracle, "pole_nan")
    assert (np.isnan(mx) & np.isnan(my)).sum() >= 1
    for name in ic.POLE_CASES:  # the pole pixels are where the GPU test looks for them
        mx, my = ic.oracle_maps(oracle, name)
        bad = ~(np.isfinite(mx) & np.isfinite(my))
        assert sorted(map(tuple, np.argwhere(bad).tolist())) == ic.POLE_PIXELS, name


@pytest.mark.parametrize("mutant", list(ic.MUTANTS))
def test_cases_see_a_wrong_rule(oracle, mutant):
    name, fn = ic.MUTANTS[mutant]
    c = ic.CASES[name]
    src = ic.source(name)[0]
    out, mx, my, _ = oracle.undistort_image(src, c["kd"], np.float32(c["dist"]))
    assert np.array_equal(out, ic.remap_reference(src, mx, my))
    assert (fn(src, mx, my) != out).any(), (mutant, "the inputs of", name, "cannot see this error")


def test_fixed_point_out_of_range():
    """The conversion rule at the edges of int range (float32 products)."""
    f = np.float32
    u = np.array([np.nan, np.inf, -np.inf, f(2.0 ** 26), -f(2.0 ** 26), f(2.0 ** 26) - f(4), -f(2.0 ** 26) - f(8), 0.515625,
                  0.546875, -0.015625, 3e38], np.float32)
    got = ic.fixed_point(u).tolist()
    lo = ic.INT_MIN
    assert got == [lo, lo, lo, lo, lo, 2 ** 31 - 128, lo, 16, 18, 0, lo]


def test_reference_is_fast():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (192, 384), dtype=np.uint8)
    mx = rng.uniform(-20, 404, (192, 384)).astype(np.float32)
    my = rng.uniform(-20, 212, (192, 384)).astype(np.float32)
    t0 = time.perf_counter()
    ic.remap_reference(src, mx, my)
    assert time.perf_counter() - t0 < 1.0
