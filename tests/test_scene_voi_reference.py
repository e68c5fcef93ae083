"""The volume of interest on the CPU: the three math functions of csrc/scene_math.hpp against fp64,
mage_voi_teardrop_host against the fp64 formula, and mage_volume_of_interest_host (the plain C++ twin
of the kernels) against the fp64 restatement of tests/scene_ref.py level by level, each level fed the
twin's own box from the level before; then the statuses, and a literal float32 restatement of the
frustum box and of what the keyframe scores decide, compared exactly."""
import ctypes as C
import dataclasses
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import _lib, scene
from tests import scene_cases as sc
from tests import scene_ref as sr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mageslam_amd" / "csrc"

# The largest errors measured over the dense samples below, rounded up to the next whole ulp
# (measured: acos 0.92, exp 1.19, cbrt 0.74).
ACOS_ULPS, EXP_ULPS, CBRT_ULPS = 1, 2, 1

MATH_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scene_math.hpp"
using namespace mage::scene;
int main(int argc, char** argv) {  // voi_math_probe FUNCTION < float32 values > float32 results
    if (argc != 2) return 2;
    float x;
    while (fread(&x, 4, 1, stdin) == 1) {
        const float y = argv[1][0] == 'a' ? voi_acosf(x) : (argv[1][0] == 'e' ? voi_expf(x) : voi_cbrtf(x));
        fwrite(&y, 4, 1, stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def math_probe():
    """The three functions as the twin compiles them (plain host C++, -ffp-contract=off)."""
    out = ROOT / "mageslam_amd" / "_lib" / "voi_math_probe"
    src = out.with_suffix(".cpp")
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [CSRC / "scene_math.hpp", CSRC / "newpoints_math.hpp", ROOT / "include" / "mage_hot.h"]
    if not out.exists() or not src.exists() or src.read_text() != MATH_PROBE or \
            out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        src.write_text(MATH_PROBE)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(src), "-o",
                        str(out)], check=True)

    def run(fn, x):
        x = np.ascontiguousarray(x, np.float32)
        r = subprocess.run([str(out), fn], input=x.tobytes(), capture_output=True, check=True)
        return np.frombuffer(r.stdout, np.float32)

    return run


def ulps(got, ref64):
    """|got - ref| in units of the float32 spacing at ref."""
    r32 = np.abs(ref64).astype(np.float32)
    spacing = np.spacing(np.maximum(r32, np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
    spacing = np.where(r32 < np.finfo(np.float32).tiny, float(np.float32(1e-45)), spacing)
    return np.abs(got.astype(np.float64) - ref64) / spacing


def test_acos_against_fp64(math_probe):
    x = np.concatenate([np.linspace(-1, 1, 2_000_001), [-1.0, 1.0, 0.0, 0.5, -0.5]]).astype(np.float32)
    e = ulps(math_probe("a", x), np.arccos(x.astype(np.float64)))
    print("voi_acosf: largest error", e.max(), "ulps")
    assert e.max() <= ACOS_ULPS
    # the clamp: past +-1 the end values, where libm gives NaN
    got = math_probe("a", np.array([1.0000001, 2.0, np.inf, -1.0000001, -3.0, -np.inf], np.float32))
    assert np.all(got[:3] == 0) and np.all(got[3:] == np.float32(np.pi))
    assert np.isnan(math_probe("a", np.array([np.nan], np.float32))[0])


def test_exp_against_fp64(math_probe):
    x = np.concatenate([-np.linspace(0, 104, 4_000_001), [-0.0, -1.0, -87.33655, -103.97]]).astype(np.float32)
    e = ulps(math_probe("e", x), np.exp(x.astype(np.float64)))
    print("voi_expf: largest error", e.max(), "ulps")
    assert e.max() <= EXP_ULPS
    got = math_probe("e", np.array([0.0, -0.0, -104.5, -1000.0, -np.inf], np.float32))
    assert got[0] == 1 and got[1] == 1
    assert np.all(got[2:] == 0) and not np.signbit(got[2:]).any()  # underflow to +0


def test_cbrt_against_fp64(math_probe):
    bits = np.arange(1, 0x7F800000, 997, dtype=np.uint32)  # positive floats across the exponent range, subnormals included
    x = bits.view(np.float32)
    e = ulps(math_probe("c", x), np.cbrt(x.astype(np.float64)))
    print("voi_cbrtf: largest error", e.max(), "ulps")
    assert e.max() <= CBRT_ULPS
    k = np.arange(1, 201, dtype=np.float32)
    assert np.array_equal(math_probe("c", k * k * k), k)  # exact cubes
    assert np.array_equal(math_probe("c", np.array([0.0, 8.0, -27.0], np.float32)), np.array([0.0, 2.0, -3.0], np.float32))


# ------------------------------------------------------------------------------------------------


@dataclasses.dataclass
class Level:
    lod: int
    side64: float
    dims64: tuple
    thr64: float
    margin: float           # the smallest |value - threshold| over fp64 voxels and centroids
    set64: np.ndarray       # fp64 voxels above the threshold
    cset64: np.ndarray
    set32: np.ndarray       # the twin's, rebuilt from its own teardrop function summed in keyframe order
    cset32: np.ndarray
    box64: tuple
    e_t: float              # the largest |twin teardrop - fp64 teardrop| over the level's points


def sum_in_order(scores):
    """Float32 sums over the keyframes in keyframe order, as one thread sums a voxel."""
    v = np.zeros(len(scores), np.float32)
    for k in range(scores.shape[1]):
        v = v + scores[:, k]
    return v


def analyse_scene(c):
    """The twin's run and, per level, the fp64 restatement fed the twin's box from the level before."""
    cs = c.settings.to_c()
    t = scene.calculate_volume_of_interest(cs, c.keyframes, c.depths, backend="host")
    K = sr.voi_keyframes(cs, c.keyframes, c.depths)
    n = len(c.keyframes)
    cen32 = sr.voi_keyframes(cs, c.keyframes, c.depths, np.float32).centroid
    kf64 = sr.teardrop(cs, K, K.centroid).sum(1)
    kf32 = sum_in_order(scene.teardrop_scores(cs, c.keyframes, c.depths, cen32))
    vmin, vmax = kf64.min(), max(kf64.max(), float(np.finfo(np.float32).tiny))
    levels = []
    twin_box0 = scene.calculate_volume_of_interest(dataclasses.replace(c.settings, iterations=0).to_c(), c.keyframes, c.depths,
                                                   backend="host")
    bmin, bmax = twin_box0.min, twin_box0.max
    for li in range(t.levels_done if t.status != scene.VOI_OK else int(cs.iterations)):
        L = t.trace[li]
        lod = int(cs.iterations) - li
        diag = bmax.astype(np.float64) - bmin.astype(np.float64)
        side64 = float(np.cbrt(diag.prod() / (int(cs.voxel_count_floor) // 2 ** lod)))
        dims64 = tuple(int(np.ceil(d / side64)) for d in diag)
        # the twin's voxel points (its side, float32 operations), so that both sides score the same points
        pts32 = bmin[None] + sr.voi_grid_points(np.zeros(3), 1.0, L["dims"]).astype(np.float32) * np.float32(L["side"])
        pts = pts32.astype(np.float64)
        s64 = sr.teardrop(cs, K, pts)
        s32 = scene.teardrop_scores(cs, c.keyframes, c.depths, pts32)
        e_t = float(np.abs(s32.astype(np.float64) - s64).max())
        v64 = s64.sum(1)
        vmin, vmax = min(vmin, v64.min()), max(vmax, v64.max())
        thr64 = (vmax - vmin) * (float(np.float32(cs.threshold)) / lod) + vmin
        margin = min(np.abs(v64 - thr64).min(), np.abs(kf64 - thr64).min())
        half = float(L["side"]) / 2
        set64, cset64 = v64 > thr64, kf64 > thr64
        lo = np.concatenate([pts[set64] - half, K.centroid[cset64] - half])
        hi = np.concatenate([pts[set64] + half, K.centroid[cset64] + half])
        # the maxima start at numeric_limits<float>::min(), so none drops below it
        box64 = (lo.min(0), np.maximum(hi.max(0), float(np.finfo(np.float32).tiny))) if len(lo) else (None, None)
        v32 = sum_in_order(s32)
        levels.append(Level(lod, side64, dims64, thr64, float(margin), set64, cset64, v32 > L["threshold"],
                            kf32 > L["threshold"], box64, e_t))
        bmin, bmax = L["box_min"], L["box_max"]
    return t, levels, n


@functools.lru_cache(maxsize=None)
def analyse(name):
    return analyse_scene(sc.voi_scene(name))


def test_teardrop_against_fp64():
    """mage_voi_teardrop_host over every scene's voxel points; e_t is what the level tests scale with."""
    worst = 0.0
    for name in sc.VOI_OK_NAMES:
        _, levels, _ = analyse(name)
        e = max(L.e_t for L in levels)
        print(name, "e_t", e)
        worst = max(worst, e)
    # Recorded, not bounded by the issue: the largest differences sit at points close to a keyframe's
    # view axis, where acos(dot / distance) turns a float rounding of the ratio near 1 into an angle
    # error of up to sqrt(2 x 2^-23) = 5e-4 rad, in float as in the reference.  Measured: at most 1e-3.
    print("largest e_t", worst)
    assert np.isfinite(worst)


def test_teardrop_special_points():
    c = sc.voi_scene("line")
    cs = c.settings.to_c()
    K32 = sr.voi_keyframes(cs, c.keyframes, c.depths, np.float32)
    K = sr.voi_keyframes(cs, c.keyframes, c.depths)
    # a point that coincides with a centroid scores exactly 1 against that keyframe
    s = scene.teardrop_scores(cs, c.keyframes, c.depths, K32.centroid)
    assert np.all(np.diag(s) == 1.0)
    # points along a view axis: dot / distance rounds past 1 for some of them, where libm's acos is NaN
    t = np.linspace(0.05, 5.0, 4000, dtype=np.float32)[:, None]
    pts = K32.centroid[0][None] + t * K32.forward[0][None]
    a = pts - K32.centroid[0][None]
    ratio = ((a[:, 0] * K32.forward[0, 0] + a[:, 1] * K32.forward[0, 1]) + a[:, 2] * K32.forward[0, 2]) / \
        np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    assert (ratio > 1).any()  # the clamp is reached
    s = scene.teardrop_scores(cs, c.keyframes, c.depths, pts)
    assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all()


@pytest.mark.parametrize("name", sc.VOI_OK_NAMES)
def test_twin_level_by_level(name):
    c = sc.voi_scene(name)
    t, levels, n = analyse(name)
    assert t.status == scene.VOI_OK and t.levels_done == c.settings.iterations == len(levels)
    for li, L in enumerate(levels):
        T = t.trace[li]
        # the condition on the scene: no fp64 value within 4 n_kf e_t of the fp64 threshold
        assert L.margin > 4 * n * L.e_t, (name, li, L.margin, 4 * n * L.e_t)
        assert abs(float(T["side"]) - L.side64) <= 4 * np.spacing(np.float32(L.side64))
        assert tuple(T["dims"]) == L.dims64
        assert abs(float(T["threshold"]) - L.thr64) <= n * L.e_t
        assert np.array_equal(L.set32, L.set64) and np.array_equal(L.cset32, L.cset64)
        assert (int(T["n_voxels"]), int(T["n_centroids"])) == (int(L.set64.sum()), int(L.cset64.sum()))
        # each coordinate is three rounded operations on terms no larger than the level's boxes
        mag = max(np.abs(T["box_min"]).max(), np.abs(T["box_max"]).max(), np.abs(L.box64[0]).max(), np.abs(L.box64[1]).max())
        tol = 2 * float(np.spacing(np.float32(mag)))
        assert np.abs(T["box_min"] - L.box64[0]).max() <= tol and np.abs(T["box_max"] - L.box64[1]).max() <= tol
    assert np.array_equal(t.min, t.trace[-1]["box_min"]) and np.array_equal(t.max, t.trace[-1]["box_max"])
    # the voxel minimum and maximum run on across the levels
    assert np.all(np.diff(t.trace["voxel_min"]) <= 0) and np.all(np.diff(t.trace["voxel_max"]) >= 0)


def test_scene_properties():
    S = sc.voi_scenes()
    assert [len(S[n].keyframes) for n in ("kf1", "kf2_floor16000", "kf3_iter1", "kf65_circle", "kf129_chunk_plus_one")] == \
        [1, 2, 3, 65, sc.VOI_CHUNK + 1]
    assert S["kf3_iter1"].settings.iterations == 1 and S["kf1"].settings.iterations == 3
    assert S["kf2_floor16000"].settings.voxel_count_floor == 16000
    t, _, _ = analyse("floor64")
    assert int(np.prod(t.trace[0]["dims"])) >= 8 and 64 // 2 ** 3 == 8  # 8 voxels asked for at the coarsest of three levels
    t, _, _ = analyse("flat_box")
    d = t.trace[0]
    assert min(d["dims"]) == 1  # one diagonal of the first box is smaller than the side
    assert np.all(sc.voi_scene("one_place").keyframes == sc.voi_scene("one_place").keyframes[0])
    # a keyframe with depth -1 is passed through: its ModifiedDistanceAlphaToOmega is 0, its slope infinite, and it
    # scores exp(-inf) = 0 everywhere, in float as in fp64
    m = sc.voi_scene("depth_minus_one")
    assert (m.depths == -1).all(1).sum() == 1
    s = scene.teardrop_scores(m.settings, m.keyframes, m.depths, np.random.default_rng(0).uniform(-3, 3, (50, 3)))
    assert np.all(s[:, len(m.keyframes) // 2] == 0) and np.all(s.sum(1) > 0)


@pytest.mark.parametrize("name", [n for n in sc.VOI_NAMES if n not in sc.VOI_OK_NAMES])
def test_statuses(name):
    c = sc.voi_scene(name)
    t = scene.calculate_volume_of_interest(c.settings, c.keyframes, c.depths, backend="host", prefill=0xA5)
    assert t.status == c.status, scene.VOI_STATUS_NAMES[t.status]
    if name == "no_keyframes":
        # the reference returns false: the bounds and the trace keep their bytes
        assert t.levels_done == 0 and np.all(t.result["min"].view(np.uint8) == 0xA5) and np.all(t.result["max"].view(np.uint8) == 0xA5)
        assert np.all(t.trace.view(np.uint8) == 0xA5)
        assert scene.try_get_volume_of_interest(c.keyframes, c.depths, c.settings, backend="host") is None
        return
    box0 = scene.calculate_volume_of_interest(dataclasses.replace(c.settings, iterations=0), c.keyframes, c.depths, backend="host")
    if name == "floor4_degenerate":  # 4 / 2^3 = 0 voxels at the first level: the frustum box stays
        assert t.levels_done == 0 and np.array_equal(t.min, box0.min) and np.array_equal(t.max, box0.max)
        assert np.all(t.trace.view(np.uint8) == 0)
    if name == "threshold1_empty":
        # Threshold / lod = 1 at the last level only: the threshold is the maximum and nothing is above it
        assert t.levels_done == 2 and t.trace[2]["n_voxels"] == 0 and t.trace[2]["n_centroids"] == 0
        assert t.trace[2]["threshold"] == t.trace[2]["voxel_max"]
        assert np.array_equal(t.min, t.trace[1]["box_min"]) and np.array_equal(t.max, t.trace[1]["box_max"])
    assert scene.try_get_volume_of_interest(c.keyframes, c.depths, c.settings, backend="host") is not None


@pytest.mark.parametrize("name", ["kf3_iter1", "kf65_circle", "line", "one_place", "flat_box"])
def test_frustum_box_and_keyframe_scores_literal(name):
    """Float32 restatement, operation by operation: the box of the frusta equals the twin's exactly;
    the keyframe scores (the twin's own teardrop values summed in keyframe order by a literal loop)
    decide the voxel minimum / maximum and the centroids above the threshold exactly."""
    c = sc.voi_scene(name)
    cs = c.settings.to_c()
    K = sr.voi_keyframes(cs, c.keyframes, c.depths, np.float32)
    tiny, big = np.float32(np.finfo(np.float32).tiny), np.float32(np.finfo(np.float32).max)
    bmin, bmax = np.full(3, big), np.full(3, tiny)  # the maxima start at numeric_limits<float>::min()
    for k in range(len(c.keyframes)):
        for corner in K.corners[k]:
            bmin, bmax = np.minimum(bmin, corner), np.maximum(bmax, corner)
    t0 = scene.calculate_volume_of_interest(dataclasses.replace(c.settings, iterations=0), c.keyframes, c.depths, backend="host")
    assert t0.status == scene.VOI_OK and t0.levels_done == 0
    assert np.array_equal(t0.min, bmin) and np.array_equal(t0.max, bmax)
    pair = scene.teardrop_scores(cs, c.keyframes, c.depths, K.centroid)
    scores = []
    for a in range(len(c.keyframes)):
        v = np.float32(0)
        for b in range(len(c.keyframes)):
            v = np.float32(v + pair[a, b])
        scores.append(v)
    scores = np.array(scores, np.float32)
    # one level at its coarsest: few voxels, whose values are rebuilt the same way
    one = dataclasses.replace(c.settings, iterations=1, voxel_count_floor=16)
    t1 = scene.calculate_volume_of_interest(one, c.keyframes, c.depths, backend="host")
    L = t1.trace[0]
    idx = sr.voi_grid_points(np.zeros(3), 1.0, L["dims"]).astype(np.float32)
    pts = bmin[None] + idx * np.float32(L["side"])
    vox = sum_in_order(scene.teardrop_scores(cs, c.keyframes, c.depths, pts))
    allv = np.concatenate([scores, vox])
    assert L["voxel_min"] == allv.min() and L["voxel_max"] == max(allv.max(), tiny)
    assert int(L["n_centroids"]) == int((scores > L["threshold"]).sum()) and int(L["n_voxels"]) == int((vox > L["threshold"]).sum())


@pytest.mark.parametrize("field, value", [("iterations", -1), ("iterations", 31)])
def test_bad_settings(field, value):
    c = sc.voi_scene("kf3_iter1")
    with pytest.raises(_lib.MageError) as e:
        scene.calculate_volume_of_interest(dataclasses.replace(c.settings, **{field: value}), c.keyframes, c.depths, backend="host")
    assert e.value.status == _lib.MAGE_EINVAL
    cs = c.settings.to_c()
    cs.struct_size -= 4
    with pytest.raises(_lib.MageError):
        scene.calculate_volume_of_interest(cs, c.keyframes, c.depths, backend="host")


def test_settings_prepare():
    cs = scene.VolumeOfInterestSettings().to_c()
    yaw = np.float32(np.deg2rad(np.float32(5.0)))
    assert np.allclose(np.array(list(cs.kernel_rotation)).reshape(3, 3),
                       [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]], atol=1e-7)
    assert cs.tan_min_angle == pytest.approx(np.tan(np.deg2rad(40.0)), rel=1e-6)
    assert cs.tan_half_angle_x == pytest.approx(np.tan(np.deg2rad(30.0)), rel=1e-6)
    assert cs.tan_half_angle_y == pytest.approx(np.tan(np.deg2rad(20.0)), rel=1e-6)
    assert C.sizeof(cs) == 100 and _lib.VOI_RESULT_DTYPE.itemsize == 32 and _lib.VOI_LEVEL_DTYPE.itemsize == 60
