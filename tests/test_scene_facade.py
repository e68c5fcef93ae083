"""BoundingDepthSettings and mage::hot::CalculateBoundingPlaneDepthsForKeyframe
(include/mage/mage.hpp): the defaults are the reference's, and the C++ facade compiled against
include/ gives the Python module's bytes, the twin's on the CPU backend and the kernel's on a GPU."""
import ctypes as C
import dataclasses
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import _lib, scene
from tests import scene_cases as sc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "scene_demo.cpp"

# MageSettings.h:216-223, in the reference's order
REFERENCE_DEFAULTS = [("RegionOfInterestMinX", 0.1), ("RegionOfInterestMinY", 0.1), ("RegionOfInterestMaxX", 0.9),
                      ("RegionOfInterestMaxY", 0.9), ("NearDepthSoftness", 0.0), ("FarDepthSoftness", 0.0)]


def snake(name):
    return re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower()


def test_settings_defaults_and_order():
    s = scene.BoundingDepthSettings()
    fields = [f.name for f in dataclasses.fields(s)]
    assert fields == [snake(n) for n, _ in REFERENCE_DEFAULTS]
    for (_, v), f in zip(REFERENCE_DEFAULTS, fields):
        assert getattr(s, f) == pytest.approx(v)
    cs = s.to_c()
    assert [n for n, _ in cs._fields_] == ["struct_size"] + fields
    assert cs.struct_size == C.sizeof(cs) == 28
    assert _lib.BD_RESULT_DTYPE.itemsize == 20 and _lib.PP_DTYPE.itemsize == 16
    # the C++ facade's defaults are the same text
    hpp = (ROOT / "include" / "mage" / "mage.hpp").read_text()
    body = hpp[hpp.index("struct BoundingDepthSettings {"):hpp.index("mage_bounding_depth_settings ToC() const")]
    for n, v in REFERENCE_DEFAULTS:
        m = re.search(rf"\b{n}\{{([0-9.]+)f?\}}", body)
        assert m and float(m.group(1)) == pytest.approx(v), n


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "scene_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, name, device):
    c = sc.depth_scene(name)
    f, s = c.frame, c.settings
    raw, outf = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    raw.write_bytes(np.array([len(f.kp), len(f.map_xyzi), f.width, f.height, device + 1], np.uint32).tobytes() +
                    np.array(dataclasses.astuple(s), np.float32).tobytes() + f.pos3.tobytes() + f.r9.tobytes() +
                    f.intr4.tobytes() + f.kp.tobytes() + f.map_xyzi.tobytes() + f.kp_index.tobytes())
    return subprocess.run([str(build_demo()), str(raw), str(outf)], capture_output=True, text=True), outf


def expected(name, backend):
    c = sc.depth_scene(name)
    d = scene.calculate_bounding_plane_depths(c.settings, c.frame, backend=backend)
    return np.array([d.near, d.far], np.float32).tobytes() + d.result.tobytes() + d.sparse.tobytes()


@pytest.mark.parametrize("name", ["n0", "all_outside", "soft_025_01", "depth_zero", "nonpositive"])
def test_facade_cpu_backend(tmp_path, name):
    r, outf = run_demo(tmp_path, name, -1)
    assert r.returncode == 0, r.stderr
    assert outf.read_bytes() == expected(name, "host")


def test_facade_throws_for_a_bad_index(tmp_path):
    r, _ = run_demo(tmp_path, "bad_index", -1)
    assert r.returncode == 5, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_facade_kernel(gpu, tmp_path):
    r, outf = run_demo(tmp_path, "soft_025_01", 0)
    assert r.returncode == 0, r.stderr
    assert outf.read_bytes() == expected("soft_025_01", "host")


# ------------------------------------------------------------------------------------------------
# mage::hot::CalculateVolumeOfInterest

VOI_SRC = ROOT / "tests" / "cpp" / "scene_voi_demo.cpp"
# MageSettings.h:290-307
VOI_REFERENCE_DEFAULTS = [("Threshold", 0.5), ("Iterations", 3), ("VoxelCountFloor", 16000), ("AwayProminence", 1.2),
                          ("TowardProminence", 0.1), ("SideProminence", 1.0), ("KernelAngleXRads", np.deg2rad(60.0)),
                          ("KernelAngleYRads", np.deg2rad(40.0)), ("KernelPitchRads", 0.0), ("KernelRollRads", 0.0),
                          ("KernelYawRads", np.deg2rad(5.0)), ("KernelDepthModifier", 1.0)]


def test_voi_settings_defaults_and_order():
    s = scene.VolumeOfInterestSettings()
    fields = [f.name for f in dataclasses.fields(s)]
    assert fields == [snake(n) for n, _ in VOI_REFERENCE_DEFAULTS]
    for (_, v), f in zip(VOI_REFERENCE_DEFAULTS, fields):
        assert getattr(s, f) == pytest.approx(v)
    assert [n for n, _ in s.to_c()._fields_][:13] == ["struct_size"] + fields
    hpp = (ROOT / "include" / "mage" / "mage.hpp").read_text()
    body = hpp[hpp.index("struct VolumeOfInterestSettings {"):hpp.index("mage_voi_settings ToC() const")]
    for n, v in VOI_REFERENCE_DEFAULTS:
        m = re.search(rf"\b{n}\{{([0-9.]+)f?\}}", body)
        assert m and float(m.group(1)) == pytest.approx(v, rel=1e-6), n


def build_voi_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "scene_voi_demo"
    if not out.exists() or out.stat().st_mtime < max(VOI_SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(VOI_SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_voi_demo(tmp_path, name, device):
    c = sc.voi_scene(name)
    s = c.settings
    raw, outf = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    fl = [s.threshold, s.away_prominence, s.toward_prominence, s.side_prominence, s.kernel_angle_x_rads, s.kernel_angle_y_rads,
          s.kernel_pitch_rads, s.kernel_roll_rads, s.kernel_yaw_rads, s.kernel_depth_modifier]
    rows = np.concatenate([c.keyframes.reshape(-1, 12), c.depths.reshape(-1, 2)], 1).astype(np.float32)
    raw.write_bytes(np.array([len(c.keyframes), device + 1], np.uint32).tobytes() +
                    np.array([s.iterations, s.voxel_count_floor], np.int32).tobytes() + np.array(fl, np.float32).tobytes() +
                    rows.tobytes())
    return subprocess.run([str(build_voi_demo()), str(raw), str(outf)], capture_output=True, text=True), outf


def voi_expected(name):
    c = sc.voi_scene(name)
    v = scene.calculate_volume_of_interest(c.settings, c.keyframes, c.depths, backend="host")
    none = v.status == scene.VOI_NO_KEYFRAMES
    box = np.full(6, 7.0, np.float32) if none else np.concatenate([v.min, v.max])
    return (np.array([not none, v.status, v.levels_done], np.uint32).tobytes() + box.tobytes() +
            (b"" if none else v.trace.tobytes()))


@pytest.mark.parametrize("name", ["kf3_iter1", "line", "floor4_degenerate", "threshold1_empty", "no_keyframes"])
def test_voi_facade_cpu_backend(tmp_path, name):
    r, outf = run_voi_demo(tmp_path, name, -1)
    assert r.returncode == 0, r.stderr
    assert outf.read_bytes() == voi_expected(name)


@pytest.mark.gpu
def test_voi_facade_kernel(gpu, tmp_path):
    r, outf = run_voi_demo(tmp_path, "line", 0)
    assert r.returncode == 0, r.stderr
    assert outf.read_bytes() == voi_expected("line")
