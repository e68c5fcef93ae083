"""mage_bounding_plane_depths_host's and mage_volume_of_interest_host's code under AddressSanitizer and UndefinedBehaviorSanitizer: the
twins' translation units are compiled into a stand-alone program (tests/cpp/scene_host_check.cpp, its
own main, no library, no GPU, nothing loaded into Python) with g++ -fsanitize=address,undefined, run
over three scenes with buffers of exactly the counts, and must exit clean with the library twin's bytes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import scene
from tests import scene_cases as sc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "scene_host_check.cpp"
CSRC = ROOT / "mageslam_amd" / "csrc"


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "mageslam_amd" / "_lib" / "scene_host_check_san"
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [SRC, ROOT / "include" / "mage_hot.h", CSRC / "scene_depth.cpp", CSRC / "scene_voi.cpp", *CSRC.glob("*.hpp")]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out)], check=True)
    return out


# ranks inside a list with equal depths, keypoint indices outside the frame's keypoints, and a frame
# one point over its cap (its sparse buffer holds cap records and none may be written)
@pytest.mark.parametrize("name", ["soft_025_01", "bad_index", "cap_plus_one"])
def test_twin_runs_clean_under_sanitizers(exe, tmp_path, name):
    c = sc.depth_scene(name)
    f = c.frame
    n = len(f.map_xyzi)
    cap = n if c.cap is None else c.cap
    h = scene.calculate_bounding_plane_depths(c.settings, f, backend="host", cap=cap)
    hdr = np.array([f.width, f.height, len(f.kp), n, cap], np.uint32)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(bytes(c.settings.to_c()) + hdr.tobytes() + f.pos3.tobytes() + f.r9.tobytes() + f.intr4.tobytes() +
                    f.kp.tobytes() + f.map_xyzi.tobytes() + f.kp_index.tobytes())
    # the sanitizer runtimes are linked statically: the program does not depend on what else the
    # environment loads into a process, and the environment is passed on as it is
    p = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr
    got = fout.read_bytes()
    assert len(got) == 20 + 16 * len(h.sparse)
    assert (name == "cap_plus_one") == (len(h.sparse) == 0)
    # the library is built -O3 and this program -O1 with another compiler: the same bits all the same
    assert got == h.result.tobytes() + h.sparse.tobytes()


# a single keyframe, every centroid on the others' view axes (the clamp), all keyframes at one place
# (scores of exactly 1), a level without voxels (DEGENERATE) and no keyframes at all
@pytest.mark.parametrize("name", ["kf1", "line", "one_place", "floor4_degenerate", "no_keyframes"])
def test_voi_twin_runs_clean_under_sanitizers(exe, tmp_path, name):
    c = sc.voi_scene(name)
    h = scene.calculate_volume_of_interest(c.settings, c.keyframes, c.depths, backend="host", prefill=0xA5)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(bytes(c.settings.to_c()) + np.array([len(c.keyframes)], np.uint32).tobytes() + c.keyframes.tobytes() +
                    c.depths.tobytes())
    p = subprocess.run([str(exe), "voi", str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr
    assert fout.read_bytes() == h.result.tobytes() + h.trace.tobytes()
