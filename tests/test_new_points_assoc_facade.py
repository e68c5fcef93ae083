"""mage::hot::LocallyAssociateNewAssociations (include/mage/mage.hpp) and
mage::hot::NewMapPointsCreation compile against include/ and give what the Python binding gives: the
CPU backend here, the kernel on a GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import mapping
from tests import new_points_assoc_cases as ac

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "new_points_assoc_demo.cpp"


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "new_points_assoc_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, c, device, creation=None):
    """`creation`: (ki, matches per keyframe, max_grid_count) — the demo then runs NewMapPointsCreation."""
    raw = tmp_path / f"{c.name}.bin"
    a = c.assoc
    with open(raw, "wb") as f:
        f.write(np.array([len(c.points), len(c.ki_desc), len(c.kfs), device + 1, c.settings.num_levels],
                         np.uint32).tobytes())
        f.write(np.array([a.search_radius, a.max_keyframe_angle_degrees, a.image_border], np.float32).tobytes())
        f.write(np.array([a.max_hamming_distance, a.min_hamming_difference], np.int32).tobytes())
        f.write(c.points.tobytes() + c.ki_desc.tobytes())
        for kf in c.kfs:
            f.write(np.concatenate([kf.pos3, kf.r9, kf.intr4]).astype(np.float32).tobytes())
            f.write(np.int32(kf.slot).tobytes() + np.uint32(len(kf.kp)).tobytes())
            f.write(kf.kp.tobytes() + kf.desc.tobytes() + kf.mask.astype(np.uint8).tobytes())
        if creation:
            ki, matches, grid_cap = creation
            f.write(np.concatenate([ki.pos3, ki.r9, ki.intr4]).astype(np.float32).tobytes())
            f.write(ki.keypoints.tobytes() + np.array([grid_cap, 1], np.uint32).tobytes())
            f.write(np.asarray(ki.associated, np.uint8).tobytes())
            for m in matches:
                f.write(np.uint32(len(m)).tobytes() + m.tobytes())
    outf = tmp_path / f"{c.name}.out"
    r = subprocess.run([str(build_demo()), str(raw), str(outf)] + (["creation"] if creation else []),
                       capture_output=True, text=True)
    return r, outf


def check_output(c, outf):
    rec, v, masks, status = mapping.new_points_associate(*c.args(), backend="host")
    assert status == 0 and (v == ac.ASSOCIATED).sum() > 0
    data = outf.read_bytes()
    n = rec.size
    assert data[: 16 * n] == rec.tobytes()
    assert data[16 * n: 17 * n] == v.tobytes()
    assert data[17 * n:] == b"".join(m.astype(np.uint8).tobytes() for m in masks)


@pytest.mark.parametrize("name", ["contend", "levels4"])
def test_facade_cpu_backend(tmp_path, name):
    c = ac.cases()[name]
    r, outf = run_demo(tmp_path, c, -1)
    assert r.returncode == 0, r.stderr
    check_output(c, outf)


def test_facade_reports_no_device(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, _ = run_demo(tmp_path, ac.cases()["contend"], 0)
    assert r.returncode == 3, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_facade_kernel(gpu, tmp_path):
    c = ac.cases()["base"]
    r, outf = run_demo(tmp_path, c, 0)
    assert r.returncode == 0, r.stderr
    check_output(c, outf)


def creation_problem():
    """The composition scene in the facade's terms: the covisible keyframes in the sorted order, the
    IndexedMatch results of the keyframes CreateInitialAssociations uses (empty for the others), and
    what mapping.new_map_points_creation makes of it on the CPU backend."""
    ki, cov, matcher, s, a = ac.composition_scene()
    want = mapping.new_map_points_creation(ki, cov, s, a, backend="host", matcher=matcher)
    kfs = [ac.Kf(cov[i].pos3, cov[i].r9, cov[i].intr4, cov[i].keypoints, cov[i].descriptors, ~cov[i].associated, -1)
           for i in want.order]
    matches = [want.initial.matches[want.initial.frames.index(i)] if i in want.initial.frames
               else np.zeros(0, want.initial.matches[0].dtype) for i in want.order]
    c = ac.Case("creation", s, a, np.zeros(0, want.initial.points.dtype), ki.descriptors, kfs)
    return c, (ki, matches, s.max_grid_count), want


def check_creation(outf, want):
    data = outf.read_bytes()
    n = int(np.frombuffer(data[:4], np.uint32)[0])
    assert n == len(want.points) > 20
    pos = 4
    pair = np.dtype([("keyframe", "<i4"), ("keypoint", "<u4")])
    where = {i: k for k, i in enumerate(want.order)}  # the facade counts keyframes in the order it was given
    for m in want.points:
        assert data[pos:pos + 48] == m.point.tobytes()
        na = int(np.frombuffer(data[pos + 48:pos + 52], np.uint32)[0])
        got = np.frombuffer(data[pos + 52:pos + 52 + 8 * na], pair)
        assert [(int(g["keyframe"]), int(g["keypoint"])) for g in got] == [
            (-1 if i < 0 else where[i], t) for i, t in m.keyframes]
        pos += 52 + 8 * na
    assert sum(1 for m in want.points if len(m.keyframes) >= 3) >= n // 2
    assert data[pos:] == b"".join(m.astype(np.uint8).tobytes() for m in want.local.masks)


def test_facade_creation_cpu_backend(tmp_path):
    c, creation, want = creation_problem()
    r, outf = run_demo(tmp_path, c, -1, creation)
    assert r.returncode == 0, r.stderr
    check_creation(outf, want)


@pytest.mark.gpu
def test_facade_creation_kernel(gpu, tmp_path):
    c, creation, want = creation_problem()
    r, outf = run_demo(tmp_path, c, 0, creation)
    assert r.returncode == 0, r.stderr
    check_creation(outf, want)
