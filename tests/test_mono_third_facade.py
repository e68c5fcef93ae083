"""mage::hot::MonoMapInit::LocateThirdFrame (include/mage/mage.hpp) compiles against include/ and gives
what the Python binding gives: the CPU backend here (with and without the bundle adjustment's
outcome), the kernels on a GPU; it throws where the reference would read out of bounds."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import mono
from tests import mono_third_cases as tc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "mono_third_demo.cpp"


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "mono_third_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, c, device, ba=None):
    raw = tmp_path / f"{c.name}.bin"
    with open(raw, "wb") as f:
        f.write(np.array([len(c.points), len(c.desc0), len(c.desc1), len(c.kp2), device + 1,
                          0 if ba is None else len(ba[0]) + 1], np.uint32).tobytes())
        for a in (tc.INTR, c.pos3, c.r9, c.points, c.idx0, c.idx1, c.desc0, c.desc1, c.kp2, c.desc2):
            f.write(np.ascontiguousarray(a).tobytes())
        if ba is not None:
            f.write(np.ascontiguousarray(ba[0], np.uint8).tobytes() + np.asarray(ba[1], np.float32).tobytes() +
                    np.asarray(ba[2], np.float32).tobytes() + np.float32(ba[3]).tobytes())
    outf = tmp_path / f"{c.name}.out"
    r = subprocess.run([str(build_demo()), str(raw), str(outf)], capture_output=True, text=True)
    return r, outf


def expected(h, finished):
    e = h.result.tobytes()
    if h.verdict == mono.M3_OK:
        na = len(h.obs_pt) if finished else 0
        e += (np.uint32(na).tobytes() + h.pos3.tobytes() + h.r9.tobytes() + h.keypoint.tobytes() + h.point_verdict.tobytes() +
              h.dist.tobytes() + h.proj.tobytes() + h.mask.astype(np.uint8).tobytes())
        if finished:
            e += h.obs_uv.tobytes() + h.obs_pt.tobytes() + h.obs_cam.tobytes() + h.obs_info.tobytes()
    return e


DEFAULT = [n for n, c in tc.cases().items() if c.settings == mono.MonoMapInitializationSettings()]


@pytest.mark.parametrize("name", ["n65", "rules", "gate_short", "behind"])
def test_facade_cpu_backend_first_half(tmp_path, name):
    assert name in DEFAULT
    c = tc.case(name)
    r, outf = run_demo(tmp_path, c, -1)
    assert r.returncode == 0, r.stderr
    h = mono.locate_third_frame(*c.args(), backend="host")
    assert (h.verdict == mono.M3_OK) == (name != "gate_short")
    assert outf.read_bytes() == expected(h, False)


@pytest.mark.parametrize("name", ["decoys", "cull_tips"])
def test_facade_cpu_backend_with_outcome(tmp_path, name):
    c = tc.case(name)
    h = mono.locate_third_frame(*c.args(), backend="host")
    flags = np.zeros(int(h.result["n_matched"]), np.uint8)
    flags[-3:] = 1  # the decoys come last among the matched points
    ba = (flags, np.array([0.1, 0.2, 0.3]), np.eye(3).reshape(9), 0.75)
    r, outf = run_demo(tmp_path, c, -1, ba)
    assert r.returncode == 0, r.stderr
    t = mono.locate_third_frame(*c.args(), backend="host", outlier=ba[0], opt_pos3=ba[1], opt_r9=ba[2], mean_sq=ba[3])
    assert t.verdict == (mono.M3_OK if name == "decoys" else mono.M3_FEW_AFTER_CULL)
    assert int(t.result["n_outliers"]) == 3 and float(t.result["mean_sq"]) == 0.75
    assert outf.read_bytes() == expected(t, True)


def test_facade_throws_where_the_reference_would_read_out_of_bounds(tmp_path):
    r, _ = run_demo(tmp_path, tc.case("bad_idx1"), -1)
    assert r.returncode == 5, (r.returncode, r.stderr)
    r, _ = run_demo(tmp_path, tc.case("kp4097"), -1)
    assert r.returncode == 6, (r.returncode, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n257", "decoys"])
def test_facade_kernel(gpu, tmp_path, name):
    c = tc.case(name)
    r, outf = run_demo(tmp_path, c, 0)
    assert r.returncode == 0, r.stderr
    g = mono.locate_third_frame(*c.args(), backend="gpu")
    assert g.verdict == mono.M3_OK and int(g.result["n_outliers"]) == (3 if name == "decoys" else 0)
    assert outf.read_bytes() == expected(g, True)
