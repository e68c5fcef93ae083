"""mage::hot::MonoMapInit::InitializeWithFrames (include/mage/mage.hpp) compiles against include/
and gives what the Python binding gives: the CPU backend here, the kernels with and without the
matcher on a GPU; it throws where the reference asserts."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import mono
from tests import mono_init_cases as mc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "mono_init_demo.cpp"


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "mono_init_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, c, device, descriptors, matches=None):
    matches = c.matches if matches is None else matches
    raw = tmp_path / f"{c.name}.bin"
    with open(raw, "wb") as f:
        f.write(np.array([len(c.kp0), len(c.kp1), 0 if descriptors else len(matches), device + 1, int(descriptors),
                          c.settings.min_feature_matches], np.uint32).tobytes())
        f.write(mc.INTR.tobytes())
        for kp, desc in ((c.kp0, c.desc0), (c.kp1, c.desc1)):
            f.write(kp.tobytes())
            if descriptors:
                f.write(desc.tobytes())
        if not descriptors:
            f.write(matches.tobytes())
    outf = tmp_path / f"{c.name}.out"
    r = subprocess.run([str(build_demo()), str(raw), str(outf)], capture_output=True, text=True)
    return r, outf


def expected(h):
    e = h.result.tobytes() + np.array([len(h.matches), len(h.points)], np.uint32).tobytes() + h.matches.tobytes()
    if h.verdict == mono.OK:
        e += (h.pos3[1].tobytes() + h.r9[1].tobytes() + h.points.tobytes() + h.ba_points.tobytes() + h.ba_uv.tobytes() +
              h.ba_cam.tobytes() + h.ba_pt.tobytes() + h.ba_info.tobytes())
    return e


def host(c, matches=None):
    return mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=c.matches if matches is None else matches,
                                       backend="host")


@pytest.mark.parametrize("name", ["clean64", "outliers128", "few40", "tiny_baseline"])
def test_facade_cpu_backend(tmp_path, name):
    c = mc.case(name)
    r, outf = run_demo(tmp_path, c, -1, False)
    assert r.returncode == 0, r.stderr
    h = host(c)
    assert (h.verdict == mono.OK) == (name in ("clean64", "outliers128"))
    assert outf.read_bytes() == expected(h)


def test_facade_throws_where_the_reference_asserts(tmp_path):
    c = mc.case("clean64")
    bad = c.matches.copy()
    bad["query_idx"][3] = -1
    r, _ = run_demo(tmp_path, c, -1, False, matches=bad)
    assert r.returncode == 5, (r.returncode, r.stderr)
    r, _ = run_demo(tmp_path, mc.over_limit_case(), -1, False)
    assert r.returncode == 6, (r.returncode, r.stderr)
    # the CPU backend has no matcher
    r, _ = run_demo(tmp_path, mc.matcher_case(), -1, True)
    assert r.returncode != 0 and "descriptor" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("descriptors", [False, True])
def test_facade_kernel(gpu, tmp_path, descriptors):
    c = mc.matcher_case() if descriptors else mc.case("clean128")
    r, outf = run_demo(tmp_path, c, 0, descriptors)
    assert r.returncode == 0, r.stderr
    if descriptors:
        from mageslam_amd import matcher

        m0, m1 = mc.octave0_masks(c)
        h = host(c, matcher.Match(c.desc0, c.desc1, m0, m1, 30, 1))
    else:
        h = host(c)
    assert h.verdict == mono.OK and len(h.points) == 128
    assert outf.read_bytes() == expected(h)
