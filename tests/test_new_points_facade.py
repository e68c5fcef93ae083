"""mage::hot::CreateInitialAssociations (include/mage/mage.hpp) compiles against include/ and gives
what the Python binding gives: the CPU backend here, the kernel on a GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import mapping
from tests import new_points_cases as nc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "new_points_demo.cpp"


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "new_points_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, p, device):
    raw = tmp_path / f"{p.name}.bin"
    with open(raw, "wb") as f:
        f.write(np.array([len(p.ki_kp), len(p.kc_kp), p.ki_assoc is not None, device + 1], np.uint32).tobytes())
        f.write(np.concatenate([p.ki_pos3, p.ki_r9, p.ki_intr4]).astype(np.float32).tobytes())
        f.write(p.ki_kp.tobytes())
        if p.ki_assoc is not None:
            f.write(p.ki_assoc.astype(np.uint8).tobytes())
        for k in range(len(p.kc_kp)):
            f.write(np.concatenate([p.kc_pos3[k], p.kc_r9[k], p.kc_intr4[k]]).astype(np.float32).tobytes())
            f.write(np.uint32(len(p.kc_kp[k])).tobytes() + p.kc_kp[k].tobytes())
            f.write(np.uint32(len(p.matches[k])).tobytes() + p.matches[k].tobytes())
    outf = tmp_path / f"{p.name}.out"
    r = subprocess.run([str(build_demo()), str(raw), str(outf)], capture_output=True, text=True)
    return r, outf


def check_output(p, outf):
    h = mapping.new_map_points(p.settings, *p.args(), backend="host")
    data = outf.read_bytes()
    n = int(np.frombuffer(data[:4], np.uint32)[0])
    assert n == len(h.points) > 0
    assert data[4:4 + 48 * n] == h.points.tobytes()
    assert np.array_equal(np.frombuffer(data[4 + 48 * n:], np.uint8), np.concatenate(h.verdicts))


@pytest.mark.parametrize("name", ["taken", "grid_start"])
def test_facade_cpu_backend(tmp_path, name):
    p = nc.cases()[name]
    r, outf = run_demo(tmp_path, p, -1)
    assert r.returncode == 0, r.stderr
    check_output(p, outf)


def test_facade_reports_no_device(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, _ = run_demo(tmp_path, nc.cases()["taken"], 0)
    assert r.returncode == 3, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_facade_kernel(gpu, tmp_path):
    p = nc.cases()["grid_start"]
    r, outf = run_demo(tmp_path, p, 0)
    assert r.returncode == 0, r.stderr
    check_output(p, outf)
