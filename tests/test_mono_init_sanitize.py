"""mage_mono_init_two_view_host's code under AddressSanitizer and UndefinedBehaviorSanitizer: the
twin's translation unit is compiled into a stand-alone program (tests/cpp/mono_init_host_check.cpp,
its own main, no library, no GPU, nothing loaded into Python) with g++ -fsanitize=address,undefined,
run over three cases, and must exit clean with the library twin's bytes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import mono
from mageslam_amd._lib import MI_RESULT_DTYPE, SP_DTYPE
from tests import mono_init_cases as mc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "mono_init_host_check.cpp"
CSRC = ROOT / "mageslam_amd" / "csrc"


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "mageslam_amd" / "_lib" / "mono_init_host_check_san"
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [SRC, ROOT / "include" / "mage_hot.h", CSRC / "monoinit.cpp", *CSRC.glob("*.hpp")]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}",
                        f"-I{ROOT / 'include'}", str(SRC), "-o", str(out)], check=True)
    return out


@pytest.mark.parametrize("name", ["clean128", "outliers128", "clustered"])
def test_twin_runs_clean_under_sanitizers(exe, tmp_path, name):
    c = mc.case(name)
    cs = c.settings.to_c()
    cap = len(c.matches)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(bytes(cs) + mc.INTR.tobytes() +
                    np.array([len(c.kp0), len(c.kp1), len(c.matches), cap], np.uint32).tobytes() +
                    c.kp0.tobytes() + c.kp1.tobytes() + c.matches.tobytes())
    # the sanitizer runtimes are linked statically: the program does not depend on what else the
    # environment loads into a process, and the environment is passed on as it is
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    h = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=c.matches, backend="host",
                                    want_trace=True)
    n = len(h.points)
    expect = (h.result.tobytes() + h.points.tobytes() + h.ba_points.tobytes() + h.ba_uv.tobytes() + h.ba_cam.tobytes() +
              h.ba_pt.tobytes() + h.ba_info.tobytes() + h.trace.tobytes())
    got = fout.read_bytes()
    assert len(got) == MI_RESULT_DTYPE.itemsize + n * (SP_DTYPE.itemsize + 12 + 16 + 8 + 8 + 8) + h.trace.nbytes
    # the library is built -O3 and this program -O1 with another compiler: the same bits all the same
    assert got == expect
