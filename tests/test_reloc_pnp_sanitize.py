"""mage_reloc_pnp_host's code under AddressSanitizer and UndefinedBehaviorSanitizer: the twin's
translation unit is compiled into a stand-alone program (tests/cpp/reloc_pnp_host_check.cpp, its own
main, no library, no GPU, nothing loaded into Python) with g++ -fsanitize=address,undefined, run over
three cases, and must exit clean with the library twin's bytes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd._lib import RP_RESULT_DTYPE
from tests import reloc_pnp_cases as rc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "reloc_pnp_host_check.cpp"
CSRC = ROOT / "mageslam_amd" / "csrc"


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "mageslam_amd" / "_lib" / "reloc_pnp_host_check_san"
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [SRC, ROOT / "include" / "mage_hot.h", CSRC / "reloc_pnp.cpp", *CSRC.glob("*.hpp")]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out)], check=True)
    return out


@pytest.mark.parametrize("name", ["n5", "mix40_i65", "behind60"])
def test_twin_runs_clean_under_sanitizers(exe, tmp_path, name):
    c = rc.case(name)
    cs = c.settings.to_c()
    cap = len(c.matches)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(bytes(cs) + rc.INTR.tobytes() +
                    np.array([len(c.map_xyzi), len(c.kp), len(c.matches), cap], np.uint32).tobytes() +
                    c.map_xyzi.tobytes() + c.kp.tobytes() + c.matches.tobytes())
    # the sanitizer runtimes are linked statically: the program does not depend on what else the
    # environment loads into a process, and the environment is passed on as it is
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    h = rc.twin(name)
    expect = (h.result.tobytes() + h.inliers.tobytes() + h.points3.tobytes() + h.uv.tobytes() + h.info.tobytes() +
              h.trace.tobytes())
    got = fout.read_bytes()
    assert len(got) == RP_RESULT_DTYPE.itemsize + len(h.inliers) * (4 + 12 + 8 + 4) + h.trace.nbytes
    # the library is built -O3 and this program -O1 with another compiler: the same bits all the same
    assert got == expect
