"""mage_reloc_guided_host's code under AddressSanitizer and UndefinedBehaviorSanitizer: the twin's
translation unit is compiled into a stand-alone program (tests/cpp/reloc_guided_host_check.cpp, its
own main, no library, no GPU, nothing loaded into Python) with g++ -fsanitize=address,undefined, run
over three cases with buffers of exactly the counts, and must exit clean with the library twin's bytes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd._lib import DM_DTYPE, RG_RESULT_DTYPE
from tests import reloc_guided_cases as gc
from tests import reloc_guided_ref as gr

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "reloc_guided_host_check.cpp"
CSRC = ROOT / "mageslam_amd" / "csrc"


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "mageslam_amd" / "_lib" / "reloc_guided_host_check_san"
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [SRC, ROOT / "include" / "mage_hot.h", CSRC / "reloc_guided.cpp", *CSRC.glob("*.hpp")]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out)], check=True)
    return out


# a natural scene with an order list through all three phases, the scene at the gate values, the
# one that stops at the MinMapPoints gate with depth-zero points removed
@pytest.mark.parametrize("name", ["n257_order", "gates_exact", "short_points"])
def test_twin_runs_clean_under_sanitizers(exe, tmp_path, name):
    s, r = gc.scene(name), gr.run(name, 0)
    cand, h = s.cands[0], r.final
    cs = s.settings.to_c()
    nq = int(r.g1.result["n_queries"])
    cap = max(nq, 1)  # exactly the queries: one more write would be past the allocation
    order = cand.order if cand.order is not None else np.zeros(0, np.int32)
    rm = r.rm if r.rm is not None else np.zeros(0, DM_DTYPE)
    flags = r.second[2] if r.second is not None else np.zeros(0, np.uint8)
    second = np.concatenate(r.second[:2]) if r.second is not None else np.zeros(12, np.float32)
    hdr = np.array([int(r.ok), len(cand.kp), cand.order is not None, len(order), len(s.kp), cap, r.rm is not None, len(rm),
                    r.second is not None, len(flags)], np.uint32)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(bytes(cs) + hdr.tobytes() + gc.INTR.tobytes() + np.concatenate(r.first).astype(np.float32).tobytes() +
                    second.astype(np.float32).tobytes() + cand.map_xyzi.tobytes() + cand.kp.tobytes() + cand.desc.tobytes() +
                    order.tobytes() + s.kp.tobytes() + rm.tobytes() + flags.tobytes())
    # the sanitizer runtimes are linked statically: the program does not depend on what else the
    # environment loads into a process, and the environment is passed on as it is
    p = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr
    expect = (h.result.tobytes() + h.query_kp.tobytes() + h.query_pos.tobytes() + h.query_desc.tobytes() +
              h.query_ref.tobytes() + h.assoc.tobytes() + h.ba_points3.tobytes() + h.ba_uv.tobytes() + h.ba_info.tobytes())
    got = fout.read_bytes()
    n = len(h.assoc)
    assert len(got) == RG_RESULT_DTYPE.itemsize + nq * (28 + 8 + 32 + 4) + 8 * n + len(h.ba_info) * (12 + 8 + 4)
    # the library is built -O3 and this program -O1 with another compiler: the same bits all the same
    assert got == expect
