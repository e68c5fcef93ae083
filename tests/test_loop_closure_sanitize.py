"""mage_cheap_loop_closure_host's code under AddressSanitizer and UndefinedBehaviorSanitizer: the
twin's translation unit is compiled into a stand-alone program (tests/cpp/loop_closure_host_check.cpp,
its own main, no library, no GPU, nothing loaded into Python) with g++ -fsanitize=address,undefined,
run over three cases with buffers of exactly the counts, and must exit clean with the library twin's
bytes.  The same program checks the kernels' sampling arithmetic against the reference's counter loop."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import loopclosure as lcm
from tests import loop_closure_cases as lc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "loop_closure_host_check.cpp"
CSRC = ROOT / "mageslam_amd" / "csrc"


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "mageslam_amd" / "_lib" / "loop_closure_host_check_san"
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [SRC, ROOT / "include" / "mage_hot.h", CSRC / "loopclose.cpp", *CSRC.glob("*.hpp")]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out)], check=True)
    return out


# a second round of 64 in the take, a pitch one short (refused before anything is written) and a
# keyframe of 4097 keypoints between two normal ones
@pytest.mark.parametrize("name", ["two_rounds", "obs_full", "many_kp"])
def test_twin_runs_clean_under_sanitizers(exe, tmp_path, name):
    c = lc.cases()[name]
    p, s = c.problem, c.settings
    h = lcm.cheap_loop_closure_and_connect(s, p, backend="host", prefill=0xA5)
    L = int(h.counts[0])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(lc.input_bytes(c, L))
    # the sanitizer runtimes are linked statically: the program does not depend on what else the
    # environment loads into a process, and the environment is passed on as it is
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    want = (np.array([5 if h.refused else 0, *h.counts, h.status], np.uint32).tobytes() + h.state.tobytes() + h.obs.tobytes() +
            h.sample_index[:L].tobytes() + h.closure[:L].tobytes() + h.closure_verdict[:L].tobytes() +
            np.ascontiguousarray(h.connect[:L]).tobytes() + np.ascontiguousarray(h.connect_verdict[:L]).tobytes() +
            h.ki_mask.tobytes() + b"".join(m.tobytes() for m in h.kf_masks) + h.kf_modified.tobytes())
    # the library is built -O3 and this program -O1 with another compiler: the same bits all the same
    assert fout.read_bytes() == want
    assert (name == "obs_full") == h.refused and (name == "many_kp") == bool(h.status & lcm.STATUS_OVER_LIMIT)


def test_sampling_arithmetic_equals_the_counter_loop(exe):
    r = subprocess.run([str(exe), "sampler"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
