"""CheapLoopClosureSettings, mage::hot::CheapLoopClosureAndConnect and UpdateMapPoint
(include/mage/mage.hpp): the defaults are the reference's, and the C++ facade compiled against
include/ gives the Python module's results, the twin's on the CPU backend and the kernels' on a GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import loopclosure as lcm
from tests import loop_closure_cases as lc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "loop_closure_demo.cpp"

# MageSettings.h:197-207 (LoopClosureSettings and its CheapLoopClosureMatchingSettings), :181, :36-39
REFERENCE_DEFAULTS = [("MaxMapPoints", "max_map_points", 200), ("MinKeyframe", "min_keyframes", 10),
                      ("MatchSearchRadius", "search_radius", 18.0),
                      ("MinDegreesBetweenCurrentViewAndMapPointView", "min_view_degrees", 60.0),
                      ("CheapLoopClosureMaxHammingDistance", "closure_max_hamming_distance", 30),
                      ("CheapLoopClosureMinHammingDifference", "closure_min_hamming_difference", 1),
                      ("ConnectMaxHammingDistance", "connect_max_hamming_distance", 30),
                      ("ConnectMinHammingDifference", "connect_min_hamming_difference", 1)]


def test_settings_defaults():
    s = lcm.LoopClosureSettings()
    hpp = (ROOT / "include" / "mage" / "mage.hpp").read_text()
    body = hpp[hpp.index("struct CheapLoopClosureSettings {"):hpp.index("mage_loop_closure_settings ToC() const")]
    for cpp, py, v in REFERENCE_DEFAULTS:
        assert getattr(s, py) == v
        m = re.search(rf"\b{cpp}\{{([0-9.]+)f?\}}", body)
        assert m and float(m.group(1)) == v, cpp


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "loop_closure_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, name, device):
    raw, outf = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    raw.write_bytes(lc.input_bytes(lc.cases()[name], 0))
    return subprocess.run([str(build_demo()), str(raw), str(outf), str(device)], capture_output=True, text=True), outf


def expected(name):
    """The facade's output file from the Python module on the host backend.  The facade sizes the
    observation pitch itself (room for every association), which changes no result."""
    c = lc.cases()[name]
    p = c.problem
    room = int(p.state["n_obs"].max(initial=0)) + 1 + len(p.kfs)
    obs = np.zeros((len(p.state), room), p.obs.dtype)
    w = min(room, p.obs.shape[1])
    obs[:, :w] = p.obs[:, :w]
    h = lcm.cheap_loop_closure_and_connect(c.settings, lc.dataclasses.replace(p, obs=obs), backend="host")
    L = int(h.counts[0])
    u32 = lambda *v: np.array(v, np.uint32).tobytes()  # noqa: E731

    def pairs(rec):
        took = np.nonzero(rec["keypoint"] >= 0)[0]
        return u32(len(took)) + b"".join(u32(h.sample_index[j], rec["keypoint"][j]) for j in took)

    out = u32(L) + h.sample_index[:L].tobytes() + pairs(h.closure[:L])
    for k in range(len(p.kfs)):
        out += pairs(h.connect[:L, k]) + bytes([int(h.kf_modified[k]) if L else 0])
    for i in range(len(h.state)):
        out += h.state[i:i + 1].tobytes() + h.obs[i, :h.state["n_obs"][i]].tobytes()
    out += b"".join((m != 0).astype(np.uint8).tobytes() for m in h.kf_masks)
    if len(h.state):
        out += lcm.refresh_map_points(c.settings, h.state["pos"][:1], h.obs[:1], h.state["n_obs"][:1], backend="host").tobytes()
    return out


@pytest.mark.parametrize("name", ["base", "state_flows", "no_keyframes", "empty_map", "below_min_keyframes", "obs_full"])
def test_facade_cpu_backend(tmp_path, name):
    r, outf = run_demo(tmp_path, name, -1)
    assert r.returncode == 0, r.stderr
    assert outf.read_bytes() == expected(name)


def test_facade_throws_over_the_keypoint_limit(tmp_path):
    r, _ = run_demo(tmp_path, "many_kp", -1)
    assert r.returncode == 5, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_facade_kernel(gpu, tmp_path):
    r, outf = run_demo(tmp_path, "state_flows", 0)
    assert r.returncode == 0, r.stderr
    assert outf.read_bytes() == expected("state_flows")
