"""RelocalizationSettings and mage::hot::PoseEstimator::PNPRansac (include/mage/mage.hpp): the
defaults are the reference's, bad settings are refused, and the C++ facade compiled against include/
gives the twin's bytes on the CPU backend and the kernels' on a GPU."""
import ctypes as C
import dataclasses
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import _lib, reloc
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE
from tests import reloc_pnp_cases as rc

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "reloc_pnp_demo.cpp"

# MageSettings.h:236-250 and OrbMatcherSettings (:36-39), in the reference's order
REFERENCE_DEFAULTS = [("MinBruteForceCorrespondences", 20), ("MinRadiusMatchCorrespondences", 15), ("MinMapPoints", 10),
                      ("RansacInliersPctRequired", 0.4), ("BundleAdjustInliersPctRequired", 0.4),
                      ("RansacConfidence", 0.6), ("RoundRobinIterations", 5), ("RansacIterations", 2),
                      ("BundleAdjustIterations", 10), ("SearchRadius", 20), ("MaxBundleAdjustReprojectionError", 8),
                      ("MaxBundlePnPReprojectionError", 8), ("MaxHammingDistance", 30), ("MinHammingDifference", 1)]


def snake(name):
    return re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower().replace("pn_p", "pnp")


def test_settings_defaults_and_order():
    s = reloc.RelocalizationSettings()
    fields = [f.name for f in dataclasses.fields(s)]
    assert fields == [snake(n) for n, _ in REFERENCE_DEFAULTS]
    for (_, v), f in zip(REFERENCE_DEFAULTS, fields):
        assert getattr(s, f) == pytest.approx(v)
    cs = s.to_c()
    assert [n for n, _ in cs._fields_] == ["struct_size"] + fields
    assert cs.struct_size == C.sizeof(cs) == 60
    assert _lib.RP_RESULT_DTYPE.itemsize == 104
    # the C++ facade's defaults are the same text
    hpp = (ROOT / "include" / "mage" / "mage.hpp").read_text()
    body = hpp[hpp.index("struct RelocalizationSettings {"):hpp.index("mage_reloc_settings ToC() const")]
    for n, v in REFERENCE_DEFAULTS:
        m = re.search(rf"\b{n}\{{([0-9.]+)f?\}}", body)
        assert m and float(m.group(1)) == pytest.approx(v), n


def run_host(settings):
    c = rc.case("n6")
    return reloc.pnp_ransac(settings, rc.INTR, c.map_xyzi, c.kp, c.matches, backend="host")


@pytest.mark.parametrize("field, value", [("ransac_confidence", 0.0), ("ransac_confidence", 1.0), ("ransac_confidence", -0.5),
                                          ("ransac_confidence", float("nan")), ("ransac_iterations", 0),
                                          ("ransac_iterations", 257), ("ransac_inliers_pct_required", float("nan")),
                                          ("max_bundle_pnp_reprojection_error", -1.0),
                                          ("max_bundle_pnp_reprojection_error", float("inf"))])
def test_range_errors(field, value):
    with pytest.raises(_lib.MageError) as e:
        run_host(dataclasses.replace(rc.case("n6").settings, **{field: value}))
    assert e.value.status == _lib.MAGE_EINVAL


def test_struct_size_is_checked():
    cs = rc.case("n6").settings.to_c()
    cs.struct_size -= 4
    with pytest.raises(_lib.MageError) as e:
        run_host(cs)
    assert e.value.status == _lib.MAGE_EINVAL and "struct_size" in str(e.value)
    assert run_host(dataclasses.replace(rc.case("n6").settings, ransac_iterations=256, ransac_confidence=0.999)).ok


def test_bad_index_and_limits_on_the_host():
    c = rc.case("n6")
    for col, val in (("query_idx", -1), ("query_idx", len(c.map_xyzi)), ("train_idx", len(c.kp)), ("train_idx", -3)):
        bad = c.matches.copy()
        bad[col][2] = val
        h = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, bad, backend="host")
        assert h.status == reloc.STATUS_BAD_INDEX and len(h.inliers) == 0
    unassociated = np.flatnonzero(c.map_xyzi[:, 3] <= 0)[0]
    bad = c.matches.copy()
    bad["query_idx"][0] = unassociated
    assert reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, bad, backend="host").status == reloc.STATUS_BAD_INDEX
    over = np.zeros(reloc.MAX_MATCHES + 1, DM_DTYPE)
    assert reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, over, backend="host").status == reloc.STATUS_OVER_LIMIT
    # a small cap: the count is kept, the bit set, nothing written past the cap
    h = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, c.matches, backend="host", cap=4)
    assert h.status == reloc.STATUS_OVER_CAP and int(h.result["n_in_front"]) == 6 and len(h.inliers) == 4


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "reloc_pnp_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, name, device, n=None):
    c = rc.case(name)
    pw, uv = rc.correspondences(c)
    if n is not None:
        pw, uv = np.resize(pw, (n, 3)), np.resize(uv, (n, 2))
    s = c.settings
    raw, outf = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    raw.write_bytes(np.array([len(pw), device + 1, s.ransac_iterations], np.uint32).tobytes() +
                    np.array([s.ransac_confidence, s.max_bundle_pnp_reprojection_error], np.float32).tobytes() +
                    rc.INTR.tobytes() + pw.astype(np.float32).tobytes() + uv.astype(np.float32).tobytes())
    return subprocess.run([str(build_demo()), str(raw), str(outf)], capture_output=True, text=True), outf


def expected(name, backend):
    """PNPRansac through the binding: the points as their own candidate and frame, the gates open."""
    c = rc.case(name)
    pw, uv = rc.correspondences(c)
    n = len(pw)
    mp = np.concatenate([pw.astype(np.float32), np.ones((n, 1), np.float32)], 1)
    kp = np.zeros(n, KP_DTYPE)
    kp["x"], kp["y"] = uv[:, 0], uv[:, 1]
    mm = np.zeros(n, DM_DTYPE)
    mm["query_idx"] = mm["train_idx"] = np.arange(n)
    s = dataclasses.replace(c.settings, min_brute_force_correspondences=0, ransac_inliers_pct_required=0.0)
    h = reloc.pnp_ransac(s, rc.INTR, mp, kp, mm, backend=backend)
    found = h.verdict == reloc.OK
    e = h.result.tobytes() + np.array([found, len(h.inliers) if found else 0], np.uint32).tobytes()
    if found:
        e += h.pos3.tobytes() + h.r9.tobytes() + h.inliers.astype(np.int32).tobytes()
    return h, e


@pytest.mark.parametrize("name", ["n4", "n5", "mix40_i65", "behind60"])
def test_facade_cpu_backend(tmp_path, name):
    r, outf = run_demo(tmp_path, name, -1)
    assert r.returncode == 0, r.stderr
    h, e = expected(name, "host")
    assert (h.verdict == reloc.OK) == (name != "n4")
    assert outf.read_bytes() == e
    if name == "behind60":  # the pose and the kept inliers are the stage's own
        t = rc.twin(name)
        assert np.array_equal(h.inliers, t.inliers) and h.pos3.tobytes() == t.pos3.tobytes()


def test_facade_throws_over_the_limit(tmp_path):
    r, _ = run_demo(tmp_path, "n6", -1, n=reloc.MAX_MATCHES + 1)
    assert r.returncode == 6, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_facade_kernel(gpu, tmp_path):
    r, outf = run_demo(tmp_path, "mix40_i65", 0)
    assert r.returncode == 0, r.stderr
    h, e = expected("mix40_i65", "host")
    assert h.verdict == reloc.OK
    assert outf.read_bytes() == e
