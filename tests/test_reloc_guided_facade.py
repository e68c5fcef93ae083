"""The guided half of the relocalisation at its interfaces: the defaults are the reference's, the
records and argument blocks have the sizes the header gives them, bad arguments are MAGE_EINVAL
before anything touches a device, and mage::hot::PoseEstimator::TryEstimatePoseFromCandidates
(include/mage/mage.hpp) compiles against include/ and returns what the Python call returns."""
import ctypes as C
import dataclasses
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import _lib, reloc
from mageslam_amd._lib import DM_DTYPE, RG_FRAME_DTYPE, RG_RESULT_DTYPE
from tests import reloc_guided_cases as gc
from tests import reloc_guided_ref as gr

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "reloc_guided_demo.cpp"


def test_defaults_are_the_reference_values():
    s = reloc.RelocalizationSettings()
    # RelocalizationSettings (MageSettings.h:236-250): what the guided half reads
    assert (s.min_brute_force_correspondences, s.min_radius_match_correspondences, s.min_map_points) == (20, 15, 10)
    assert s.bundle_adjust_inliers_pct_required == pytest.approx(0.4) and s.round_robin_iterations == 5
    assert (s.bundle_adjust_iterations, s.search_radius, s.max_bundle_adjust_reprojection_error) == (10, 20.0, 8.0)
    # PoseEstimationSettings.OrbMatcherSettings (MageSettings.h:36-39) and BundleAdjustSettings' HuberWidth
    assert reloc.POSE_MATCHER == (30, 1) and reloc.HUBER_WIDTH == 1.8
    hpp = (ROOT / "include" / "mage" / "mage.hpp").read_text()
    assert hpp.count("int poseMaxHammingDist = 30") == 2 and hpp.count("int poseMinHammingDifference = 1") == 2
    math = (ROOT / "mageslam_amd" / "csrc" / "reloc_guided_math.hpp").read_text()
    assert "constexpr float RG_HUBER = 1.8f;" in math
    assert (reloc.RG_OK, reloc.RG_SKIPPED, reloc.RG_FEW_RADIUS_MATCHES, reloc.RG_FEW_MAP_POINTS, reloc.RG_FEW_BA_INLIERS) == (0, 1, 2, 3, 4)


def test_struct_sizes_match_the_header(tmp_path):
    sizes = dict(mage_reloc_guided_result=RG_RESULT_DTYPE.itemsize, mage_reloc_frame_result=RG_FRAME_DTYPE.itemsize,
                 mage_reloc_guided_args=C.sizeof(_lib.RelocGuidedArgsC), mage_reloc_candidates_args=C.sizeof(_lib.RelocCandidatesArgsC))
    assert sizes == dict(mage_reloc_guided_result=124, mage_reloc_frame_result=56, mage_reloc_guided_args=344,
                         mage_reloc_candidates_args=128)
    src = tmp_path / "sizes.cpp"
    src.write_text('#include "mage_hot.h"\n' + "".join(f"static_assert(sizeof({k}) == {v}, \"{k}\");\n" for k, v in sizes.items()) +
                   "static_assert(offsetof(mage_reloc_guided_args, d_scratch) == 336, \"d_scratch\");\n"
                   "static_assert(offsetof(mage_reloc_guided_args, kf_pitch) == 32, \"kf_pitch\");\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-include", "cstddef", f"-I{ROOT / 'include'}", str(src)], check=True)
    assert _lib.RelocGuidedArgsC.d_scratch.offset == 336 and _lib.RelocGuidedArgsC.kf_pitch.offset == 32


def host(settings, name="n24", **kw):
    s, r = gc.scene(name), gr.run(name, 0)
    return reloc.guided_host(settings, True, gc.INTR, s.cands[0], s.kp, *r.first, **kw)


@pytest.mark.parametrize("field, value", [("bundle_adjust_inliers_pct_required", float("nan")),
                                          ("bundle_adjust_inliers_pct_required", -0.1), ("search_radius", -1.0),
                                          ("search_radius", float("inf")), ("max_bundle_adjust_reprojection_error", -1.0),
                                          ("max_bundle_adjust_reprojection_error", float("nan")), ("ransac_iterations", 0)])
def test_range_errors(field, value):
    with pytest.raises(_lib.MageError) as e:
        host(dataclasses.replace(reloc.RelocalizationSettings(), **{field: value}))
    assert e.value.status == _lib.MAGE_EINVAL


def einval(call):
    with pytest.raises(_lib.MageError) as e:
        _lib.check(call())
    assert e.value.status == _lib.MAGE_EINVAL
    return str(e.value)


def test_wrong_struct_sizes_and_null_pointers_are_einval():
    """Every entry refuses them before it touches a device (there is none here)."""
    L = _lib.load()
    good = reloc.RelocalizationSettings().to_c()
    bad = reloc.RelocalizationSettings().to_c()
    bad.struct_size -= 4
    with pytest.raises(_lib.MageError) as e:
        host(bad)
    assert e.value.status == _lib.MAGE_EINVAL and "struct_size" in str(e.value)
    args = _lib.RelocGuidedArgsC.make(frames=1, candidates_per_frame=1, cap=8, pnp_cap=8, kf_pitch=8, kp_pitch=8)
    cargs = _lib.RelocCandidatesArgsC.make(match_cap=8)
    # the batched entries: settings, the blocks' own struct_size, NULL blocks, NULL required buffers
    assert "struct_size" in einval(lambda: L.mage_reloc_guided_batch_device(C.byref(bad), C.byref(args), None))
    assert "null" in einval(lambda: L.mage_reloc_guided_batch_device(None, C.byref(args), None))
    assert "struct_size" in einval(lambda: L.mage_reloc_guided_batch_device(C.byref(good), None, None))
    assert "null buffer" in einval(lambda: L.mage_reloc_guided_batch_device(C.byref(good), C.byref(args), None))
    short = _lib.RelocGuidedArgsC.make(frames=1, candidates_per_frame=1, cap=8, pnp_cap=8, kf_pitch=8, kp_pitch=8)
    short.struct_size -= 8
    assert "mage_reloc_guided_args" in einval(lambda: L.mage_reloc_guided_batch_device(C.byref(good), C.byref(short), None))
    assert "struct_size" in einval(lambda: L.mage_reloc_candidates_batch_device(C.byref(bad), C.byref(cargs), C.byref(args), None))
    assert "null buffer" in einval(lambda: L.mage_reloc_candidates_batch_device(C.byref(good), C.byref(cargs), C.byref(args), None))
    assert "mage_reloc_guided_args" in einval(lambda: L.mage_reloc_candidates_batch_device(C.byref(good), C.byref(cargs), C.byref(short), None))
    cshort = _lib.RelocCandidatesArgsC.make(match_cap=8)
    cshort.struct_size += 8
    assert "mage_reloc_candidates_args" in einval(lambda: L.mage_reloc_candidates_batch_device(C.byref(good), C.byref(cshort), C.byref(args), None))
    assert "mage_reloc_candidates_args" in einval(lambda: L.mage_reloc_candidates_batch_device(C.byref(good), None, C.byref(args), None))
    # no problem at all is no error, with every buffer NULL
    empty = _lib.RelocGuidedArgsC.make(frames=0, candidates_per_frame=4)
    assert L.mage_reloc_guided_batch_device(C.byref(good), C.byref(empty), None) == _lib.MAGE_OK
    # the host-buffer entry and the twin
    frame = np.zeros(1, RG_FRAME_DTYPE)

    def single(settings, n_candidates, intr4):  # every buffer but intr4 and the frame's record NULL
        return L.mage_reloc_guided(C.byref(settings), 30, 1, n_candidates, _lib.ptr(intr4), None, None, None, None, 8, None,
                                   None, None, None, None, 0, None, 8, None, 8, None, None, _lib.ptr(frame), None, 0)

    assert "null" in einval(lambda: single(good, 1, None))
    assert "null" in einval(lambda: single(good, 1, gc.INTR))
    assert "struct_size" in einval(lambda: single(bad, 0, gc.INTR))
    assert single(good, 0, gc.INTR) == _lib.MAGE_OK  # no candidate: nothing tried, no device
    assert int(frame[0]["index"]) == -1 and frame[0]["r9"].tobytes() == gr.IDENT[1].tobytes()
    assert "null" in einval(lambda: L.mage_reloc_guided_host(C.byref(good), 1, None, None, None, None, 0, None, 0, None, 0, None,
                                                              None, 0, None, None, None, None, None, None, 0, None, None,
                                                              None, None, None, None, None))
    assert "null" in einval(lambda: L.mage_reloc_guided_choose_host(C.byref(good), None, 0, None))


def test_twin_refuses_matches_that_name_nothing():
    st = reloc.RelocalizationSettings()
    r = gr.run("n24", 0)
    for col, val in (("query_idx", -1), ("query_idx", 24), ("train_idx", len(gc.scene("n24").kp)), ("train_idx", -2)):
        rm = r.rm.copy()
        rm[col][3] = val
        with pytest.raises(_lib.MageError) as e:
            host(st, radius_matches=rm)
        assert e.value.status == _lib.MAGE_EINVAL
    with pytest.raises(_lib.MageError):
        host(st, radius_matches=np.concatenate([r.rm, r.rm[:1]]))  # more matches than queries
    assert host(st, radius_matches=r.rm).result.tobytes() == r.g2.result.tobytes()


def build_demo():
    from mageslam_amd import build

    lib = build.build()
    out = ROOT / "mageslam_amd" / "_lib" / "reloc_guided_demo"
    if not out.exists() or out.stat().st_mtime < max(SRC.stat().st_mtime, lib.stat().st_mtime,
                                                       (ROOT / "include" / "mage" / "mage.hpp").stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                        f"-L{lib.parent}", "-lmage_hot", f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def run_demo(tmp_path, name, device):
    s = gc.scene(name)
    raw, outf = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    blob = np.array([len(s.cands), device + 1, len(s.kp)], np.uint32).tobytes() + gc.INTR.tobytes() + s.kp.tobytes() + s.desc.tobytes()
    for c, mm in zip(s.cands, s.matches):
        order = c.order if c.order is not None else np.zeros(0, np.int32)
        blob += (np.array([len(c.kp), len(order), len(mm)], np.uint32).tobytes() + c.map_xyzi.tobytes() + c.kp.tobytes() +
                 c.desc.tobytes() + order.tobytes() + np.ascontiguousarray(mm, DM_DTYPE).tobytes())
    raw.write_bytes(blob)
    return subprocess.run([str(build_demo()), str(raw), str(outf)], capture_output=True, text=True), outf


def test_facade_compiles_and_refuses_the_cpu_backend(tmp_path):
    r, _ = run_demo(tmp_path, "f3_middle", -1)
    assert r.returncode == 6, (r.returncode, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f5_two", "n64_order"])
def test_facade_returns_the_python_result(gpu, tmp_path, name):
    r, outf = run_demo(tmp_path, name, 0)
    assert r.returncode == 0, r.stderr
    s = gc.scene(name)
    e = reloc.guided_search(s.settings, gc.INTR, s.cands, s.kp, s.desc, s.matches, backend="hip")
    assert e.index == s.expect_index >= 0
    want = (np.array([e.index], np.int32).tobytes() + np.array([len(e.associations)], np.uint32).tobytes() + e.pos3.tobytes() +
            e.r9.tobytes() + e.associations.tobytes() + e.results.tobytes())
    assert outf.read_bytes() == want
