"""The C++ twin of the stereo-initialisation device stage (mage_stereo_init_triangulate_host)
against the independent fp64 formulation of tests/stereo_init_cases.py, the crop mask against its
NumPy restatement, the coverage of the case table and the argument checks.  No GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from mageslam_amd import _lib, stereo
from tests import stereo_init_cases as sc

NAMES = list(sc.cases())


@pytest.mark.parametrize("name", NAMES)
def test_fragile_share_fp64(name):
    """At most MAX_FRAGILE_SHARE of a case's matches sit within FRAGILE of a threshold (fp64 alone)."""
    ref = sc.reference(name)
    assert ref.share <= sc.MAX_FRAGILE_SHARE, ref.share


@pytest.mark.parametrize("name", NAMES)
def test_host_verdicts_match_fp64(name):
    c, ref, r = sc.cases()[name], sc.reference(name), sc.host_result(name)
    assert r.status == ref.status
    if ref.status & stereo.STATUS_OVER_LIMIT:
        assert r.n_masked == 0 and len(r.points) == 0
        return
    keep = ~ref.excluded
    assert np.array_equal(r.verdicts[keep], ref.verdict[keep])
    # the records are the accepted matches in match order, cut at cap
    acc = np.nonzero(r.verdicts == sc.ACCEPTED)[0][: c.cap]
    assert len(r.points) == len(acc)
    assert np.array_equal(r.points["query_idx"], c.matches["query_idx"][acc])
    assert np.array_equal(r.points["train_idx"], c.matches["train_idx"][acc])
    assert np.array_equal(r.points["distance"], c.matches["distance"][acc])
    sure = keep[acc] & (ref.verdict[acc] == sc.ACCEPTED)
    assert np.array_equal(r.points["near_parallel"][sure].astype(bool), ref.parallel[acc][sure])


def test_host_positions_within_tolerance():
    """Accepted positions within K_TOL eps32 |X - C0| / sin^2(parallax) of fp64; prints the worst
    ratio (K_MEASURED in stereo_init_cases.py)."""
    worst, where = 0.0, None
    for name in NAMES:
        c, ref, r = sc.cases()[name], sc.reference(name), sc.host_result(name)
        acc = np.nonzero(r.verdicts == sc.ACCEPTED)[0][: c.cap]
        for k, j in enumerate(acc):
            g = ref.geometry[j]
            if g is None or ref.excluded[j]:
                continue
            unit = sc.EPS32 * g["d0"] / g["sin2"]
            ratio = float(np.max(np.abs(r.points["position"][k].astype(np.float64) - g["X"]))) / unit
            if ratio > worst:
                worst, where = ratio, (name, int(j))
    print(f"worst position error / (eps32 |X - C0| / sin^2): {worst:.3f} at {where}")
    assert sc.K_TOL == 2.0 * sc.K_MEASURED
    assert 0.0 < worst <= sc.K_TOL, (worst, where)


@pytest.mark.parametrize("name", NAMES)
def test_host_ba_inputs(name):
    """The bundle adjustment's inputs restate the records: frame 0's observations, then frame 1's."""
    c, r = sc.cases()[name], sc.host_result(name)
    n = len(r.points)
    assert r.ba_points.shape == (n, 3) and r.ba_uv.shape == (2 * n, 2)
    assert np.array_equal(r.ba_points, r.points["position"])
    q, t = r.points["query_idx"], r.points["train_idx"]
    uv = np.concatenate([np.stack([c.kp0["x"][q], c.kp0["y"][q]], 1), np.stack([c.kp1["x"][t], c.kp1["y"][t]], 1)])
    assert np.array_equal(r.ba_uv, uv.astype(np.float32).reshape(2 * n, 2))
    assert np.array_equal(r.ba_cam, np.repeat([0, 1], n))
    assert np.array_equal(r.ba_pt, np.tile(np.arange(n), 2))
    info = np.float32(1) - np.float32(1) / (np.float32(2.5) * np.float32(2.5))  # MapPointRefinementConfidence(1)
    assert np.all(r.ba_info == info)


@pytest.mark.parametrize("name", NAMES)
def test_crop_mask_and_count(name):
    c, r = sc.cases()[name], sc.host_result(name)
    if r.status & stereo.STATUS_OVER_LIMIT:
        return
    x, y, w, h = (int(v) for v in c.crop)
    expect = (c.kp0["x"] >= x) & (c.kp0["x"] < x + w) & (c.kp0["y"] >= y) & (c.kp0["y"] <= y + h)
    assert np.array_equal(r.mask0, expect)
    assert r.n_masked == int(expect.sum())
    for i, inside in (c.edges or {}).items():
        assert bool(r.mask0[i]) == inside, (i, c.kp0[i])
    assert np.all(r.mask0[c.matches["query_idx"][(c.matches["query_idx"] >= 0) & (c.matches["query_idx"] < len(c.kp0))]])


def test_coverage():
    """Every verdict occurs, the match counts cross the compaction's boundaries, the near-parallel
    branch is taken, every crop edge is probed, both status bits occur."""
    seen, counts, parallel, flags, status = set(), set(), 0, 0, 0
    for name in NAMES:
        ref, r = sc.reference(name), sc.host_result(name)
        seen |= set(int(v) for v in ref.verdict[~ref.excluded] if v >= 0)
        counts.add(len(sc.cases()[name].matches))
        parallel += int(ref.parallel.sum())
        flags += int(r.points["near_parallel"].sum())
        status |= r.status
    assert seen == set(range(6)), seen
    assert set(sc.MATCH_COUNTS) <= counts
    assert parallel >= 8 and flags >= 1, (parallel, flags)
    assert status == stereo.STATUS_OVER_LIMIT | stereo.STATUS_OVER_CAP
    r = sc.host_result("all_accepted")
    assert len(r.points) == len(r.verdicts) > 0 and not r.verdicts.any()
    r = sc.host_result("none_accepted")
    assert len(r.points) == 0 and len(r.verdicts) > 0 and r.verdicts.all()
    e = sc.cases()["edges"]
    x, y, w, h = sc.CROP
    on = {"left": 0, "right": 0, "top": 0, "bottom": 0}
    for i, inside in e.edges.items():
        px, py = float(e.kp0["x"][i]), float(e.kp0["y"][i])
        for edge, hit, want in (("left", px == x, True), ("right", px == x + w, False), ("top", py == y, True),
                                ("bottom", py == y + h, True)):
            if hit and (edge in ("left", "right") and y <= py <= y + h or edge in ("top", "bottom") and x <= px < x + w):
                assert inside == want, (edge, px, py)
                on[edge] += 1
    assert all(on.values()), on


def test_matches_are_what_a_two_way_match_finds():
    """The designed matches are mutual nearest neighbours within MaxHammingDistance with no rival
    (brute force in NumPy on a mid-sized case)."""
    c = sc.cases()["base"]
    bits0, bits1 = np.unpackbits(c.desc0, axis=1).astype(np.int32), np.unpackbits(c.desc1, axis=1).astype(np.int32)
    inside = sc.crop_mask(c.kp0, c.crop)
    d = bits0 @ (1 - bits1).T + (1 - bits0) @ bits1.T
    d[~inside] = 10 ** 6
    best1 = d.argmin(1)
    mutual = [(q, int(best1[q])) for q in range(len(d)) if d[q, best1[q]] <= 30 and d[:, best1[q]].argmin() == q]
    assert mutual == [(int(m["query_idx"]), int(m["train_idx"])) for m in c.matches]
    part = np.partition(d[c.matches["query_idx"]], 1, axis=1)
    assert np.all(part[:, 1] - part[:, 0] > 30)


def _host_status(settings_c):
    c = sc.cases()["m1"]
    n_masked, n_out, status = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    mask0, verdict = np.zeros(len(c.kp0), np.uint8), np.zeros(1, np.uint8)
    out = np.zeros(1, _lib.SP_DTYPE)
    ba = [np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.uint32), np.zeros(8, np.uint32),
          np.zeros(8, np.float32)]
    p = _lib.ptr
    f32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1)  # noqa: E731
    return _lib.load().mage_stereo_init_triangulate_host(
        C.byref(settings_c), p(f32(c.pos3)), p(f32(c.r9)), p(f32(c.intr4)), p(c.crop), p(c.kp0), len(c.kp0), p(c.kp1),
        len(c.kp1), p(c.matches), 1, p(mask0), C.byref(n_masked), p(verdict), p(out), 1, C.byref(n_out),
        *(p(b) for b in ba), C.byref(status))


def test_settings_are_checked():
    good = stereo.StereoMapInitializationSettings()
    assert _host_status(good.to_c()) == _lib.MAGE_OK
    bad_size = good.to_c()
    bad_size.struct_size -= 4
    assert _host_status(bad_size) == _lib.MAGE_EINVAL
    for field, value in (("max_epipolar_error", -1.0), ("max_epipolar_error", float("nan")),
                         ("min_accepted_distance_ratio", -0.5), ("max_hamming_distance", 257),
                         ("max_hamming_distance", -2), ("min_hamming_difference", -1), ("max_depth_meters", 0.0),
                         ("amount_ba_can_change_pose", 0.5), ("ba_num_steps_per_run", 0), ("ba_min_steps", 2),
                         ("ba_huber_width", 0.0), ("ba_max_outlier_error", -7.25),
                         ("ba_min_mean_square_error", float("nan"))):
        assert _host_status(dataclasses.replace(good, **{field: value}).to_c()) == _lib.MAGE_EINVAL, field


def test_python_argument_checks():
    c = sc.cases()["m1"]
    with pytest.raises(ValueError):
        stereo.triangulate_points(c.settings, *c.args(), matches=c.matches, backend="cpu")
    with pytest.raises(ValueError):
        stereo.triangulate_points(c.settings, *c.args(), backend="host")
    with pytest.raises(ValueError):
        stereo.triangulate_points(c.settings, *c.args(), desc0=c.desc0, desc1=c.desc1, matches=c.matches)


def test_gpu_backend_without_gpu_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = sc.cases()["m1"]
    with pytest.raises(_lib.MageError) as e:
        stereo.triangulate_points(c.settings, *c.args(), matches=c.matches, backend="gpu")
    assert e.value.status == _lib.MAGE_EDEVICE


def test_crop_from_frame0_to_frame1(oracle):
    """CalculateOverlapCropSourceInTarget from the matrix itself equals the stereo-scale geometry on
    the equivalent pair of extrinsics (target at identity, source at the matrix: targetToSource =
    M * inverse(I) = M exactly), library and oracle."""
    from mageslam_amd import image
    from mageslam_amd._lib import CameraConfig
    from tests.test_stereo_scale import rigid

    eye = np.eye(4, dtype=np.float32)
    for M, k0, wh0, k1, wh1 in (
            (rigid(t=(-0.06, 0, 0)), (500, 500, 320, 240), (640, 480), (500, 500, 320, 240), (640, 480)),
            (rigid(0.02, -0.01, (0.06, 0.01, 0)), (800, 800, 400, 300), (800, 600), (500, 505, 320, 240), (640, 480)),
            (rigid(0.0, 0.03, (0.0, 0.05, 0.02)), (900, 900, 640, 360), (1280, 720), (600, 610, 330, 230), (640, 480)),
            (rigid(t=(5.0, 0, 0)), (900, 900, 640, 360), (1280, 720), (900, 900, 640, 360), (1280, 720))):
        cam0, cam1 = CameraConfig.make(eye, *k0, *wh0), CameraConfig.make(M, *k1, *wh1)
        crop = stereo.overlap_crop(M, cam0, cam1, 2.3)
        assert crop == image.scale_geometry(cam1, cam0, 2.3)[1]
        assert crop == oracle.scale_geometry(M, k1, wh1, eye, k0, wh0, 2.3)[1]
    with pytest.raises(_lib.MageError) as e:
        stereo.overlap_crop(eye, CameraConfig.make(eye, 500, 500, 320, 240, 0, 480), cam1)
    assert e.value.status == _lib.MAGE_EINVAL


def _rigid(rng, t):
    from tests.stereo_init_cases import _rot

    M = np.eye(4)
    M[:3, :3] = _rot(*rng.normal(0, 0.4, 3))
    M[:3, 3] = t
    return M.astype(np.float32)


def test_host_scalars_against_float32_numpy():
    """The normalisation, the pose from the double inverse and the tether parameters, bit for bit
    against NumPy float32 with the same LU."""
    rng = np.random.default_rng(5)
    mats = [_rigid(rng, rng.normal(0, s, 3)) for s in (0.06, 0.06, 1.0, 30.0, 1e-3) for _ in range(4)]
    big = np.eye(4, dtype=np.float32)
    big[:3, :3] = np.array([[-0.8, 0.6, 0], [0.6, 0.8, 0], [0, 0, -1]], np.float32)  # trace < 0: the other quaternion branch
    big[:3, 3] = (0.05, 0.01, -0.02)
    for M in mats + [big]:
        zero, nrm, pos3, r9, t7 = stereo.host_scalars(M)
        ezero, enrm, epos3, er9, et7 = sc.host_scalars_f32(M)
        assert not zero and not ezero
        assert nrm.tobytes() == enrm.tobytes()
        assert pos3.tobytes() == epos3.tobytes() and r9.tobytes() == er9.tobytes()
        assert t7.tobytes() == et7.tobytes()
        # the double inverse gives back the normalised matrix up to rounding: frame 1's view matrix
        V = np.eye(4)
        V[:3, :3], V[:3, 3] = r9.reshape(3, 3).T, pos3
        assert np.allclose(V, nrm, atol=1e-5)
        assert abs(np.linalg.norm(nrm[:3, 3]) - 1) < 1e-6
    for length, expect in ((0.9e-5, True), (1.1e-5, False), (0.0, True)):
        M = np.eye(4, dtype=np.float32)
        M[0, 3] = length
        assert stereo.host_scalars(M)[0] == expect == sc.host_scalars_f32(M)[0]


def test_culling_against_the_literal_loop():
    rng = np.random.default_rng(6)
    for n in (0, 1, 2, 5, 40, 200):
        for share in (0.0, 0.1, 0.5, 1.0):
            k = int(round(share * 2 * n))
            outl = rng.choice(2 * n, k, replace=False) if n else np.zeros(0, np.int64)
            outl = np.concatenate([outl, outl[: k // 3]])  # an association reported by two runs
            assert stereo.cull_order(n, outl).tolist() == sc.cull_literal(n, outl.tolist()), (n, share)
    assert stereo.cull_order(6, [1, 7, 3, 11]).tolist() == [0, 4, 2]


def test_validation_thresholds():
    """ValidateInitializationData at and on both sides of each threshold."""
    s = stereo.StereoMapInitializationSettings()
    eye = np.eye(3, dtype=np.float32).reshape(9)

    def at(world):  # identity rotation: view-space t = -world
        return -np.asarray(world, np.float32)

    assert stereo.validate(s, 15, at((1, 0, 0)), eye) and not stereo.validate(s, 14, at((1, 0, 0)), eye)
    up = np.float32(0.10)
    for z, ok in ((up, True), (np.nextafter(up, np.float32(1)), False), (np.nextafter(up, np.float32(0)), True),
                  (-np.nextafter(up, np.float32(1)), False)):
        w = np.array([np.sqrt(1 - float(z) ** 2), 0, z], np.float32)
        assert stereo.validate(s, 20, at(w), eye) == ok == sc.validate_f32(s, 20, at(w), eye), z
    a = np.float32(1.65)
    lo = np.float32(1) / a
    for scale, ok in ((a, True), (np.nextafter(a, np.float32(9)), False), (np.nextafter(a, np.float32(0)), True),
                      (lo, True), (np.nextafter(lo, np.float32(0)), False), (np.nextafter(lo, np.float32(9)), True)):
        assert stereo.validate(s, 20, at((scale, 0, 0)), eye) == ok == sc.validate_f32(s, 20, at((scale, 0, 0)), eye), scale
    rng = np.random.default_rng(7)
    for _ in range(50):
        M = _rigid(rng, rng.normal(0, 0.8, 3))
        pos3, r9 = M[:3, 3], M[:3, :3].T.reshape(9)
        assert stereo.validate(s, 20, pos3, r9) == sc.validate_f32(s, 20, pos3, r9)


def _frames(c):
    from mageslam_amd._lib import CameraConfig

    cam = CameraConfig.make(np.eye(4, dtype=np.float32), sc.F, sc.F, sc.W / 2, sc.H / 2, sc.W, sc.H)
    return stereo.Frame(cam, c.kp0, c.desc0), stereo.Frame(cam, c.kp1, c.desc1)


def test_map_init_without_gpu_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = sc.cases()["base"]
    M = np.eye(4, dtype=np.float32)
    M[0, 3] = -0.06
    with pytest.raises(_lib.MageError) as e:
        stereo.StereoMapInit().Initialize(*_frames(c), M)
    assert e.value.status == _lib.MAGE_EDEVICE
    with pytest.raises(_lib.MageError) as e:
        stereo.StereoMapInit(stereo.StereoMapInitializationSettings(ba_num_steps_per_run=0)).Initialize(*_frames(c), M)
    assert e.value.status == _lib.MAGE_EINVAL


def test_every_result_code_occurs(oracle):
    """The whole call's cases reach OK, FEW_MATCHES, FEW_POINTS and FAILED_VALIDATION in the composed
    oracle, and a pair without displacement ZERO_DISPLACEMENT (the GPU tests run the same pairs)."""
    codes = {name: sc.composed_oracle(c, c.frame0_to_frame1, oracle)["code"] for name, c in sc.whole_cases().items()}
    assert codes == dict(base=stereo.OK, m1=stereo.FEW_MATCHES, none_accepted=stereo.FEW_POINTS,
                         axial=stereo.FAILED_VALIDATION, all_accepted=stereo.OK, mismatch=stereo.OK)
    still = sc.whole_cases()["m1"].frame0_to_frame1.copy()
    still[:3, 3] = 0
    assert sc.composed_oracle(sc.whole_cases()["m1"], still, oracle)["code"] == stereo.ZERO_DISPLACEMENT
    e = sc.composed_oracle(sc.whole_cases()["mismatch"], sc.whole_cases()["mismatch"].frame0_to_frame1, oracle)
    assert e["runs"] == 3 and len(e["outliers"]) >= 10 and len(e["points"]) < int((e["verdicts"] == 0).sum())
