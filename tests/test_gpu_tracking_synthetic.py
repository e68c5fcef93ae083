"""GPU parity of the tracking loop on the synthetic-feature cases of tests/track_cases.py: the
Python loop on the GPU kernels, the native host loop (mage_track_sequence) and the device-resident
loop (mage_track_sequence_device) against the same loop on the CPU oracle.  The cases need no ORB
extraction (both native entries take keypoints and descriptors) and reach what the rendered
fronto-parallel plane of test_gpu_tracking.py cannot: map points behind the predicted camera (`sel`
is a real compaction), rings of 2 and 8 keyframes, pitch 4096, count == pitch == 1025, varying,
short and empty frames, mixed octaves, the local BA's halt / re-run / write-back with a non-identity
`sel`, and a count above the pitch.  test_track_cases_reference.py asserts on the oracle alone that
each case reaches its path.  Bar, as in test_gpu_tracking.py: identical match / inlier / local-map
association counts, keyframe decisions and BA outlier counts, pose RMSE <= 1e-4 (translation,
rotation in rad), the native loops bit-identical to the Python loop over the same kernels."""
import functools

import numpy as np
import pytest

from mageslam_amd import tracking
from tests import track_cases as tc

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert a.matches == b.matches and a.inliers == b.inliers and a.keyframes == b.keyframes
    assert all(np.array_equal(x.R, y.R) and np.array_equal(x.t, y.t) for x, y in zip(a.poses, b.poses))


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    from oracle.tracking_backend import OracleBackend

    c = tc.CASES[name]
    f, poses, K, plane_z = tc.case_scene(name)
    return tracking.track(f, K, poses[0], plane_z, OracleBackend(c.scene["cap"]), c.tracker_settings())


def _device_run(name, settings):
    c = tc.CASES[name]
    f, poses, K, plane_z = tc.case_scene(name)
    return tracking.track_native_device(*tracking.features_to_device(f, c.pitch), len(f), K, poses[0], plane_z,
                                        settings=settings)


def _against_oracle(r, o):
    assert r.matches == o.matches and r.inliers == o.inliers and r.keyframes == o.keyframes
    rt, rr = tracking.pose_rmse(r, o)
    print("pose rmse vs oracle", rt, rr)
    assert rt <= 1e-4 and rr <= 1e-4, (rt, rr)


@pytest.mark.parametrize("name", [n for n in tc.CASES if n not in tc.LOCAL_BA_CASES])
def test_synthetic_case_vs_oracle(gpu, oracle, name):
    c = tc.CASES[name]
    f, poses, K, plane_z = tc.case_scene(name)
    s = c.tracker_settings()
    o = _oracle_run(name)
    g = tracking.track(f, K, poses[0], plane_z, tracking.GpuBackend(c.scene["cap"]), s)
    n = tracking.track_native(f, K, poses[0], plane_z, settings=s)
    d = _device_run(name, s)
    for r in (g, n, d):
        _against_oracle(r, o)
    assert g.local_matches == o.local_matches
    assert d.ba_outliers == [] and o.ba_outliers == []
    _same(n, g)
    _same(d, g)
    assert tuple(t for t in range(1, len(f)) if d.inliers[t] == 0) == c.lost


@pytest.mark.parametrize("name", tc.LOCAL_BA_CASES)
def test_synthetic_local_ba_vs_oracle(gpu, oracle, name):
    """The device loop's halt / re-run / write-back with map points behind the camera."""
    c = tc.CASES[name]
    f, poses, K, plane_z = tc.case_scene(name)
    s = c.tracker_settings()
    o = _oracle_run(name)
    gb = tracking.GpuBackend(c.scene["cap"])
    g = tracking.track(f, K, poses[0], plane_z, gb, s)
    d = _device_run(name, s)
    assert len(o.ba_outliers) >= 2 and any(k > 0 for _, k in o.ba_outliers), o.ba_outliers
    for r in (g, d):
        _against_oracle(r, o)
        assert r.ba_outliers == o.ba_outliers
    assert g.local_matches == o.local_matches
    _same(d, g)
    # the BA changed the map: without it the same frames give other poses
    e = tracking.track(f, K, poses[0], plane_z, gb, c.tracker_settings(local_ba=False))
    assert any(not np.array_equal(a.t, b.t) for a, b in zip(e.poses, g.poses))


@pytest.mark.parametrize("frame", [0, 7])
def test_count_above_pitch_is_reported(gpu, frame):
    """A device count above the frame pitch: mage_track_sequence_device returns MAGE_ECAPACITY
    (frame 0: trk_init's frame_count clamps to the slot; a later frame: RadiusMatch refuses the
    target set, the frame is lost, and no kernel indexes past the frame's slot), and the next call
    with the true counts gives what it gave before."""
    from mageslam_amd._lib import MAGE_ECAPACITY, MageError

    name = "short_empty"
    c = tc.CASES[name]
    f, poses, K, plane_z = tc.case_scene(name)
    s = c.tracker_settings()
    assert 0 <= frame < len(f) - 1 and frame not in c.lost
    d_kp, d_desc, pitch, d_counts = tracking.features_to_device(f, c.pitch)
    before = tracking.track_native_device(d_kp, d_desc, pitch, d_counts, len(f), K, poses[0], plane_z, settings=s)
    bad = d_counts.clone()
    bad[frame] = pitch + 3
    with pytest.raises(MageError) as err:
        tracking.track_native_device(d_kp, d_desc, pitch, bad, len(f), K, poses[0], plane_z, settings=s)
    assert err.value.status == MAGE_ECAPACITY
    after = tracking.track_native_device(d_kp, d_desc, pitch, d_counts, len(f), K, poses[0], plane_z, settings=s)
    _same(after, before)
    assert len(before.keyframes) >= 2 and after.ba_outliers == before.ba_outliers == []
