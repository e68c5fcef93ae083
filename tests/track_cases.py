"""Helpers of the synthetic-feature tracker tests (test_track_cases_reference.py,
test_gpu_tracking_synthetic.py): a scene built as features directly (no images, no ORB extraction),
the case table, and a probe that records what the Python loop decided per frame.  Not a test module
(nothing is collected).

The scene is a plane seen by a tilted camera with the horizon inside the image.  Keypoints beyond
the horizon ("sky") back-project onto the plane with a negative ray parameter, so a keyframe owns
map points behind the camera: the tracker's compaction of the points in front (`sel`) is then a
real compaction and not the identity it is on a fronto-parallel plane.  Per-frame dropout gives
older keyframes points the reference keyframe lacks (local-map associations), and varying counts.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from mageslam_amd import tracking
from mageslam_amd._lib import KP_DTYPE

PLANE_Z = 5.0
FOOTPRINT_X = (-40.0, 60.0)   # wider than any frame of the cases sees
FOOTPRINT_Y = (-5.0, 120.0)
SKY_DISTANCE = 1e4
SKY_ELEVATION_DEG = (1.5, 25.0)  # above the horizon (away from the plane)
SKY_AZIMUTH_DEG = 50.0           # either side of the viewing direction
MARGIN_PX = 8.0
MIN_HORIZON_DEG = 1.0
MAX_PLANE_RANGE = 150.0
YAW_DEG_PER_FRAME = 0.05
BIT_FLIP = 0.02


def _rotx(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _roty(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def scene(T, W, H, n_plane, n_sky, tilt_deg, step, seed, cap, keep=0.8, levels=1):
    """-> (features, true_poses, K, plane_z): per frame (keypoints KP_DTYPE, descriptors (n, 32)),
    the frames' true tracking.Pose, (fx, fy, cx, cy) and the plane's depth."""
    rng = np.random.default_rng(seed)
    N = n_plane + n_sky
    plane = np.stack([rng.uniform(*FOOTPRINT_X, n_plane), rng.uniform(*FOOTPRINT_Y, n_plane),
                      np.full(n_plane, PLANE_Z)], 1)
    az = np.deg2rad(rng.uniform(-SKY_AZIMUTH_DEG, SKY_AZIMUTH_DEG, n_sky))
    el = np.deg2rad(rng.uniform(*SKY_ELEVATION_DEG, n_sky))
    sky = SKY_DISTANCE * np.stack([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), -np.sin(el)], 1)
    order = rng.permutation(N)  # sky and plane points interleave in index order
    world = np.concatenate([plane, sky])[order]
    is_plane = (np.arange(N) < n_plane)[order]
    wdesc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    woct = rng.integers(0, levels, N).astype(np.int32)
    fx = fy = 0.7 * W
    cx, cy = W / 2.0, H / 2.0
    features, poses = [], []
    for t in range(T):
        R = _rotx(math.radians(tilt_deg)) @ _roty(math.radians(YAW_DEG_PER_FRAME * t))
        C = np.array([step * t, 0.3 * step * t, 0.0])
        poses.append(tracking.Pose(R, -R @ C))
        ray = world - C
        rng_ = np.linalg.norm(ray, axis=1)
        Xc = ray @ R.T
        z = np.where(Xc[:, 2] > 0, Xc[:, 2], 1.0)
        u, v = fx * Xc[:, 0] / z + cx, fy * Xc[:, 1] / z + cy
        ok = (Xc[:, 2] > 0) & (u > MARGIN_PX) & (u < W - MARGIN_PX) & (v > MARGIN_PX) & (v < H - MARGIN_PX)
        ok &= np.abs(ray[:, 2] / rng_) > math.sin(math.radians(MIN_HORIZON_DEG))
        ok &= ~is_plane | (rng_ < MAX_PLANE_RANGE)
        ok &= rng.random(N) < keep
        idx = np.nonzero(ok)[0][:cap]
        kp = np.zeros(len(idx), KP_DTYPE)
        kp["x"], kp["y"], kp["octave"], kp["size"] = u[idx], v[idx], woct[idx], 31.0
        flips = np.packbits(rng.random((len(idx), 256)) < BIT_FLIP, axis=1)
        features.append((kp, wdesc[idx] ^ flips))
    return features, poses, (fx, fy, cx, cy), PLANE_Z


@dataclasses.dataclass(frozen=True)
class Case:
    scene: dict            # scene()'s arguments
    settings: dict         # TrackerSettings' (width / height come from the scene)
    pitch: int             # frame pitch of the device loop
    cuts: tuple = ()       # (frame, keypoints kept) applied to the scene's frames
    lost: tuple = ()       # the frames meant to be lost
    min_keyframes: int = 2

    def tracker_settings(self, **over):
        return tracking.TrackerSettings(width=self.scene["W"], height=self.scene["H"], **{**self.settings, **over})


_VGA = dict(T=24, W=640, H=480, n_plane=2500, n_sky=900, tilt_deg=72.0, step=4.0, seed=101, cap=1025)
_QVGA = dict(T=16, W=320, H=240, n_plane=1500, n_sky=600, tilt_deg=72.0, step=4.0, seed=202, cap=700)
_MIN_MATCHES = tracking.TrackerSettings().min_matches
_CUT = 8  # the short / empty case: frame 8 empty, 9 one keypoint short of min_matches, 10 exactly min_matches

CASES = {
    # count = pitch = 1025 (one past the 1024-thread stride) on frames 0-10, keyframes 0 and 7 among
    # them (later frames see the footprint's edge and hold fewer), ring of 2 overwritten by every
    # keyframe after the second, 24 frames cross the band-index chunk at frame 16
    "horizon_ring2": Case(_VGA, dict(local_map_keyframes=2), 1025, min_keyframes=7),
    # the largest block layout (ring 8 = NKMAX, pitch 4096) with counts that vary below the cap;
    # 34 frames wrap the 32-slot band ring.  step 2.2 instead of the other cases' 4.0: at 4.0 the
    # camera leaves the footprint after frame 16 and frames 25.. are lost; at 2.2 the oracle loop
    # makes 6 keyframes and loses no frame
    "largest_layout": Case(dict(_QVGA, T=34, step=2.2), dict(local_map_keyframes=8), 4096, min_keyframes=3),
    "ring1": Case(_QVGA, dict(local_map_keyframes=1), 700),
    "ring0": Case(_QVGA, dict(local_map_keyframes=0), 700),
    "mixed_octaves": Case(dict(_QVGA, levels=3), dict(local_map_keyframes=3, num_levels=3), 700),
    "local_ba_exact": Case(_QVGA, dict(local_map_keyframes=3, local_ba=True), 700),
    "local_ba_noisy": Case(_QVGA, dict(local_map_keyframes=3, local_ba=True, map_point_depth_noise=0.02), 700),
    # the 20 keypoints of frame 10 are the scene's first 20 in index order: with the dropout and the
    # sky points among them fewer than min_matches match, so the frame is lost like the two before
    "short_empty": Case(_QVGA, dict(local_map_keyframes=3), 700,
                        cuts=((_CUT, 0), (_CUT + 1, _MIN_MATCHES - 1), (_CUT + 2, _MIN_MATCHES)),
                        lost=(_CUT, _CUT + 1, _CUT + 2)),
}
LOCAL_BA_CASES = [n for n, c in CASES.items() if c.settings.get("local_ba")]


@functools.lru_cache(maxsize=None)
def case_scene(name):
    """The case's (features, true poses, K, plane_z), built once and shared (read-only)."""
    c = CASES[name]
    features, poses, K, plane_z = scene(**c.scene)
    for f, n in c.cuts:
        kp, d = features[f]
        features[f] = (kp[:n].copy(), d[:n].copy())
    for kp, d in features:
        kp.setflags(write=False)
        d.setflags(write=False)
    return tuple(features), tuple(poses), K, plane_z


class Probe(tracking.Backend):
    """A backend that delegates to `inner` and records every RadiusMatch call's matches."""

    def __init__(self, inner):
        self.inner = inner
        self.radius_calls = []  # the matches, in call order

    def radius_match(self, qkp, qdesc, tkp, tdesc, radius, qpos, max_hamming, min_diff):
        m = self.inner.radius_match(qkp, qdesc, tkp, tdesc, radius, qpos, max_hamming, min_diff)
        self.radius_calls.append(m)
        return m

    def optimize_pose(self, *a):
        return self.inner.optimize_pose(*a)

    def local_map_match(self, *a):
        return self.inner.local_map_match(*a)

    def bundle_adjust(self, *a):
        return self.inner.bundle_adjust(*a)


@dataclasses.dataclass
class FrameRecord:
    points: int            # map points of the reference keyframe
    finite: bool           # all of them finite
    front: np.ndarray      # tracking.project's mask under the frame's prediction
    passes: int            # RadiusMatch passes run
    matches: np.ndarray    # the last pass's matches (query_idx indexes the points in front)

    @property
    def behind(self):
        return int((~self.front).sum())

    @property
    def moved(self):
        """Matches whose point's index among the points in front differs from its index in the keyframe."""
        sel = np.nonzero(self.front)[0]
        q = self.matches["query_idx"].astype(np.int64)
        return int((sel[q] != q).sum())


def probe_track(features, K, first_pose, plane_z, backend, settings):
    """tracking.track on `backend`, and per frame t >= 1 a FrameRecord (index t - 1): what
    tracking.project and the frame's RadiusMatch passes gave inside the loop."""
    probe = Probe(backend)
    fronts = []
    project = tracking.project

    def recording_project(points, pose, K_):
        pos, ok = project(points, pose, K_)
        fronts.append((ok.copy(), len(probe.radius_calls), bool(np.isfinite(points).all())))
        return pos, ok

    tracking.project = recording_project
    try:
        res = tracking.track(features, K, first_pose, plane_z, probe, settings)
    finally:
        tracking.project = project
    records = []
    for i, (ok, first, finite) in enumerate(fronts):
        last = fronts[i + 1][1] if i + 1 < len(fronts) else len(probe.radius_calls)
        records.append(FrameRecord(len(ok), finite, ok, last - first, probe.radius_calls[last - 1]))
    return res, records
