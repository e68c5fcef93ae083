"""Stereo map initialisation — host mirror of StereoMapInit
(Core/MAGESLAM/Source/Stereo/StereoMapInit.cpp:97-194).

`StereoMapInit(settings).Initialize(frame0, frame1, frame0ToFrame1)` is the whole call
(mage_stereo_map_init); the rest of the module is its device stage.

`triangulate_points` is one stereo pair through the crop mask, the two-way matcher and
MapInitialization::TriangulatePoints (Tracking/MapInitialization.cpp:911-986): backend "gpu" runs
mage_stereo_init_triangulate (the gfx950 kernels on one pair of host arrays), "host" runs
mage_stereo_init_triangulate_host (their plain C++ twin, which takes the matches as input);
`triangulate_batch_device` is the thin wrapper of the batched device entry; `overlap_crop` is the
crop rectangle Initialize computes from frame0ToFrame1 before all that (:100).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import DM_DTYPE, KP_DTYPE, SP_DTYPE, StereoInitSettingsC, check, ptr

ACCEPTED, EPIPOLAR, BEHIND, DISTANCE_RATIO, OCTAVE, BAD_INDEX = range(6)
MAX_KEYPOINTS = 4096
STATUS_OVER_LIMIT, STATUS_OVER_CAP = 1, 2


@dataclasses.dataclass
class StereoMapInitializationSettings:
    """StereoMapInitializationSettings (MageSettings.h:135-147) with its OrbMatcherSettings and
    BundleAdjustSettings bags (:36-52), in the reference's order."""
    min_init_map_points: int = 15
    min_feature_matches: int = 40
    max_outlier_error: float = 2.5  # Initialize never reads it (the bundle adjustment bag's is used)
    max_epipolar_error: float = 5.5
    min_accepted_distance_ratio: float = 2.0
    initialization_tether_strength: float = 50.0
    max_pose_contribution_z: float = 0.10
    amount_ba_can_change_pose: float = 1.65
    max_depth_meters: float = 2.3
    max_hamming_distance: int = 30
    min_hamming_difference: int = 1
    ba_num_steps: int = 1
    ba_num_steps_per_run: int = 1
    ba_min_steps: int = 1
    ba_huber_width: float = 1.8
    ba_huber_width_scale: float = 0.95
    ba_max_outlier_error: float = 7.25
    ba_max_outlier_error_scale_factor: float = 0.95
    ba_min_mean_square_error: float = 0.25
    ba_distance_tether_weight: float = 50.0
    ba_low_connectivity_iterations_scale: float = 1.5

    def to_c(self) -> StereoInitSettingsC:
        return StereoInitSettingsC.make(**dataclasses.asdict(self))


@dataclasses.dataclass
class StereoTriangulation:
    mask0: np.ndarray      # bool per frame-0 keypoint: inside the crop
    n_masked: int
    matches: np.ndarray    # DM_DTYPE, queryIdx = frame 0's keypoint, trainIdx = frame 1's
    verdicts: np.ndarray   # one code per match
    points: np.ndarray     # SP_DTYPE records, the accepted matches in match order (at most cap)
    ba_points: np.ndarray  # (n, 3)
    ba_uv: np.ndarray      # (2n, 2): frame 0's observations, then frame 1's
    ba_cam: np.ndarray     # (2n,)
    ba_pt: np.ndarray      # (2n,)
    ba_info: np.ndarray    # (2n,)
    status: int            # STATUS_* bits


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def scratch_bytes(pairs: int, pitch0: int) -> int:
    """Size of triangulate_batch_device's scratch: the packed descriptors and their indices."""
    return pairs * pitch0 * 36


def overlap_crop(frame0_to_frame1, camera0, camera1, max_depth_meters: float = 2.3):
    """The crop StereoMapInit::Initialize masks frame 0 with (StereoMapInit.cpp:100):
    CalculateOverlapCropSourceInTarget(frame0ToFrame1, frame 0's camera, frame 1's camera,
    MaxDepthMeters) -> (x, y, width, height) in frame 0.  The cameras are _lib.CameraConfig (their
    extrinsics are not read); the matrix is a row-major 4 x 4."""
    m = _f32(frame0_to_frame1, 16)
    crop = (C.c_int32 * 4)()
    check(_lib.load().mage_overlap_crop_source_in_target(ptr(m), C.byref(camera0), C.byref(camera1),
                                                         float(max_depth_meters), crop))
    return tuple(crop)


def triangulate_batch_device(settings, pairs: int, pos3, r9, intr4, crop, kp0, desc0, pitch0: int, n0, kp1, desc1,
                             pitch1: int, n1, mask0, n_masked, matches, match_cap: int, n_matches, verdict, out,
                             cap: int, n_out, ba_points, ba_uv, ba_cam, ba_pt, ba_info, status, scratch,
                             stream=None) -> None:
    """Batched device form over `pairs` stereo pairs (torch device tensors): crop mask, two-way
    match, triangulation and the bundle adjustment's inputs, three launches on `stream`.  With
    desc0 None the matcher is skipped and `matches` / `n_matches` are inputs (desc1 and scratch
    may be None too)."""
    cs = settings if isinstance(settings, StereoInitSettingsC) else settings.to_c()
    check(_lib.load().mage_stereo_init_triangulate_batch_device(
        C.byref(cs), pairs, ptr(pos3), ptr(r9), ptr(intr4), ptr(crop), ptr(kp0), ptr(desc0), pitch0, ptr(n0), ptr(kp1),
        ptr(desc1), pitch1, ptr(n1), ptr(mask0), ptr(n_masked), ptr(matches), match_cap, ptr(n_matches), ptr(verdict),
        ptr(out), cap, ptr(n_out), ptr(ba_points), ptr(ba_uv), ptr(ba_cam), ptr(ba_pt), ptr(ba_info), ptr(status),
        ptr(scratch), C.c_void_p(stream) if stream else None))


def _result(n0, mask0, n_masked, matches, n_matches, verdict, out, n_out, ba, status):
    n, nm = int(n_out), int(n_matches)
    over = bool(status & STATUS_OVER_LIMIT)
    return StereoTriangulation(
        np.zeros(n0, bool) if over else mask0[:n0].astype(bool), int(n_masked), matches[:nm].copy(), verdict[:nm].copy(),
        out[:n].copy(), ba[0][:3 * n].reshape(-1, 3).copy(), ba[1][:4 * n].reshape(-1, 2).copy(), ba[2][:2 * n].copy(),
        ba[3][:2 * n].copy(), ba[4][:2 * n].copy(), int(status))


def triangulate_points(settings, pos3, r9, intr4, crop, kp0, kp1, desc0=None, desc1=None, matches=None, cap=None,
                       backend: str = "gpu", device: int = 0) -> StereoTriangulation:
    """One stereo pair.  Poses as mage_ba_set_cameras takes them, frame 0 then frame 1: pos3 (2, 3)
    the view-space t, r9 (2, 9) the column-major R, intr4 (2, 4) {cx, cy, fx, fy}; crop the overlap
    rectangle {x, y, width, height} in frame 0; kp0 / kp1 KP_DTYPE arrays.  Either the descriptors
    (n x 32 bytes per frame; the GPU matcher runs, backend "gpu" only) or `matches` (DM_DTYPE,
    queryIdx = frame 0's keypoint) are given.  `cap` bounds the accepted points (default: every
    match)."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    if (matches is None) == (desc0 is None) or (desc0 is None) != (desc1 is None):
        raise ValueError("give either both descriptor sets or the matches")
    if backend == "host" and matches is None:
        raise ValueError("the host backend has no matcher: give the matches")
    cs = settings if isinstance(settings, StereoInitSettingsC) else settings.to_c()
    kp0 = np.ascontiguousarray(kp0, KP_DTYPE)
    kp1 = np.ascontiguousarray(kp1, KP_DTYPE)
    n0, n1 = len(kp0), len(kp1)
    pos3, r9, intr4 = _f32(pos3, 6), _f32(r9, 18), _f32(intr4, 8)
    crop = np.ascontiguousarray(np.asarray(crop, np.int32).reshape(4))
    ds = [None, None]
    if matches is not None:
        mm = np.ascontiguousarray(matches, DM_DTYPE).copy()
        match_cap = max(len(mm), 1)
        n_matches = C.c_uint32(len(mm))
        if len(mm) == 0:
            mm = np.zeros(1, DM_DTYPE)
    else:
        ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in (desc0, desc1)]
        if len(ds[0]) != n0 or len(ds[1]) != n1:
            raise ValueError("one 32-byte descriptor per keypoint")
        ds = [d if len(d) else np.zeros((1, 32), np.uint8) for d in ds]
        match_cap = max(n0, 1)
        mm = np.zeros(match_cap, DM_DTYPE)
        n_matches = C.c_uint32(0)
    cap = match_cap if cap is None else int(cap)
    ncap = max(cap, 1)
    mask0 = np.zeros(max(n0, 1), np.uint8)
    verdict = np.full(match_cap, 0xFF, np.uint8)
    out = np.zeros(ncap, SP_DTYPE)
    ba = [np.zeros(3 * ncap, np.float32), np.zeros(4 * ncap, np.float32), np.zeros(2 * ncap, np.uint32),
          np.zeros(2 * ncap, np.uint32), np.zeros(2 * ncap, np.float32)]
    n_masked, n_out, status = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    L = _lib.load()
    if backend == "host":
        check(L.mage_stereo_init_triangulate_host(
            C.byref(cs), ptr(pos3), ptr(r9), ptr(intr4), ptr(crop), ptr(kp0), n0, ptr(kp1), n1, ptr(mm),
            n_matches.value, ptr(mask0), C.byref(n_masked), ptr(verdict), ptr(out), cap, C.byref(n_out),
            *(ptr(b) for b in ba), C.byref(status)))
    else:
        check(L.mage_stereo_init_triangulate(
            C.byref(cs), ptr(pos3), ptr(r9), ptr(intr4), ptr(crop), ptr(kp0), ptr(ds[0]), n0, ptr(kp1), ptr(ds[1]), n1,
            ptr(mm), match_cap, C.byref(n_matches), ptr(mask0), C.byref(n_masked), ptr(verdict), ptr(out), cap,
            C.byref(n_out), *(ptr(b) for b in ba), C.byref(status), device))
    return _result(n0, mask0, n_masked.value, mm, n_matches.value, verdict, out, n_out.value, ba, status.value)


# ------------------------------------------------------------------------------------------
# StereoMapInit::Initialize as one call (mage_stereo_map_init)
# ------------------------------------------------------------------------------------------
OK, ZERO_DISPLACEMENT, FEW_MATCHES, FEW_POINTS, FAILED_VALIDATION = range(5)


@dataclasses.dataclass
class Frame:
    """What Initialize reads of an AnalyzedImage: the undistorted calibration and size (a
    _lib.CameraConfig; its extrinsics are not read), the keypoints and their descriptors."""
    camera: _lib.CameraConfig
    keypoints: np.ndarray    # KP_DTYPE
    descriptors: np.ndarray  # (n, 32) uint8


@dataclasses.dataclass
class InitializationData:
    """The reference's InitializationData for a stereo pair: two keyframe builders (frame 0 at the
    identity, frame 1 at `pos3` / `r9`: view-space t and column-major R) and the map points; point i
    is associated with keypoint associations[i, 0] of frame 0 and associations[i, 1] of frame 1."""
    pos3: np.ndarray
    r9: np.ndarray
    points: np.ndarray        # (n, 3)
    associations: np.ndarray  # (n, 2)


@dataclasses.dataclass
class StereoMapInitResult:
    code: int                # OK, ZERO_DISPLACEMENT, FEW_MATCHES, FEW_POINTS or FAILED_VALIDATION
    crop: tuple
    mask0: np.ndarray
    n_masked: int
    matches: np.ndarray      # DM_DTYPE
    verdicts: np.ndarray     # empty until TriangulatePoints ran
    pos3: np.ndarray         # frame 1's pose
    r9: np.ndarray
    points: np.ndarray       # SP_DTYPE: the surviving points, positions from the bundle adjustment
    ba_outliers: np.ndarray  # observation indices over the runs
    ba_runs: int


class StereoMapInit:
    """StereoMapInit (Stereo/StereoMapInit.h:23-35) over mage_stereo_map_init."""

    def __init__(self, settings: StereoMapInitializationSettings | None = None, device: int = 0):
        self.settings = settings or StereoMapInitializationSettings()
        self.device = device
        self.last = None  # the StereoMapInitResult of the last Initialize

    def run(self, frame0: Frame, frame1: Frame, frame0ToFrame1) -> StereoMapInitResult:
        cs = self.settings.to_c()
        kp0, kp1 = np.ascontiguousarray(frame0.keypoints, KP_DTYPE), np.ascontiguousarray(frame1.keypoints, KP_DTYPE)
        d0 = np.ascontiguousarray(frame0.descriptors, np.uint8).reshape(-1, 32)
        d1 = np.ascontiguousarray(frame1.descriptors, np.uint8).reshape(-1, 32)
        n0, n1 = len(kp0), len(kp1)
        if len(d0) != n0 or len(d1) != n1:
            raise ValueError("one 32-byte descriptor per keypoint")
        cap = max(n0, 1)
        runs = self.settings.ba_num_steps // max(self.settings.ba_num_steps_per_run, 1) + 2
        res = _lib.StereoMapInitResultC()
        mask0, verdict = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        matches, points = np.zeros(cap, DM_DTYPE), np.zeros(cap, SP_DTYPE)
        outl = np.zeros(2 * cap * runs, np.uint32)
        check(_lib.load().mage_stereo_map_init(
            C.byref(cs), ptr(_f32(frame0ToFrame1, 16)), C.byref(frame0.camera), C.byref(frame1.camera), ptr(kp0), ptr(d0),
            n0, ptr(kp1), ptr(d1), n1, C.byref(res), ptr(mask0), ptr(matches), ptr(verdict), ptr(points), ptr(outl),
            self.device))
        self.last = StereoMapInitResult(
            int(res.code), tuple(res.crop), mask0[:n0].astype(bool), int(res.n_masked), matches[: res.n_matches].copy(),
            verdict[: res.n_verdicts].copy(), np.array(res.frame1_pos3, np.float32), np.array(res.frame1_r9, np.float32),
            points[: res.n_points].copy(), outl[: res.n_ba_outliers].copy(), int(res.ba_runs))
        return self.last

    def Initialize(self, frame0: Frame, frame1: Frame, frame0ToFrame1):
        """-> InitializationData, or None where the reference returns boost::none (self.last.code says
        why)."""
        r = self.run(frame0, frame1, frame0ToFrame1)
        if r.code != OK:
            return None
        return InitializationData(r.pos3, r.r9, r.points["position"].copy(),
                                  np.stack([r.points["query_idx"], r.points["train_idx"]], 1))


def host_scalars(frame0_to_frame1, settings=None):
    """Initialize's float scalars (mage_debug_stereo_init_host): (zero displacement, normalised
    frame0ToFrame1 (4, 4), frame 1's pos3, r9 column-major, the 7 tether parameters)."""
    cs = (settings or StereoMapInitializationSettings()).to_c()
    zero = C.c_int32(0)
    nrm, pos3, r9, t7 = (np.zeros(k, np.float32) for k in (16, 3, 9, 7))
    check(_lib.load().mage_debug_stereo_init_host(C.byref(cs), ptr(_f32(frame0_to_frame1, 16)), C.byref(zero), ptr(nrm),
                                                  ptr(pos3), ptr(r9), ptr(t7), 0, None, 0, None, None, None, None, None))
    return bool(zero.value), nrm.reshape(4, 4), pos3, r9, t7


def cull_order(n_points: int, outliers, settings=None) -> np.ndarray:
    """The surviving points' indices after BundleAdjustInitializationData's culling."""
    cs = (settings or StereoMapInitializationSettings()).to_c()
    o = np.ascontiguousarray(outliers, np.uint32)
    order, left = np.zeros(max(n_points, 1), np.uint32), C.c_uint32(0)
    check(_lib.load().mage_debug_stereo_init_host(C.byref(cs), None, None, None, None, None, None, n_points, ptr(o), len(o),
                                                  ptr(order), C.byref(left), None, None, None))
    return order[: left.value].copy()


def validate(settings, n_points: int, pos3, r9) -> bool:
    """ValidateInitializationData for frame 1's pose and the surviving point count."""
    cs = settings.to_c()
    ok = C.c_int32(0)
    check(_lib.load().mage_debug_stereo_init_host(C.byref(cs), None, None, None, None, None, None, n_points, None, 0, None,
                                                  None, ptr(_f32(pos3, 3)), ptr(_f32(r9, 9)), C.byref(ok)))
    return bool(ok.value)
