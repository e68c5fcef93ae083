"""Monocular map initialisation — host mirror of the two-view geometry of
MapInitialization::InitializeWithFrames (Core/MAGESLAM/Source/Tracking/MapInitialization.cpp:988-1094).

`initialize_with_frames` is one frame pair through CollectMatchPoints, FindPossiblePoses (the
five-point RANSAC), FindEssentialPotientialPoses and FindCorrectPose: backend "gpu" runs
mage_mono_init_two_view (the gfx950 kernels on one pair of host arrays, with the two-way matcher in
front when descriptors are given), "host" runs mage_mono_init_two_view_host (their plain C++ twin,
which takes the matches as input).  `two_view_batch_device` is the thin wrapper of the batched
device entry over torch tensors.

`locate_third_frame` is the third frame of TryIntializeMapWithProvidedFrames (:695-840): backend
"gpu" runs mage_mono_init_third_frame (match kernel, pack, the pose-only bundle adjustment, finish),
"host" runs mage_mono_init_third_frame_host, which takes the bundle adjustment's outcome as input.
`third_frame_batch_device` is the batched device entry over torch tensors.  The rest of
TryIntializeMapWithProvidedFrames (new points, the init bundle adjustments, validation) is composed by
the caller from the calls the package already has.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import DM_DTYPE, KP_DTYPE, M3_RESULT_DTYPE, MI_RESULT_DTYPE, SP_DTYPE, MonoInitSettingsC, check, ptr

OK, FEW_MATCHES, NO_HYPOTHESIS, NO_VALID_POSE, TOO_SIMILAR, Z_BIASED = range(6)
VERDICT_NAMES = ("ok", "few matches", "no hypothesis", "no pose with a valid score", "best poses too similar",
                 "pose too biased in Z")
STATUS_OVER_LIMIT, STATUS_OVER_CAP, STATUS_BAD_INDEX = 1, 2, 4
POSE_TWISTED, POSE_ENOUGH, POSE_MEDIAN_OK = 1, 2, 4
MAX_KEYPOINTS = 4096
MAX_MATCHES = 4096
MAX_ITERATIONS = 256


@dataclasses.dataclass
class MonoMapInitializationSettings:
    """MonoMapInitializationSettings (MageSettings.h:95-128) with its two OrbMatcherSettings bags, in
    the reference's order."""
    fundamental_transfer_error_threshold: float = 1.1
    min_feature_matches: int = 65
    min_scoring_inliers: int = 50
    min_inlier_percentage: float = 0.5
    min_initial_map_points: int = 40
    min_map_points: int = 60
    min_third_frame_match_percentage: float = 0.5
    feature_covisibility_threshold: float = 0.35
    max_parallax_3d_distance: float = 500.0
    max_parallax_3d_median_distance: float = 20.0
    min_candidate_pose_disimilarity: float = 0.3
    max_pose_contribution_z: float = 0.66
    bundle_adjustment_g2o_steps: int = 5
    bundle_adjustment_huber_width: float = 1.5
    ransac_iterations_for_models: int = 90
    max_epipolar_error: float = 3.5
    max_outlier_error: float = 2.5
    amount_ba_can_change_pose: float = 1.65
    map_initialization_new_points_creation_min_distance: float = 0.25
    map_init_frame_interval_milliseconds: int = 0
    min_initialization_interval_milliseconds: int = 150
    max_initialization_interval_milliseconds: int = 540
    min_pixel_spread: float = 40.0
    final_ba_huber_width: float = 0.9
    final_ba_max_outlier_error: float = 4.0
    final_ba_max_outlier_error_scale_factor: float = 0.75
    final_ba_min_mean_square_error: float = 0.0
    final_ba_num_steps_per_run: int = 5
    final_ba_num_steps: int = 15
    extra_frame_max_outlier_error: float = 8.0
    extra_frame_bundle_adjustment_steps: int = 5
    extra_frame_huber_width: float = 4.0
    extra_frame_search_radius: float = 40.0
    five_point_max_hamming_distance: int = 30
    five_point_min_hamming_difference: int = 1
    extra_frame_max_hamming_distance: int = 30
    extra_frame_min_hamming_difference: int = 1

    def to_c(self) -> MonoInitSettingsC:
        return MonoInitSettingsC.make(**dataclasses.asdict(self))


def trace_bytes(iterations: int) -> int:
    return int(_lib.load().mage_mono_init_trace_bytes(iterations))


def scratch_bytes(iterations: int, pairs: int, pitch0: int, pitch1: int, with_trace: bool, with_matcher: bool) -> int:
    """Size of two_view_batch_device's scratch."""
    return int(_lib.load().mage_mono_init_scratch_bytes(iterations, pairs, pitch0, pitch1, int(with_trace),
                                                        int(with_matcher)))


def trace_dtype(iterations: int) -> np.dtype:
    """One pair's trace as a structured scalar (mage_hot.h, mage_mono_init_trace_bytes)."""
    it = iterations
    return np.dtype([("indices", "<i4", (it, 5)), ("candidates", "<i4", (it,)), ("E", "<f4", (it, 10, 3, 3)),
                     ("score", "<f4", (it, 10)), ("inliers", "<u4", (it, 10)), ("cheirality", "<u4", (it, 10))])


@dataclasses.dataclass
class TwoView:
    verdict: int             # OK ... Z_BIASED
    status: int              # STATUS_* bits
    result: np.void          # the whole mage_mono_init_result (MI_RESULT_DTYPE)
    matches: np.ndarray      # DM_DTYPE, the matches the stage ran on
    pos3: np.ndarray         # (2, 3) view-space t of frame 0 (zero) and frame 1
    r9: np.ndarray           # (2, 9) column-major R of frame 0 (identity) and frame 1
    points: np.ndarray       # SP_DTYPE records, the accepted matches in match order
    ba_points: np.ndarray    # (n, 3)
    ba_uv: np.ndarray        # (2n, 2): frame 0's observations, then frame 1's
    ba_cam: np.ndarray       # (2n,)
    ba_pt: np.ndarray        # (2n,)
    ba_info: np.ndarray      # (2n,)
    trace: np.void | None    # trace_dtype(iterations) scalar when asked for and the stage ran

    @property
    def ok(self) -> bool:
        return self.status & (STATUS_OVER_LIMIT | STATUS_BAD_INDEX) == 0 and self.verdict == OK


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def two_view_batch_device(settings, pairs: int, intr4, kp0, desc0, pitch0: int, n0, kp1, desc1, pitch1: int, n1,
                          matches, match_cap: int, n_matches, result, out, cap: int, ba_points, ba_uv, ba_cam, ba_pt,
                          ba_info, trace=None, scratch=None, stream=None) -> None:
    """Batched device form over `pairs` frame pairs (torch device tensors), launches on `stream`.
    With desc0 None the matcher is skipped and `matches` / `n_matches` are inputs.  `result`: pairs x
    408 bytes (MI_RESULT_DTYPE); `trace`: None or pairs x trace_bytes(iterations) bytes; `scratch`:
    scratch_bytes(...) bytes."""
    cs = settings if isinstance(settings, MonoInitSettingsC) else settings.to_c()
    check(_lib.load().mage_mono_init_two_view_batch_device(
        C.byref(cs), pairs, ptr(intr4), ptr(kp0), ptr(desc0), pitch0, ptr(n0), ptr(kp1), ptr(desc1), pitch1, ptr(n1),
        ptr(matches), match_cap, ptr(n_matches), ptr(result), ptr(out), cap, ptr(ba_points), ptr(ba_uv), ptr(ba_cam),
        ptr(ba_pt), ptr(ba_info), ptr(trace), ptr(scratch), C.c_void_p(stream) if stream else None))


def initialize_with_frames(settings, intr4, kp0, kp1, desc0=None, desc1=None, matches=None, cap=None,
                           backend: str = "gpu", device: int = 0, want_trace: bool = False) -> TwoView:
    """One frame pair.  intr4 (2, 4) = {cx, cy, fx, fy} of frame 0 (the reference frame, the matches'
    queryIdx side) and frame 1; kp0 / kp1 KP_DTYPE arrays of undistorted keypoints.  Either the
    descriptors (n x 32 bytes per frame; the GPU matcher runs over the octave-0 keypoints, backend
    "gpu" only) or `matches` (DM_DTYPE) are given.  `cap` bounds the accepted points (default: every
    match)."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    if (matches is None) == (desc0 is None) or (desc0 is None) != (desc1 is None):
        raise ValueError("give either both descriptor sets or the matches")
    if backend == "host" and matches is None:
        raise ValueError("the host backend has no matcher: give the matches")
    cs = settings if isinstance(settings, MonoInitSettingsC) else settings.to_c()
    kp0 = np.ascontiguousarray(kp0, KP_DTYPE)
    kp1 = np.ascontiguousarray(kp1, KP_DTYPE)
    n0, n1 = len(kp0), len(kp1)
    intr4 = _f32(intr4, 8)
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
        match_cap = max(min(n0, MAX_MATCHES), 1)
        mm = np.zeros(match_cap, DM_DTYPE)
        n_matches = C.c_uint32(0)
    cap = match_cap if cap is None else int(cap)
    ncap = max(cap, 1)
    result = np.zeros(1, MI_RESULT_DTYPE)
    out = np.zeros(ncap, SP_DTYPE)
    ba = [np.zeros(3 * ncap, np.float32), np.zeros(4 * ncap, np.float32), np.zeros(2 * ncap, np.uint32),
          np.zeros(2 * ncap, np.uint32), np.zeros(2 * ncap, np.float32)]
    iters = int(cs.ransac_iterations_for_models)
    L = _lib.load()
    trace = np.zeros(1, trace_dtype(iters)) if want_trace else None
    if trace is not None and trace.nbytes != L.mage_mono_init_trace_bytes(iters):
        raise RuntimeError("trace layout mismatch")
    if backend == "host":
        check(L.mage_mono_init_two_view_host(
            C.byref(cs), ptr(intr4), ptr(kp0), n0, ptr(kp1), n1, ptr(mm), n_matches.value, ptr(result), ptr(out), cap,
            *(ptr(b) for b in ba), ptr(trace)))
    else:
        check(L.mage_mono_init_two_view(
            C.byref(cs), ptr(intr4), ptr(kp0), ptr(ds[0]), n0, ptr(kp1), ptr(ds[1]), n1, ptr(mm), match_cap,
            C.byref(n_matches), ptr(result), ptr(out), cap, *(ptr(b) for b in ba), ptr(trace), device))
    r = result[0]
    n, nm = int(r["n_points"]), int(n_matches.value)
    ran = not (int(r["status"]) & (STATUS_OVER_LIMIT | STATUS_BAD_INDEX)) and int(r["verdict"]) != FEW_MATCHES
    return TwoView(int(r["verdict"]), int(r["status"]), r.copy(), mm[:nm].copy(), r["pos3"].reshape(2, 3).copy(),
                   r["r9"].reshape(2, 9).copy(), out[:n].copy(), ba[0][:3 * n].reshape(-1, 3).copy(),
                   ba[1][:4 * n].reshape(-1, 2).copy(), ba[2][:2 * n].copy(), ba[3][:2 * n].copy(),
                   ba[4][:2 * n].copy(), trace[0].copy() if want_trace and ran else None)


# ---------------------------------------------------------------------------------------------
# the third frame (MapInitialization.cpp:695-840)
# ---------------------------------------------------------------------------------------------
M3_OK, M3_FEW_MATCHES, M3_FEW_AFTER_CULL = range(3)
M3_VERDICT_NAMES = ("ok", "too few matches", "too few after culling")
M3_STATUS_OVER_LIMIT, M3_STATUS_BAD_INDEX = 1, 2
M3_PT_BEHIND, M3_PT_NO_MATCH, M3_PT_FRAME0, M3_PT_FRAME1, M3_PT_CULLED = range(5)
M3_MAX_POINTS = 4096
M3_SCRATCH_ARRAYS = ("obs_start", "ba_count", "ba_pos3", "ba_r9", "matched", "ba_points", "ba_uv", "ba_info", "outlier",
                     "opt_pos3", "opt_r9", "mean_sq", "opt_qt7")


def third_scratch_layout(problems: int, cap: int) -> tuple[int, dict]:
    """(bytes, {array: byte offset}) of third_frame_batch_device's scratch (mage_hot.h)."""
    off = (C.c_uint64 * len(M3_SCRATCH_ARRAYS))()
    n = int(_lib.load().mage_mono_init_third_scratch_bytes(problems, cap, off))
    return n, dict(zip(M3_SCRATCH_ARRAYS, (int(o) for o in off)))


@dataclasses.dataclass
class ThirdFrame:
    verdict: int             # M3_OK / M3_FEW_MATCHES / M3_FEW_AFTER_CULL
    status: int              # M3_STATUS_* bits
    result: np.void          # the whole mage_mono_init_third_result (M3_RESULT_DTYPE)
    pos3: np.ndarray         # the frame's pose: the midpoint pose (the reference keeps it, :840)
    r9: np.ndarray
    opt_pos3: np.ndarray     # OptimizeCameraPose's result
    opt_r9: np.ndarray
    keypoint: np.ndarray     # (n,) the point's keypoint in the third frame, or -1
    point_verdict: np.ndarray  # (n,) M3_PT_*
    dist: np.ndarray         # (n, 2) best distance of frame 0's / frame 1's query, or -1
    proj: np.ndarray         # (n, 2) the point's projection through the midpoint pose
    mask: np.ndarray         # (n2,) bool: still unassociated after the matching
    obs_uv: np.ndarray       # (n_associated, 2) the surviving associations as BA observations
    obs_pt: np.ndarray
    obs_cam: np.ndarray
    obs_info: np.ndarray
    outlier: np.ndarray | None  # gpu: (n_matched,) the bundle adjustment's flags in point order
    ba_points: np.ndarray | None  # host: the bundle adjustment's inputs, (n_matched, 3)
    ba_uv: np.ndarray | None
    ba_info: np.ndarray | None

    @property
    def ok(self) -> bool:
        return self.status == 0 and self.verdict == M3_OK


def locate_third_frame(settings, intr4, pos3, r9, points, idx0, idx1, desc0, desc1, kp2, desc2, cam_index: int = 1,
                       backend: str = "gpu", device: int = 0, outlier=None, opt_pos3=None, opt_r9=None,
                       mean_sq: float = 0.0) -> ThirdFrame:
    """One third frame.  intr4 {cx, cy, fx, fy} of the third frame; pos3 (2, 3) / r9 (2, 9) the poses of
    frame 0 and frame 1 (view-space t, column-major R); points (n, 3) in MapPoints order with their
    keypoint indices idx0 / idx1 into desc0 / desc1 (n x 32 bytes each); kp2 / desc2 the third frame.
    backend "host" has no bundle adjustment: without `outlier` it stops after the first gate, with it
    (n_matched flags in point order, plus opt_pos3, opt_r9, mean_sq) it finishes."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    cs = settings if isinstance(settings, MonoInitSettingsC) else settings.to_c()
    pts = _f32(points, (-1, 3))
    n = len(pts)
    i0 = np.ascontiguousarray(idx0, np.int32).reshape(-1)
    i1 = np.ascontiguousarray(idx1, np.int32).reshape(-1)
    if len(i0) != n or len(i1) != n:
        raise ValueError("one keypoint index per point and frame")
    d0 = np.ascontiguousarray(desc0, np.uint8).reshape(-1, 32)
    d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
    kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
    d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    n2 = len(kp2)
    if len(d2) != n2:
        raise ValueError("one 32-byte descriptor per keypoint")
    intr4, pos3, r9 = _f32(intr4, 4), _f32(pos3, 6), _f32(r9, 18)
    m = max(n, 1)
    result = np.zeros(1, M3_RESULT_DTYPE)
    keypoint, verdict, dist = np.full(m, -1, np.int32), np.zeros(m, np.uint8), np.full((m, 2), -1, np.int32)
    proj = np.zeros((m, 2), np.float32)
    mask = np.ones(max(n2, 1), np.uint8)
    obs = [np.zeros((m, 2), np.float32), np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.float32)]
    L = _lib.load()
    flags = ba = None
    if backend == "host":
        ba = [np.zeros((m, 3), np.float32), np.zeros((m, 2), np.float32), np.zeros(m, np.float32)]
        if outlier is not None:
            outlier = np.ascontiguousarray(outlier, np.uint8)
            opt_pos3, opt_r9 = _f32(opt_pos3, 3), _f32(opt_r9, 9)
        check(L.mage_mono_init_third_frame_host(
            C.byref(cs), ptr(intr4), ptr(pos3), ptr(r9), ptr(pts), n, ptr(i0), ptr(i1), ptr(d0), len(d0), ptr(d1), len(d1),
            ptr(kp2), ptr(d2), n2, cam_index, ptr(outlier), ptr(opt_pos3), ptr(opt_r9), float(mean_sq), ptr(result),
            ptr(keypoint), ptr(verdict), ptr(dist), ptr(proj), ptr(mask), *(ptr(o) for o in obs), *(ptr(b) for b in ba)))
    else:
        flags = np.zeros(m, np.uint8)
        check(L.mage_mono_init_third_frame(
            C.byref(cs), ptr(intr4), ptr(pos3), ptr(r9), ptr(pts), n, ptr(i0), ptr(i1), ptr(d0), len(d0), ptr(d1), len(d1),
            ptr(kp2), ptr(d2), n2, cam_index, ptr(result), ptr(keypoint), ptr(verdict), ptr(dist), ptr(proj),
            ptr(mask), *(ptr(o) for o in obs), ptr(flags), device))
    r = result[0]
    bad = int(r["status"]) != 0
    nm = 0 if bad else int(r["n_matched"])
    finished = not bad and (backend == "gpu" or outlier is not None or int(r["verdict"]) == M3_FEW_MATCHES)
    na = int(r["n_associated"]) if finished else 0
    nk = 0 if bad else n
    ran = not bad and int(r["verdict"]) != M3_FEW_MATCHES
    return ThirdFrame(int(r["verdict"]), int(r["status"]), r.copy(), r["pos3"].copy(), r["r9"].copy(), r["opt_pos3"].copy(),
                      r["opt_r9"].copy(), keypoint[:nk].copy(), verdict[:nk].copy(), dist[:nk].copy(), proj[:nk].copy(),
                      mask[:0 if bad else n2].astype(bool), obs[0][:na].copy(), obs[1][:na].copy(), obs[2][:na].copy(),
                      obs[3][:na].copy(), flags[:nm if ran else 0].copy() if flags is not None else None,
                      *((b[:nm].copy() for b in ba) if ba is not None else (None, None, None)))


def third_frame_batch_device(settings, problems: int, intr4, pos3, r9, points, cap: int, n_points, idx0, idx1, desc0,
                             pitch0: int, n0, desc1, pitch1: int, n1, kp2, desc2, pitch2: int, n2, cam_index: int, result,
                             keypoint, verdict, dist, proj, mask, obs_uv, obs_pt, obs_cam, obs_info, scratch,
                             stream=None) -> None:
    """Batched device form over `problems` third frames (torch device tensors), launches on `stream`;
    layouts in mage_hot.h.  `result`: problems x 128 bytes (M3_RESULT_DTYPE); `scratch`:
    third_scratch_layout(problems, cap)[0] bytes, 256-byte aligned."""
    cs = settings if isinstance(settings, MonoInitSettingsC) else settings.to_c()
    check(_lib.load().mage_mono_init_third_frame_batch_device(
        C.byref(cs), problems, ptr(intr4), ptr(pos3), ptr(r9), ptr(points), cap, ptr(n_points), ptr(idx0), ptr(idx1),
        ptr(desc0), pitch0, ptr(n0), ptr(desc1), pitch1, ptr(n1), ptr(kp2), ptr(desc2), pitch2, ptr(n2), cam_index,
        ptr(result), ptr(keypoint), ptr(verdict), ptr(dist), ptr(proj), ptr(mask), ptr(obs_uv), ptr(obs_pt), ptr(obs_cam),
        ptr(obs_info), ptr(scratch), C.c_void_p(stream) if stream else None))
