"""Relocalisation — host mirror of PoseEstimator::PNPRansac with the steps around it in
TryEstimatePoseFromCandidates (Core/MAGESLAM/Source/Tracking/PoseEstimator.cpp:291-342, :610-638).

`pnp_ransac` is one (lost frame, candidate keyframe) problem: the MinBruteForceCorrespondences gate,
the RANSAC over EPnP on five points, the winner's inliers without those behind the camera, the
RansacInliersPctRequired gate, and for an OK problem the inputs of BundleAdjustPose.  Backend "hip"
runs mage_reloc_pnp (the gfx950 kernels on host arrays), "host" runs mage_reloc_pnp_host (their plain
C++ twin).  `pnp_ransac_batch_device` is the thin wrapper of the batched device entry over torch
tensors, and `pose_inputs` hands its outputs to the bundler's batched pose-only bundle adjustment.
The rest of TryEstimatePoseFromCandidates (the candidates, the matcher, the guided search, the second
bundle adjustment) is composed by the caller from the calls the package already has.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import DM_DTYPE, KP_DTYPE, RP_RESULT_DTYPE, RelocSettingsC, check, ptr

OK, FEW_MATCHES, NO_MODEL, FEW_INLIERS = range(4)
VERDICT_NAMES = ("ok", "few matches", "no model", "few inliers")
STATUS_OVER_LIMIT, STATUS_OVER_CAP, STATUS_BAD_INDEX = 1, 2, 4
MAX_MATCHES = 4096
MAX_ITERATIONS = 256


@dataclasses.dataclass
class RelocalizationSettings:
    """RelocalizationSettings (MageSettings.h:236-250) with its OrbMatcherSettings bag, in the
    reference's order."""
    min_brute_force_correspondences: int = 20
    min_radius_match_correspondences: int = 15
    min_map_points: int = 10
    ransac_inliers_pct_required: float = 0.4
    bundle_adjust_inliers_pct_required: float = 0.4
    ransac_confidence: float = 0.6
    round_robin_iterations: int = 5
    ransac_iterations: int = 2
    bundle_adjust_iterations: int = 10
    search_radius: float = 20.0
    max_bundle_adjust_reprojection_error: float = 8.0
    max_bundle_pnp_reprojection_error: float = 8.0
    max_hamming_distance: int = 30
    min_hamming_difference: int = 1

    def to_c(self) -> RelocSettingsC:
        return RelocSettingsC.make(**dataclasses.asdict(self))


def _c(settings) -> RelocSettingsC:
    return settings if isinstance(settings, RelocSettingsC) else settings.to_c()


def trace_bytes(iterations: int) -> int:
    return int(_lib.load().mage_reloc_pnp_trace_bytes(iterations))


def scratch_bytes(iterations: int, problems: int, match_cap: int, with_trace: bool) -> int:
    """Size of pnp_ransac_batch_device's scratch."""
    return int(_lib.load().mage_reloc_pnp_scratch_bytes(iterations, problems, match_cap, int(with_trace)))


def trace_dtype(iterations: int) -> np.dtype:
    """One problem's trace as a structured scalar (mage_hot.h, mage_reloc_pnp_trace_bytes)."""
    it = iterations
    fields = [("R", "<f8", (it, 3, 3)), ("t", "<f8", (it, 3)), ("err", "<f8", (it, 3)), ("indices", "<i4", (it, 5)),
              ("solved", "<i4", (it,)), ("inliers", "<u4", (it,))]
    if it % 2:
        fields.append(("pad", "<u4"))
    return np.dtype(fields)


@dataclasses.dataclass
class PnPRansac:
    verdict: int             # OK ... FEW_INLIERS
    status: int              # STATUS_* bits
    result: np.void          # the whole mage_reloc_pnp_result (RP_RESULT_DTYPE)
    pos3: np.ndarray         # view-space t of the winning hypothesis (zero without one)
    r9: np.ndarray           # its column-major R (the identity without one)
    inliers: np.ndarray      # (n_kept,) the winner's in-front inliers as match indices, in match order
    points3: np.ndarray      # (n_kept, 3) BundleAdjustPose's map points (OK only)
    uv: np.ndarray           # (n_kept, 2) its observations
    info: np.ndarray         # (n_kept,) their information values
    trace: np.void | None    # trace_dtype(iterations) scalar when asked for and the RANSAC ran

    @property
    def ok(self) -> bool:
        return self.status & (STATUS_OVER_LIMIT | STATUS_BAD_INDEX) == 0 and self.verdict == OK


def pnp_ransac(settings, intr4, map_xyzi, kp, matches, backend: str = "hip", want_trace: bool = False, cap=None,
               device: int = 0) -> PnPRansac:
    """One problem.  intr4 = {cx, cy, fx, fy} of the current frame's undistorted calibration; map_xyzi
    (n_kf, 4) the candidate keyframe's keypoints' map points {x, y, z, information}, information <= 0
    for a keypoint with none; kp the current frame's KP_DTYPE keypoints; matches DM_DTYPE with
    query_idx into the candidate and train_idx into the current frame.  `cap` bounds the kept inliers
    (default: every match)."""
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    cs = _c(settings)
    intr4 = np.ascontiguousarray(np.asarray(intr4, np.float32).reshape(4))
    mp = np.ascontiguousarray(np.asarray(map_xyzi, np.float32).reshape(-1, 4))
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    mm = np.ascontiguousarray(matches, DM_DTYPE)
    cap = len(mm) if cap is None else int(cap)
    ncap = max(cap, 1)
    result = np.zeros(1, RP_RESULT_DTYPE)
    idx = np.zeros(ncap, np.uint32)
    points3, uv, info = np.zeros((ncap, 3), np.float32), np.zeros((ncap, 2), np.float32), np.zeros(ncap, np.float32)
    iters = int(cs.ransac_iterations)
    L = _lib.load()
    trace = np.zeros(1, trace_dtype(iters)) if want_trace else None
    if trace is not None and trace.nbytes != L.mage_reloc_pnp_trace_bytes(iters):
        raise RuntimeError("trace layout mismatch")
    args = (C.byref(cs), ptr(intr4), ptr(mp), len(mp), ptr(kp), len(kp), ptr(mm), len(mm), ptr(result), ptr(idx), cap,
            ptr(points3), ptr(uv), ptr(info), ptr(trace))
    if backend == "host":
        check(L.mage_reloc_pnp_host(*args))
    else:
        check(L.mage_reloc_pnp(*args, device))
    r = result[0]
    stopped = int(r["status"]) & (STATUS_OVER_LIMIT | STATUS_BAD_INDEX) or int(r["verdict"]) == FEW_MATCHES
    ran = not stopped and len(mm) >= 5
    n = 0 if stopped else int(r["n_kept"])
    nb = n if int(r["verdict"]) == OK else 0
    return PnPRansac(int(r["verdict"]), int(r["status"]), r.copy(), r["pos3"].copy(), r["r9"].copy(), idx[:n].copy(),
                     points3[:nb].copy(), uv[:nb].copy(), info[:nb].copy(), trace[0].copy() if want_trace and ran else None)


def pnp_ransac_batch_device(settings, problems: int, intr4, map_xyzi, kf_pitch: int, kp, kp_pitch: int, n_kp, matches,
                            match_cap: int, n_matches, result, inlier_idx, cap: int, obs_start, points3, uv, info, pos3,
                            r9, trace=None, scratch=None, stream=None) -> None:
    """Batched device form over `problems` problems (torch device tensors), launches on `stream`;
    layouts in mage_hot.h.  `result`: problems x 104 bytes (RP_RESULT_DTYPE); `trace`: None or problems
    x trace_bytes(iterations) bytes; `scratch`: scratch_bytes(...) bytes, 256-byte aligned."""
    check(_lib.load().mage_reloc_pnp_batch_device(
        C.byref(_c(settings)), problems, ptr(intr4), ptr(map_xyzi), kf_pitch, ptr(kp), kp_pitch, ptr(n_kp), ptr(matches),
        match_cap, ptr(n_matches), ptr(result), ptr(inlier_idx), cap, ptr(obs_start), ptr(points3), ptr(uv), ptr(info),
        ptr(pos3), ptr(r9), ptr(trace), ptr(scratch), C.c_void_p(stream) if stream else None))


def pose_inputs(intr4, obs_start, points3, uv, info, pos3, r9) -> dict:
    """The stage's outputs as the keyword arguments of the bundler's batched pose-only bundle
    adjustment (bundler.pose_batch_device / mage_ba_pose_batch_device), unchanged: BundleAdjustPose (:346)
    on every problem's in-front inliers, a problem that is not OK contributing no observation."""
    return dict(pos3=pos3, r9=r9, intr4=intr4, obs_start=obs_start, points3=points3, uv=uv, info=info)
