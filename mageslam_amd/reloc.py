"""Relocalisation — host mirror of PoseEstimator::PNPRansac with the steps around it in
TryEstimatePoseFromCandidates (Core/MAGESLAM/Source/Tracking/PoseEstimator.cpp:291-342, :610-638).

`pnp_ransac` is one (lost frame, candidate keyframe) problem: the MinBruteForceCorrespondences gate,
the RANSAC over EPnP on five points, the winner's inliers without those behind the camera, the
RansacInliersPctRequired gate, and for an OK problem the inputs of BundleAdjustPose.  Backend "hip"
runs mage_reloc_pnp (the gfx950 kernels on host arrays), "host" runs mage_reloc_pnp_host (their plain
C++ twin).  `pnp_ransac_batch_device` is the thin wrapper of the batched device entry over torch
tensors, and `pose_inputs` hands its outputs to the bundler's batched pose-only bundle adjustment.

`guided_search` is the rest of the routine behind PNPRansac (:346-436) for one lost frame and its
candidates: the first BundleAdjustPose, the guided search over each candidate's map points, the
second BundleAdjustPose, the three gates and the choice of the candidate.  Backend "hip" runs
mage_reloc_guided (the PnP stage and the guided stage on one stream); "host" runs the plain C++ twins
phase by phase, with the pose bundle adjustment and RadiusMatch between the phases supplied by the
caller (default: the package's host-buffer GPU entries, which the library has no CPU form of).
`guided_search_batch_device` and `candidates_batch_device` are the thin wrappers of the batched
device entries, and `try_estimate_pose_from_candidates` is the routine from IndexedMatch on.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import (DM_DTYPE, KP_DTYPE, RG_FRAME_DTYPE, RG_RESULT_DTYPE, RP_RESULT_DTYPE, RelocCandidatesArgsC,
                   RelocGuidedArgsC, RelocSettingsC, check, ptr)

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


# ----------------------------------------------------------------------------------------------
# The rest of TryEstimatePoseFromCandidates behind PNPRansac (:346-436)
# ----------------------------------------------------------------------------------------------
RG_OK, RG_SKIPPED, RG_FEW_RADIUS_MATCHES, RG_FEW_MAP_POINTS, RG_FEW_BA_INLIERS = range(5)
RG_VERDICT_NAMES = ("ok", "skipped", "few radius matches", "few map points", "few BA inliers")
RG_STATUS_OVER_LIMIT, RG_STATUS_OVER_CAP, RG_STATUS_BAD_ORDER = 1, 2, 4
MAX_KEYPOINTS = 4096
HUBER_WIDTH = 1.8            # BundleAdjustSettings' default HuberWidth, used by both BundleAdjustPose calls
POSE_MATCHER = (30, 1)       # PoseEstimationSettings.OrbMatcherSettings (MageSettings.h:170-)


@dataclasses.dataclass
class Candidate:
    """A candidate keyframe: per keypoint its map point {x, y, z, information} (information <= 0:
    none), the keypoints and descriptors; `order` None, or the associated keypoints' indices in
    IterateAssociations' order; `ba_intr4` None (the lost frame's) or the candidate's intrinsics."""
    map_xyzi: np.ndarray
    kp: np.ndarray
    desc: np.ndarray
    order: np.ndarray | None = None
    ba_intr4: np.ndarray | None = None

    def __post_init__(self):
        self.map_xyzi = np.ascontiguousarray(np.asarray(self.map_xyzi, np.float32).reshape(-1, 4))
        self.kp = np.ascontiguousarray(self.kp, KP_DTYPE)
        self.desc = np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32)
        if not len(self.map_xyzi) == len(self.kp) == len(self.desc):
            raise ValueError("one map point slot and one descriptor per candidate keypoint")
        if self.order is not None:
            self.order = np.ascontiguousarray(self.order, np.int32)

    @property
    def associated_mask(self) -> np.ndarray:
        return self.map_xyzi[:, 3] > 0


@dataclasses.dataclass
class GuidedHost:
    """What mage_reloc_guided_host leaves after the phases that ran."""
    result: np.void            # RG_RESULT_DTYPE
    query_kp: np.ndarray       # (n_queries,) KP_DTYPE
    query_pos: np.ndarray      # (n_queries, 2)
    query_desc: np.ndarray     # (n_queries, 32)
    query_ref: np.ndarray      # (n_queries,) candidate keypoint of each query
    assoc: np.ndarray          # (n_in_front, 2) {candidate keypoint, frame keypoint}
    ba_points3: np.ndarray     # the second bundle adjustment's inputs (empty unless it is reached)
    ba_uv: np.ndarray
    ba_info: np.ndarray

    @property
    def verdict(self) -> int:
        return int(self.result["verdict"])

    @property
    def status(self) -> int:
        return int(self.result["status"])


def guided_host(settings, pnp_ok: bool, intr4, cand: Candidate, kp, pos3_first, r9_first, radius_matches=None,
                outlier=None, pos3_second=None, r9_second=None, cap=None) -> GuidedHost:
    """mage_reloc_guided_host: phase 1 from the first refined pose; phase 2 when `radius_matches`
    (DM_DTYPE, in query order) is given; phase 3 when `outlier` and the second pose are given."""
    cs = _c(settings)
    intr4 = np.ascontiguousarray(np.asarray(intr4, np.float32).reshape(4))
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    p1 = np.ascontiguousarray(np.asarray(pos3_first, np.float32).reshape(3))
    r1 = np.ascontiguousarray(np.asarray(r9_first, np.float32).reshape(9))
    n_kf = len(cand.kp)
    cap = max(n_kf, len(cand.order) if cand.order is not None else 0) if cap is None else int(cap)
    ncap = max(cap, 1)
    result = np.zeros(1, RG_RESULT_DTYPE)
    qkp, qpos, qdesc = np.zeros(ncap, KP_DTYPE), np.zeros((ncap, 2), np.float32), np.zeros((ncap, 32), np.uint8)
    qref, assoc = np.zeros(ncap, np.int32), np.zeros((ncap, 2), np.int32)
    pts, uv, info = np.zeros((ncap, 3), np.float32), np.zeros((ncap, 2), np.float32), np.zeros(ncap, np.float32)
    # an empty array still has to arrive as a pointer: NULL is "stop before this phase"
    rm = None if radius_matches is None else np.ascontiguousarray(radius_matches, DM_DTYPE)
    n_rm = 0 if rm is None else len(rm)
    rm_p = None if rm is None else ptr(rm if n_rm else np.zeros(1, DM_DTYPE))
    fl = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
    fl_p = None if fl is None else ptr(fl if len(fl) else np.zeros(1, np.uint8))
    p2 = None if pos3_second is None else np.ascontiguousarray(np.asarray(pos3_second, np.float32).reshape(3))
    r2 = None if r9_second is None else np.ascontiguousarray(np.asarray(r9_second, np.float32).reshape(9))
    order = cand.order
    check(_lib.load().mage_reloc_guided_host(
        C.byref(cs), int(bool(pnp_ok)), ptr(intr4), ptr(cand.map_xyzi), ptr(cand.kp), ptr(cand.desc), n_kf,
        None if order is None else (ptr(order) if len(order) else ptr(np.zeros(1, np.int32))),
        0 if order is None else len(order), ptr(kp), len(kp), ptr(p1), ptr(r1), cap, ptr(result), ptr(qkp), ptr(qpos),
        ptr(qdesc), ptr(qref), rm_p, n_rm, ptr(assoc), ptr(pts), ptr(uv), ptr(info), fl_p, ptr(p2), ptr(r2)))
    r = result[0]
    nq, n = int(r["n_queries"]), int(r["n_in_front"])
    nb = n if int(r["verdict"]) in (RG_OK, RG_FEW_BA_INLIERS) and radius_matches is not None else 0
    return GuidedHost(r.copy(), qkp[:nq].copy(), qpos[:nq].copy(), qdesc[:nq].copy(), qref[:nq].copy(), assoc[:n].copy(),
                      pts[:nb].copy(), uv[:nb].copy(), info[:nb].copy())


def choose_host(settings, results) -> np.void:
    """The frame's record (RG_FRAME_DTYPE) from its candidates' records, as the decide kernel writes it."""
    res = np.ascontiguousarray(results, RG_RESULT_DTYPE)
    frame = np.zeros(1, RG_FRAME_DTYPE)
    check(_lib.load().mage_reloc_guided_choose_host(C.byref(_c(settings)), ptr(res) if len(res) else None, len(res),
                                                    ptr(frame)))
    return frame[0].copy()


@dataclasses.dataclass
class GuidedSearch:
    index: int                 # indexOfSuccess, or -1
    pos3: np.ndarray           # the frame's pose (the identity without success)
    r9: np.ndarray
    n_assoc: int               # the associations the frame takes
    frame: np.void             # RG_FRAME_DTYPE
    results: np.ndarray        # (n_candidates,) RG_RESULT_DTYPE
    pnp: np.ndarray            # (n_candidates,) RP_RESULT_DTYPE
    assoc: list                # per candidate (n_in_front, 2) {candidate keypoint, frame keypoint}

    @property
    def associations(self) -> np.ndarray:
        """The winner's associations (all of them, the bundle adjustment's outliers included, :428-430)."""
        return self.assoc[self.index] if self.index >= 0 else np.zeros((0, 2), np.int32)


def _default_pose_ba(pos3, r9, intr4, points3, uv, info, nsteps, huber, max_error):
    import types

    from . import bundler

    pb = types.SimpleNamespace(pos=np.asarray(pos3, np.float32).reshape(1, 3), r9=np.asarray(r9, np.float32).reshape(1, 9),
                               intr=np.asarray(intr4, np.float32).reshape(1, 4),
                               obs_start=np.array([0, len(points3)], np.uint32), points=points3, uv=uv, info=info)
    o = bundler.OptimizeCameraPoses(pb, nsteps, max_error, huber)
    return o["pos"][0], o["r9"][0], o["outlier"]


def _default_radius_match(qkp, qdesc, tkp, tdesc, radius, qpos, max_distance, min_difference):
    from . import matcher

    return matcher.RadiusMatch(qkp, qdesc, tkp, tdesc, radius, max_distance, min_difference,
                               queryKeypointPositionOverrides=qpos)


def guided_search(settings, intr4, candidates, kp, desc, matches, backend: str = "hip", pose_matcher=POSE_MATCHER,
                  cap=None, device: int = 0, pose_ba=None, radius_match=None) -> GuidedSearch:
    """One lost frame (keypoints `kp`, descriptors `desc`, undistorted intrinsics `intr4`) against
    `candidates` (Candidate records) with `matches[c]` the IndexedMatch records of candidate c
    (query_idx into the candidate, train_idx into the frame): PNPRansac and everything behind it.
    For backend "host", pose_ba(pos3, r9, intr4, points3, uv, info, nsteps, huber, max_error) ->
    (pos3, r9, outlier flags) and radius_match(qkp, qdesc, tkp, tdesc, radius, qpos, max_distance,
    min_difference) -> DM_DTYPE records supply the two steps between the twin's phases."""
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    cs = _c(settings)
    intr4 = np.ascontiguousarray(np.asarray(intr4, np.float32).reshape(4))
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    if len(desc) != len(kp):
        raise ValueError("one descriptor per keypoint")
    cands = list(candidates)
    mm = [np.ascontiguousarray(m, DM_DTYPE) for m in matches]
    if len(mm) != len(cands):
        raise ValueError("one match list per candidate")
    P = len(cands)
    if P == 0:
        frame = choose_host(cs, np.zeros(0, RG_RESULT_DTYPE))
        return GuidedSearch(-1, frame["pos3"].copy(), frame["r9"].copy(), 0, frame, np.zeros(0, RG_RESULT_DTYPE),
                            np.zeros(0, RP_RESULT_DTYPE), [])
    slots = [max(len(c.kp), len(c.order) if c.order is not None else 0) for c in cands]
    cap = max(max(slots), 1) if cap is None else int(cap)
    results, pnp = np.zeros(P, RG_RESULT_DTYPE), np.zeros(P, RP_RESULT_DTYPE)
    assoc_out = []
    if backend == "hip":
        kf_pitch = max(max(slots), 1)
        match_cap = max(max(len(m) for m in mm), 1)
        mp = np.zeros((P, kf_pitch, 4), np.float32)
        kfkp, kfd = np.zeros((P, kf_pitch), KP_DTYPE), np.zeros((P, kf_pitch, 32), np.uint8)
        n_kf, n_order, n_m = np.zeros(P, np.uint32), np.zeros(P, np.uint32), np.zeros(P, np.uint32)
        ordered = any(c.order is not None for c in cands)
        order = np.zeros((P, kf_pitch), np.int32)
        bai = np.zeros((P, 4), np.float32)
        marr = np.zeros((P, match_cap), DM_DTYPE)
        for i, c in enumerate(cands):
            n = len(c.kp)
            mp[i, :n], kfkp[i, :n], kfd[i, :n], n_kf[i] = c.map_xyzi, c.kp, c.desc, n
            o = c.order if c.order is not None or not ordered else np.nonzero(c.associated_mask)[0].astype(np.int32)
            if o is not None:
                order[i, : len(o)], n_order[i] = o, len(o)
            bai[i] = intr4 if c.ba_intr4 is None else np.asarray(c.ba_intr4, np.float32).reshape(4)
            marr[i, : len(mm[i])], n_m[i] = mm[i], len(mm[i])
        frame = np.zeros(1, RG_FRAME_DTYPE)
        assoc = np.zeros((P, cap, 2), np.int32)
        check(_lib.load().mage_reloc_guided(
            C.byref(cs), int(pose_matcher[0]), int(pose_matcher[1]), P, ptr(intr4), ptr(bai), ptr(mp), ptr(kfkp), ptr(kfd),
            kf_pitch, ptr(n_kf), ptr(order) if ordered else None, ptr(n_order) if ordered else None, ptr(kp), ptr(desc),
            len(kp), ptr(marr), match_cap, ptr(n_m), cap, ptr(results), ptr(pnp), ptr(frame), ptr(assoc), device))
        assoc_out = [assoc[i, : int(results[i]["n_in_front"])].copy() for i in range(P)]
        fr = frame[0].copy()
    else:
        pose_ba = pose_ba or _default_pose_ba
        radius_match = radius_match or _default_radius_match
        nsteps, maxe = int(cs.bundle_adjust_iterations), float(cs.max_bundle_adjust_reprojection_error)
        ident = (np.zeros(3, np.float32), np.eye(3, dtype=np.float32).reshape(9))
        for i, c in enumerate(cands):
            bai = intr4 if c.ba_intr4 is None else np.asarray(c.ba_intr4, np.float32).reshape(4)
            pr = pnp_ransac(cs, intr4, c.map_xyzi, kp, mm[i], backend="host")
            pnp[i] = pr.result
            first = ident
            # a frame or candidate over the limit is refused by the twin before anything is read
            small = len(kp) <= MAX_KEYPOINTS and len(c.kp) <= MAX_KEYPOINTS
            if pr.ok and small and len(kp) >= int(cs.min_brute_force_correspondences):
                first = pose_ba(pr.pos3, pr.r9, bai, pr.points3, pr.uv, pr.info, nsteps, HUBER_WIDTH, maxe)[:2]
            g = guided_host(cs, pr.ok, intr4, c, kp, first[0], first[1], cap=cap)
            if g.verdict == RG_OK and g.status & (RG_STATUS_OVER_LIMIT | RG_STATUS_BAD_ORDER) == 0:
                rm = radius_match(g.query_kp, g.query_desc, kp, desc, float(cs.search_radius), g.query_pos,
                                  int(pose_matcher[0]), int(pose_matcher[1]))
                g = guided_host(cs, pr.ok, intr4, c, kp, first[0], first[1], radius_matches=rm, cap=cap)
                if g.verdict == RG_OK:
                    p2, r2, flags = pose_ba(first[0], first[1], bai, g.ba_points3, g.ba_uv, g.ba_info, nsteps, HUBER_WIDTH,
                                            maxe)
                    g = guided_host(cs, pr.ok, intr4, c, kp, first[0], first[1], radius_matches=rm, outlier=flags,
                                    pos3_second=p2, r9_second=r2, cap=cap)
            results[i] = g.result
            assoc_out.append(g.assoc)
        fr = choose_host(cs, results)
    return GuidedSearch(int(fr["index"]), fr["pos3"].copy(), fr["r9"].copy(), int(fr["n_assoc"]), fr, results, pnp, assoc_out)


def guided_scratch_bytes(problems: int, cap: int, pnp_cap: int) -> int:
    return int(_lib.load().mage_reloc_guided_scratch_bytes(problems, cap, pnp_cap))


def guided_search_batch_device(settings, stream=None, **buffers) -> None:
    """mage_reloc_guided_batch_device over torch device tensors: the keyword arguments are the fields
    of mage_reloc_guided_args (include/mage_hot.h), pointers given as tensors or raw addresses."""
    args = buffers.pop("args", None) or RelocGuidedArgsC.make(**buffers)
    check(_lib.load().mage_reloc_guided_batch_device(C.byref(_c(settings)), C.byref(args),
                                                     C.c_void_p(stream) if stream else None))


def candidates_batch_device(settings, candidates_args: dict, guided_args: dict, stream=None) -> None:
    """mage_reloc_candidates_batch_device: IndexedMatch, the PnP stage and the guided stage on one
    stream; the two dicts hold the fields of mage_reloc_candidates_args and mage_reloc_guided_args."""
    ca = RelocCandidatesArgsC.make(**candidates_args)
    ga = RelocGuidedArgsC.make(**guided_args)
    check(_lib.load().mage_reloc_candidates_batch_device(C.byref(_c(settings)), C.byref(ca), C.byref(ga),
                                                         C.c_void_p(stream) if stream else None))


def try_estimate_pose_from_candidates(settings, tree, intr4, candidates, kp, desc, backend: str = "hip",
                                      pose_matcher=POSE_MATCHER, device: int = 0, **kw) -> GuidedSearch:
    """PoseEstimator::TryEstimatePoseFromCandidates (:219-437) for one lost frame: IndexedMatch of
    every candidate's associated keypoints against the frame over the vocabulary `tree`
    (bow.OnlineBowTree) with the relocaliser's matcher settings, then guided_search."""
    from . import bow

    cs = _c(settings)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    cands = list(candidates)
    matches = []
    for c in cands:
        if len(desc) == 0 or len(c.desc) == 0 or len(desc) > MAX_KEYPOINTS or len(c.desc) > MAX_KEYPOINTS:
            matches.append(np.zeros(0, DM_DTYPE))
            continue
        matches.append(bow.IndexedMatch(tree, c.desc, desc, maskA=c.associated_mask,
                                        maxHammingDist=int(cs.max_hamming_distance),
                                        minHammingDifference=int(cs.min_hamming_difference)))
    return guided_search(cs, intr4, cands, kp, desc, matches, backend=backend, pose_matcher=pose_matcher, device=device, **kw)
