"""What the guided-relocalisation tests compare against: the twin's phases driven by the oracle's
pose bundle adjustment and RadiusMatch (run), and restatements of the reference's code written
independently of csrc/reloc_guided_math.hpp — the query set of PoseEstimator.cpp:351-371 in NumPy
float32, :391-409 and :421-433 as literal Python, and the candidate loop of :261-434 with its
rounds and `worthwhile` flags.
"""
from __future__ import annotations

import functools
import types

import numpy as np

from mageslam_amd import reloc
from mageslam_amd._lib import DM_DTYPE
from tests import pose_cases as P
from tests import reloc_guided_cases as gc

INTR = gc.INTR
IDENT = (np.zeros(3, np.float32), np.eye(3, dtype=np.float32).reshape(9))


def pnp_outputs(s: gc.Scene, c: int) -> dict:
    """The PnP stage's outputs for candidate c: crafted, or the twin's on the scene's matches."""
    if s.pnp is not None:
        return s.pnp[c]
    return _twin_pnp(s.name, c)


@functools.lru_cache(maxsize=None)
def _twin_pnp(name, c):
    s = gc.scene(name)
    r = reloc.pnp_ransac(s.settings, INTR, s.cands[c].map_xyzi, s.kp, s.matches[c], backend="host")
    return dict(result=r.result, points3=r.points3, uv=r.uv, info=r.info, pos3=r.pos3, r9=r.r9)


def pnp_ok(p: dict) -> bool:
    r = p["result"]
    return int(r["verdict"]) == reloc.OK and int(r["status"]) & (reloc.STATUS_OVER_LIMIT | reloc.STATUS_BAD_INDEX) == 0


def pose_batch_of(pos3, r9, intr4, points3, uv, info):
    return types.SimpleNamespace(pos=np.asarray(pos3, np.float32).reshape(1, 3), r9=np.asarray(r9, np.float32).reshape(1, 9),
                                 intr=np.asarray(intr4, np.float32).reshape(1, 4),
                                 obs_start=np.array([0, len(points3)], np.uint32),
                                 points=np.asarray(points3, np.float32).reshape(-1, 3),
                                 uv=np.asarray(uv, np.float32).reshape(-1, 2), info=np.asarray(info, np.float32).reshape(-1))


def ba_arguments(settings):
    """(steps, Huber width, max_error_square as passed) of both BundleAdjustPose calls."""
    return int(settings.bundle_adjust_iterations), reloc.HUBER_WIDTH, float(settings.max_bundle_adjust_reprojection_error)


def oracle_ba(pos3, r9, intr4, points3, uv, info, nsteps, huber, max_error):
    from oracle import oracle as O

    o = O.pose_batch(pose_batch_of(pos3, r9, intr4, points3, uv, info), nsteps, huber, max_error)
    return o["pos"][0], o["r9"][0], o["outlier"]


def oracle_rm(qkp, qdesc, tkp, tdesc, radius, qpos, max_distance, min_difference):
    from oracle import oracle as O

    if len(qkp) == 0 or len(tkp) == 0:
        return np.zeros(0, DM_DTYPE)
    return O.radius_match(qkp, qdesc, tkp, tdesc, radius, qpos=qpos, max_distance=max_distance, min_difference=min_difference)


@functools.lru_cache(maxsize=None)
def run(name: str, c: int):
    """Candidate c of scene `name` through the twin's phases with the oracle between them.  Fields
    (None where the routine did not get there): pnp, ok, first (pos3, r9), pb1, g1, rm, g2, pb2,
    second (pos3, r9, flags), g3, final (the last phase's GuidedHost)."""
    s = gc.scene(name)
    cand, st = s.cands[c], s.settings
    p = pnp_outputs(s, c)
    ok = pnp_ok(p)
    out = types.SimpleNamespace(pnp=p, ok=ok, first=IDENT, pb1=None, g1=None, rm=None, g2=None, pb2=None, second=None, g3=None)
    steps, huber, maxe = ba_arguments(st)
    small = len(s.kp) <= reloc.MAX_KEYPOINTS and len(cand.kp) <= reloc.MAX_KEYPOINTS
    if ok and small and len(s.kp) >= st.min_brute_force_correspondences:
        out.pb1 = pose_batch_of(p["pos3"], p["r9"], INTR, p["points3"], p["uv"], p["info"])
        out.first = oracle_ba(p["pos3"], p["r9"], INTR, p["points3"], p["uv"], p["info"], steps, huber, maxe)[:2]
    out.g1 = out.final = reloc.guided_host(st, ok, INTR, cand, s.kp, *out.first)
    if out.g1.verdict != reloc.RG_OK:
        return out
    out.rm = oracle_rm(out.g1.query_kp, out.g1.query_desc, s.kp, s.desc, st.search_radius, out.g1.query_pos, *reloc.POSE_MATCHER)
    out.g2 = out.final = reloc.guided_host(st, ok, INTR, cand, s.kp, *out.first, radius_matches=out.rm)
    if out.g2.verdict != reloc.RG_OK:
        return out
    out.pb2 = pose_batch_of(*out.first, INTR, out.g2.ba_points3, out.g2.ba_uv, out.g2.ba_info)
    out.second = oracle_ba(*out.first, INTR, out.g2.ba_points3, out.g2.ba_uv, out.g2.ba_info, steps, huber, maxe)
    out.g3 = out.final = reloc.guided_host(st, ok, INTR, cand, s.kp, *out.first, radius_matches=out.rm, outlier=out.second[2],
                                           pos3_second=out.second[0], r9_second=out.second[1])
    return out


@functools.lru_cache(maxsize=None)
def margins(name: str, c: int, which: int):
    """pose_cases.reference() of candidate c's first (which = 1) or second bundle adjustment, or None."""
    r = run(name, c)
    pb = r.pb1 if which == 1 else r.pb2
    if pb is None or len(pb.points) == 0:
        return None
    return P.reference(pb, *ba_arguments(gc.scene(name).settings))


# ---------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------
def query_set(cand: reloc.Candidate, pos3, r9, intr4):
    """:351-371 — (referenceIndex, predictedPositions (n, 2) float32) in iteration order."""
    idx = cand.order if cand.order is not None else np.flatnonzero(cand.map_xyzi[:, 3] > 0)
    ref, pos = [], []
    for k in idx:
        u, v, depth = gc._project32(pos3, r9, intr4, cand.map_xyzi[k, :3])
        if depth >= 0:
            ref.append(int(k))
            pos.append((u, v))
    return np.array(ref, np.int32), np.array(pos, np.float32).reshape(-1, 2)


def after_radius_match(settings, cand, reference_index, good_matches, pos3, r9):
    """:391-409 — (verdict, mapPoints as [(candidate keypoint, frame keypoint)])."""
    if len(good_matches) < settings.min_radius_match_correspondences:
        return reloc.RG_FEW_RADIUS_MATCHES, []
    map_points = [(int(reference_index[m["query_idx"]]), int(m["train_idx"])) for m in good_matches]
    map_points = [(k, t) for k, t in map_points if not gc._behind32(pos3, r9, cand.map_xyzi[k, :3])]
    if len(map_points) < settings.min_map_points:
        return reloc.RG_FEW_MAP_POINTS, map_points
    return reloc.RG_OK, map_points


def after_second_ba(settings, n, outliers):
    """:421-426 — the verdict."""
    inliers = n - outliers
    share = np.float32(inliers) / np.float32(n) if n else np.float32(np.nan)
    return reloc.RG_FEW_BA_INLIERS if share < np.float32(settings.bundle_adjust_inliers_pct_required) else reloc.RG_OK


def routine(settings, n_frame_kp, outcomes):
    """:233-436 literally: `outcomes[c]` = (associated keypoints, the PnP stage's verdict, the guided
    half's verdict) of one pass over candidate c, which every round repeats.  Returns
    (indexOfSuccess or -1, the passes made as (round, candidate))."""
    if n_frame_kp < settings.min_brute_force_correspondences:
        return -1, []
    worthwhile = [True] * len(outcomes)
    index, passes = -1, []
    for it in range(settings.round_robin_iterations):
        if index >= 0:
            break
        for c, (n_assoc, pnp, guided) in enumerate(outcomes):
            if index >= 0:
                break
            if not worthwhile[c]:
                continue
            if n_assoc < settings.min_brute_force_correspondences:
                worthwhile[c] = False
                continue
            passes.append((it, c))
            if it == 0 and pnp == reloc.FEW_MATCHES:
                worthwhile[c] = False
                continue
            if pnp in (reloc.NO_MODEL, reloc.FEW_MATCHES):  # PNPRansac returns false
                worthwhile[c] = False
                continue
            if pnp == reloc.FEW_INLIERS:
                continue
            if guided in (reloc.RG_FEW_RADIUS_MATCHES, reloc.RG_FEW_MAP_POINTS):
                continue
            if guided == reloc.RG_FEW_BA_INLIERS:
                worthwhile[c] = False
                continue
            assert guided == reloc.RG_OK
            index = c
    return index, passes
