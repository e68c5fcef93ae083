"""Scene extent — host mirror of CalculateBoundingPlaneDepthsForKeyframe
(Core/MAGESLAM/Source/Tracking/BoundingPlaneDepths.cpp:16-87): a tracked frame's near and far plane
depths and its sparse depth map, what the reference's tracking thread computes right behind
TrackLocalMap (Tasks/TrackLocalMapWorker.cpp:202-204) and hands to the client as `Depth`
(Data/Data.h:388-403).

`calculate_bounding_plane_depths` takes one `DepthFrame` or a sequence of them.  Backend "hip" runs
the gfx950 kernel (one frame: mage_bounding_plane_depths on host arrays; a sequence: the frames packed
into pitched device tensors and ONE launch of mage_bounding_plane_depths_batch_device), "host" runs
mage_bounding_plane_depths_host, the plain C++ twin, frame by frame.  Both give the same bytes.
`bounding_plane_depths_batch_device` is the thin wrapper of the batched device entry over torch
tensors.

`calculate_volume_of_interest` / `try_get_volume_of_interest` are CalculateVolumeOfInterest
(VolumeOfInterest/VolumeOfInterest.cpp:45-259) over a pose history's keyframes and their depths, with
the same two backends; `volume_of_interest_batch_device` wraps the batched device chain, which can
read the depth stage's records by index on the same stream.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import (BD_RESULT_DTYPE, KP_DTYPE, PP_DTYPE, VOI_LEVEL_DTYPE, VOI_RESULT_DTYPE, BoundingDepthSettingsC, VoiSettingsC,
                   check, ptr)

INVALID_DEPTH = -1.0
MAX_POINTS = 8192
STATUS_BAD_INDEX, STATUS_NONPOSITIVE, STATUS_OVER_LIMIT = 1, 2, 4


@dataclasses.dataclass
class BoundingDepthSettings:
    """BoundingDepthSettings (MageSettings.h:216-223) in the reference's order."""
    region_of_interest_min_x: float = 0.1
    region_of_interest_min_y: float = 0.1
    region_of_interest_max_x: float = 0.9
    region_of_interest_max_y: float = 0.9
    near_depth_softness: float = 0.0
    far_depth_softness: float = 0.0

    def to_c(self) -> BoundingDepthSettingsC:
        return BoundingDepthSettingsC.make(**dataclasses.asdict(self))


def _c(settings) -> BoundingDepthSettingsC:
    return settings if isinstance(settings, BoundingDepthSettingsC) else settings.to_c()


@dataclasses.dataclass
class DepthFrame:
    """What the routine reads of a tracked frame: the view matrix in the bundler form (pos3
    view-space t, r9 column-major R), intr4 = {cx, cy, fx, fy} of the undistorted calibration, the
    image size, the KP_DTYPE keypoints, the associated map points (n, 4) {x, y, z, id bits} (see
    `map_points`) and per point the index of its keypoint."""
    pos3: np.ndarray
    r9: np.ndarray
    intr4: np.ndarray
    width: int
    height: int
    kp: np.ndarray
    map_xyzi: np.ndarray
    kp_index: np.ndarray


def map_points(xyz, ids) -> np.ndarray:
    """(n, 4) float32 rows {x, y, z, the int32 id's bits}."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.empty((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    out[:, 3] = np.asarray(ids, np.int32).reshape(-1).view(np.float32)
    return out


@dataclasses.dataclass
class Depth:
    """Depth (Data/Data.h:388-403) with the counts and status of mage_depth_result."""
    near: float            # NearPlaneDepth, INVALID_DEPTH without a valid depth
    far: float             # FarPlaneDepth
    sparse: np.ndarray     # (n_points,) PP_DTYPE: SparseDepth in point order (empty for an OVER_LIMIT frame)
    n_valid: int
    status: int            # STATUS_* bits
    result: np.void        # the whole mage_depth_result (BD_RESULT_DTYPE)

    @property
    def valid(self) -> bool:
        return self.near != INVALID_DEPTH or self.far != INVALID_DEPTH


def _depth(r, sparse) -> Depth:
    n = 0 if int(r["status"]) & STATUS_OVER_LIMIT else int(r["n_points"])
    return Depth(float(r["near"]), float(r["far"]), sparse[:n].copy(), int(r["n_valid"]), int(r["status"]), r.copy())


def _arrays(f: DepthFrame):
    return (np.ascontiguousarray(np.asarray(f.pos3, np.float32).reshape(3)),
            np.ascontiguousarray(np.asarray(f.r9, np.float32).reshape(9)),
            np.ascontiguousarray(np.asarray(f.intr4, np.float32).reshape(4)),
            np.ascontiguousarray(f.kp, KP_DTYPE),
            np.ascontiguousarray(np.asarray(f.map_xyzi, np.float32).reshape(-1, 4)),
            np.ascontiguousarray(np.asarray(f.kp_index, np.int32).reshape(-1)))


def _one(cs, f: DepthFrame, backend: str, cap, device: int) -> Depth:
    pos3, r9, intr4, kp, mp, idx = _arrays(f)
    if len(idx) != len(mp):
        raise ValueError("one keypoint index per map point")
    cap = len(mp) if cap is None else int(cap)
    result = np.zeros(1, BD_RESULT_DTYPE)
    sparse = np.zeros(max(cap, 1), PP_DTYPE)
    args = (C.byref(cs), ptr(pos3), ptr(r9), ptr(intr4), int(f.width), int(f.height), ptr(kp), len(kp), ptr(mp), ptr(idx),
            len(mp), cap, ptr(result), ptr(sparse))
    L = _lib.load()
    if backend == "host":
        check(L.mage_bounding_plane_depths_host(*args))
    else:
        check(L.mage_bounding_plane_depths(*args, device))
    return _depth(result[0], sparse)


def pack_frames(frames: Sequence[DepthFrame], kp_pitch=None, point_pitch=None, device="cuda", fill: int = 0) -> dict:
    """The frames as the pitched device tensors of mage_bounding_plane_depths_batch_device (its
    keyword arguments, outputs included); every byte no frame owns is `fill`."""
    import torch

    fs = [_arrays(f) for f in frames]
    n = len(fs)
    kp_pitch = max([len(a[3]) for a in fs] + [1]) if kp_pitch is None else int(kp_pitch)
    point_pitch = max([len(a[4]) for a in fs] + [1]) if point_pitch is None else int(point_pitch)

    def filled(shape, dtype):
        a = np.empty(shape, dtype)
        a.view(np.uint8).fill(fill)
        return a

    pos3, r9, intr4 = filled((n, 3), np.float32), filled((n, 9), np.float32), filled((n, 4), np.float32)
    size, n_kp, n_points = filled((n, 2), np.uint32), filled(n, np.uint32), filled(n, np.uint32)
    kp, mp = filled((n, kp_pitch), KP_DTYPE), filled((n, point_pitch, 4), np.float32)
    idx = filled((n, point_pitch), np.int32)
    for i, (f, a) in enumerate(zip(frames, fs)):
        pos3[i], r9[i], intr4[i] = a[0], a[1], a[2]
        size[i] = (f.width, f.height)
        n_kp[i], n_points[i] = len(a[3]), len(a[4])
        nk, npt = min(len(a[3]), kp_pitch), min(len(a[4]), point_pitch)  # a frame over its pitch keeps its count
        kp[i, :nk] = a[3][:nk]
        mp[i, :npt] = a[4][:npt]
        idx[i, :npt] = a[5][:npt]

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)

    return dict(frames=n, pos3=dev(pos3), r9=dev(r9), intr4=dev(intr4), size=dev(size), kp=dev(kp), kp_pitch=kp_pitch,
                n_kp=dev(n_kp), map_xyzi=dev(mp), kp_index=dev(idx), point_pitch=point_pitch, n_points=dev(n_points),
                result=dev(filled(n, BD_RESULT_DTYPE)), sparse=dev(filled((n, point_pitch), PP_DTYPE)))


def bounding_plane_depths_batch_device(settings, frames: int, pos3, r9, intr4, size, kp, kp_pitch: int, n_kp, map_xyzi,
                                       kp_index, point_pitch: int, n_points, cap: int, result, sparse, stream=None) -> None:
    """Batched device form over `frames` frames (torch device tensors), one launch on `stream`;
    layouts in mage_hot.h.  `result`: frames x 20 bytes (BD_RESULT_DTYPE); `sparse`: frames x
    point_pitch x 16 bytes (PP_DTYPE)."""
    check(_lib.load().mage_bounding_plane_depths_batch_device(
        C.byref(_c(settings)), frames, ptr(pos3), ptr(r9), ptr(intr4), ptr(size), ptr(kp), kp_pitch, ptr(n_kp),
        ptr(map_xyzi), ptr(kp_index), point_pitch, ptr(n_points), cap, ptr(result), ptr(sparse),
        C.c_void_p(stream) if stream else None))


def unpack_results(packed: dict) -> list:
    """The Depth records of a packed batch after the launch (synchronises through the copies)."""
    n, pitch = packed["frames"], packed["point_pitch"]
    res = packed["result"].cpu().numpy().view(BD_RESULT_DTYPE)
    sp = packed["sparse"].cpu().numpy().view(PP_DTYPE).reshape(n, pitch)
    return [_depth(res[i], sp[i]) for i in range(n)]


def calculate_bounding_plane_depths(settings, frames, backend: str = "hip", cap=None, device: int = 0):
    """CalculateBoundingPlaneDepthsForKeyframe for one DepthFrame (returns a Depth) or a sequence of
    them (returns a list).  `cap` bounds a frame's points (default: one frame: its own count, a
    sequence: the largest count); a frame over it, or a cap over MAX_POINTS, is STATUS_OVER_LIMIT."""
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    cs = _c(settings)
    if isinstance(frames, DepthFrame):
        return _one(cs, frames, backend, cap, device)
    frames = list(frames)
    if cap is None:
        cap = max([len(np.asarray(f.kp_index).reshape(-1)) for f in frames] + [0])
    if backend == "host":
        return [_one(cs, f, backend, cap, device) for f in frames]
    if not frames:
        return []
    packed = pack_frames(frames, point_pitch=max(cap, 1), device=f"cuda:{device}")
    bounding_plane_depths_batch_device(cs, cap=cap, **packed)
    return unpack_results(packed)


# ----------------------------------------------------------------------------------------------
# The volume of interest (VolumeOfInterest/VolumeOfInterest.cpp:45-259)
# ----------------------------------------------------------------------------------------------
VOI_OK, VOI_NO_KEYFRAMES, VOI_DEGENERATE, VOI_EMPTY = range(4)
VOI_STATUS_NAMES = ("ok", "no keyframes", "degenerate", "empty")


@dataclasses.dataclass
class VolumeOfInterestSettings:
    """VolumeOfInterestSettings (MageSettings.h:290-307) in the reference's order."""
    threshold: float = 0.5
    iterations: int = 3
    voxel_count_floor: int = 16000
    away_prominence: float = 1.2
    toward_prominence: float = 0.1
    side_prominence: float = 1.0
    kernel_angle_x_rads: float = float(np.deg2rad(np.float32(60.0)))
    kernel_angle_y_rads: float = float(np.deg2rad(np.float32(40.0)))
    kernel_pitch_rads: float = 0.0
    kernel_roll_rads: float = 0.0
    kernel_yaw_rads: float = float(np.deg2rad(np.float32(5.0)))
    kernel_depth_modifier: float = 1.0

    def to_c(self) -> VoiSettingsC:
        """The C struct with its derived constants filled in (mage_voi_settings_prepare)."""
        cs = VoiSettingsC.make(**dataclasses.asdict(self))
        check(_lib.load().mage_voi_settings_prepare(C.byref(cs)))
        return cs


def _cv(settings) -> VoiSettingsC:
    return settings if isinstance(settings, VoiSettingsC) else settings.to_c()


@dataclasses.dataclass
class VolumeOfInterest:
    """AxisAlignedVolume (Data/Data.h) with the status and the per-level trace."""
    min: np.ndarray        # (3,)
    max: np.ndarray
    status: int            # VOI_*
    levels_done: int
    result: np.void        # the whole mage_voi_result (VOI_RESULT_DTYPE)
    trace: np.ndarray      # (iterations,) VOI_LEVEL_DTYPE


def _keyframes(keyframes, depths):
    kf = np.ascontiguousarray(np.asarray(keyframes, np.float32).reshape(-1, 3, 4))
    if depths is not None and len(depths) and isinstance(depths[0], Depth):
        depths = [(d.near, d.far) for d in depths]
    nf = np.ascontiguousarray(np.asarray(depths, np.float32).reshape(-1, 2))
    if len(nf) != len(kf):
        raise ValueError("one {near, far} pair per keyframe")
    return kf, nf


def teardrop_scores(settings, keyframes, depths, points) -> np.ndarray:
    """TeardropScore of every point against every keyframe, (n_points, n_kf): the twin's function."""
    kf, nf = _keyframes(keyframes, depths)
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    out = np.zeros((len(pts), len(kf)), np.float32)
    check(_lib.load().mage_voi_teardrop_host(C.byref(_cv(settings)), ptr(kf), ptr(nf), len(kf), ptr(pts), len(pts), ptr(out)))
    return out


def calculate_volume_of_interest(settings, keyframes, depths, backend: str = "hip", device: int = 0,
                                 prefill=None) -> VolumeOfInterest:
    """CalculateVolumeOfInterest for one pose history: keyframes (n, 3, 4) world-from-camera matrices,
    depths (n, 2) {near, far} pairs or a sequence of Depth records.  `prefill`: the bytes the result
    record starts with (what NO_KEYFRAMES leaves untouched)."""
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    cs = _cv(settings)
    kf, nf = _keyframes(keyframes, depths)
    result = np.zeros(1, VOI_RESULT_DTYPE)
    trace = np.zeros(max(int(cs.iterations), 1), VOI_LEVEL_DTYPE)
    if prefill is not None:
        result.view(np.uint8)[:] = prefill
        trace.view(np.uint8)[:] = prefill
    args = (C.byref(cs), ptr(kf), ptr(nf), None, 0, None, len(kf), ptr(result), ptr(trace))
    L = _lib.load()
    if backend == "host":
        check(L.mage_volume_of_interest_host(*args))
    else:
        check(L.mage_volume_of_interest(*args, device))
    r = result[0]
    return VolumeOfInterest(r["min"].copy(), r["max"].copy(), int(r["status"]), int(r["levels_done"]), r.copy(),
                            trace[:int(cs.iterations)].copy())


def try_get_volume_of_interest(keyframes, depths, settings, backend: str = "hip", device: int = 0):
    """PoseHistory::TryGetVolumeOfInterest (Map/PoseHistory.cpp:58-75): None where the reference
    returns false (no keyframes), else the VolumeOfInterest."""
    v = calculate_volume_of_interest(settings, keyframes, depths, backend=backend, device=device)
    return None if v.status == VOI_NO_KEYFRAMES else v


def volume_of_interest_scratch_bytes(problems: int, kf_pitch: int) -> int:
    return int(_lib.load().mage_volume_of_interest_scratch_bytes(problems, kf_pitch))


def volume_of_interest_batch_device(settings, problems: int, kf_world, kf_pitch: int, n_kf, result, scratch, near_far=None,
                                    depth_records=None, n_depth_records: int = 0, depth_index=None, trace=None,
                                    stream=None) -> None:
    """Batched device form over `problems` problems (torch device tensors), one chain of launches on
    `stream`; layouts in mage_hot.h.  Depths: `near_far`, or the depth stage's `depth_records` with
    `depth_index`.  `result`: problems x 32 bytes; `trace`: None or problems x iterations x 60 bytes."""
    check(_lib.load().mage_volume_of_interest_batch_device(
        C.byref(_cv(settings)), problems, ptr(kf_world), kf_pitch, ptr(n_kf), ptr(near_far), ptr(depth_records),
        n_depth_records, ptr(depth_index), ptr(result), ptr(trace), ptr(scratch), C.c_void_p(stream) if stream else None))
