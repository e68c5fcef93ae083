"""The mapping thread's cheap loop closure (Tasks/MappingWorker.cpp:160-181): CheapLoopClosure's
sampled map points into the new keyframe (:20-73), InsertKeyframe's effect on the points it
associated (Map/ThreadSafeMap.cpp:242-249), TryConnectMapPoints over the covisible keyframes
(ThreadSafeMap.cpp:715-787), and the map-point refresh after an association
(MapPoint::UpdateRepresentativeDescriptor / UpdateMeanViewDirectionAndDistances, Map/MapPoint.cpp:
80-155) as a call of its own.

Two backends with the same bytes: "hip" (the kernels of csrc/loopclose.hip) and "host" (the plain
C++ twin, csrc/loopclose.cpp, no GPU).  `cheap_loop_closure_batch_device` wraps the batched device
chain (three launches on one stream); `pack_problems` / `unpack_problems` lay problems out for it.
Layouts and rules are in include/mage_hot.h.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (KP_DTYPE, LC_DTYPE, MP_OBS_DTYPE, MP_STATE_DTYPE, LoopClosureBatchC, LoopClosureProblemC,
                   LoopClosureSettingsC, MageError, check, ptr)

(ASSOCIATED, NOT_SAMPLED, HAS_POINT, BEHIND, BORDER, ANGLE, DISTANCE, OCTAVE, NO_MATCH) = range(9)
VERDICT_NAMES = ("associated", "not sampled", "has point", "behind", "border", "angle", "distance", "octave", "no match")
STATUS_OVER_LIMIT, STATUS_OBS_FULL = 1, 2
MAX_KEYPOINTS = 4096
MAX_MAP_POINTS = 1024
MAX_OBSERVATIONS = 65536


@dataclasses.dataclass
class LoopClosureSettings:
    """What the step reads of the settings: LoopClosureSettings (MageSettings.h:197-207),
    TrackLocalMapSettings' view angle and matcher (:180-194), the keyframes' image border and size and
    the pyramid."""
    max_map_points: int = 200
    min_keyframes: int = 10
    search_radius: float = 18.0
    min_view_degrees: float = 60.0
    image_border: float = 7.5
    width: int = 640
    height: int = 480
    num_levels: int = 1
    pyramid_scale: float = 1.5
    closure_max_hamming_distance: int = 30
    closure_min_hamming_difference: int = 1
    connect_max_hamming_distance: int = 30
    connect_min_hamming_difference: int = 1

    def to_c(self) -> LoopClosureSettingsC:
        return LoopClosureSettingsC.make(**dataclasses.asdict(self))

    def octave_factors(self):
        """ComputeDMax / ComputeDMin factors per octave in float32 (MappingMath.h:32-40)."""
        o = np.arange(8, dtype=np.float32) + np.float32(0.5)
        s = np.float32(self.pyramid_scale)
        return np.power(s, np.float32(self.num_levels) - o), np.power(s, -o)


def _c(settings) -> LoopClosureSettingsC:
    return settings if isinstance(settings, LoopClosureSettingsC) else settings.to_c()


def _backend(backend: str) -> None:
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")


def refresh_map_points(settings, positions, obs, n_obs, backend: str = "hip", device: int = 0, prefill=None) -> np.ndarray:
    """The refresh of n points: `positions` (n, 3), `obs` (n, pitch) MP_OBS_DTYPE with point i's
    observations in obs[i, :n_obs[i]].  Returns (n,) MP_STATE_DTYPE.  `prefill`: the byte the state
    buffer holds before the call."""
    _backend(backend)
    positions = np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1, 3))
    obs = np.ascontiguousarray(obs, MP_OBS_DTYPE)
    n_obs = np.ascontiguousarray(np.asarray(n_obs, np.uint32).reshape(-1))
    n = len(positions)
    if obs.ndim != 2 or len(obs) != n or len(n_obs) != n:
        raise ValueError("one row of observations and one count per point")
    state = np.zeros(n, MP_STATE_DTYPE)
    if prefill is not None:
        state.view(np.uint8).fill(prefill)
    args = (C.byref(_c(settings)), n, ptr(positions), ptr(obs), obs.shape[1], ptr(n_obs), ptr(state))
    L = _lib.load()
    if backend == "host":
        check(L.mage_map_points_refresh_host(*args))
    else:
        check(L.mage_map_points_refresh(*args, device))
    return state


def refresh_map_points_batch_device(settings, n_points: int, positions, obs, obs_pitch: int, n_obs, state, status,
                                    stream=None) -> None:
    """Device form over torch tensors, one wave per point, asynchronous on `stream`."""
    check(_lib.load().mage_map_points_refresh_batch_device(
        C.byref(_c(settings)), n_points, ptr(positions), ptr(obs), obs_pitch, ptr(n_obs), ptr(state), ptr(status),
        C.c_void_p(stream) if stream else None))


@dataclasses.dataclass
class Keyframe:
    """What the step reads of a keyframe: its id, the view matrix in the bundler form (pos3 the
    view-space t, r9 the column-major R), intr4 = {cx, cy, fx, fy}, the KP_DTYPE keypoints, their
    (n, 32) descriptors and kp_point[t] = the map-point index keypoint t is associated with, or -1.
    `mask` (covisible keyframes): the unassociated-keypoint bytes; None = kp_point < 0."""
    id: int
    pos3: np.ndarray
    r9: np.ndarray
    intr4: np.ndarray
    kp: np.ndarray
    desc: np.ndarray
    kp_point: np.ndarray
    mask: Optional[np.ndarray] = None

    def arrays(self):
        kp = np.ascontiguousarray(self.kp, KP_DTYPE)
        mask = (np.asarray(self.kp_point) < 0) if self.mask is None else (np.asarray(self.mask) != 0)
        return (np.ascontiguousarray(np.asarray(self.pos3, np.float32).reshape(3)),
                np.ascontiguousarray(np.asarray(self.r9, np.float32).reshape(9)),
                np.ascontiguousarray(np.asarray(self.intr4, np.float32).reshape(4)), kp,
                np.ascontiguousarray(np.asarray(self.desc, np.uint8).reshape(len(kp), 32)),
                np.ascontiguousarray(np.asarray(self.kp_point, np.int32).reshape(len(kp))),
                np.ascontiguousarray(mask.astype(np.uint8).reshape(len(kp))))


@dataclasses.dataclass
class Problem:
    """One mapping task: the map (state (N,) MP_STATE_DTYPE, obs (N, pitch) MP_OBS_DTYPE), the task's
    frame counter, the map's keyframe count, the new keyframe and the covisible ones in order."""
    state: np.ndarray
    obs: np.ndarray
    offset: int
    n_keyframes: int
    ki: Keyframe
    kfs: Sequence[Keyframe] = ()


@dataclasses.dataclass
class LoopClosureResult:
    """What the step leaves: the map after it, the sample, the records and verdicts of both stages
    (connect ones (L, n_kf)), the masks, the per-keyframe modified flags, counts = {sampled,
    associated by the closure, by the connect stage} and the status bits.  Arrays past the counts
    hold what they held before the call."""
    state: np.ndarray
    obs: np.ndarray
    sample_index: np.ndarray
    closure: np.ndarray
    closure_verdict: np.ndarray
    connect: np.ndarray
    connect_verdict: np.ndarray
    ki_mask: np.ndarray
    kf_masks: list
    kf_modified: np.ndarray
    counts: np.ndarray
    status: int
    refused: bool = False  # MAGE_ECAPACITY: STATUS_OBS_FULL

    @property
    def n_sampled(self) -> int:
        return int(self.counts[0])


def cheap_loop_closure_and_connect(settings, problem: Problem, backend: str = "hip", device: int = 0,
                                   prefill: int = 0) -> LoopClosureResult:
    """MappingWorker.cpp:160-181 for one mapping task.  The problem's arrays are left as they are;
    the result carries the map after the step.  Output bytes nothing is written to are `prefill`."""
    _backend(backend)
    cs = _c(settings)
    state = np.ascontiguousarray(problem.state, MP_STATE_DTYPE).copy()
    obs = np.ascontiguousarray(problem.obs, MP_OBS_DTYPE).copy()
    if obs.ndim != 2 or len(obs) != len(state):
        raise ValueError("one row of observations per map point")
    ki = problem.ki.arrays()
    kfs = [k.arrays() for k in problem.kfs]
    nkf, mx = len(kfs), int(cs.max_map_points)
    start = np.zeros(nkf + 1, np.uint32)
    start[1:] = np.cumsum([len(k[3]) for k in kfs])

    def cat(i, dtype, shape=()):
        return np.ascontiguousarray(np.concatenate([k[i] for k in kfs]) if kfs else np.zeros((0,) + shape, dtype))

    def filled(shape, dtype):
        a = np.empty(shape, dtype)
        a.view(np.uint8).fill(prefill)
        return a

    kf_id = np.array([k.id for k in problem.kfs], np.int32)
    kf_pos3, kf_r9, kf_intr4 = cat(0, np.float32), cat(1, np.float32), cat(2, np.float32)
    kf_kp, kf_desc, kf_point, kf_mask = cat(3, KP_DTYPE), cat(4, np.uint8, (32,)), cat(5, np.int32), cat(6, np.uint8)
    out = dict(sample_index=filled(mx, np.uint32), closure=filled(mx, LC_DTYPE), closure_verdict=filled(mx, np.uint8),
               connect=filled((mx, max(nkf, 1)), LC_DTYPE), connect_verdict=filled((mx, max(nkf, 1)), np.uint8),
               ki_mask=filled(max(len(ki[3]), 1), np.uint8), kf_modified=filled(max(nkf, 1), np.uint8),
               counts=filled(3, np.uint32), status=filled(1, np.uint32))
    pc = LoopClosureProblemC.make(
        n_map=len(state), state=state, obs=obs, obs_pitch=obs.shape[1], offset=int(problem.offset) & 0xFFFFFFFF,
        n_keyframes=int(problem.n_keyframes), ki_id=int(problem.ki.id), n_ki=len(ki[3]), ki_pos3=ki[0], ki_r9=ki[1],
        ki_intr4=ki[2], ki_kp=ki[3], ki_desc=ki[4], ki_point=ki[5], n_kf=nkf, kf_id=kf_id, kf_pos3=kf_pos3, kf_r9=kf_r9,
        kf_intr4=kf_intr4, kf_kp=kf_kp, kf_desc=kf_desc, kf_point=kf_point, kf_start=start, kf_mask=kf_mask, **out)
    L = _lib.load()
    refused = False
    try:
        if backend == "host":
            check(L.mage_cheap_loop_closure_host(C.byref(cs), C.byref(pc)))
        else:
            check(L.mage_cheap_loop_closure(C.byref(cs), C.byref(pc), device))
    except MageError as e:
        if e.status != _lib.MAGE_ECAPACITY:
            raise
        refused = True
    masks = [kf_mask[start[k]:start[k + 1]].copy() for k in range(nkf)]
    return LoopClosureResult(state, obs, out["sample_index"], out["closure"], out["closure_verdict"],
                             out["connect"][:, :nkf], out["connect_verdict"][:, :nkf], out["ki_mask"][:len(ki[3])], masks,
                             out["kf_modified"][:nkf], out["counts"], int(out["status"][0]), refused)


def cheap_loop_closure(settings, problem: Problem, backend: str = "hip", device: int = 0, prefill: int = 0):
    """CheapLoopClosure and InsertKeyframe's associations alone: the step without covisible keyframes."""
    return cheap_loop_closure_and_connect(settings, dataclasses.replace(problem, kfs=()), backend, device, prefill)


# ----------------------------------------------------------------------------------------------
# The batched device chain
# ----------------------------------------------------------------------------------------------
def pack_problems(settings, problems: Sequence[Problem], kf_slots=None, map_pitch=None, obs_pitch=None, ki_pitch=None,
                  kf_pitch=None, device="cuda", fill: int = 0) -> dict:
    """The problems as the pitched device tensors of mage_cheap_loop_closure_batch_device, outputs
    included; every byte no problem owns is `fill`.  A count over its pitch is kept (the entry
    reports it), its data cut."""
    import torch

    n, mx = len(problems), int(_c(settings).max_map_points)
    kis = [p.ki.arrays() for p in problems]
    kfs = [[k.arrays() for k in p.kfs] for p in problems]

    def pitch(given, sizes):
        return max(list(sizes) + [1]) if given is None else int(given)

    slots = pitch(kf_slots, [len(k) for k in kfs])
    map_pitch = pitch(map_pitch, [len(p.state) for p in problems])
    obs_pitch = pitch(obs_pitch, [np.asarray(p.obs).shape[1] for p in problems])
    ki_pitch = pitch(ki_pitch, [len(k[3]) for k in kis if len(k[3]) <= MAX_KEYPOINTS])
    kf_pitch = pitch(kf_pitch, [len(k[3]) for ks in kfs for k in ks if len(k[3]) <= MAX_KEYPOINTS])

    def filled(shape, dtype):
        a = np.empty(shape, dtype)
        a.view(np.uint8).fill(fill)
        return a

    h = dict(d_n_map=filled(n, np.uint32), d_state=filled((n, map_pitch), MP_STATE_DTYPE),
             d_obs=filled((n, map_pitch, obs_pitch), MP_OBS_DTYPE), d_offset=filled(n, np.uint32),
             d_n_keyframes=filled(n, np.uint32), d_ki_id=filled(n, np.int32), d_n_ki=filled(n, np.uint32),
             d_ki_pos3=filled((n, 3), np.float32), d_ki_r9=filled((n, 9), np.float32), d_ki_intr4=filled((n, 4), np.float32),
             d_ki_kp=filled((n, ki_pitch), KP_DTYPE), d_ki_desc=filled((n, ki_pitch, 32), np.uint8),
             d_ki_point=filled((n, ki_pitch), np.int32), d_n_kf=filled(n, np.uint32), d_kf_id=filled((n, slots), np.int32),
             d_kf_pos3=filled((n, slots, 3), np.float32), d_kf_r9=filled((n, slots, 9), np.float32),
             d_kf_intr4=filled((n, slots, 4), np.float32), d_kf_kp=filled((n, slots, kf_pitch), KP_DTYPE),
             d_kf_desc=filled((n, slots, kf_pitch, 32), np.uint8), d_kf_point=filled((n, slots, kf_pitch), np.int32),
             d_n_kf_kp=filled((n, slots), np.uint32), d_kf_mask=filled((n, slots, kf_pitch), np.uint8),
             d_sample_index=filled((n, mx), np.uint32), d_closure=filled((n, mx), LC_DTYPE),
             d_closure_verdict=filled((n, mx), np.uint8), d_connect=filled((n, mx, slots), LC_DTYPE),
             d_connect_verdict=filled((n, mx, slots), np.uint8), d_ki_mask=filled((n, ki_pitch), np.uint8),
             d_kf_modified=filled((n, slots), np.uint8), d_counts=filled((n, 3), np.uint32), d_status=filled(n, np.uint32))
    for i, p in enumerate(problems):
        nm = min(len(p.state), map_pitch)
        po = min(np.asarray(p.obs).shape[1], obs_pitch)
        h["d_n_map"][i], h["d_offset"][i], h["d_n_keyframes"][i] = len(p.state), int(p.offset) & 0xFFFFFFFF, p.n_keyframes
        h["d_state"][i, :nm] = np.asarray(p.state, MP_STATE_DTYPE)[:nm]
        h["d_obs"][i, :nm, :po] = np.asarray(p.obs, MP_OBS_DTYPE)[:nm, :po]
        a = kis[i]
        nk = min(len(a[3]), ki_pitch)
        h["d_ki_id"][i], h["d_n_ki"][i], h["d_n_kf"][i] = p.ki.id, len(a[3]), len(kfs[i])
        h["d_ki_pos3"][i], h["d_ki_r9"][i], h["d_ki_intr4"][i] = a[0], a[1], a[2]
        h["d_ki_kp"][i, :nk], h["d_ki_desc"][i, :nk], h["d_ki_point"][i, :nk] = a[3][:nk], a[4][:nk], a[5][:nk]
        for k, (kf, a) in enumerate(zip(p.kfs, kfs[i])):
            if k >= slots:
                break
            nk = min(len(a[3]), kf_pitch)
            h["d_kf_id"][i, k], h["d_n_kf_kp"][i, k] = kf.id, len(a[3])
            h["d_kf_pos3"][i, k], h["d_kf_r9"][i, k], h["d_kf_intr4"][i, k] = a[0], a[1], a[2]
            h["d_kf_kp"][i, k, :nk], h["d_kf_desc"][i, k, :nk] = a[3][:nk], a[4][:nk]
            h["d_kf_point"][i, k, :nk], h["d_kf_mask"][i, k, :nk] = a[5][:nk], a[6][:nk]
    packed = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(device) for k, v in h.items()}
    packed.update(problems=n, kf_slots=slots, map_pitch=map_pitch, obs_pitch=obs_pitch, ki_pitch=ki_pitch, kf_pitch=kf_pitch)
    packed["_shapes"] = {k: (v.shape, v.dtype) for k, v in h.items()}
    return packed


def cheap_loop_closure_batch_device(settings, packed: dict, stream=None) -> None:
    """The chain of three launches over a packed batch (its d_* entries: torch device tensors or raw
    device pointers), asynchronous on `stream`."""
    args = {k: v for k, v in packed.items() if not k.startswith("_")}
    check(_lib.load().mage_cheap_loop_closure_batch_device(C.byref(_c(settings)), C.byref(LoopClosureBatchC.make(**args)),
                                                           C.c_void_p(stream) if stream else None))


def unpack_problems(packed: dict) -> dict:
    """The packed batch's arrays on the host in their shapes (synchronises through the copies)."""
    return {k: packed[k].cpu().numpy().view(dt).reshape(shape) for k, (shape, dt) in packed["_shapes"].items()}
