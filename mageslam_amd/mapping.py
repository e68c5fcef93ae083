"""New map points — host mirror of NewMapPointsCreation
(Core/MAGESLAM/Source/Mapping/NewMapPointsCreation.cpp:171-446).

`new_map_points` is one problem through mage_new_map_points (the gfx950 kernel) or
mage_new_map_points_host (its plain C++ twin, the CPU backend); `create_initial_associations` adds
the reference's keyframe bookkeeping (:217-248) and IndexedMatch around it;
`new_map_points_batch_device` is the thin wrapper of the batched device entry, which reads the
matches exactly as mage_indexed_match_batch_device leaves them.

`locally_associate_new_associations` is the second half (LocallyAssociateNewAssociations, :337-424)
through mage_new_points_associate (the gfx950 kernel) or mage_new_points_associate_host (its twin);
`new_points_associate_batch_device` wraps the batched device entry, which reads the points exactly
as new_map_points_batch_device leaves them; `new_map_points_creation` is the whole function.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import DM_DTYPE, KP_DTYPE, NA_DTYPE, NP_DTYPE, NewPointsAssocSettingsC, NewPointsSettingsC, check, ptr

ACCEPTED, EPIPOLAR, BEHIND, DISTANCE_RATIO, SCALE, PARALLAX, GRID_FULL, KI_TAKEN, BAD_INDEX = range(9)
MAX_KC_SLOTS = 8
MAX_KI_KEYPOINTS = 4096
STATUS_OVER_LIMIT, STATUS_OVER_CAP = 1, 2


@dataclasses.dataclass
class NewMapPointsCreationSettings:
    """NewMapPointsCreationSettings (MageSettings.h:55-61) with the new-point grid of CameraSettings
    (MageSettings.h:311-313) and the pyramid and image size of Ki."""
    min_parallax_degrees: float = 0.0238961594253207
    max_epipolar_error: float = 3.84385518580709
    min_accepted_distance_ratio: float = 2.0
    min_keyframe_distance_squared: float = 0.0  # MinKeyframeDistanceForCreatingMapPointsSquared
    max_frames: int = 5                         # MaxFramesForNewPointsCreation
    grid_width: int = 4                         # NewPointGridWidth
    grid_height: int = 3                        # NewPointGridHeight
    max_grid_count: int = 6                     # NewPointMaxGridCount
    pyramid_scale: float = 1.2
    num_levels: int = 8
    image_width: int = 1280
    image_height: int = 720

    def to_c(self) -> NewPointsSettingsC:
        return NewPointsSettingsC.make(
            max_epipolar_error=self.max_epipolar_error, min_accepted_distance_ratio=self.min_accepted_distance_ratio,
            min_parallax_degrees=self.min_parallax_degrees, pyramid_scale=self.pyramid_scale,
            num_levels=self.num_levels, grid_width=self.grid_width, grid_height=self.grid_height,
            max_grid_count=self.max_grid_count, image_width=self.image_width, image_height=self.image_height)


@dataclasses.dataclass
class NewPointsResult:
    points: np.ndarray   # NP_DTYPE records in the order of the reference's newMapPoints.push_back
    verdicts: list       # per Kc slot, one verdict code per match
    status: int          # bit 0: over a limit (no points); bit 1: more points than `cap`


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def new_map_points(settings, ki_pos3, ki_r9, ki_intr4, ki_kp, ki_associated, kc_pos3, kc_r9, kc_intr4, kc_kps, matches,
                   cap=None, backend: str = "gpu", device: int = 0) -> NewPointsResult:
    """One Ki against its Kc slots in processing order.  Poses as mage_ba_set_cameras takes them
    (pos3 the view-space t, r9 the column-major R, intr4 {cx, cy, fx, fy}); kc_kps / matches are one
    KP_DTYPE / DM_DTYPE array per slot (queryIdx = Kc keypoint, trainIdx = Ki keypoint);
    ki_associated is Ki's associated-keypoint mask or None.  backend "gpu" runs the kernel on
    `device`, "host" the C++ twin."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    cs = settings if isinstance(settings, NewPointsSettingsC) else settings.to_c()
    n_kc = len(kc_kps)
    if len(matches) != n_kc:
        raise ValueError("one match array per Kc slot")
    ki_kp = np.ascontiguousarray(ki_kp, KP_DTYPE)
    mask = None if ki_associated is None else np.ascontiguousarray(np.asarray(ki_associated, bool), np.uint8)
    if mask is not None and len(mask) != len(ki_kp):
        raise ValueError("ki_associated length must equal the number of Ki keypoints")
    kps = [np.ascontiguousarray(k, KP_DTYPE) for k in kc_kps]
    ms = [np.ascontiguousarray(m, DM_DTYPE) for m in matches]
    kp_start = np.zeros(n_kc + 1, np.uint32)
    m_start = np.zeros(n_kc + 1, np.uint32)
    kp_start[1:] = np.cumsum([len(k) for k in kps])
    m_start[1:] = np.cumsum([len(m) for m in ms])
    kc_kp = np.concatenate(kps) if n_kc else np.zeros(0, KP_DTYPE)
    mm = np.concatenate(ms) if n_kc else np.zeros(0, DM_DTYPE)
    total = int(m_start[-1])
    cap = max(total, 1) if cap is None else int(cap)
    out = np.zeros(max(cap, 1), NP_DTYPE)
    verdict = np.full(max(total, 1), 0xFF, np.uint8)
    n_out, status = C.c_uint32(0), C.c_uint32(0)
    args = [C.byref(cs), ptr(_f32(ki_pos3, 3)), ptr(_f32(ki_r9, 9)), ptr(_f32(ki_intr4, 4)), ptr(ki_kp), len(ki_kp),
            ptr(mask), n_kc, ptr(_f32(kc_pos3, (n_kc, 3))), ptr(_f32(kc_r9, (n_kc, 9))), ptr(_f32(kc_intr4, (n_kc, 4))),
            ptr(kc_kp), ptr(kp_start), ptr(mm), ptr(m_start), ptr(out), cap, C.byref(n_out), ptr(verdict),
            C.byref(status)]
    L = _lib.load()
    if backend == "gpu":
        check(L.mage_new_map_points(*args, device))
    else:
        check(L.mage_new_map_points_host(*args))
    return NewPointsResult(out[: n_out.value].copy(),
                           [verdict[int(m_start[s]):int(m_start[s + 1])].copy() for s in range(n_kc)], int(status.value))


def new_map_points_batch_device(settings, problems: int, kc_slots: int, ki_pos3, ki_r9, ki_intr4, ki_kp, ki_pitch: int,
                                n_ki, ki_associated, n_kc, kc_pos3, kc_r9, kc_intr4, kc_kp, kc_pitch: int, n_kc_kp,
                                matches, match_cap: int, n_matches, out, cap: int, n_out, verdict, status,
                                stream=None) -> None:
    """Batched device form over `problems` Ki with `kc_slots` Kc slots each (torch device tensors;
    ki_associated may be None); pair = problem * kc_slots + slot.  `matches` / `n_matches` are the
    `out` / `n_out` of indexed_match_batch_device with A = Kc and B = Ki, capacity `match_cap`."""
    cs = settings if isinstance(settings, NewPointsSettingsC) else settings.to_c()
    check(_lib.load().mage_new_map_points_batch_device(
        C.byref(cs), problems, kc_slots, ptr(ki_pos3), ptr(ki_r9), ptr(ki_intr4), ptr(ki_kp), ki_pitch, ptr(n_ki),
        ptr(ki_associated), ptr(n_kc), ptr(kc_pos3), ptr(kc_r9), ptr(kc_intr4), ptr(kc_kp), kc_pitch, ptr(n_kc_kp),
        ptr(matches), match_cap, ptr(n_matches), ptr(out), cap, ptr(n_out), ptr(verdict), ptr(status),
        C.c_void_p(stream) if stream else None))


@dataclasses.dataclass(eq=False)
class Keyframe:
    """What CreateInitialAssociations reads of a MappingKeyframe: the pose, the undistorted
    calibration, the keypoints with their descriptors and the associated-keypoint mask."""
    pos3: np.ndarray
    r9: np.ndarray
    intr4: np.ndarray
    keypoints: np.ndarray    # KP_DTYPE
    descriptors: np.ndarray  # (n, 32) uint8
    associated: np.ndarray   # (n,) bool

    def world_position(self) -> np.ndarray:
        """GetWorldSpacePosition: -(R^T t), float32."""
        R = np.asarray(self.r9, np.float32).reshape(3, 3).T  # r9 is column-major
        return -(R.T @ np.asarray(self.pos3, np.float32))


@dataclasses.dataclass
class InitialAssociations:
    points: np.ndarray      # NP_DTYPE; kc_slot indexes `frames`
    frames: list            # indexes into the covisible list, in processing order (the Kc slots)
    kc_associated: list     # per frame, the Kc keypoints that became associated (:314)
    verdicts: list          # per frame, one verdict per match
    matches: list           # per frame, the IndexedMatch result
    status: int


def select_frames(ki: Keyframe, covisible, settings: NewMapPointsCreationSettings, map_scale: float = 1.0) -> list:
    """The covisible keyframes CreateInitialAssociations matches against, in its order (:217-248):
    sorted by squared distance from Ki, a keyframe without unassociated keypoints skipped without
    counting, one closer than MinKeyframeDistanceForCreatingMapPointsSquared * scale^2 skipped too,
    at most MaxFramesForNewPointsCreation counted."""
    c = ki.world_position()
    d2 = []
    for k in covisible:
        d = (k.world_position() - c).astype(np.float32)
        d2.append(np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])))
    order = sorted(range(len(covisible)), key=lambda i: d2[i])  # stable where std::sort leaves ties open
    floor = np.float32(np.float32(settings.min_keyframe_distance_squared) * np.float32(np.float32(map_scale) ** 2))
    frames = []
    for i in order:
        if len(frames) >= settings.max_frames:
            break
        if not np.any(~np.asarray(covisible[i].associated, bool)):
            continue
        if d2[i] < floor:
            continue
        frames.append(i)
    return frames


def create_initial_associations(ki: Keyframe, covisible, settings: NewMapPointsCreationSettings, tree=None,
                                max_hamming: int = 30, min_hamming_difference: int = 1, map_scale: float = 1.0,
                                backend: str = "gpu", device: int = 0, matcher=None) -> InitialAssociations:
    """CreateInitialAssociations (:171-329): the frames of select_frames, IndexedMatch(Kc, Ki) per
    frame under the unassociated masks, then every match through the new-point checks.  `matcher
    (kc, ki, kc_mask, ki_mask) -> DM_DTYPE array` replaces the GPU IndexedMatch over `tree` (the
    CPU backend has no matcher of its own).  A frame without matches keeps its place in the count,
    as in the reference (:248, :271)."""
    ki_un = ~np.asarray(ki.associated, bool)
    if not ki_un.any():  # :203-207
        return InitialAssociations(np.zeros(0, NP_DTYPE), [], [], [], [], 0)
    if len(ki.keypoints) > MAX_KI_KEYPOINTS:
        raise _lib.MageError(_lib.MAGE_EUNSUPPORTED, "more than 4096 Ki keypoints")
    if settings.max_frames > MAX_KC_SLOTS:
        raise _lib.MageError(_lib.MAGE_EINVAL, "max_frames must be <= 8")
    if matcher is None:
        if tree is None:
            raise ValueError("a vocabulary tree or a matcher is needed")
        from .bow import IndexedMatch

        def matcher(kc, ki_, kc_mask, ki_mask):
            return IndexedMatch(tree, kc.descriptors, ki_.descriptors, kc_mask, ki_mask, max_hamming,
                                min_hamming_difference)
    frames = select_frames(ki, covisible, settings, map_scale)
    matches = [np.ascontiguousarray(matcher(covisible[i], ki, ~np.asarray(covisible[i].associated, bool), ki_un),
                                    DM_DTYPE) for i in frames]
    kcs = [covisible[i] for i in frames]
    r = new_map_points(settings, ki.pos3, ki.r9, ki.intr4, ki.keypoints, ki.associated,
                       [k.pos3 for k in kcs], [k.r9 for k in kcs], [k.intr4 for k in kcs],
                       [k.keypoints for k in kcs], matches, backend=backend, device=device)
    if r.status & STATUS_OVER_LIMIT:
        raise _lib.MageError(_lib.MAGE_EUNSUPPORTED, "new map points: over a limit")
    assoc = [np.sort(r.points["kc_index"][r.points["kc_slot"] == s]).astype(np.int64) for s in range(len(frames))]
    return InitialAssociations(r.points, frames, assoc, r.verdicts, matches, r.status)


# ------------------------------------------------------------------------------------------
# LocallyAssociateNewAssociations (NewMapPointsCreation.cpp:337-424)
# ------------------------------------------------------------------------------------------
(NA_ASSOCIATED, NA_SAME_FRAME, NA_BEHIND, NA_BORDER, NA_ANGLE, NA_DISTANCE, NA_OCTAVE, NA_NO_MATCH,
 NA_BAD_INDEX) = range(9)
MAX_KF_KEYPOINTS = 4096


@dataclasses.dataclass
class NewPointsAssociationSettings:
    """The association part of NewMapPointsCreationSettings (MageSettings.h:55-61:
    NewMapPointsSearchRadius, MaxKeyframeAngleDegrees, AssociateMatcherSettings) and Ki's image
    border."""
    search_radius: float = 11.8816156
    max_keyframe_angle_degrees: float = 60.0
    image_border: float = 0.0
    max_hamming_distance: int = 30
    min_hamming_difference: int = 1

    def to_c(self) -> NewPointsAssocSettingsC:
        return NewPointsAssocSettingsC.make(
            search_radius=self.search_radius, max_keyframe_angle_degrees=self.max_keyframe_angle_degrees,
            image_border=self.image_border, max_hamming_distance=self.max_hamming_distance,
            min_hamming_difference=self.min_hamming_difference)


@dataclasses.dataclass
class LocalAssociations:
    associations: list   # per point, [(frame, keypoint)] in keyframe order
    records: np.ndarray  # (n_points, n_kf) NA_DTYPE: projection, predicted octave, keypoint or -1
    verdicts: np.ndarray  # (n_points, n_kf) uint8 NA_* codes (0xFF where a keyframe is over the limit)
    masks: list          # per keyframe, the updated unassociated mask (bool)
    status: int          # bit 0: a keyframe has more than 4096 keypoints


def new_points_associate(settings, assoc_settings, points, ki_desc, kf_pos3, kf_r9, kf_intr4, kf_kps, kf_descs,
                         kf_slot, kf_masks, backend: str = "gpu", device: int = 0):
    """mage_new_points_associate / _host on arrays: `points` as new_map_points wrote them, Ki's
    descriptors, per keyframe the pose, keypoints, descriptors, kf_slot (the Kc slot it had, or -1)
    and the unassociated mask as IndexedMatch saw it.  -> (records, verdicts, masks, status)."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    cs = settings if isinstance(settings, NewPointsSettingsC) else settings.to_c()
    ca = assoc_settings if isinstance(assoc_settings, NewPointsAssocSettingsC) else assoc_settings.to_c()
    n_kf = len(kf_kps)
    if not (len(kf_descs) == len(kf_masks) == len(kf_slot) == n_kf):
        raise ValueError("one keypoint / descriptor / mask array and one kf_slot per keyframe")
    pts = np.ascontiguousarray(points, NP_DTYPE)
    kid = np.ascontiguousarray(ki_desc, np.uint8).reshape(-1, 32)
    kps = [np.ascontiguousarray(k, KP_DTYPE) for k in kf_kps]
    ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in kf_descs]
    ms = [np.ascontiguousarray(np.asarray(m, bool), np.uint8) for m in kf_masks]
    for k in range(n_kf):
        if not (len(kps[k]) == len(ds[k]) == len(ms[k])):
            raise ValueError("a keyframe's keypoints, descriptors and mask must have one length")
    start = np.zeros(n_kf + 1, np.uint32)
    start[1:] = np.cumsum([len(k) for k in kps])
    kp = np.concatenate(kps) if n_kf else np.zeros(0, KP_DTYPE)
    desc = np.concatenate(ds) if n_kf else np.zeros((0, 32), np.uint8)
    mask = np.concatenate(ms) if n_kf else np.zeros(0, np.uint8)
    slot = np.ascontiguousarray(kf_slot, np.int32)
    n = len(pts)
    out = np.zeros((n, n_kf), NA_DTYPE)
    out["keypoint"] = -1
    verdict = np.full((n, n_kf), 0xFF, np.uint8)
    status = C.c_uint32(0)
    args = [C.byref(cs), C.byref(ca), ptr(pts), n, ptr(kid), len(kid), n_kf, ptr(_f32(kf_pos3, (n_kf, 3))),
            ptr(_f32(kf_r9, (n_kf, 9))), ptr(_f32(kf_intr4, (n_kf, 4))), ptr(kp), ptr(desc), ptr(start), ptr(slot),
            ptr(mask), ptr(out), ptr(verdict), C.byref(status)]
    L = _lib.load()
    if backend == "gpu":
        check(L.mage_new_points_associate(*args, device))
    else:
        check(L.mage_new_points_associate_host(*args))
    masks = [mask[int(start[k]):int(start[k + 1])].astype(bool) for k in range(n_kf)]
    return out, verdict, masks, int(status.value)


def sort_covisible(ki: Keyframe, covisible) -> list:
    """Indexes of `covisible` in the order CreateInitialAssociations' std::sort leaves (:217):
    ascending squared distance from Ki (stable)."""
    c = ki.world_position()
    d2 = []
    for k in covisible:
        d = (k.world_position() - c).astype(np.float32)
        d2.append(np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])))
    return sorted(range(len(covisible)), key=lambda i: d2[i])


def locally_associate_new_associations(ki: Keyframe, keyframes, kf_slot, points, settings, assoc_settings,
                                       backend: str = "gpu", device: int = 0) -> LocalAssociations:
    """LocallyAssociateNewAssociations (:337-424) over Keyframe objects in the reference's order:
    kf_slot[k] is the slot keyframes[k] had in create_initial_associations (its index in `frames`)
    or -1, and each keyframe's `associated` mask is the one IndexedMatch saw.  The keyframes are not
    modified; the updated unassociated masks are returned."""
    rec, verdict, masks, status = new_points_associate(
        settings, assoc_settings, points, ki.descriptors, [k.pos3 for k in keyframes], [k.r9 for k in keyframes],
        [k.intr4 for k in keyframes], [k.keypoints for k in keyframes], [k.descriptors for k in keyframes], kf_slot,
        [~np.asarray(k.associated, bool) for k in keyframes], backend=backend, device=device)
    assoc = [[(k, int(rec[p, k]["keypoint"])) for k in range(len(keyframes)) if verdict[p, k] == NA_ASSOCIATED]
             for p in range(len(rec))]
    return LocalAssociations(assoc, rec, verdict, masks, status)


def new_points_associate_batch_device(settings, assoc_settings, problems: int, kf_slots: int, points, cap: int,
                                      n_points, ki_desc, ki_pitch: int, n_ki, n_kf, kf_pos3, kf_r9, kf_intr4, kf_kp,
                                      kf_desc, kf_mask, kf_pitch: int, n_kf_kp, kf_slot, assoc, verdict, status,
                                      stream=None) -> None:
    """Batched device form (torch device tensors), one workgroup per pair = problem * kf_slots + k.
    `points` / `n_points` are the `out` / `n_out` of new_map_points_batch_device with capacity
    `cap`; kf_mask is in/out."""
    cs = settings if isinstance(settings, NewPointsSettingsC) else settings.to_c()
    ca = assoc_settings if isinstance(assoc_settings, NewPointsAssocSettingsC) else assoc_settings.to_c()
    check(_lib.load().mage_new_points_associate_batch_device(
        C.byref(cs), C.byref(ca), problems, kf_slots, ptr(points), cap, ptr(n_points), ptr(ki_desc), ki_pitch,
        ptr(n_ki), ptr(n_kf), ptr(kf_pos3), ptr(kf_r9), ptr(kf_intr4), ptr(kf_kp), ptr(kf_desc), ptr(kf_mask), kf_pitch,
        ptr(n_kf_kp), ptr(kf_slot), ptr(assoc), ptr(verdict), ptr(status), C.c_void_p(stream) if stream else None))


@dataclasses.dataclass
class MapPointKeyframeAssociations:
    """The reference's MapPointKeyframeAssociations: the new point and its Keyframes list, (keyframe,
    keypoint) pairs starting [Ki, Kc]; a keyframe is an index into `covisible`, Ki is -1."""
    point: np.void
    keyframes: list


@dataclasses.dataclass
class NewMapPoints:
    points: list                  # MapPointKeyframeAssociations in push_back order
    initial: InitialAssociations
    local: LocalAssociations
    order: list                   # indexes into `covisible` in the association's keyframe order


def new_map_points_creation(ki: Keyframe, covisible, settings: NewMapPointsCreationSettings,
                            assoc_settings: NewPointsAssociationSettings, tree=None, max_hamming: int = 30,
                            min_hamming_difference: int = 1, map_scale: float = 1.0, backend: str = "gpu",
                            device: int = 0, matcher=None) -> NewMapPoints:
    """NewMapPointsCreation (:426-446): create_initial_associations, then
    locally_associate_new_associations over all covisible keyframes in the sorted order of :217; a
    keyframe that made no points (outside `frames`) has kf_slot -1."""
    init = create_initial_associations(ki, covisible, settings, tree, max_hamming, min_hamming_difference, map_scale,
                                       backend, device, matcher)
    order = sort_covisible(ki, covisible)
    slot_of = {f: s for s, f in enumerate(init.frames)}
    loc = locally_associate_new_associations(ki, [covisible[i] for i in order], [slot_of.get(i, -1) for i in order],
                                             init.points, settings, assoc_settings, backend, device)
    if loc.status & STATUS_OVER_LIMIT:
        raise _lib.MageError(_lib.MAGE_EUNSUPPORTED, "new map points: a keyframe has more than 4096 keypoints")
    out = []
    for p, pt in enumerate(init.points):
        kfs = [(-1, int(pt["ki_index"])), (init.frames[int(pt["kc_slot"])], int(pt["kc_index"]))]
        kfs += [(order[k], t) for k, t in loc.associations[p]]
        out.append(MapPointKeyframeAssociations(pt, kfs))
    return NewMapPoints(out, init, loc, order)
