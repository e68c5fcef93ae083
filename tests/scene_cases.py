"""Named scenes of the scene-extent tests: frames for CalculateBoundingPlaneDepthsForKeyframe
(mageslam_amd.scene), each a seeded camera, map points in front of it, keypoints at their
projections and an association list.  The CPU tests compare the twin with the fp64 restatement of
tests/scene_ref.py on them, the GPU test the kernel with the twin."""
import dataclasses
import functools

import numpy as np

from mageslam_amd import scene
from mageslam_amd._lib import KP_DTYPE

WIDTH, HEIGHT = 640, 480
INTR = np.array([320.0, 240.0, 500.0, 500.0], np.float32)  # cx, cy, fx, fy
DEFAULTS = scene.BoundingDepthSettings()

# A softness and a count of valid depths whose product, taken in float as the reference takes it
# (BoundingPlaneDepths.cpp:69), lies just under an integer: float32(0.53) * 100 = 52.999996, so the
# rank is 52, where 0.53 * 100 on paper is 53.  Found by a search over k / 100 and counts below 300.
UNDER_SOFTNESS, UNDER_COUNT, UNDER_RANK = 0.53, 100, 52
assert int(np.float32(UNDER_SOFTNESS) * np.float32(UNDER_COUNT)) == UNDER_RANK
assert round(UNDER_SOFTNESS * UNDER_COUNT) == UNDER_RANK + 1


@dataclasses.dataclass
class DepthScene:
    name: str
    settings: scene.BoundingDepthSettings
    frame: scene.DepthFrame
    cap: int | None = None   # None: the frame's own count


def rotation(rng, angle):
    """A rotation by `angle` radians about a seeded axis, float32 entries."""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


def bounds(settings, width=WIDTH, height=HEIGHT):
    """The region of interest in pixels as the reference forms it: float products."""
    w, h = np.float32(width), np.float32(height)
    f = np.float32
    return (f(settings.region_of_interest_min_x) * w, f(settings.region_of_interest_min_y) * h,
            f(settings.region_of_interest_max_x) * w, f(settings.region_of_interest_max_y) * h)


def make_frame(seed, n_inside, n_outside=0, extra_kp=3, identity=False, duplicates=0, depth_range=(2.0, 10.0),
               settings=DEFAULTS):
    """n_inside points whose keypoints lie inside the region of interest and n_outside whose keypoints
    lie in the image's border outside it, in a seeded order; `duplicates` of the inside points repeat
    another's position (equal depths); extra_kp keypoints carry no point."""
    rng = np.random.default_rng(seed)
    R = np.eye(3, dtype=np.float32) if identity else rotation(rng, 0.3)
    t = np.zeros(3, np.float32) if identity else rng.uniform(-0.5, 0.5, 3).astype(np.float32)
    x0, y0, x1, y1 = [float(b) for b in bounds(settings)]
    n = n_inside + n_outside
    uv = np.empty((n, 2))
    uv[:n_inside, 0] = rng.uniform(x0 + 1, x1 - 1, n_inside)
    uv[:n_inside, 1] = rng.uniform(y0 + 1, y1 - 1, n_inside)
    # outside: in the left or the top border strip
    left = rng.random(n_outside) < 0.5
    uv[n_inside:, 0] = np.where(left, rng.uniform(0, x0 - 1, n_outside), rng.uniform(0, WIDTH, n_outside))
    uv[n_inside:, 1] = np.where(left, rng.uniform(0, HEIGHT, n_outside), rng.uniform(0, y0 - 1, n_outside))
    z = rng.uniform(*depth_range, n)
    cam = np.stack([(uv[:, 0] - INTR[0]) / INTR[2] * z, (uv[:, 1] - INTR[1]) / INTR[3] * z, z], 1)
    if duplicates:
        src = rng.integers(0, n_inside, duplicates)
        dst = rng.choice(n_inside, duplicates, replace=False)
        cam[dst] = cam[src]
    world = ((cam - t.astype(np.float64)) @ R.astype(np.float64)).astype(np.float32)  # R^T (Xc - t)
    order = rng.permutation(n)
    world, uv = world[order], uv[order]
    n_kp = n + extra_kp
    slots = rng.permutation(n_kp)[:n]  # point i is seen at keypoint slots[i]
    kp = np.zeros(n_kp, KP_DTYPE)
    kp["x"], kp["y"] = rng.uniform(0, WIDTH, n_kp), rng.uniform(0, HEIGHT, n_kp)
    kp["x"][slots], kp["y"][slots] = uv[:, 0], uv[:, 1]
    kp["size"], kp["angle"] = 31.0, -1.0
    ids = rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32)  # any 32 bits, NaN patterns included
    return scene.DepthFrame(pos3=t, r9=np.ascontiguousarray(R.T).reshape(9), intr4=INTR.copy(), width=WIDTH, height=HEIGHT,
                            kp=kp, map_xyzi=scene.map_points(world, ids), kp_index=slots.astype(np.int32))


def _with(frame, **kw):
    return dataclasses.replace(frame, **kw)


def _set_point(frame, i, xyz=None, uv=None):
    """Point i moved to xyz and / or its keypoint to uv (copies)."""
    mp, kp = frame.map_xyzi.copy(), frame.kp.copy()
    if xyz is not None:
        mp[i, :3] = xyz
    if uv is not None:
        kp["x"][frame.kp_index[i]], kp["y"][frame.kp_index[i]] = uv
    return _with(frame, map_xyzi=mp, kp=kp)


def _edges():
    """Eight points: keypoints exactly on the four edges of the region (inside: the region is
    closed) and one float step outside each."""
    f = make_frame(11, 8, identity=True)
    x0, y0, x1, y1 = bounds(DEFAULTS)
    inf = np.float32(np.inf)
    spots = [(x0, 200), (x1, 200), (300, y0), (300, y1),
             (np.nextafter(x0, -inf), 200), (np.nextafter(x1, inf), 200), (300, np.nextafter(y0, -inf)),
             (300, np.nextafter(y1, inf))]
    for i, uv in enumerate(spots):
        f = _set_point(f, i, uv=uv)
    return f


def _equal_depths():
    """Identity pose, every point on the plane z = 4: all depths are exactly 4."""
    f = make_frame(12, 40, 6, identity=True)
    mp = f.map_xyzi.copy()
    mp[:, 2] = 4.0
    return _with(f, map_xyzi=mp)


def _depth_zero():
    """Identity pose and a point with z = 0: camera depth exactly 0, the division guard of
    ProjectUndistorted.  Its keypoint lies outside the region, so it is no valid depth."""
    f = make_frame(13, 20, 4, identity=True)
    return _set_point(f, 5, xyz=(0.25, -0.5, 0.0), uv=(3.0, 3.0))


def _bad_index():
    f = make_frame(14, 30, 5)
    idx = f.kp_index.copy()
    idx[3], idx[17] = -1, len(f.kp)
    return _with(f, kp_index=idx)


def _nonpositive():
    """A point behind the camera whose keypoint lies inside the region."""
    f = make_frame(15, 30, 5, identity=True)
    return _set_point(f, 7, xyz=(0.1, 0.2, -1.5))


def signed_zero_frame(order=(0, 1)):
    """Two valid depths, -0 and +0.  (p - c) . f of a rotation is -0 only by underflow, so the
    frame's matrix has a zero third row instead: the forward is (+0, +0, +0), and the depths of
    (-1, -1, -1) and (1, 1, 1) are sums of three products -0 and of three products +0."""
    f = make_frame(22, 2, identity=True)
    r = np.eye(3, dtype=np.float32)
    r[2, 2] = 0.0
    mp = f.map_xyzi.copy()
    mp[:, :3] = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]
    order = list(order)
    return _with(f, r9=np.ascontiguousarray(r.T).reshape(9), map_xyzi=mp[order], kp_index=f.kp_index[order])


@functools.lru_cache(maxsize=None)
def scenes():
    soft = dataclasses.replace
    s = [
        DepthScene("n0", DEFAULTS, make_frame(1, 0)),
        DepthScene("n1", DEFAULTS, make_frame(2, 1)),
        DepthScene("n2", DEFAULTS, make_frame(3, 2)),
        DepthScene("all_outside", DEFAULTS, make_frame(4, 0, 25)),
        DepthScene("edges", DEFAULTS, _edges()),
        DepthScene("equal_depths", soft(DEFAULTS, near_depth_softness=0.25, far_depth_softness=0.1), _equal_depths()),
        DepthScene("soft0", DEFAULTS, make_frame(5, 200, 40, duplicates=10)),
        DepthScene("soft_under_integer", soft(DEFAULTS, near_depth_softness=UNDER_SOFTNESS), make_frame(6, UNDER_COUNT, 20)),
        DepthScene("soft_under_integer_far", soft(DEFAULTS, far_depth_softness=UNDER_SOFTNESS),
                   make_frame(6, UNDER_COUNT, 20)),
        DepthScene("soft_025_01", soft(DEFAULTS, near_depth_softness=0.25, far_depth_softness=0.1),
                   make_frame(7, 257, 30, duplicates=8)),
        DepthScene("depth_zero", DEFAULTS, _depth_zero()),
        DepthScene("bad_index", DEFAULTS, _bad_index()),
        DepthScene("nonpositive", DEFAULTS, _nonpositive()),
        DepthScene("cap_exact", DEFAULTS, make_frame(8, 33, 7), cap=40),
        DepthScene("cap_plus_one", DEFAULTS, make_frame(9, 34, 7), cap=40),
        DepthScene("cap_over_limit", DEFAULTS, make_frame(10, 5, 1), cap=scene.MAX_POINTS + 1),
    ]
    return {c.name: c for c in s}


NAMES = list(scenes())


def depth_scene(name) -> DepthScene:
    return scenes()[name]


# ----------------------------------------------------------------------------------------------
# Volume-of-interest scenes: pose histories for CalculateVolumeOfInterest
# ----------------------------------------------------------------------------------------------
VOI_DEFAULTS = scene.VolumeOfInterestSettings()
VOI_CHUNK = 128  # csrc/scene_voi.hip VOI_CHUNK: keyframe records staged in LDS at a time


@dataclasses.dataclass
class VoiScene:
    name: str
    settings: scene.VolumeOfInterestSettings
    keyframes: np.ndarray   # (n, 3, 4) float32 world-from-camera
    depths: np.ndarray      # (n, 2) float32 {near, far}
    status: int = scene.VOI_OK


def look_at(pos, target, up=(0.0, 1.0, 0.0)):
    """World-from-camera matrix of a camera at pos looking at target: columns right, up, forward, pos."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    f = (target - pos) / np.linalg.norm(target - pos)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    return np.stack([r, u, f, pos], 1).astype(np.float32)


def voi_history(kind, n, seed):
    """n keyframes: 'circle' on a jittered ring looking inward, 'line' along a line looking along
    it (every centroid on the others' view axes), 'place' all at one place, 'flat' in a row looking the same way, 'cloud' scattered and
    looking at a common region."""
    rng = np.random.default_rng(seed)
    kf = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        if kind == "circle":
            a = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / n
            pos = np.array([3 * np.cos(a), rng.uniform(-0.3, 0.3), 3 * np.sin(a)])
            kf[i] = look_at(pos, rng.uniform(-0.2, 0.2, 3))
        elif kind == "line":
            d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
            pos = d * (0.7 * i + rng.uniform(0, 0.1))
            kf[i] = look_at(pos, pos + d, up=(0.0, 1.0, 0.1))
        elif kind == "flat":
            pos = np.array([0.8 * i + rng.uniform(0, 0.1), 0.0, 0.0])
            kf[i] = look_at(pos, pos + np.array([0.0, 0.0, 1.0]))
        elif kind == "place":
            kf[i] = look_at([0.5, 0.25, -1.0], [0.0, 0.0, 2.0])
        else:
            pos = rng.uniform(-2, 2, 3) + np.array([0, 0, -4.0])
            kf[i] = look_at(pos, rng.uniform(-0.5, 0.5, 3))
    near = rng.uniform(1.0, 1.6, n)
    depths = np.stack([near, near + rng.uniform(1.5, 3.0, n)], 1).astype(np.float32)
    if kind == "place":
        depths[:] = depths[0]
    return kf, depths


def _voi(name, kind, n, seed, status=scene.VOI_OK, minus_one=False, **kw):
    kf, d = voi_history(kind, n, seed)
    if minus_one:
        d[n // 2] = -1.0
    return VoiScene(name, dataclasses.replace(VOI_DEFAULTS, **kw), kf, d, status)


# The seeds are chosen on the CPU by search (tests/test_scene_voi_reference.py asserts the condition for
# every scene) so that on every level no fp64 voxel or centroid value lies within
# 4 x n_kf x e_t of the fp64 threshold and the fp64 grid dimensions are the twin's.
@functools.lru_cache(maxsize=None)
def voi_scenes():
    s = [
        _voi("kf1", "cloud", 1, VOI_SEEDS["kf1"], voxel_count_floor=2000),
        _voi("kf2_floor16000", "cloud", 2, VOI_SEEDS["kf2_floor16000"]),
        _voi("kf3_iter1", "cloud", 3, VOI_SEEDS["kf3_iter1"], iterations=1, voxel_count_floor=2000),
        _voi("kf65_circle", "circle", 65, VOI_SEEDS["kf65_circle"], voxel_count_floor=1000),
        _voi("kf129_chunk_plus_one", "circle", VOI_CHUNK + 1, VOI_SEEDS["kf129_chunk_plus_one"], voxel_count_floor=1000),
        _voi("floor64", "cloud", 5, VOI_SEEDS["floor64"], voxel_count_floor=64),
        _voi("line", "line", 6, VOI_SEEDS["line"], voxel_count_floor=2000),
        _voi("one_place", "place", 5, VOI_SEEDS["one_place"], voxel_count_floor=2000),
        _voi("flat_box", "flat", 4, VOI_SEEDS["flat_box"], voxel_count_floor=2000, kernel_angle_y_rads=0.004),
        _voi("depth_minus_one", "cloud", 5, VOI_SEEDS["depth_minus_one"], minus_one=True, voxel_count_floor=2000),
        _voi("floor4_degenerate", "cloud", 4, 8, status=scene.VOI_DEGENERATE, voxel_count_floor=4),
        _voi("threshold1_empty", "cloud", 4, 9, status=scene.VOI_EMPTY, threshold=1.0, voxel_count_floor=2000),
        _voi("no_keyframes", "cloud", 0, 10, status=scene.VOI_NO_KEYFRAMES),
    ]
    return {c.name: c for c in s}


VOI_SEEDS = {"kf1": 1, "kf2_floor16000": 1, "kf3_iter1": 1, "kf65_circle": 4, "kf129_chunk_plus_one": 5, "floor64": 1,
             "line": 1, "one_place": 1, "flat_box": 2, "depth_minus_one": 7}
VOI_NAMES = list(voi_scenes())
VOI_OK_NAMES = [n for n in VOI_NAMES if voi_scenes()[n].status == scene.VOI_OK]


def voi_scene(name) -> VoiScene:
    return voi_scenes()[name]
