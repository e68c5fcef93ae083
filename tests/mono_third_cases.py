"""Synthetic third-frame problems for the monocular map initialisation tests
(test_mono_third_reference.py, test_gpu_mono_third.py, test_mono_third_facade.py) and the independent
fp64 formulations the twin is compared with.  640 x 480, f = 500, like mono_init_cases.py; everything
is built in fp64 and rounded once.

A case is a list of point specifications (`Pt`): where the point projects in the true midpoint
camera, and which keypoints the third frame holds near that projection, each with its descriptor's
Hamming distance `a` from the point's frame-0 descriptor and `b` from its frame-1 descriptor (the two
descriptors themselves are `c` bits apart, and a keypoint's descriptor is built so that both
distances hold exactly).  Unrelated descriptors are random, about 128 bits from everything.

Tolerances.  The float32 midpoint pose and projection are compared with the geodesic midpoint
R0 exp(1/2 log(R0^T R1)) and the projection through it in fp64:
  * projection within K_TOL eps32 (|px - cx| + |cx| + fx |X - C| / |depth|), the unit of
    new_points_assoc_cases.py, K_TOL = 8 x the measured worst ratio rounded up to a power of two;
  * the midpoint rotation within ANGLE_TOL = 4 x the measured worst angle (the convention of
    mono_init_cases.py); the centre is exact (one float add and one halving per component);
  * behind verdicts equal where |depth| / |X - C| >= FRAGILE.
test_mono_third_reference.py prints the measured figures.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from mageslam_amd import mono
from mageslam_amd._lib import KP_DTYPE

W, H, F = 640, 480, 500.0
INTR = np.array([W / 2, H / 2, F, F], np.float32)
EPS32 = float(np.finfo(np.float32).eps)
FRAGILE = 1e-2
MAX_FRAGILE_SHARE = 0.05
# Measured by test_mono_third_reference.py over the cases below:
K_MEASURED = 0.99         # worst projection error ratio (n257)
K_TOL = 8.0               # 8 x K_MEASURED (7.92), rounded up to a power of two
ANGLE_MEASURED = 1.2e-7   # radians, worst angle between the twin's midpoint rotation and the geodesic one
ANGLE_TOL = 4 * ANGLE_MEASURED


def rot(yaw, pitch=0.0, roll=0.0):
    """World-from-camera rotation, angles in degrees."""
    y, p, r = np.deg2rad([yaw, pitch, roll])
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return rz @ rx @ ry


def geodesic_midpoint(R0, R1):
    """R0 exp(1/2 log(R0^T R1)) in fp64 (Rodrigues; relative angles below 180 degrees)."""
    Rr = R0.T @ R1
    c = min(1.0, max(-1.0, (np.trace(Rr) - 1.0) / 2.0))
    th = np.arccos(c)
    w = np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])
    n = np.linalg.norm(w)
    if th < 1e-12 or n == 0:
        return R0.copy()
    k = w / n
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    h = th / 2
    return R0 @ (np.eye(3) + np.sin(h) * Kx + (1 - np.cos(h)) * (Kx @ Kx))


@dataclasses.dataclass
class Pt:
    kps: list = dataclasses.field(default_factory=list)  # (dx, dy, octave, a, b) per nearby keypoint
    c: int = 0                 # Hamming distance between the point's two descriptors
    uv: tuple | None = None    # its pixel in the true midpoint camera (default: the next grid slot)
    z: float = 5.0             # its depth there (negative: behind)
    xc: tuple | None = None    # or its camera-space position outright
    like: int | None = None    # same two descriptors (copies) and same pixel as this earlier point


@dataclasses.dataclass
class Case:
    name: str
    settings: mono.MonoMapInitializationSettings
    pos3: np.ndarray
    r9: np.ndarray
    points: np.ndarray
    idx0: np.ndarray
    idx1: np.ndarray
    desc0: np.ndarray
    desc1: np.ndarray
    kp2: np.ndarray
    desc2: np.ndarray
    kp_of: dict                 # (point, j) -> index in kp2 of the point's j-th specified keypoint
    cam_index: int = 1
    Rw: tuple = ()              # the two world rotations in fp64, as built
    expect_status: int = 0

    def args(self):
        return (self.settings, INTR, self.pos3, self.r9, self.points, self.idx0, self.idx1, self.desc0, self.desc1,
                self.kp2, self.desc2, self.cam_index)


def settings(**kw):
    return mono.MonoMapInitializationSettings(**kw)


def _flip(desc, bits):
    d = np.unpackbits(desc)
    d[bits] ^= 1
    return np.packbits(d)


def _keypoints(xy, octave):
    kp = np.zeros(len(xy), KP_DTYPE)
    if len(xy):
        kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    kp["size"], kp["angle"], kp["octave"] = 31.0, -1.0, octave
    return kp


GRID = [(70.0 + 90 * i, 70.0 + 100 * j) for j in range(4) for i in range(6)]  # 24 slots, search boxes of radius 40 apart


def build(name, pts, seed, R0=None, C0=(0, 0, 0), R1=None, C1=(1.0, 0.1, 0.05), s=None, distractors=0, extra01=3,
          n2_total=None, shuffle=True, expect_status=0):
    """The case of the point specifications `pts` seen from the two given frames (world rotations,
    centres).  `distractors` unrelated third-frame keypoints (every fourth at octave 1); n2_total pads
    the third frame with far-away unrelated keypoints up to that count."""
    rng = np.random.default_rng(seed)
    R0 = np.eye(3) if R0 is None else R0
    R1 = rot(4, -2, 1) if R1 is None else R1
    C0, C1 = np.asarray(C0, np.float64), np.asarray(C1, np.float64)
    # the poses as the library receives them: float32, bundler form (view-space t, column-major view R)
    r9 = np.stack([R0.reshape(9), R1.reshape(9)]).astype(np.float32)
    pos3 = np.stack([-(R0.T @ C0), -(R1.T @ C1)]).astype(np.float32)
    Rm, Cm = geodesic_midpoint(R0, R1), (C0 + C1) / 2
    n = len(pts)
    X = np.zeros((n, 3))
    uvs = np.zeros((n, 2))
    q0 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q1 = q0.copy()
    perm_bits = [rng.permutation(256) for _ in range(n)]
    slot = 0
    kxy, koct, kdesc, owner = [], [], [], []
    for i, p in enumerate(pts):
        if p.like is not None:
            q0[i], q1[i], perm_bits[i], uvs[i] = q0[p.like], q1[p.like], perm_bits[p.like], uvs[p.like]
        else:
            if p.uv is None and p.xc is None:
                uvs[i] = GRID[slot % len(GRID)]
                slot += 1
            elif p.uv is not None:
                uvs[i] = p.uv
            q1[i] = _flip(q0[i], perm_bits[i][:p.c])
        c = p.c if p.like is None else pts[p.like].c
        xc = np.array(p.xc) if p.xc is not None else np.array([(uvs[i, 0] - W / 2) / F * p.z, (uvs[i, 1] - H / 2) / F * p.z,
                                                               p.z])
        if p.xc is not None and p.xc[2] != 0:
            uvs[i] = (xc[0] / xc[2] * F + W / 2, xc[1] / xc[2] * F + H / 2)
        X[i] = Rm @ xc + Cm
        for j, (dx, dy, octv, a, b) in enumerate(p.kps):
            y2 = a - b + c
            assert y2 % 2 == 0 and 0 <= y2 // 2 <= c and a - y2 // 2 >= 0 and a - y2 // 2 <= 256 - c, (name, i, j)
            y, x = y2 // 2, a - y2 // 2
            inside = rng.permutation(perm_bits[i][:c])[:y]
            outside = rng.permutation(perm_bits[i][c:])[:x]
            kdesc.append(_flip(q0[i], np.concatenate([inside, outside]).astype(np.int64)))
            kxy.append((uvs[i, 0] + dx, uvs[i, 1] + dy))
            koct.append(octv)
            owner.append((i, j))
    for d in range(distractors):
        kxy.append((rng.uniform(10, W - 10), rng.uniform(10, H - 10)))
        koct.append(1 if d % 4 == 3 else 0)
        kdesc.append(rng.integers(0, 256, 32, dtype=np.uint8))
        owner.append(None)
    while n2_total is not None and len(kxy) < n2_total:
        kxy.append((rng.uniform(10, W - 10), rng.uniform(10, H - 10)))
        koct.append(0)
        kdesc.append(rng.integers(0, 256, 32, dtype=np.uint8))
        owner.append(None)
    n2 = len(kxy)
    order = rng.permutation(n2) if shuffle else np.arange(n2)
    kxy = np.array(kxy, np.float64).reshape(-1, 2)[order]
    kp2 = _keypoints(kxy.astype(np.float32), np.array(koct, np.int32)[order] if n2 else 0)
    desc2 = np.array(kdesc, np.uint8).reshape(-1, 32)[order]
    kp_of = {owner[o]: k for k, o in enumerate(order) if owner[o] is not None}
    # frames 0 and 1: the points' descriptors among a few others, in another order
    def frame(q):
        m = n + extra01
        d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        where = rng.permutation(m)[:n]
        d[where] = q
        return d, where.astype(np.int32)
    desc0, idx0 = frame(q0)
    desc1, idx1 = frame(q1)
    return Case(name, s or settings(), pos3, r9, X.astype(np.float32), idx0, idx1, desc0, desc1, kp2, desc2, kp_of,
                Rw=(R0, R1), expect_status=expect_status)


def put_first(case, i, j_first, j_second):
    """Keypoint j_first of point i gets a lower index in the third frame than keypoint j_second (the
    best / second rule visits candidates in ascending index, so their order decides)."""
    a, b = case.kp_of[(i, j_first)], case.kp_of[(i, j_second)]
    if a > b:
        case.kp2[[a, b]] = case.kp2[[b, a]]
        case.desc2[[a, b]] = case.desc2[[b, a]]
        case.kp_of[(i, j_first)], case.kp_of[(i, j_second)] = b, a
    return case


def _generic(name, n, seed, noise=0.0, **kw):
    """n points at random pixels, each with its true keypoint a few bits from both descriptors, at the
    projection plus a common (0.3, -0.2).  Without `noise` the scene is fronto-parallel (depth 5): the
    pose is then weakly determined, Levenberg-Marquardt's damping keeps the pose-only bundle adjustment
    converging through its fifth step, and every accept / reject decision has a clear margin.  With
    `noise` (pixels, per keypoint) the depths vary in 4..8 and the loop reaches its noise floor early:
    its last decisions are taken at cost changes of 1e-15 (POSE_FRAGILE below)."""
    rng = np.random.default_rng(seed + 7)
    pts = []
    for _ in range(n):
        a, b = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        c = abs(a - b) + 2 * int(rng.integers(0, min(a, b) + 1))
        pts.append(Pt([(0.3 + noise * float(rng.uniform(-1, 1)), -0.2 + noise * float(rng.uniform(-1, 1)), 0, a, b)], c,
                      uv=(float(rng.uniform(60, W - 60)), float(rng.uniform(60, H - 60))), z=float(rng.uniform(4, 8)) if noise else 5.0))
    return build(name, pts, seed, **kw)


def _true(n, a=4, b=6, c=6):
    return [Pt([(0.3, -0.2, 0, a, b)], c) for _ in range(n)]


def _decoy(dx, dy):
    return Pt([(dx, dy, 0, 3, 5)], 4)


def _ring(n, r=20.0):
    """n decoys, 20 px off in directions spread round the circle."""
    return [_decoy(r * np.cos(2 * np.pi * k / n + 0.3), r * np.sin(2 * np.pi * k / n + 0.3)) for k in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case; built once per process, treat as read-only."""
    c = {}

    def add(case):
        c[case.name] = case

    # sizes: the resolver's rounds of 64 and the block's 256
    for n in (0, 1, 63, 64, 65, 257):
        add(_generic(f"n{n}", n, 100 + n, distractors=40 if n else 5))
    # the third frame's limits
    add(build("kp0", [Pt() for _ in range(3)], 201))
    add(build("kp1", [Pt([(0.5, 0.5, 0, 2, 2)], 0), Pt(), Pt()], 202))
    add(_generic("kp4096", 20, 203, n2_total=4096))
    add(_generic("kp4097", 20, 204, n2_total=4097, expect_status=mono.M3_STATUS_OVER_LIMIT))
    bad = _generic("bad_idx0", 10, 205)
    bad.idx0[4] = len(bad.desc0)
    bad.expect_status = mono.M3_STATUS_BAD_INDEX
    add(bad)
    bad = _generic("bad_idx1", 10, 206)
    bad.idx1[7] = -1
    bad.expect_status = mono.M3_STATUS_BAD_INDEX
    add(bad)
    # resolver and matching (on the grid: the boxes do not overlap).  Point 0 and 1 compete for one
    # keypoint and the later falls back to the second; 2 and 3 compete and the later fails; 4: both
    # queries match different keypoints at equal distance (frame 0's wins); 5: frame 1's strictly
    # better; 6: only query 0 matches; 7: only query 1; 8: an octave-1 keypoint with the perfect
    # descriptor beside a worse octave-0 one; 9: the ratio test fails for both (8, then 7).
    rules = build("rules", [
        Pt([(1, 1, 0, 5, 5), (-3, 2, 0, 12, 12)], 0), Pt(like=0, z=6.0),
        Pt([(1, -1, 0, 4, 4)], 0), Pt(like=2, z=7.0),
        Pt([(2, 0, 0, 6, 20), (-2, 0, 0, 20, 6)], 14),
        Pt([(2, 0, 0, 9, 21), (-2, 0, 0, 21, 5)], 16),
        Pt([(0, 1, 0, 10, 50)], 40),
        Pt([(0, -1, 0, 50, 10)], 40),
        Pt([(0, 0, 1, 0, 0), (5, 5, 0, 8, 8)], 0),
        Pt([(3, 0, 0, 8, 8), (-3, 0, 0, 7, 7)], 0),
        Pt([(45, 0, 0, 1, 1)], 0),  # its only keypoint is outside the box
    ] + _true(4), 301, distractors=10)
    add(put_first(rules, 9, 0, 1))  # 8 then 7: second - best = 1 is not more than MinHammingDifference
    # the two bags set differently, descriptors between the thresholds: query 0 under 25 / 0, query 1
    # under 35 / 3.  Swapping the bags changes every one of these points.
    bags = build("bags", [
        Pt([(0.3, -0.2, 0, 30, 30)], 0),                         # 30: too far for query 0, fine for query 1
        Pt([(0.3, -0.2, 0, 28, 32)], 4),                         # likewise, different descriptors
        Pt([(-2, 1, 0, 12, 14), (0.3, -0.2, 0, 10, 12)], 2),     # differences of 2: enough for query 0 only
        Pt([(0.3, -0.2, 0, 31, 27)], 6),                         # 27 <= 35 but 31 > 25
        Pt([(2, 1, 0, 23, 23), (0.3, -0.2, 0, 20, 20)], 0),      # difference 3: query 1 needs more than 3
    ] + _true(3), 302, s=settings(extra_frame_max_hamming_distance=25, extra_frame_min_hamming_difference=0,
                                  five_point_max_hamming_distance=35, five_point_min_hamming_difference=3))
    add(put_first(put_first(bags, 2, 0, 1), 4, 0, 1))  # the worse candidate first: the difference is tested
    # 100 points over 40 near-identical keypoints in one box: long conflict chains, kept lists overflow
    blob = [Pt([(float(3 * (k % 8) - 10), float(3 * (k // 8) - 6), 0, 2 + k % 3, 3 + k % 3) for k in range(40)], 1,
               uv=(320.0, 240.0))]
    blob += [Pt(like=0, z=4.0 + 0.03 * k) for k in range(99)]
    add(build("blob", blob, 303, s=settings(extra_frame_min_hamming_difference=0, five_point_min_hamming_difference=0,
                                            min_third_frame_match_percentage=0.3)))
    # contention under different bags (25 / 0 against 35 / 3): 30 points with one pair of descriptors
    # over 14 keypoints whose distances lie round the two thresholds.  Some are candidates of query 1
    # alone (d0 > 25, d1 <= 35), and taking one of them changes only query 1's ratio test of the next
    # point, so a resolver has to look for earlier marks among the candidates of both queries.
    ab = [(28, 30), (30, 28), (26, 34), (27, 33), (20, 26), (22, 24), (24, 30), (31, 29), (33, 35), (29, 27), (18, 28),
          (21, 31), (34, 34), (23, 29)]
    bb = [Pt([(float(4 * (k % 5) - 8), float(4 * (k // 5) - 4), 0, a, b) for k, (a, b) in enumerate(ab)], 10,
             uv=(320.0, 240.0))]
    bb += [Pt(like=0, z=4.0 + 0.05 * k) for k in range(29)]
    add(build("bags_blob", bb, 304, s=settings(extra_frame_max_hamming_distance=25, extra_frame_min_hamming_difference=0,
                                               five_point_max_hamming_distance=35, five_point_min_hamming_difference=3,
                                               min_third_frame_match_percentage=0.1)))
    # projection and midpoint pose
    add(build("behind", _true(12) + [Pt([(0, 0, 0, 2, 2)], 0, z=-5.0), Pt(z=-0.5)] + _true(2), 401))
    # identical rotations (the identity, so that the depth of a point in the camera plane is exactly 0)
    add(build("rot_same", _true(17) + [Pt(xc=(0.3, 0.2, 0.0))] + _true(5), 402, R0=np.eye(3), R1=np.eye(3),
              C1=(1.0, 0.0, 0.0)))
    add(build("rot_neg_dot", _true(14), 403, R0=rot(100, 3, -2), R1=rot(-100, -4, 1), C0=(0.2, 0, 0), C1=(-0.3, 0.1, 1.0)))
    add(build("rot120", _true(14), 404, R0=rot(-60, 5, 0), R1=rot(60, -5, 3)))
    add(_generic("rot_small_w", 30, 405, R0=rot(170, 10, 40), R1=rot(-175, -5, 60), distractors=20))
    # gates and culling (MinThirdFrameMatchPercentage 0.5)
    add(build("gate_exact", _true(5) + [Pt() for _ in range(5)], 501))
    add(build("gate_short", _true(4) + [Pt() for _ in range(6)], 502))
    add(build("cull_tips", _true(12) + _ring(3) + [Pt() for _ in range(12)], 503))
    add(build("decoys", _true(12) + _ring(3), 504))
    add(_generic("noisy60", 60, 505, noise=1.0, distractors=30))
    return c


def case(name):
    return cases()[name]


# Cases whose pose-only bundle adjustment is fragile in the sense of tests/pose_cases.py (an accept /
# reject decision of the fp64 reference at a relative cost change below 1e-9, which another rounding may
# take the other way): n1 has one observation and its cost reaches zero, noisy60 sits at its noise
# floor.  Their outlier flags are still compared (those margins are wide); only the pose bound is not.
# test_mono_third_reference.py asserts that these are the fragile cases, all of them and no others.
POSE_FRAGILE = ("n1", "noisy60")

FINISH_CASES = ["n1", "n63", "n257", "rules", "bags", "blob", "bags_blob", "behind", "rot120", "gate_exact", "gate_short", "cull_tips",
                "decoys", "noisy60"]


# ------------------------------------------------------------------------------------------
# the fp64 side
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Ref:
    Rm: np.ndarray       # world rotation of the geodesic midpoint
    Cm: np.ndarray
    x: np.ndarray        # (n,) projection (nan at depth 0)
    y: np.ndarray
    xscale: np.ndarray   # the tolerance's unit
    yscale: np.ndarray
    depth: np.ndarray
    margin: np.ndarray   # |depth| / |X - C|
    share: float


@functools.lru_cache(maxsize=None)
def reference(name) -> Ref:
    """The geodesic midpoint pose of the float32 input poses and the projection through it, in fp64."""
    c = case(name)
    Rw = [c.r9[k].astype(np.float64).reshape(3, 3) for k in range(2)]  # column-major view R = row-major world R
    C = [-(Rw[k] @ c.pos3[k].astype(np.float64)) for k in range(2)]
    Rm, Cm = geodesic_midpoint(Rw[0], Rw[1]), (C[0] + C[1]) / 2
    X = c.points.astype(np.float64)
    cx, cy, fx, fy = (float(v) for v in INTR)
    xc = (X - Cm) @ Rm
    depth = xc[:, 2] if len(X) else np.zeros(0)
    with np.errstate(all="ignore"):
        div = np.where(depth != 0, depth, 1.0)
        x, y = xc[:, 0] / div * fx + cx, xc[:, 1] / div * fy + cy
        dist = np.linalg.norm(X - Cm, axis=1)
        xs = np.abs(x - cx) + abs(cx) + fx * dist / np.abs(div)
        ys = np.abs(y - cy) + abs(cy) + fy * dist / np.abs(div)
        margin = np.abs(depth) / dist
    share = float((margin < FRAGILE).sum()) / max(len(X), 1)
    return Ref(Rm, Cm, x, y, xs, ys, depth, margin, share)


def rotation_angle(Ra, Rb):
    """Angle (radians) of Ra^T Rb, from the skew part (accurate for small angles)."""
    Rr = Ra.T @ Rb
    w = np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])
    return float(np.arctan2(np.linalg.norm(w) / 2, (np.trace(Rr) - 1) / 2))


def pose_batch_of(h, c):
    """The twin's bundle-adjustment inputs as the synth.PoseBatch oracle.pose_batch takes."""
    from mageslam_amd import synth

    n = len(h.ba_uv)
    return synth.PoseBatch(pos=h.pos3.reshape(1, 3).copy(), r9=h.r9.reshape(1, 9).copy(), intr=INTR.reshape(1, 4).copy(),
                           obs_start=np.array([0, n], np.uint32), points=h.ba_points.reshape(-1, 3).copy(),
                           uv=h.ba_uv.reshape(-1, 2).copy(), info=h.ba_info.copy(), true_pos=np.zeros((1, 3)),
                           true_rot=np.eye(3)[None])
