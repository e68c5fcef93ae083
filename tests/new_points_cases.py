"""Helpers of the new-map-point tests (test_new_points_reference.py, test_gpu_new_points.py): the
case table and a plain fp64 NumPy formulation of CreateInitialAssociations' match loop written from
the algorithm (the header of mageslam_amd/csrc/newpoints.hip and include/mage_hot.h) that shares no
code with the library.  Not a test module (nothing is collected).

Inputs are built in fp64 and rounded to float32 once; both sides get the same arrays, and the fp64
side takes the rounded values as exact.

Decisions and fragility.  Every geometry verdict is a chain of comparisons; the fp64 side records,
per match, the smallest relative margin to any threshold the match was actually tested against:

    epipolar   |sum - 2 eps| / (2 eps)
    depth      min |depth| / distance              (both cheirality tests)
    ratio      |ratio - min| / min
    octave     distance of the pre-rounding octave value from a rounding boundary, in octaves
    parallax   |cos - cmin| / (1 - cmin)
    branch     |D - 1e-5| / 1e-5                   (the near-parallel switch of the triangulation)

A match with a margin below FRAGILE may legitimately decide differently in float32.  The bookkeeping
is then run with three-valued state (a cell count is an interval, a Ki keypoint is taken / free /
maybe): a match whose verdict is not the same under every outcome of the fragile matches before it
is left out of the decision comparison too.  At most MAX_FRAGILE_SHARE of a case's matches may be
left out (asserted on the fp64 side alone).

The two grid formulas are float32 expressions of the reference (NewMapPointsCreation.cpp:197-199
and :287-298); the fp64 side evaluates them in NumPy float32, since their roundings are the point.

Tolerance.  The midpoint triangulation divides by D = |u|^2 |v|^2 sin^2(parallax), formed as a
difference of two products of size |u|^2 |v|^2: one float32 rounding of those moves the point by
eps32 |X - Ci| / sin^2(parallax).  A regular-branch point is within K_TOL times that of fp64.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from mageslam_amd._lib import DM_DTYPE, KP_DTYPE
from mageslam_amd.mapping import NewMapPointsCreationSettings

EPS32 = float(np.finfo(np.float32).eps)
FRAGILE = 1e-2
MAX_FRAGILE_SHARE = 0.05
# Worst ratio of the C++ twin's error to eps32 |X - Ci| / sin^2(parallax) over the committed cases
# (position, unit vector, dMin / dMax after their 8 eps32), measured by
# test_new_points_reference.py::test_host_outputs_within_tolerance, which prints it.
K_MEASURED = 4.09
K_TOL = 64.0  # eight times K_MEASURED (32.7), rounded up to a power of two

W, H, F = 1280, 720, 900.0
(ACCEPTED, EPIPOLAR, BEHIND, DISTANCE_RATIO, SCALE, PARALLAX, GRID_FULL, KI_TAKEN, BAD_INDEX) = range(9)


@dataclasses.dataclass
class Problem:
    name: str
    settings: NewMapPointsCreationSettings
    ki_pos3: np.ndarray
    ki_r9: np.ndarray
    ki_intr4: np.ndarray
    ki_kp: np.ndarray
    ki_assoc: np.ndarray  # bool per Ki keypoint, or None
    kc_pos3: np.ndarray   # (n_kc, 3)
    kc_r9: np.ndarray     # (n_kc, 9)
    kc_intr4: np.ndarray  # (n_kc, 4)
    kc_kp: list
    matches: list
    cap: int

    @property
    def n_matches(self):
        return sum(len(m) for m in self.matches)

    def args(self):
        """Positional arguments of mapping.new_map_points after the settings."""
        return (self.ki_pos3, self.ki_r9, self.ki_intr4, self.ki_kp, self.ki_assoc, self.kc_pos3, self.kc_r9,
                self.kc_intr4, self.kc_kp, self.matches)


# ------------------------------------------------------------------------------------------
# scene generator (fp64, rounded to float32 once)
# ------------------------------------------------------------------------------------------
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx





# camera centres of the Kc slots: baselines 0.25 to 0.4, slot 2 mostly along the optical axis
KC_CENTRES = [(0.30, 0.02, 0.01), (-0.08, 0.24, 0.04), (0.03, -0.02, 0.36), (-0.33, -0.05, 0.02), (0.10, -0.30, -0.03),
              (0.27, 0.20, 0.05), (-0.22, 0.25, -0.02), (0.05, 0.38, 0.03)]

# matches of one slot of the base scene, by kind
BASE_KINDS = dict(true=42, near=8, far=8, mid=12, octave=8, wrong=12, mirror=6)


def _project(cam, R, C, X):
    W, H, F = cam
    c = R @ (X - C)
    return np.array([F * c[0] / c[2] + W / 2, F * c[1] / c[2] + H / 2]), c[2]


class _Scene:
    def __init__(self, seed, n_kc, scale=1.2, cam=(W, H, F)):
        self.cam = cam
        self.kmat = np.array([[cam[2], 0, cam[0] / 2], [0, cam[2], cam[1] / 2], [0, 0, 1.0]])
        self.intr = np.array([cam[0] / 2, cam[1] / 2, cam[2], cam[2]], np.float32)
        self.rng = np.random.default_rng(seed)
        r = self.rng
        self.scale = scale
        self.Ri = _rot(*r.normal(0, 0.01, 3))
        self.Ci = r.normal(0, 0.01, 3)
        self.Rc = [_rot(*r.normal(0, 0.03, 3)) for _ in range(n_kc)]
        self.Cc = [np.array(KC_CENTRES[k]) + r.normal(0, 0.005, 3) for k in range(n_kc)]
        self.ki = []                         # (x, y, octave)
        self.kc = [[] for _ in range(n_kc)]  # (x, y, octave)
        self.m = [[] for _ in range(n_kc)]   # (kc index, ki index)
        self.ki_clean, self.ki_depth = {}, {}  # noise-free pixel and depth of the keypoints add() made

    def ki_point(self, depth, pix=None):
        """A Ki keypoint (noise-free pixel) and the world point at `depth` on its ray."""
        r = self.rng
        W, H, _ = self.cam
        p = np.array([r.uniform(20, W - 20), r.uniform(20, H - 20)]) if pix is None else np.asarray(pix, float)
        X = self.Ci + self.Ri.T @ (depth * np.linalg.solve(self.kmat, np.array([p[0], p[1], 1.0])))
        return p, X

    def predicted_octave(self, k, X, oi):
        di, dc = np.linalg.norm(X - self.Ci), np.linalg.norm(X - self.Cc[k])
        return int(math.floor(math.log2(dc / (di * self.scale ** -(oi + 0.5))) / math.log2(self.scale) - 0.5 + 0.5))

    def add_ki(self, p, octave):
        self.ki.append((p[0], p[1], octave))
        return len(self.ki) - 1

    def add_match(self, k, kc_xy, kc_octave, ki_index):
        self.kc[k].append((kc_xy[0], kc_xy[1], kc_octave))
        self.m[k].append((len(self.kc[k]) - 1, ki_index))

    def add(self, k, kind, ki_index=None):
        """One match of `kind` in slot k; a fresh Ki keypoint unless ki_index reuses one that add()
        made (the same world point, seen from another Kc)."""
        r = self.rng
        W, H, F = self.cam
        depth = {"near": r.uniform(0.2, 0.7), "far": r.uniform(800, 5000), "mid": r.uniform(12, 80)}.get(
            kind, r.uniform(2, 9))
        pix = None
        if ki_index is not None:
            pix = self.ki_clean[ki_index]
            depth = self.ki_depth[ki_index]
        p, X = self.ki_point(depth, pix)
        noise = 0.7
        if ki_index is None:
            oi = int(r.integers(0, 4))
            ki_index = self.add_ki(p + r.normal(0, noise, 2), oi)
            self.ki_clean[ki_index] = p
            self.ki_depth[ki_index] = depth
        oi = self.ki[ki_index][2]
        q, _ = _project(self.cam, self.Rc[k], self.Cc[k], X)
        oc = self.predicted_octave(k, X, oi)
        if kind == "octave":
            oc += int(r.choice([-1, 1]))
        if kind == "wrong":
            q = np.array([r.uniform(20, W - 20), r.uniform(20, H - 20)])
        elif kind == "mirror":
            # mirrored about the image of the ray's point at infinity: the rays meet behind the cameras
            d = self.Rc[k] @ (X - self.Ci)
            inf = np.array([F * d[0] / d[2] + W / 2, F * d[1] / d[2] + H / 2])
            q = 2 * inf - q
        else:
            q = q + r.normal(0, noise, 2)
        self.add_match(k, q, oc, ki_index)

    def fill(self, k, kinds):
        order = [kind for kind, n in kinds.items() for _ in range(n)]
        self.rng.shuffle(order)
        for kind in order:
            self.add(k, kind)

    def shuffle_ki(self):
        """Ki keypoints in random order, so trainIdx is not monotone in the match order."""
        perm = self.rng.permutation(len(self.ki))  # new index of old keypoint i is perm[i]
        ki = [None] * len(self.ki)
        for old, new in enumerate(perm):
            ki[new] = self.ki[old]
        self.ki = ki
        self.m = [[(q, int(perm[t])) for q, t in ms] for ms in self.m]
        return perm

    def problem(self, name, settings=None, assoc=None, cap=None, extra_ki=0):
        r = self.rng
        for _ in range(extra_ki):
            self.add_ki((r.uniform(0, self.cam[0]), r.uniform(0, self.cam[1])), int(r.integers(0, 4)))

        def kps(rows):
            a = np.zeros(len(rows), KP_DTYPE)
            for i, (x, y, o) in enumerate(rows):
                a[i] = (x, y, 31.0, -1.0, 10.0, o, -1)
            return a

        def dms(rows):
            a = np.zeros(len(rows), DM_DTYPE)
            for i, (q, t) in enumerate(rows):
                a[i] = (q, t, -1, 20.0)
            return a

        def pose(R, Cw):
            return (-(R @ Cw)).astype(np.float32), R.T.reshape(9).astype(np.float32)  # t; column-major R

        n_kc = len(self.kc)
        ti, ri = pose(self.Ri, self.Ci)
        kc_pose = [pose(self.Rc[k], self.Cc[k]) for k in range(n_kc)]
        s = settings or NewMapPointsCreationSettings()
        s = dataclasses.replace(s, pyramid_scale=self.scale, num_levels=8, image_width=self.cam[0], image_height=self.cam[1])
        ki_kp = kps(self.ki)
        mask = None
        if assoc is not None:
            mask = np.zeros(len(ki_kp), bool)
            mask[list(assoc)] = True
        total = sum(len(m) for m in self.m)
        return Problem(name, s, ti, ri, self.intr, ki_kp, mask,
                       np.array([p[0] for p in kc_pose], np.float32).reshape(n_kc, 3),
                       np.array([p[1] for p in kc_pose], np.float32).reshape(n_kc, 9),
                       np.tile(self.intr, (n_kc, 1)), [kps(k) for k in self.kc],
                       [dms(m) for m in self.m], max(total, 1) if cap is None else cap)


def _base(seed=11, **kw):
    sc = _Scene(seed, 3)
    for k in range(3):
        sc.fill(k, BASE_KINDS)
    sc.shuffle_ki()
    return sc.problem(kw.pop("name", "base"), extra_ki=40, **kw)


def _grid_start():
    """Cells that start at 5 and at 6 of 6: associated Ki keypoints inside cell 5 (column 1, row 1)
    and cell 10 (column 2, row 2) on top of the base scene's matches."""
    sc = _Scene(12, 3)
    for k in range(3):
        sc.fill(k, BASE_KINDS)
    sc.shuffle_ki()
    r = sc.rng
    assoc = []
    for _ in range(5):
        assoc.append(sc.add_ki((r.uniform(330, 630), r.uniform(250, 470)), 0))
    for _ in range(6):
        assoc.append(sc.add_ki((r.uniform(650, 950), r.uniform(490, 710)), 0))
    return sc.problem("grid_start", assoc=assoc, extra_ki=10)


def _taken():
    """Ki keypoints matched from three Kc (30) and from two (30): the later matches are KI_TAKEN
    unless their cell filled first."""
    sc = _Scene(13, 3)
    for i in range(60):
        sc.add(0, "true")
        t = len(sc.ki) - 1
        sc.add(1, "true", ki_index=t)
        if i < 30:
            sc.add(2, "true", ki_index=t)
    return sc.problem("taken", extra_ki=5)


def _grid_edges(name="grid_edges", cam=(W, H, F), seed=14):
    """Ki keypoints exactly on the cell boundaries (x = 320, 640, 960 and y = 240, 480 at 1280 x
    720): as associated keypoints they go through the first grid formula, as matched keypoints
    through the second.  At 1280 x 720 float32 rounds both 4 / 1280 and 3 / 720 up, so the second
    formula agrees with the first on every boundary; at 752 x 480 it rounds 4 / 752 down and tests
    x = 188 and x = 376 against the column to the left of the one the first formula counted them in."""
    sc = _Scene(seed, 2, cam=cam)
    r = sc.rng
    assoc = []
    xs, ys = tuple(cam[0] * k / 4 for k in (1, 2, 3)), tuple(cam[1] * k / 3 for k in (1, 2))
    pts = ([(x, y) for x in xs for y in ys] + [(x, r.uniform(30, cam[1] - 20)) for x in xs] +
           [(r.uniform(30, cam[0] - 30), y) for y in ys])
    for rep in range(2):
        for (x, y) in pts:
            # a match whose Ki keypoint sits exactly on the boundary (no noise on the Ki side)
            p, X = sc.ki_point(r.uniform(2, 9), (x, y))
            oi = int(r.integers(0, 4))
            t = sc.add_ki(p, oi)
            q, _ = _project(sc.cam, sc.Rc[rep], sc.Cc[rep], X)
            sc.add_match(rep, q + r.normal(0, 0.7, 2), sc.predicted_octave(rep, X, oi), t)
            assoc.append(sc.add_ki((x, y), 0))  # and an associated keypoint at the same place
    return sc.problem(name, assoc=assoc)


def _counts():
    """Slots with 0, 1, 63, 65 and 257 matches (the kernel takes 256 matches per pass, 64 per wave)."""
    sc = _Scene(15, 5)
    for k, n in enumerate((0, 1, 63, 65, 257)):
        kinds = ["true", "true", "true", "wrong", "mid", "octave", "near", "far"]
        for i in range(n):
            sc.add(k, kinds[i % len(kinds)])
    sc.shuffle_ki()
    return sc.problem("counts", settings=NewMapPointsCreationSettings(max_grid_count=40))


def _m257():
    sc = _Scene(16, 1)
    for i in range(257):
        sc.add(0, ["true", "true", "wrong", "mid"][i % 4])
    sc.shuffle_ki()
    return sc.problem("m257", settings=NewMapPointsCreationSettings(max_grid_count=30))


def _empty():
    sc = _Scene(17, 0)
    return sc.problem("empty", extra_ki=12)


def _bad_index():
    sc = _Scene(18, 3)
    for k in range(3):
        sc.fill(k, dict(true=20, wrong=4))
    sc.shuffle_ki()
    p = sc.problem("bad_index", extra_ki=3)
    n_ki = len(p.ki_kp)
    p.matches[0]["query_idx"][3] = -1
    p.matches[0]["train_idx"][7] = n_ki
    p.matches[1]["query_idx"][5] = len(p.kc_kp[1])
    p.matches[1]["train_idx"][9] = -5
    p.matches[2]["train_idx"][0] = 2 ** 31 - 1
    p.matches[2]["query_idx"][23] = 2 ** 30
    return p


def _slots8():
    sc = _Scene(19, 8)
    for k in range(8):
        sc.fill(k, dict(true=14, wrong=3, mid=3, near=2))
    sc.shuffle_ki()
    return sc.problem("slots8", settings=NewMapPointsCreationSettings(max_grid_count=12))


def _many_ki(n_ki, name):
    sc = _Scene(20, 2)
    for k in range(2):
        sc.fill(k, dict(true=24, wrong=4))
    p = sc.problem(name, extra_ki=n_ki - len(sc.ki))
    # the last keypoint takes part in a match
    last = n_ki - 1
    t = int(p.matches[1]["train_idx"][5])
    p.ki_kp[last] = p.ki_kp[t]
    p.matches[1]["train_idx"][5] = last
    assert len(p.ki_kp) == n_ki
    return p


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Problem, in a fixed order."""
    out = [
        _base(),
        _base(name="parallax", settings=NewMapPointsCreationSettings(min_parallax_degrees=1.0)),
        _base(name="open_grid", seed=21, settings=NewMapPointsCreationSettings(max_grid_count=10 ** 6)),
        _base(name="open_parallax", seed=22,
              settings=NewMapPointsCreationSettings(max_grid_count=10 ** 6, min_parallax_degrees=1.0)),
        _grid_start(),
        _taken(),
        _grid_edges(),
        _grid_edges("grid_edges_752", cam=(752, 480, 458.0), seed=23),
        _counts(),
        _m257(),
        _empty(),
        _bad_index(),
        _slots8(),
        _many_ki(4096, "ki4096"),
        _many_ki(4097, "ki4097"),
        _base(name="over_cap", cap=10),
    ]
    return {p.name: p for p in out}


BATCH_CASES = ("base", "parallax", "grid_start", "empty", "m257")


# ------------------------------------------------------------------------------------------
# the fp64 formulation
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Reference:
    verdict: list        # per slot, int array
    excluded: list       # per slot, bool array: left out of the decision comparison
    parallel: list       # per slot, bool array: the near-parallel branch was taken (where triangulated)
    geometry: list       # per slot, list of dicts (X, dir, dmin, dmax, di, sin2) or None
    accepted: list       # (slot, match index) in processing order, certain or not
    status: int
    n_parallel: int      # near-parallel branches among the triangulated matches
    cell_at_cap: bool    # some cell was full at a match's turn
    grid_disagree: int   # Ki keypoints whose two grid formulas name different columns or rows
    share: float         # excluded share of the matches


def _cells_f32(s, x, y):
    """(count cell, test cell) of a Ki keypoint: the reference's two float32 formulas."""
    f = np.float32
    x, y = f(x), f(y)
    gw, gh, iw, ih = f(s.grid_width), f(s.grid_height), f(s.image_width), f(s.image_height)
    cx = int(f(f(x * gw) / iw))
    cy = int(f(f(y * gh) / ih))
    tx = min(max(int(math.floor(f(x * f(gw / iw)))), 0), s.grid_width - 1)
    ty = min(max(int(math.floor(f(y * f(gh / ih)))), 0), s.grid_height - 1)
    return (cx, cy), (tx, ty)


def _geometry64(s, Vi, Vc, Ki_inv, Kc_inv, Fci, Fic, kc, ki):
    """(verdict, margin, parallel or None, outputs or None) of one match in fp64."""
    def epi(Fm, p1, p2):
        l = Fm @ np.array([p1[0], p1[1], 1.0])
        nu = l[0] * l[0] + l[1] * l[1]
        nu = 1.0 / math.sqrt(nu) if nu else 1.0
        return abs(p2[0] * l[0] + p2[1] * l[1] + l[2]) * nu

    pc, pi = (float(kc["x"]), float(kc["y"])), (float(ki["x"]), float(ki["y"]))
    thr = 2.0 * float(np.float32(s.max_epipolar_error))
    tot = epi(Fic, pi, pc) + epi(Fci, pc, pi)
    margin = abs(tot - thr) / thr
    if tot > thr:
        return EPIPOLAR, margin, None, None
    Wi, Wc = np.linalg.inv(np.vstack([Vi, [0, 0, 0, 1]])), np.linalg.inv(np.vstack([Vc, [0, 0, 0, 1]]))
    Ci, Cc = Wi[:3, 3], Wc[:3, 3]
    u = Wc[:3, :3] @ (Kc_inv @ np.array([pc[0], pc[1], 1.0]))
    v = Wi[:3, :3] @ (Ki_inv @ np.array([pi[0], pi[1], 1.0]))
    w = Cc - Ci
    a, b, c, d, e = u @ u, u @ v, v @ v, u @ w, v @ w
    D = a * c - b * b
    margin = min(margin, abs(D - 1e-5) / 1e-5)
    parallel = D < float(np.float32(0.00001))
    if parallel:
        sc, tc = 0.0, (d / b if b > c else e / c)
    else:
        sc, tc = (b * e - c * d) / D, (a * e - b * d) / D
    X = (Cc + sc * u + Ci + tc * v) * 0.5
    zi, zc = Vi[2, :3] @ X + Vi[2, 3], Vc[2, :3] @ X + Vc[2, 3]
    di, dc = np.linalg.norm(X - Ci), np.linalg.norm(X - Cc)
    margin = min(margin, abs(zi) / di if di else 0.0)
    if zi <= 0:
        return BEHIND, margin, parallel, None
    margin = min(margin, abs(zc) / dc if dc else 0.0)
    if zc <= 0:
        return BEHIND, margin, parallel, None
    rmin = float(np.float32(s.min_accepted_distance_ratio))
    ratio = di / np.linalg.norm(Ci - Cc)
    margin = min(margin, abs(ratio - rmin) / rmin)
    if ratio < rmin:
        return DISTANCE_RATIO, margin, parallel, None
    scale = float(np.float32(s.pyramid_scale))
    oi = int(ki["octave"])
    dmin = di * scale ** -(oi + 0.5)
    val = math.log2(dc / dmin) / math.log2(scale) - 0.5
    frac = (val - 0.5) % 1.0  # roundf's boundaries are the half-integers
    margin = min(margin, min(frac, 1.0 - frac))
    pred = int(math.floor(abs(val) + 0.5)) * (1 if val >= 0 else -1)  # roundf: halves away from zero
    if pred != int(kc["octave"]):
        return SCALE, margin, parallel, None
    ni, nc = (X - Ci) / di, (X - Cc) / dc
    cos = float(ni @ nc)
    cmin = math.cos(math.radians(float(np.float32(s.min_parallax_degrees))))
    margin = min(margin, abs(cos - cmin) / (1.0 - cmin))
    if cos > cmin:
        return PARALLAX, margin, parallel, None
    m = ni + nc
    out = dict(X=X, dir=m / np.linalg.norm(m), dmin=dmin, dmax=di * scale ** (s.num_levels - (oi + 0.5)), di=di,
               sin2=float(np.sum(np.cross(ni, nc) ** 2)))
    return ACCEPTED, margin, parallel, out


def _view(pos3, r9):
    R = np.asarray(r9, np.float64).reshape(3, 3).T  # r9 is column-major
    return np.hstack([R, np.asarray(pos3, np.float64).reshape(3, 1)])


def _fund(Vfrom, Kfrom_inv, Vto, Kto_inv):
    M = Vto @ np.linalg.inv(np.vstack([Vfrom, [0, 0, 0, 1]]))
    t = M[:, 3]
    Tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return Kto_inv.T @ (Tx @ M[:, :3]) @ Kfrom_inv


def _kinv(intr4):
    cx, cy, fx, fy = (float(v) for v in intr4)
    return np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))


@functools.lru_cache(maxsize=None)
def reference(name) -> Reference:
    p = cases()[name]
    s = p.settings
    n_kc, n_ki = len(p.kc_kp), len(p.ki_kp)
    empty = Reference([np.full(len(m), -1) for m in p.matches], [np.zeros(len(m), bool) for m in p.matches],
                      [np.zeros(len(m), bool) for m in p.matches], [[None] * len(m) for m in p.matches], [], 0, 0,
                      False, 0, 0.0)
    if p.n_matches and n_ki > 4096:
        empty.status = 1
        return empty
    cells = [_cells_f32(s, p.ki_kp["x"][i], p.ki_kp["y"][i]) for i in range(n_ki)]
    disagree = sum(1 for (c, t) in cells if c != t)
    ncell = s.grid_width * s.grid_height
    # fp64's own sequential state, and bounds of it over every outcome of the fragile matches:
    # a cell count lies in [lo, hi]; a Ki keypoint is taken in every outcome (t_all) or in some (t_some)
    cnt = np.zeros(ncell, np.int64)
    if p.ki_assoc is not None:
        for i in np.nonzero(p.ki_assoc)[0]:
            (cx, cy), _ = cells[i]
            cnt[cx + cy * s.grid_width] += 1
    lo, hi = cnt.copy(), cnt.copy()
    taken, t_all, t_some = np.zeros(n_ki, bool), np.zeros(n_ki, bool), np.zeros(n_ki, bool)
    Vi, Ki_inv = _view(p.ki_pos3, p.ki_r9), _kinv(p.ki_intr4)
    ref = empty
    cap_n = s.max_grid_count
    for k in range(n_kc):
        Vc, Kc_inv = _view(p.kc_pos3[k], p.kc_r9[k]), _kinv(p.kc_intr4[k])
        Fci, Fic = _fund(Vc, Kc_inv, Vi, Ki_inv), _fund(Vi, Ki_inv, Vc, Kc_inv)
        for j, m in enumerate(p.matches[k]):
            q, t = int(m["query_idx"]), int(m["train_idx"])
            if not (0 <= q < len(p.kc_kp[k]) and 0 <= t < n_ki and 0 <= int(p.ki_kp["octave"][t]) < 8):
                ref.verdict[k][j] = BAD_INDEX
                continue
            _, (tx, ty) = cells[t]
            cell = tx + ty * s.grid_width
            gv, margin, par, out = _geometry64(s, Vi, Vc, Ki_inv, Kc_inv, Fci, Fic, p.kc_kp[k][q], p.ki_kp[t])
            sure_geo = margin >= FRAGILE
            # fp64's verdict
            if cnt[cell] >= cap_n:
                v = GRID_FULL
                ref.cell_at_cap = True
            elif taken[t]:
                v = KI_TAKEN
            else:
                v = gv
                if par is not None:
                    ref.parallel[k][j] = par
                    ref.n_parallel += int(par)
            # the same verdict under every outcome?
            if lo[cell] >= cap_n:
                sure = True
            elif hi[cell] >= cap_n:
                sure = False
            elif t_all[t]:
                sure = True
            elif t_some[t]:
                sure = False
            else:
                sure = sure_geo
            ref.verdict[k][j] = v
            ref.excluded[k][j] = not sure
            if v == ACCEPTED:
                ref.geometry[k][j] = out
                ref.accepted.append((k, j))
                cnt[cell] += 1
                taken[t] = True
            # accepted in every outcome / in some outcome (both from the state before this match)
            in_all = hi[cell] < cap_n and not t_some[t] and gv == ACCEPTED and sure_geo
            in_some = lo[cell] < cap_n and not t_all[t] and (gv == ACCEPTED or not sure_geo)
            if in_all:
                lo[cell] += 1
                t_all[t] = True
            if in_some:
                hi[cell] += 1
                t_some[t] = True
    ref.status = 2 if len(ref.accepted) > p.cap else 0
    ref.grid_disagree = disagree
    ref.share = sum(int(e.sum()) for e in ref.excluded) / max(p.n_matches, 1)
    return ref
