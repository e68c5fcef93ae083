"""Helpers of the new-point association tests (test_new_points_assoc_reference.py,
test_gpu_new_points_assoc.py): the case table and a plain fp64 NumPy formulation of
LocallyAssociateNewAssociations' projection, gate and octave (steps 1-4 of the header comment of
mage_new_points_associate in include/mage_hot.h) that shares no code with the library.  Not a test
module (nothing is collected).

Inputs are built in fp64 and rounded to float32 once; both sides get the same arrays, and the fp64
side takes the rounded values as exact.

Fragility.  The fp64 side records, per (point, keyframe), the smallest margin to a threshold the
pair was actually tested against:

    depth      |depth| / |X - C|
    border     distance of the projection to the nearest border line, in pixels
    angle      |dot - cos| / (1 - cos)
    distance   |d2 - dMin^2| / dMin^2 and |d2 - dMax^2| / dMax^2
    octave     distance of the pre-rounding octave value from a rounding boundary, in octaves

A pair with a margin below FRAGILE may legitimately decide differently in float32 and is left out of
the verdict comparison; at most MAX_FRAGILE_SHARE of a case's pairs may be (asserted on the fp64 side
alone).

Tolerance.  px = (cs0 / depth) fx + cx with cs = R X + t: the roundings of the three-term sums move
cs0 and depth by about eps32 |X - C| each, which moves px by eps32 fx |X - C| / depth (twice over,
the second through (px - cx)); the division, the product and the sum add eps32 (|px - cx| + |px|).
The float32 projection is within K_TOL eps32 (|px - cx| + |cx| + fx |X - C| / depth) of fp64.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from mageslam_amd._lib import KP_DTYPE, NP_DTYPE
from mageslam_amd.mapping import NewMapPointsCreationSettings, NewPointsAssociationSettings
from tests.new_points_cases import _rot

EPS32 = float(np.finfo(np.float32).eps)
FRAGILE = 1e-2
MAX_FRAGILE_SHARE = 0.05
# Worst ratio of the C++ twin's projection error to eps32 (|px - cx| + |cx| + fx |X - C| / depth) over
# the committed cases, measured by test_new_points_assoc_reference.py::test_projection_within_tolerance,
# which prints it.
K_MEASURED = 0.72
K_TOL = 8.0  # eight times K_MEASURED (5.76), rounded up to a power of two

W, H, F = 1280, 720, 900.0
BORDER = 20.0
(ASSOCIATED, SAME_FRAME, BEHIND, BORDER_OUT, ANGLE, DISTANCE, OCTAVE, NO_MATCH, BAD_INDEX) = range(9)

# camera centres: the first eight are the Kc slots' (as tests/new_points_cases.py), the others further
# covisible keyframes
CENTRES = [(0.30, 0.02, 0.01), (-0.08, 0.24, 0.04), (0.03, -0.02, 0.36), (-0.33, -0.05, 0.02), (0.10, -0.30, -0.03),
           (0.27, 0.20, 0.05), (-0.22, 0.25, -0.02), (0.05, 0.38, 0.03), (0.45, -0.20, 0.10), (-0.40, 0.30, 0.15),
           (0.20, 0.45, -0.10), (-0.15, -0.45, 0.20)]


@dataclasses.dataclass
class Kf:
    pos3: np.ndarray
    r9: np.ndarray
    intr4: np.ndarray
    kp: np.ndarray      # KP_DTYPE
    desc: np.ndarray    # (n, 32) uint8
    mask: np.ndarray    # bool: unassociated when IndexedMatch ran
    slot: int           # the Kc slot this keyframe had, or -1


@dataclasses.dataclass
class Case:
    name: str
    settings: NewMapPointsCreationSettings
    assoc: NewPointsAssociationSettings
    points: np.ndarray  # NP_DTYPE
    ki_desc: np.ndarray
    kfs: list

    def args(self):
        """Positional arguments of mapping.new_points_associate."""
        return (self.settings, self.assoc, self.points, self.ki_desc, [k.pos3 for k in self.kfs],
                [k.r9 for k in self.kfs], [k.intr4 for k in self.kfs], [k.kp for k in self.kfs],
                [k.desc for k in self.kfs], [k.slot for k in self.kfs], [k.mask for k in self.kfs])


def _flip(rng, d, bits):
    d = d.copy()
    for b in rng.choice(256, bits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class Scene:
    """World points seen by Ki (near the origin, looking along +z) with their new-point records, and
    keyframes that see them."""

    def __init__(self, seed, n_points, n_slots=5, octaves=(0, 1, 2, 3), twins=0, scale=1.2, levels=8, extra_ki=20,
                 window=None, depth=(3.0, 9.0)):
        self.rng = r = np.random.default_rng(seed)
        self.scale, self.levels, self.n_slots = scale, levels, n_slots
        self.kmat = np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1.0]])
        self.intr = np.array([W / 2, H / 2, F, F], np.float32)
        self.Ri, self.Ci = _rot(*r.normal(0, 0.01, 3)), r.normal(0, 0.01, 3)
        self.slotR = [_rot(*r.normal(0, 0.03, 3)) for _ in range(n_slots)]
        self.slotC = [np.array(CENTRES[k]) + r.normal(0, 0.005, 3) for k in range(n_slots)]
        n_ki = n_points + extra_ki
        self.ki_desc = r.integers(0, 256, (n_ki, 32), dtype=np.uint8)
        ki_index = r.permutation(n_ki)[:n_points]
        x0, x1, y0, y1 = window or (60, W - 60, 60, H - 60)
        self.X, self.oi, self.slot = [], [], []
        self.twin_of = {}
        for j in range(n_points):
            if j >= n_points - twins:  # the same place as an earlier point, a descriptor one bit off, another slot
                src = int(r.integers(0, n_points - twins))
                self.twin_of[j] = src
                self.X.append(self.X[src] + r.normal(0, 1e-3, 3))
                self.oi.append(self.oi[src])
                self.slot.append((self.slot[src] + 1) % n_slots)
                self.ki_desc[ki_index[j]] = _flip(r, self.ki_desc[ki_index[src]], 1)
                continue
            pix = np.array([r.uniform(x0, x1), r.uniform(y0, y1), 1.0])
            self.X.append(self.Ci + self.Ri.T @ (r.uniform(*depth) * np.linalg.solve(self.kmat, pix)))
            self.oi.append(int(r.choice(octaves)))
            self.slot.append(int(r.integers(0, n_slots)))
        self.points = np.zeros(n_points, NP_DTYPE)
        self.dmin = np.zeros(n_points)
        for j in range(n_points):
            s = self.slot[j]
            vi, vc = self.X[j] - self.Ci, self.X[j] - self.slotC[s]
            di = np.linalg.norm(vi)
            m = vi / di + vc / np.linalg.norm(vc)
            self.dmin[j] = di * scale ** -(self.oi[j] + 0.5)
            self.points[j] = (self.X[j], m / np.linalg.norm(m), self.dmin[j], di * scale ** (levels - (self.oi[j] + 0.5)),
                              ki_index[j], s, 0, j)
        self.ki_index = ki_index
        self.kfs = []

    def keyframe(self, C, R, slot=-1, distract=150, seen=0.9, flips=3, pre_assoc=0.1, noise=0.7, same_place=0):
        """A keyframe at centre C with rotation R.  Every point it sees gets a keypoint with probability
        `seen` (always when the keyframe is the point's Kc slot: that keypoint is the point's kc_index) at
        the projection plus noise, with the predicted octave and Ki's descriptor `flips` bits off.  A twin
        shares its source's keypoint.  `same_place` extra keypoints per point sit on the same pixel with
        the same descriptor and the two neighbouring octaves.  `pre_assoc` of the keypoints were
        associated before (never a claimed one)."""
        r = self.rng
        rows, descs, owner = [], [], []
        for j in range(len(self.X)):
            own = slot >= 0 and self.slot[j] == slot
            if j in self.twin_of and not own:
                continue
            c = R @ (self.X[j] - C)
            if c[2] <= 0.1 and not own:
                continue
            z = max(c[2], 0.1)
            q = np.array([F * c[0] / z + W / 2, F * c[1] / z + H / 2])
            if not own and (not (0 <= q[0] < W and 0 <= q[1] < H) or r.uniform() > seen):
                continue
            q = np.clip(q + r.normal(0, noise, 2), 0, [W - 1, H - 1])
            val = math.log2(max(np.linalg.norm(self.X[j] - C) / self.dmin[j], 1e-6)) / math.log2(self.scale) - 0.5
            oc = int(np.clip(math.floor(val + 0.5), 0, 7))
            d = _flip(r, self.ki_desc[self.ki_index[j]], flips)
            rows.append((q[0], q[1], oc))
            descs.append(d)
            owner.append(j if own else -1)
            for e in range(same_place):
                rows.append((q[0], q[1], oc + (1 if e % 2 == 0 else -1)))
                descs.append(d)
                owner.append(-1)
        n_seen, self.last_seen = len(rows), []  # last_seen: where this keyframe's point keypoints ended up
        for _ in range(distract):
            rows.append((r.uniform(0, W), r.uniform(0, H), int(r.integers(0, 4))))
            descs.append(r.integers(0, 256, 32, dtype=np.uint8))
            owner.append(-1)
        n = len(rows)
        perm = r.permutation(n)
        kp = np.zeros(n, KP_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        mask = np.ones(n, bool)
        for new, old in enumerate(perm):
            x, y, o = rows[old]
            kp[new] = (x, y, 31.0, -1.0, 10.0, o, -1)
            desc[new] = descs[old]
            if old < n_seen:
                self.last_seen.append(new)
            if owner[old] >= 0:
                self.points["kc_index"][owner[old]] = new
            elif r.uniform() < pre_assoc:
                mask[new] = False
        t = (-(R @ C)).astype(np.float32)
        kf = Kf(t, R.T.reshape(9).astype(np.float32), self.intr, kp, desc, mask, slot)
        self.kfs.append(kf)
        return kf

    def slot_keyframes(self, **kw):
        for s in range(self.n_slots):
            self.keyframe(self.slotC[s], self.slotR[s], slot=s, **kw)

    def extra_keyframes(self, n, first=None, **kw):
        r = self.rng
        first = self.n_slots if first is None else first
        for k in range(first, first + n):
            self.keyframe(np.array(CENTRES[k]) + r.normal(0, 0.005, 3), _rot(*r.normal(0, 0.03, 3)), **kw)

    def case(self, name, assoc=None, settings=None):
        s = settings or NewMapPointsCreationSettings()
        s = dataclasses.replace(s, pyramid_scale=self.scale, num_levels=self.levels, image_width=W, image_height=H)
        return Case(name, s, assoc or NewPointsAssociationSettings(image_border=BORDER), self.points, self.ki_desc,
                    self.kfs)


def _base():
    """72 points, the 5 Kc slots and 3 further keyframes, one of them with every keypoint associated."""
    sc = Scene(41, 72, twins=8)
    sc.slot_keyframes()
    sc.extra_keyframes(3)
    sc.kfs[-1].mask[:] = False
    return sc.case("base")


def _views():
    """12 keyframes: the slots, four ordinary ones and three that the gate refuses — one behind the
    points looking on, one beside them looking across (angle), one far behind Ki (distance) — plus one
    in front of Ki, closer than dMin for the coarse octaves.  min_hamming_difference 0."""
    sc = Scene(42, 60, twins=6)
    sc.slot_keyframes()
    sc.extra_keyframes(3)
    sc.keyframe(np.array([0.0, 0.0, 14.0]), _rot(0.0, 0.02, 0.0))          # the points are behind it
    sc.keyframe(np.array([9.0, 0.0, 6.0]), _rot(0.0, math.pi / 2, 0.0))    # looks along -x
    sc.keyframe(np.array([0.1, 0.0, -40.0]), _rot(0.0, 0.0, 0.01))          # beyond dMax
    sc.keyframe(np.array([0.0, 0.05, 1.6]), _rot(0.01, 0.0, 0.0))           # within dMin for many
    return sc.case("views", NewPointsAssociationSettings(image_border=BORDER, min_hamming_difference=0))


def _contend():
    """Order matters: 30 of 70 points are twins (same place, descriptor one bit off, another slot),
    keypoints are only 2 bits from Ki's descriptor and min_hamming_difference is 3.  In a non-slot
    keyframe a point and its twins want one keypoint; in the source's slot keyframe the only keypoint
    at the twin's place is the one CreateInitialAssociations claimed."""
    sc = Scene(43, 70, twins=30, n_slots=3)
    sc.slot_keyframes(flips=2, pre_assoc=0.15)
    sc.extra_keyframes(2, flips=2, pre_assoc=0.15)
    return sc.case("contend", NewPointsAssociationSettings(image_border=BORDER, min_hamming_difference=3))


def _octaves3():
    """Ki octaves 0..2 and, at every keypoint of a seen point, two more keypoints with the same pixel
    and descriptor in the neighbouring octaves: only the octave tells them apart."""
    sc = Scene(44, 48, octaves=(0, 1, 2), n_slots=2)
    sc.slot_keyframes(same_place=2)
    sc.extra_keyframes(2, same_place=2)
    return sc.case("octaves3")


def _levels4():
    """num_levels 4 with points whose dMax was made for 8 levels: a keyframe far behind Ki predicts
    octaves 5 and more (OCTAVE); the test is octave > numLevels, so octave 4 still searches."""
    sc = Scene(45, 40, n_slots=2)
    sc.slot_keyframes()
    for z in (-2.0, -6.0, -10.0, -14.0):
        sc.keyframe(np.array([0.05, 0.02, z]), _rot(0.0, 0.0, 0.02))
    c = sc.case("levels4")
    c.settings = dataclasses.replace(c.settings, num_levels=4)
    return c


def _count(n, name, seed):
    """n points against one keyframe (the chunk and workgroup boundaries of the kernel)."""
    sc = Scene(seed, n, n_slots=1, twins=n // 8)
    sc.extra_keyframes(1, first=5, distract=100)
    return sc.case(name)


def _blob(size, name):
    """100 points projecting into one search box of a keyframe that has `size` near-identical keypoints
    there, and chains of conflicts (min_hamming_difference 0, so that a point with any candidate takes
    one).  40: more candidates than any per-point capacity; 8 and 9: the kernel's kept list of 8
    exactly full, and its first overflow."""
    sc = Scene(49, 100, n_slots=1, octaves=(1,), window=(636, 644, 356, 364), depth=(6.0, 6.05))
    base = sc.ki_desc[sc.ki_index[0]]
    for j in range(100):
        sc.ki_desc[sc.ki_index[j]] = _flip(sc.rng, base, int(sc.rng.integers(0, 4)))
    r = sc.rng
    C, R = np.array(CENTRES[6]), _rot(0.0, 0.0, 0.01)
    kf = sc.keyframe(C, R, distract=60, seen=0.0)
    c = R @ (np.mean(sc.X, axis=0) - C)
    q = np.array([F * c[0] / c[2] + W / 2, F * c[1] / c[2] + H / 2])
    # the predicted octave of the blob's points in this keyframe
    val = math.log2(np.linalg.norm(np.mean(sc.X, axis=0) - C) / np.mean(sc.dmin)) / math.log2(sc.scale) - 0.5
    idx = r.choice(len(kf.kp), size, replace=False)
    for t in idx:
        kf.kp[t] = (q[0] + r.uniform(-4, 4), q[1] + r.uniform(-4, 4), 31.0, -1.0, 10.0, int(math.floor(val + 0.5)), -1)
        kf.desc[t] = _flip(r, base, int(r.integers(0, 5)))
        kf.mask[t] = True
    return sc.case(name, NewPointsAssociationSettings(image_border=BORDER, min_hamming_difference=0))


def _many_kp(n_kp, name):
    """A keyframe of n_kp keypoints between two ordinary ones."""
    sc = Scene(50, 40, n_slots=1)
    sc.slot_keyframes()
    kf = sc.keyframe(np.array(CENTRES[5]), _rot(0.0, 0.01, 0.0))
    r, more = sc.rng, n_kp - len(kf.kp)
    kp = np.zeros(more, KP_DTYPE)
    for i in range(more):
        kp[i] = (r.uniform(0, W), r.uniform(0, H), 31.0, -1.0, 10.0, int(r.integers(0, 4)), -1)
    kf.kp = np.concatenate([kf.kp, kp])
    kf.desc = np.concatenate([kf.desc, r.integers(0, 256, (more, 32), dtype=np.uint8)])
    kf.mask = np.concatenate([kf.mask, np.ones(more, bool)])
    # the last keypoint is one a point wants
    t, last = sc.last_seen[0], n_kp - 1
    for a in (kf.kp, kf.desc, kf.mask):
        a[[t, last]] = a[[last, t]]
    kf.mask[last] = True
    sc.extra_keyframes(1, first=6)
    return sc.case(name)


def _bad_index():
    sc = Scene(51, 30, n_slots=3)
    sc.slot_keyframes()
    sc.extra_keyframes(1)
    c = sc.case("bad_index")
    c.points = c.points.copy()
    c.points["ki_index"][4] = len(c.ki_desc)
    c.points["ki_index"][11] = 2 ** 32 - 1
    c.points["kc_slot"][7] = 8
    c.points["kc_slot"][19] = 2 ** 31
    c.points["kc_index"][23] = len(c.kfs[int(c.points["kc_slot"][23])].kp)
    return c


def _empty():
    sc = Scene(52, 0, n_slots=2)
    sc.slot_keyframes()
    return sc.case("empty")


def _no_keyframes():
    sc = Scene(53, 12, n_slots=2)
    sc.slot_keyframes()
    c = sc.case("no_keyframes")
    c.kfs = []
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order."""
    out = [_base(), _views(), _contend(), _octaves3(), _levels4(), _empty(), _no_keyframes(), _count(1, "n1", 46),
           _count(64, "n64", 47), _count(65, "n65", 48), _count(257, "n257", 54), _blob(40, "blob"), _blob(8, "blob8"),
           _blob(9, "blob9"), _many_kp(4096, "kp4096"), _many_kp(4097, "kp4097"), _bad_index()]
    return {c.name: c for c in out}


BATCH_CASES = ("base", "contend", "empty", "n257", "no_keyframes")


# ------------------------------------------------------------------------------------------
# the fp64 formulation of steps 1-4
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Reference:
    verdict: np.ndarray   # (n, n_kf) int; NO_MATCH stands for "goes on to the descriptor search"; -1 untouched
    margin: np.ndarray    # (n, n_kf) smallest margin met (inf where nothing was tested)
    x: np.ndarray         # (n, n_kf) fp64 projection (nan where not projected)
    y: np.ndarray
    xscale: np.ndarray    # (n, n_kf) |px - cx| + |cx| + fx |X - C| / |depth|, the unit of the tolerance
    yscale: np.ndarray
    octave: np.ndarray    # (n, n_kf) predicted octave where computed, else 0
    status: int
    share: float          # pairs left out of the verdict comparison


@functools.lru_cache(maxsize=None)
def reference(name) -> Reference:
    c = cases()[name]
    n, nk = len(c.points), len(c.kfs)
    ref = Reference(np.full((n, nk), -1), np.full((n, nk), np.inf), np.full((n, nk), np.nan), np.full((n, nk), np.nan),
                    np.zeros((n, nk)), np.zeros((n, nk)), np.zeros((n, nk), int), 0, 0.0)
    scale = float(np.float32(c.settings.pyramid_scale))
    levels = c.settings.num_levels
    border = float(np.float32(c.assoc.image_border)) - float(np.float32(c.assoc.search_radius)) / 2.0
    cosmax = math.cos(math.radians(float(np.float32(c.assoc.max_keyframe_angle_degrees))))
    iw, ih = float(c.settings.image_width), float(c.settings.image_height)
    for k, kf in enumerate(c.kfs):
        if len(kf.kp) > 4096:
            ref.status |= 1
            continue
        R = np.asarray(kf.r9, np.float64).reshape(3, 3).T  # r9 is column-major
        t = np.asarray(kf.pos3, np.float64)
        C = -(R.T @ t)
        cx, cy, fx, fy = (float(v) for v in kf.intr4)
        for p, pt in enumerate(c.points):
            if int(pt["ki_index"]) >= len(c.ki_desc) or int(pt["kc_slot"]) >= 8:
                ref.verdict[p, k] = BAD_INDEX
                continue
            if kf.slot >= 0 and int(pt["kc_slot"]) == kf.slot:
                ref.verdict[p, k] = SAME_FRAME if int(pt["kc_index"]) < len(kf.kp) else BAD_INDEX
                continue
            X = np.asarray(pt["position"], np.float64)
            cs = R @ X + t
            depth = cs[2]
            div = depth if depth != 0 else 1.0
            px, py = cs[0] / div * fx + cx, cs[1] / div * fy + cy
            dist = float(np.linalg.norm(X - C))
            ref.x[p, k], ref.y[p, k] = px, py
            ref.xscale[p, k] = abs(px - cx) + abs(cx) + fx * dist / abs(div)
            ref.yscale[p, k] = abs(py - cy) + abs(cy) + fy * dist / abs(div)
            margin = abs(depth) / dist
            ref.margin[p, k] = margin
            if depth < 0:
                ref.verdict[p, k] = BEHIND
                continue
            margin = min(margin, abs(px - border), abs(py - border), abs(iw - border - px), abs(ih - border - py))
            ref.margin[p, k] = margin
            if not (border <= px and border <= py and px < iw - border and py < ih - border):
                ref.verdict[p, k] = BORDER_OUT
                continue
            dot = float(np.asarray(pt["mean_view_dir"], np.float64) @ R[2])
            margin = min(margin, abs(dot - cosmax) / (1.0 - cosmax))
            ref.margin[p, k] = margin
            if dot < cosmax:
                ref.verdict[p, k] = ANGLE
                continue
            d2 = float((X - C) @ (X - C))
            dmin, dmax = float(pt["d_min"]), float(pt["d_max"])
            margin = min(margin, abs(d2 - dmin * dmin) / (dmin * dmin), abs(d2 - dmax * dmax) / (dmax * dmax))
            ref.margin[p, k] = margin
            if d2 < dmin * dmin or dmax * dmax < d2:
                ref.verdict[p, k] = DISTANCE
                continue
            val = math.log2(math.sqrt(d2) / dmin) / math.log2(scale) - 0.5
            frac = (val - 0.5) % 1.0  # roundf's boundaries are the half-integers
            ref.margin[p, k] = min(margin, frac, 1.0 - frac)
            pred = int(math.floor(abs(val) + 0.5)) * (1 if val >= 0 else -1)  # roundf: halves away from zero
            ref.octave[p, k] = pred
            ref.verdict[p, k] = OCTAVE if pred < 0 or pred > levels else NO_MATCH
    ref.share = float((ref.margin < FRAGILE).sum()) / max(n * nk, 1)
    return ref


def start_mask(c: Case, k: int) -> np.ndarray:
    """Keyframe k's unassociated mask with CreateInitialAssociations' claims cleared (uint8)."""
    kf = c.kfs[k]
    m = kf.mask.astype(np.uint8)
    if kf.slot >= 0:
        for pt in c.points:
            if int(pt["kc_slot"]) == kf.slot and int(pt["kc_index"]) < len(m):
                m[int(pt["kc_index"])] = 0
    return m


def start_candidates(c: Case, rec, v, k: int) -> np.ndarray:
    """Per point that went on to keyframe k's descriptor search, the keypoints it can be offered under
    the starting mask, from the records' (x, y, octave): inside the float32 box, the predicted octave,
    unassociated, Hamming distance <= max_hamming_distance."""
    kf = c.kfs[k]
    passed = np.nonzero(np.isin(v[:, k], [ASSOCIATED, NO_MATCH]))[0]
    r = np.float32(c.assoc.search_radius)
    px, py = rec["x"][passed, k][:, None], rec["y"][passed, k][:, None]
    x, y = kf.kp["x"][None], kf.kp["y"][None]
    box = (x >= px - r) & (x <= px + r) & (y >= py - r) & (y <= py + r)
    qd = c.ki_desc[c.points["ki_index"][passed].astype(np.int64)].reshape(-1, 32)
    d = np.unpackbits(qd[:, None] ^ kf.desc[None], axis=2).sum(2)
    return (box & (kf.kp["octave"][None] == rec["octave"][passed, k][:, None]) & (start_mask(c, k) != 0)[None] &
            (d <= c.assoc.max_hamming_distance)).sum(1)


def composition_scene():
    """The `taken` scene of tests/new_points_cases.py (Ki keypoints matched from three Kc and from two)
    as mapping.Keyframe objects with descriptors: a matched Kc keypoint carries Ki's descriptor three
    bits off, a tenth of the others were associated before.  max_frames = 2, so the farthest keyframe
    makes no points.  -> (ki, covisible, matcher, settings, association settings)."""
    from mageslam_amd import mapping
    from tests import new_points_cases as nc

    p = nc.cases()["taken"]
    rng = np.random.default_rng(7)
    n_ki = len(p.ki_kp)
    ki_desc = rng.integers(0, 256, (n_ki, 32), dtype=np.uint8)
    ki = mapping.Keyframe(p.ki_pos3, p.ki_r9, p.ki_intr4, p.ki_kp, ki_desc, np.zeros(n_ki, bool))
    cov, match_of = [], {}
    for k in [2, 0, 1]:
        kp = p.kc_kp[k]
        d = rng.integers(0, 256, (len(kp), 32), dtype=np.uint8)
        for m in p.matches[k]:
            d[m["query_idx"]] = _flip(rng, ki_desc[m["train_idx"]], 3)
        assoc = rng.uniform(size=len(kp)) < 0.1
        assoc[p.matches[k]["query_idx"]] = False
        kf = mapping.Keyframe(p.kc_pos3[k], p.kc_r9[k], p.kc_intr4[k], kp, d, assoc)
        cov.append(kf)
        match_of[id(kf)] = p.matches[k]

    def matcher(kc, ki_, kc_mask, ki_mask):
        return match_of[id(kc)]

    s = dataclasses.replace(p.settings, max_frames=2, max_grid_count=30)
    return ki, cov, matcher, s, NewPointsAssociationSettings(image_border=BORDER)
