"""Synthetic two-view scenes for the monocular map initialisation tests (test_mono_init_reference.py,
test_gpu_mono_init.py, test_mono_init_sanitize.py) and the independent fp64 formulations the twin is
compared with.  640 x 480, f = 500; frame-0 keypoints are integers, the 3-D point is the
back-projection of that pixel, so a clean scene is exact up to frame 1's float32 rounding.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from mageslam_amd import mono
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE

W, H, F = 640, 480, 500.0
INTR = np.array([W / 2, H / 2, F, F] * 2, np.float32)
EPS32 = float(np.finfo(np.float32).eps)
FRAGILE = 1e-2            # relative distance from a threshold within which a decision is not compared
MAX_FRAGILE_SHARE = 0.05  # of the hypotheses (or matches) of a case

# Measured by test_mono_init_reference.py over the cases below (the tests print the figures):
#   K_MEASURED_E     worst residual ratio of a traced E: the largest of the five epipolar constraints, det E
#                    and the trace constraint (E has unit Frobenius norm) over eps32 times the hypothesis's
#                    amplification (five_point_fp64: the float32 elimination's condition number times the
#                    largest root magnitude);
#   K_MEASURED_ROOT  worst distance of an fp64 solution from the nearest traced E (up to sign), same units;
#   K_MEASURED_SUM   worst |traced score - fp64 score| / (eps32 * sum of (|terms| + their rounding bound));
#   ANGLE_MEASURED   worst angle (degrees) of the selected rotation / translation direction from the truth
#                    over the clean cases.
# The tolerances are small multiples of them (the convention of stereo_init_cases.py).
K_MEASURED_E = 193.0     # outliers128
K_MEASURED_ROOT = 115.0  # clean128
K_MEASURED_SUM = 326.0   # clean2000: 4000 terms summed in order in float32
ANGLE_MEASURED = 0.0093  # clean2000's rotation
K_TOL_E = 4 * K_MEASURED_E
K_TOL_ROOT = 4 * K_MEASURED_ROOT
K_TOL_SUM = 4 * K_MEASURED_SUM
ANGLE_TOL = 2 * ANGLE_MEASURED


@dataclasses.dataclass
class Case:
    name: str
    settings: mono.MonoMapInitializationSettings
    kp0: np.ndarray
    kp1: np.ndarray
    matches: np.ndarray | None
    expect: int | None               # the verdict, or None where the outcome is free
    expect_status: int = 0
    R: np.ndarray | None = None      # the true view rotation of frame 1
    t: np.ndarray | None = None      # its view-space translation (any scale)
    clean: bool = False              # every match is an exact correspondence
    desc0: np.ndarray | None = None  # with descriptors: the matcher chain
    desc1: np.ndarray | None = None


def rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return rz @ rx @ ry


def keypoints(xy, octave=0):
    kp = np.zeros(len(xy), KP_DTYPE)
    kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    kp["size"], kp["angle"], kp["octave"] = 31.0, -1.0, octave
    return kp


def scene(seed, n, R, t, box=None, depth=(4.0, 8.0), noise=0.0, outliers=0):
    """n correspondences: integer pixels in frame 0 (inside `box` = x0, y0, x1, y1), their depths,
    the projection into frame 1 = R X + t.  `outliers` of them get a random frame-1 pixel."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = box or (20, 20, W - 20, H - 20)
    # distinct pixels
    cells = rng.permutation((x1 - x0) * (y1 - y0))[:n]
    px = np.stack([x0 + cells % (x1 - x0), y0 + cells // (x1 - x0)], 1).astype(np.float64)
    z = rng.uniform(depth[0], depth[1], n)
    X = np.stack([(px[:, 0] - W / 2) / F * z, (px[:, 1] - H / 2) / F * z, z], 1)
    Y = X @ np.asarray(R).T + np.asarray(t)
    q = np.stack([Y[:, 0] / Y[:, 2] * F + W / 2, Y[:, 1] / Y[:, 2] * F + H / 2], 1)
    if noise:
        q = q + rng.normal(0, noise, q.shape)
    if outliers:
        bad = rng.permutation(n)[:outliers]
        q[bad] = rng.uniform((0, 0), (W, H), (outliers, 2))
    return px.astype(np.float32), q.astype(np.float32)


def identity_matches(n, perm=None):
    m = np.zeros(n, DM_DTYPE)
    m["query_idx"] = np.arange(n)
    m["train_idx"] = np.arange(n) if perm is None else perm
    m["distance"] = (np.arange(n) % 17).astype(np.float32)
    return m


def _case(name, seed, n, R, t, expect, settings=None, clean=False, shuffle=True, **kw):
    p, q = scene(seed, n, R, t, **kw)
    # frame 1's keypoints in another order, so that query and train indices differ
    perm = np.random.default_rng(seed + 1000).permutation(n) if shuffle else np.arange(n)
    kp1 = np.zeros(n, np.float32).reshape(-1, 1).repeat(2, 1)
    kp1[perm] = q
    return Case(name, settings or mono.MonoMapInitializationSettings(), keypoints(p), keypoints(kp1),
                identity_matches(n, perm), expect, R=np.asarray(R, np.float64), t=np.asarray(t, np.float64), clean=clean)


SIDEWAYS_R = rot(np.deg2rad(2.0), np.deg2rad(-1.0), np.deg2rad(0.5))
SIDEWAYS_T = np.array([-1.0, 0.05, 0.1])


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    S = mono.MonoMapInitializationSettings
    out = [
        _case("clean64", 11, 64, SIDEWAYS_R, SIDEWAYS_T, mono.OK, S(min_feature_matches=60), clean=True),
        _case("clean128", 12, 128, SIDEWAYS_R, SIDEWAYS_T, mono.OK, clean=True),
        _case("clean300", 13, 300, SIDEWAYS_R, SIDEWAYS_T, mono.OK, clean=True),
        _case("noise128", 14, 128, SIDEWAYS_R, SIDEWAYS_T, mono.OK, noise=0.3),
        _case("outliers128", 15, 128, SIDEWAYS_R, SIDEWAYS_T, mono.OK, outliers=32),
        _case("clean2000", 16, 2000, SIDEWAYS_R, SIDEWAYS_T, mono.OK, clean=True),
        # every pair of points is closer than MinPixelSpread: no sample can be drawn
        _case("clustered", 17, 128, SIDEWAYS_R, SIDEWAYS_T, mono.NO_HYPOTHESIS, box=(300, 220, 325, 245)),
        # repeated draws are no-op inserts
        _case("eight", 18, 8, SIDEWAYS_R, SIDEWAYS_T, None,
              S(min_pixel_spread=0.0, min_feature_matches=5, min_scoring_inliers=5), clean=True),
        _case("few40", 19, 40, SIDEWAYS_R, SIDEWAYS_T, mono.FEW_MATCHES),
        # mostly forward: |C.z| = 0.91 of the baseline.  (Purely forward motion is the five-point
        # problem's near-tangent configuration: at every seed tried a few hypotheses of 90 have a pair of
        # real fp64 solutions that the float32 elimination merges into a complex pair.)
        _case("forward", 25, 128, rot(np.deg2rad(0.5), 0.0, 0.0), np.array([0.4, 0.2, -1.0]), mono.Z_BIASED,
              clean=True),
        # the baseline is 1/40 of the median depth: the median normalised depth exceeds 20.  The motion
        # is vertical, so that the half-turn about the baseline flips the right vector and both twisted
        # poses are skipped (a half-turn about a sideways baseline keeps it, and that pose can pass).
        _case("tiny_baseline", 21, 128, SIDEWAYS_R, 0.15 * np.array([0.05, -1.0, 0.1]), mono.NO_VALID_POSE, clean=True),
        _case("pure_rotation", 22, 128, rot(np.deg2rad(3.0), np.deg2rad(1.0), 0.0), np.zeros(3), None),
    ]
    return tuple(out)


def case(name) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def over_limit_case() -> Case:
    """One pair with more than 4096 keypoints in frame 0."""
    c = case("clean64")
    kp0 = np.concatenate([c.kp0, keypoints(np.zeros((4097 - len(c.kp0), 2), np.float32))])
    return Case("over_limit", c.settings, kp0, c.kp1, c.matches, mono.OK, expect_status=mono.STATUS_OVER_LIMIT)


@functools.lru_cache(maxsize=None)
def matcher_case() -> Case:
    """Mixed octaves with descriptors: the clean128 scene's keypoints at octave 0 with random
    descriptors shared by the two frames (frame 1's with a few bits flipped), interleaved with
    higher-octave keypoints that carry the SAME descriptors as an octave-0 keypoint — they would
    match if the masks let them through."""
    c = case("clean128")
    rng = np.random.default_rng(77)
    n = len(c.kp0)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    inv = np.argsort(c.matches["train_idx"])  # frame-1 keypoint -> frame-0 keypoint

    def build(kp, desc, seed):
        r = np.random.default_rng(seed)
        extra = keypoints(r.uniform((0, 0), (W, H), (n // 2, 2)).astype(np.float32), octave=1)
        extra["octave"] = r.integers(1, 4, len(extra))
        kk = np.concatenate([kp, extra])
        dd = np.concatenate([desc, desc[: len(extra)]])
        order = r.permutation(len(kk))
        return kk[order], np.ascontiguousarray(dd[order])

    d1 = d[inv].copy()
    flips = rng.integers(0, 256, (n, 3))
    for i in range(n):
        for b in flips[i]:
            d1[i, b // 8] ^= np.uint8(1 << (b % 8))
    kp0, desc0 = build(c.kp0, d, 78)
    kp1, desc1 = build(c.kp1, d1, 79)
    return Case("matcher", c.settings, kp0, kp1, None, mono.OK, R=c.R, t=c.t, clean=True, desc0=desc0, desc1=desc1)


def octave0_masks(c: Case):
    return c.kp0["octave"] == 0, c.kp1["octave"] == 0


def match_points(c: Case, matches=None):
    m = c.matches if matches is None else matches
    a, b = c.kp0[m["query_idx"]], c.kp1[m["train_idx"]]
    return (np.stack([a["x"], a["y"]], 1).astype(np.float32), np.stack([b["x"], b["y"]], 1).astype(np.float32))


# ------------------------------------------------------------------------------------------
# Independent formulations
# ------------------------------------------------------------------------------------------
class CvRng:
    """OpenCV 3.4.0's cv::RNG: multiply-with-carry, uniform(a, b) = a + next() % (b - a)."""

    def __init__(self, seed):
        self.state = seed or 0xFFFFFFFF

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else a + self.next() % (b - a)


def sample_reference(p0, p1, iterations, min_pixel_spread):
    """FindPossiblePoses' sampling loop (MapInitialization.cpp:196-249) on a Python set: integers
    and float32 compares.  (iterations, 5) indices, ascending, or -1."""
    f = np.float32
    rng = CvRng(12345)
    min_sq = f(min_pixel_spread) * f(min_pixel_spread)
    out = np.full((iterations, 5), -1, np.int32)
    n = len(p0)
    for it in range(iterations):
        chosen = set()
        tries = 0
        while len(chosen) < 5 and tries < 100:
            tries += 1
            c = rng.uniform(0, n)
            close = False
            for v in chosen:
                d0, d1 = p0[v] - p0[c], p1[v] - p1[c]
                close = close or bool(f(d0[0] * d0[0]) + f(d0[1] * d0[1]) < min_sq) \
                    or bool(f(d1[0] * d1[0]) + f(d1[1] * d1[1]) < min_sq)
            if not close:
                chosen.add(c)
        if len(chosen) == 5:
            out[it] = sorted(chosen)
    return out


def normalise(p, intr4):
    """(p - pp) / f in fp64 with frame 0's calibration, as FindEssentialMat does for both frames."""
    p = np.asarray(p, np.float64)
    return np.stack([(p[:, 0] - float(intr4[0])) / float(intr4[2]), (p[:, 1] - float(intr4[1])) / float(intr4[3])], 1)


def essential_residual(E, q1, q2):
    """The largest of: the five epipolar constraints q2^T E q1, det E, and the entries of
    2 E E^T E - tr(E E^T) E, for E of unit Frobenius norm, in fp64."""
    E = np.asarray(E, np.float64)
    h1, h2 = np.c_[q1, np.ones(len(q1))], np.c_[q2, np.ones(len(q2))]
    epi = np.abs(np.einsum("ni,ij,nj->n", h2, E, h1)).max()
    EEt = E @ E.T
    tr = np.abs(2 * EEt @ E - np.trace(EEt) * E).max()
    return max(epi, abs(np.linalg.det(E)), tr)


def five_point_fp64(q1, q2):
    """An fp64 five-point solve by another route: the null space from numpy's SVD, the ten cubic
    constraints sampled and fitted (no symbolic expansion), the action matrix's eigenvalues.
    constraints sampled at random (x, y, z) and fitted (no symbolic expansion), a float64
    elimination, det B(z) fitted at Chebyshev nodes, numpy's roots and SVD null vectors.  Returns
    (solutions (k, 3, 3) of unit Frobenius norm for the real roots, all roots, all ten solutions as
    complex unit 9-vectors, the error amplification of the float32 stages: the condition number of the
    eliminated 10 x 10 block times the largest root magnitude, at least 1 — B(z) is evaluated in
    float32 at the root)."""
    h1, h2 = np.c_[q1, np.ones(5)], np.c_[q2, np.ones(5)]
    Q = np.stack([np.outer(h2[i], h1[i]).ravel() for i in range(5)])
    basis = np.linalg.svd(Q)[2][5:9]  # X, Y, Z, W
    mono_exp = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1),
                (1, 1, 0), (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2),
                (0, 0, 1), (0, 0, 0)]
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-1, 1, (60, 3))
    V = np.stack([[x ** a * y ** b * z ** c for a, b, c in mono_exp] for x, y, z in xyz])
    vals = []
    for x, y, z in xyz:
        E = (x * basis[0] + y * basis[1] + z * basis[2] + basis[3]).reshape(3, 3)
        EEt = E @ E.T
        vals.append(np.r_[(2 * EEt @ E - np.trace(EEt) * E).ravel(), np.linalg.det(E)])
    A = np.linalg.lstsq(V, np.asarray(vals), rcond=None)[0].T  # 10 x 20
    A2 = np.linalg.solve(A[:, :10], A[:, 10:])
    amplification = float(np.linalg.cond(A[:, :10]))
    # m_l = -A2 m_r: rows 4..9 pairwise give B(z) [x y 1]^T = 0; its determinant by sampling and fitting
    def Bz(z):
        rows = []
        for i in range(3):
            r4, r5 = A2[4 + 2 * i], A2[5 + 2 * i]
            px = np.polyval([-r5[0], r4[0] - r5[1], r4[1] - r5[2], r4[2]], z)
            py = np.polyval([-r5[3], r4[3] - r5[4], r4[4] - r5[5], r4[5]], z)
            pw = np.polyval([-r5[6], r4[6] - r5[7], r4[7] - r5[8], r4[8] - r5[9], r4[9]], z)
            rows.append([px, py, pw])
        return np.array(rows)
    zs = np.cos(np.pi * (np.arange(11) + 0.5) / 11) * 2.0
    coeff = np.polyfit(zs, [np.linalg.det(Bz(z)) for z in zs], 10)
    roots = np.roots(coeff)
    sols, every = [], []
    for z in roots:
        v = np.linalg.svd(Bz(z))[2][-1].conj()
        Ec = v[0] * basis[0] + v[1] * basis[1] + v[2] * (z * basis[2] + basis[3])
        every.append(Ec / np.linalg.norm(Ec))
        if abs(z.imag) > 1e-6 or abs(v[2]) < 1e-10:
            continue
        E = (v[0] / v[2]).real * basis[0] + (v[1] / v[2]).real * basis[1] + z.real * basis[2] + basis[3]
        sols.append((E / np.linalg.norm(E)).reshape(3, 3))
    amplification *= max(1.0, float(np.abs(roots).max()))
    return np.asarray(sols).reshape(-1, 3, 3), roots, np.asarray(every), amplification


def fragile_hypothesis(roots, every, cut=1e-6, rel=FRAGILE):
    """A hypothesis is fragile when a root's |im| is within `rel` (relative) of the cut, or two of
    its ten (complex) solutions are closer than `rel`.  The roots are coordinates in a basis of the
    null space, which the twin and this formulation choose differently, so closeness is taken
    between the solutions themselves: unit 9-vectors up to a complex factor."""
    for z in roots:
        if abs(abs(z.imag) - cut) <= rel * cut:
            return True
    for i in range(len(every)):
        for j in range(i + 1, len(every)):
            if np.sqrt(max(0.0, 1.0 - abs(np.vdot(every[i], every[j])) ** 2)) <= rel:
                return True
    return False


def kinv(intr4):
    cx, cy, fx, fy = (float(v) for v in intr4)
    return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])


def score_fp64(E, p0, p1, intr8, threshold):
    """ScoreFundamentalMatrix (:279-322) in fp64: (inlier mask, margin to the threshold per match
    relative to it, the two terms per match, a first-order bound per match of what float32 rounding
    of the line and of its product with the point does to the two squared distances, in units of
    eps32: 2 |num| (|A x| + |B y| + |C|) / (A^2 + B^2) each way)."""
    F12 = kinv(intr8[4:]).T @ np.asarray(E, np.float64) @ kinv(intr8[:4])
    h0, h1 = np.c_[p0, np.ones(len(p0))].astype(np.float64), np.c_[p1, np.ones(len(p1))].astype(np.float64)
    l12, l21 = h0 @ F12.T, h1 @ F12
    n12, n21 = (l12 * h1).sum(1), (l21 * h0).sum(1)
    den12, den21 = l12[:, 0] ** 2 + l12[:, 1] ** 2, l21[:, 0] ** 2 + l21[:, 1] ** 2
    d12, d21 = n12 ** 2 / den12, n21 ** 2 / den21
    # the line's entries are themselves float32 sums of three products: their rounding, carried to num
    mag12 = np.abs(F12) @ np.abs(h0).T  # |F| |m| per line entry, (3, n)
    mag21 = np.abs(F12.T) @ np.abs(h1).T
    s12 = 2 * np.abs(n12) * 4 * (mag12 * np.abs(h1).T).sum(0) / den12 + 4 * d12 * (np.abs(l12[:, :2]) * mag12[:2].T).sum(1) / den12
    s21 = 2 * np.abs(n21) * 4 * (mag21 * np.abs(h0).T).sum(0) / den21 + 4 * d21 * (np.abs(l21[:, :2]) * mag21[:2].T).sum(1) / den21
    inl = (d12 < threshold) & (d21 < threshold)
    margin = np.minimum(np.abs(d12 - threshold), np.abs(d21 - threshold)) / threshold
    return inl, margin, threshold - d12, threshold - d21, s12 + s21


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    c = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))
