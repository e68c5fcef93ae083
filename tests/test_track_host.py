"""The tracker's shared host code without a GPU: csrc/track_math.hpp against tracking.py bit for
bit (on branches the synthetic sequences do not reach), csrc/track_window.hpp's build_window /
apply_window against tracking.build_ba_window / apply_ba_window on the rings of test_local_ba.py,
and csrc/track_bufs.hpp's block table.  tests/cpp/track_host_check.cpp is built with g++."""
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import tracking
from mageslam_amd._lib import KP_DTYPE
from tests.test_local_ba import _covis_ring, _kf, _structure_ring

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "track_host_check.cpp"
CSRC = ROOT / "mageslam_amd" / "csrc"
K0 = (900.0, 900.0, 640.0, 360.0)


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "mageslam_amd" / "_lib" / "track_host_check"
    out.parent.mkdir(parents=True, exist_ok=True)
    deps = [SRC, ROOT / "include" / "mage_hot.h", *CSRC.glob("*.hpp")]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out)], check=True)
    return out


def _run(exe, tmp_path, mode, parts):
    fin, fout = tmp_path / f"{mode}.in", tmp_path / f"{mode}.out"
    fin.write_bytes(b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts))
    r = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return _Reader(fout.read_bytes())


class _Reader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, dtype, n=1):
        dt = np.dtype(dtype)
        a = np.frombuffer(self.data, dt, n, self.at)
        self.at += n * dt.itemsize
        return a

    def done(self):
        return self.at == len(self.data)


def _const(s, K, plane_z=5.0):
    return [bytes(tracking._settings_c(s)), np.float64(K), np.float64([plane_z])]


def _pose12(p):
    return np.concatenate([np.asarray(p.R, np.float64).reshape(9), np.asarray(p.t, np.float64)])


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _keyframe(pose, pts, octv, mvd, dmin, dmax):
    m = len(pts)
    kp = np.zeros(m, KP_DTYPE)
    kp["octave"] = octv
    return tracking.Keyframe(pose, kp, np.zeros((m, 32), np.uint8), np.array(pts, np.float32), 7,
                             np.array(mvd, np.float32), np.array(dmin, np.float32), np.array(dmax, np.float32))


def _math(exe, tmp_path, s, K, kf_pose, q_pose, kp, cand):
    """Runs the program and tracking.py on one scene; returns what both gave for the candidates:
    (native keep mask, native octaves, tracking's kept indices)."""
    cpts, coct, cmvd, cdmin, cdmax = cand
    m, n, fid = len(cpts), len(kp), 7
    prev = tracking.Pose(_rot([1, 2, 3], 0.3), np.array([0.3, -0.2, 0.1]))
    prev2 = tracking.Pose(_rot([3, -1, 2], 0.25), np.array([0.25, -0.22, 0.14]))
    r = _run(exe, tmp_path, "math",
             _const(s, K) + [_pose12(kf_pose), _pose12(q_pose), _pose12(prev), _pose12(prev2), np.uint32([fid, n]), kp,
                             np.uint32([m]), np.float32(cpts), np.int32(coct), np.float32(cmvd), np.float32(cdmin),
                             np.float32(cdmax)])
    # tracking.make_keyframe, then tracking.point_attributes of the given points under the same pose
    kf = tracking.make_keyframe(fid, kf_pose, kp, np.zeros((n, 32), np.uint8), K, 5.0, s)
    assert _same(r.take(np.float32, 3 * n).reshape(n, 3), kf.points)
    assert _same(r.take(np.float32, 3 * n).reshape(n, 3), kf.mvd)
    assert _same(r.take(np.float32, n), kf.dmin) and _same(r.take(np.float32, n), kf.dmax)
    ka = _keyframe(kf_pose, cpts, coct, np.zeros((m, 3)), np.zeros(m), np.zeros(m))
    tracking.point_attributes(ka, s, np.arange(m))
    assert _same(r.take(np.float32, 3 * m).reshape(m, 3), ka.mvd)
    assert _same(r.take(np.float32, m), ka.dmin) and _same(r.take(np.float32, m), ka.dmax)
    # tracking.project: the positions of the points in front
    pos, front = tracking.project(np.float32(cpts), q_pose, K)
    nfront, nuv = r.take(np.uint8, m).astype(bool), r.take(np.float32, 2 * m).reshape(m, 2)
    assert np.array_equal(nfront, front) and _same(nuv[front], pos[front])
    # tracking.local_map_queries
    kq = _keyframe(q_pose, cpts, coct, cmvd, cdmin, cdmax)
    lp, lo, _, _, src = tracking.local_map_queries([kq], None, None, None, q_pose, K, s)
    keep = src[0][1]
    ok, pxy, octv = r.take(np.uint8, m).astype(bool), r.take(np.float32, 2 * m).reshape(m, 2), r.take(np.int32, m)
    assert np.array_equal(np.nonzero(ok)[0], keep)
    assert _same(pxy[keep], lp) and _same(octv[keep], lo.astype(np.int32))
    # the motion model P[f-1] * P[f-2]^-1 * P[f-1] and MapPointRefinementConfidence(0..5)
    assert _same(r.take(np.float64, 12), _pose12((prev * prev2.inverse()) * prev))
    assert _same(r.take(np.float32, 6), tracking.refinement_confidence(np.arange(6)))
    assert r.done()
    return ok, octv, keep, kf


def _keypoints(n):
    rng = np.random.default_rng(11)
    kp = np.zeros(n, KP_DTYPE)
    kp["x"], kp["y"] = rng.uniform(0, 1280, n), rng.uniform(0, 720, n)
    kp["octave"] = rng.integers(0, 8, n)
    kp["octave"][:2] = [-1, 9]  # clamped to the factor tables' 0..7
    return kp


@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_arithmetic_general_pose(exe, tmp_path, sigma):
    """64 points of a keyframe under a rotated, translated pose (every sum rounds), seen again from a
    nearby pose; plus a point at the keyframe's centre (d == 0: no normalisation)."""
    s = tracking.TrackerSettings(num_levels=3, map_point_depth_noise=sigma)
    kf_pose = tracking.Pose(_rot([0.2, 1.0, -0.3], 0.35), np.array([0.31, -0.17, 0.23]))
    q_pose = tracking.Pose(_rot([0.25, 1.0, -0.2], 0.41), np.array([0.42, -0.11, 0.3]))
    kp = _keypoints(64)
    kf = tracking.make_keyframe(7, kf_pose, kp, np.zeros((64, 32), np.uint8), K0, 5.0, s)
    C = tracking.world_position_f32(kf_pose)
    cand = (np.concatenate([kf.points, C[None]]), np.concatenate([kp["octave"], [3]]),
            np.concatenate([kf.mvd, np.zeros((1, 3), np.float32)]), np.concatenate([kf.dmin, [0]]),
            np.concatenate([kf.dmax, [0]]))
    ok, octv, keep, _ = _math(exe, tmp_path, s, K0, kf_pose, q_pose, kp, cand)
    assert 10 < len(keep) < 64  # the scene exercises both outcomes
    # the centre point: zero direction and distances
    ka = _keyframe(kf_pose, cand[0], cand[1], np.zeros((65, 3)), np.zeros(65), np.zeros(65))
    tracking.point_attributes(ka, s, np.arange(65))
    assert not ka.mvd[64].any() and ka.dmin[64] == 0 and ka.dmax[64] == 0


def test_arithmetic_edge_cases(exe, tmp_path):
    """A query pose whose arithmetic is exact (a quarter turn, dyadic translation and camera), so
    points land exactly on and one float beside every limit of ProjectMapPointIntoCurrentFrame /
    IsGoodCandidate / ComputeOctave (the neighbours are chosen so that they project exactly too: one
    float of the camera-space coordinate at the low limits, one float of the pixel at the high ones)."""
    f32 = np.float32
    L = 2
    s = tracking.TrackerSettings(num_levels=L)
    K = (512.0, 512.0, 640.0, 360.0)
    Rq = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tq = np.array([0.5, -0.25, 1.0])
    q_pose = tracking.Pose(Rq, tq)
    kf_pose = tracking.Pose(_rot([0.2, 1.0, -0.3], 0.35), np.array([0.31, -0.17, 0.23]))
    fw = Rq[2]
    scale = float(f32(s.scale_factor))
    names, pts, mvds, dmins, dmaxs = [], [], [], [], []

    def add(name, cs, mvd=fw, dmin=None, dmax=1e6):
        P = Rq.T @ (np.asarray(cs, np.float64) - tq)  # exact: one term per sum, dyadic values
        assert np.array_equal(f32(P).astype(np.float64), P)
        d = float(np.sqrt(f32(np.sum((P + Rq.T @ tq) ** 2))))
        names.append(name)
        pts.append(f32(P))
        mvds.append(f32(mvd))
        dmins.append(f32(d / scale ** 0.7 if dmin is None else dmin))  # octave 0 unless given
        dmaxs.append(f32(dmax))

    def cam_x(px, z=4.0):  # camera-space x of the point that projects to column px at depth z
        return f32((f32(px) - f32(640)) / f32(512) * f32(z))

    up, dn = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    cam_y = lambda py, z=4.0: f32((f32(py) - f32(360)) / f32(512) * f32(z))
    add("inside", [0.5, 0.25, 4.0])
    add("depth 0", [0.25, 0.125, 0.0])
    add("behind", [0.5, 0.25, -4.0])
    add("on border", [cam_x(7.5), 0.0, 4.0])
    add("left of border", [dn(cam_x(7.5)), 0.0, 4.0])
    add("on W - border", [cam_x(1272.5), 0.0, 4.0])
    add("inside W - border", [cam_x(dn(1272.5)), 0.0, 4.0])
    add("right of W - border", [cam_x(up(1272.5)), 0.0, 4.0])
    add("on top border", [0.0, cam_y(7.5), 4.0])
    add("above border", [0.0, dn(cam_y(7.5)), 4.0])
    add("on H - border", [0.0, cam_y(712.5), 4.0])
    add("inside H - border", [0.0, cam_y(dn(712.5)), 4.0])
    add("below H - border", [0.0, cam_y(up(712.5)), 4.0])
    add("view angle", [0.5, 0.25, 4.0], mvd=-fw)
    # on the optical axis at depth 4: |P - C|^2 = 16 exactly
    add("d = dmin: octave -1", [0.0, 0.0, 4.0], dmin=4.0)
    add("just inside dmin", [0.0, 0.0, 4.0], dmin=dn(4.0))
    add("just outside dmin", [0.0, 0.0, 4.0], dmin=up(4.0))
    add("d = dmax", [0.0, 0.0, 4.0], dmax=4.0)
    add("just inside dmax", [0.0, 0.0, 4.0], dmax=up(4.0))
    add("just outside dmax", [0.0, 0.0, 4.0], dmax=dn(4.0))
    add("octave num_levels", [0.0, 0.0, 4.0], dmin=4.0 / scale ** (L + 0.7))
    add("octave num_levels + 1", [0.0, 0.0, 4.0], dmin=4.0 / scale ** (L + 1.7))
    m = len(pts)
    cand = (np.array(pts), np.arange(m) % 8, np.array(mvds), np.array(dmins), np.array(dmaxs))
    ok, octv, keep, _ = _math(exe, tmp_path, s, K, kf_pose, q_pose, _keypoints(64), cand)
    kept = {names[i]: int(octv[i]) for i in keep}
    # what tracking.py (and, bit for bit, the header) decides: the cases are the ones meant
    assert kept == {"inside": 0, "depth 0": 0, "on border": 0, "inside W - border": 0, "on top border": 0,
                    "inside H - border": 0, "just inside dmin": 0, "d = dmax": 0, "just inside dmax": 0,
                    "octave num_levels": L}
    assert int(octv[names.index("d = dmin: octave -1")]) == -1
    assert int(octv[names.index("octave num_levels + 1")]) == L + 1


def _ring_parts(ring, first, theta):
    nk = len(ring)
    cap = max(len(k.points) for k in ring)
    acap = max([len(k.assoc_owner) for k in ring] + [1])
    n, ids, an = np.zeros(nk, np.uint32), np.zeros(nk, np.uint32), np.zeros(nk, np.uint32)
    kp = np.zeros((nk, cap), KP_DTYPE)
    pts, mvd = np.zeros((nk, cap, 3), np.float32), np.zeros((nk, cap, 3), np.float32)
    dmin, dmax = np.zeros((nk, cap), np.float32), np.zeros((nk, cap), np.float32)
    pose, ref, own = np.zeros((nk, 12)), np.zeros((nk, cap), np.uint32), np.zeros((nk, cap), np.uint8)
    assoc, aalive = np.zeros((nk, acap, 4), np.int32), np.zeros((nk, acap), np.uint8)
    for r, k in enumerate(ring):
        sl, c, a = (first + r) % nk, len(k.points), len(k.assoc_owner)
        n[sl], ids[sl], an[sl] = c, k.id, a
        kp[sl, :c], pts[sl, :c], mvd[sl, :c], dmin[sl, :c], dmax[sl, :c] = k.kp, k.points, k.mvd, k.dmin, k.dmax
        pose[sl], ref[sl, :c], own[sl, :c] = _pose12(k.pose), k.refine, k.own_alive
        assoc[sl, :a, 0], assoc[sl, :a, 1] = k.assoc_owner, k.assoc_idx
        assoc[sl, :a, 2:] = np.asarray(k.assoc_uv, np.float32).reshape(a, 2).view(np.int32)
        aalive[sl, :a] = k.assoc_alive
    parts = [np.uint32([nk, cap, acap, first, nk]), n, ids, an, kp, pts, mvd, dmin, dmax, pose, ref, own, assoc, aalive,
             np.uint32([theta is not None, theta or 0])]
    return parts, (nk, cap, acap)


def _check_window(exe, tmp_path, ring, s, theta, first=1, solution=None):
    """build_window against tracking.build_ba_window on `ring`; with `solution` = (outliers, pos,
    r9, points) also apply_window against tracking.apply_ba_window."""
    parts, (nk, cap, acap) = _ring_parts(ring, first, theta)
    tail = [np.uint32([0xFFFFFFFF])]
    if solution is not None:
        outl, pos, r9, xyz = solution
        tail = [np.uint32([len(outl)]), np.uint32(outl), np.float32(pos), np.float32(r9), np.float32(xyz)]
    r = _run(exe, tmp_path, "window", _const(s, K0) + parts + tail)
    w, theta_out = tracking.build_ba_window(ring, K0, s, theta)
    valid, nr, ntheta, steps = (int(v) for v in r.take(np.uint32, 4))
    huber, (E, P) = r.take(np.float32)[0], (int(v) for v in r.take(np.uint32, 2))
    assert ntheta == theta_out and valid == (w is not None)
    if w is None:
        assert r.done()
        return None
    assert nr == len(ring) and E == len(w.cam) and P == len(w.point_src)
    assert _same(r.take(np.uint32, E), w.cam) and _same(r.take(np.uint32, E), w.pt)
    assert _same(r.take(np.float32, 2 * E).reshape(E, 2), w.uv) and _same(r.take(np.float32, E), w.info)
    assert _same(r.take(np.uint8, nr), w.fixed)
    assert [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in r.take(np.uint64, P)] == w.point_src  # the point order
    assert [(("own", "assoc")[k], int(c), int(i)) for k, c, i in r.take(np.uint32, 3 * E).reshape(E, 3)] == w.obs_src
    assert max(steps, 1) == len(w.huber_widths) and float(huber) == w.huber_widths[0]
    assert _same(r.take(np.float32, 3 * nr).reshape(nr, 3), w.pos)
    assert _same(r.take(np.float32, 9 * nr).reshape(nr, 9), w.rot_colmajor)
    assert _same(r.take(np.float32, 4 * nr).reshape(nr, 4), w.intr)
    assert _same(r.take(np.float32, 3 * P).reshape(P, 3), w.points)
    if solution is None:
        assert r.done()
        return w
    tracking.apply_ba_window(ring, w, outl, np.float32(pos), np.float32(r9), np.float32(xyz), s)
    pts, mvd = r.take(np.float32, 3 * nk * cap).reshape(nk, cap, 3), r.take(np.float32, 3 * nk * cap).reshape(nk, cap, 3)
    dmin, dmax = r.take(np.float32, nk * cap).reshape(nk, cap), r.take(np.float32, nk * cap).reshape(nk, cap)
    pose, ref = r.take(np.float64, 12 * nk).reshape(nk, 12), r.take(np.uint32, nk * cap).reshape(nk, cap)
    own, aalive = r.take(np.uint8, nk * cap).reshape(nk, cap), r.take(np.uint8, nk * acap).reshape(nk, acap)
    changed = r.take(np.uint8, nk)
    assert r.done()
    for p, k in enumerate(ring):
        sl, c, a = (first + p) % nk, len(k.points), len(k.assoc_owner)
        assert _same(pts[sl, :c], k.points) and _same(mvd[sl, :c], k.mvd)
        assert _same(dmin[sl, :c], k.dmin) and _same(dmax[sl, :c], k.dmax)
        assert _same(pose[sl], _pose12(k.pose)) and _same(ref[sl, :c], k.refine)
        assert np.array_equal(own[sl, :c], k.own_alive) and np.array_equal(aalive[sl, :a], k.assoc_alive)
    assert changed.all()  # every keyframe of this ring owns a window point
    return w


def test_window_structure_and_write_back(exe, tmp_path):
    s = tracking.TrackerSettings(ba_free_keyframes=2)
    pos = np.float32([[0, 0, 0], [0.11, 0, 0], [0.21, 0, 0]])
    r9 = np.tile(np.eye(3, dtype=np.float32).reshape(9), (3, 1))
    pts = np.float32([[9, 9, 9], [8, 8, 8], [7, 7, 7], [6, 6, 6]])
    ring = _structure_ring()
    w = _check_window(exe, tmp_path, ring, s, None, solution=([2, 3], pos, r9, pts))
    assert w.point_src == [(0, 1), (1, 0), (2, 0), (2, 1)] and not ring[1].assoc_alive[0] and ring[0].dmax[1] > 0


def test_window_none(exe, tmp_path):
    assert _check_window(exe, tmp_path, [_kf(0, 3, 0.0)], tracking.TrackerSettings(), None, first=0) is None
    # two keyframes, the only free candidate is the map's first: no window (freemask == 0)
    s = tracking.TrackerSettings(covis_min_threshold=100)
    assert _check_window(exe, tmp_path, [_kf(5, 2, 0.0), _kf(0, 2, 0.1)], s, None) is None


def _ring_id0_covisible():
    ring = _covis_ring()
    ring[3].assoc_owner = np.array([0, 10, 10])
    ring[3].assoc_idx = np.array([1, 0, 1])
    ring[3].assoc_uv, ring[3].assoc_alive = np.float32([[4, 4], [2, 2], [3, 3]]), np.array([True, True, True])
    return ring


_COVIS = dict(covis_min_threshold=1, covis_ba_step=1)
COVIS_CASES = {
    "theta steps up": (_covis_ring, dict(_COVIS, ba_lower_connections=0, ba_upper_connections=9), 1, 2, [1, 0, 1, 0]),
    "max_steps 0": (_covis_ring, dict(_COVIS, ba_lower_connections=0, ba_upper_connections=9, covis_max_steps=0), 1, 2,
                    [1, 0, 0, 0]),
    "theta steps down": (_covis_ring, dict(_COVIS, ba_lower_connections=100), 3, 1, [1, 0, 1, 0]),
    "at the floor": (_covis_ring, dict(_COVIS, ba_lower_connections=100), 1, 1, [1, 0, 0, 0]),
    "id-0 keyframe": (_ring_id0_covisible, dict(_COVIS, ba_lower_connections=0), 1, 1, [1, 0, 0, 0]),
    "default theta": (_covis_ring, dict(ba_lower_connections=0), None, 15, [1, 1, 1, 0]),
}


@pytest.mark.parametrize("case", sorted(COVIS_CASES))
def test_window_covisibility(exe, tmp_path, case):
    make, kw, theta, theta_out, fixed = COVIS_CASES[case]
    w = _check_window(exe, tmp_path, make(), tracking.TrackerSettings(**kw), theta)
    _, t = tracking.build_ba_window(make(), K0, tracking.TrackerSettings(**kw), theta)
    assert t == theta_out and list(w.fixed) == fixed


N_BUFFERS = 62
RING_BUFFERS = 11


@pytest.mark.parametrize("pitch,lmk", list(itertools.product([1, 1000, 2000, 4096], [0, 1, 4, 8])))
def test_block_table(exe, tmp_path, pitch, lmk):
    for frames in (1, 2, 100):
        qcap = max(lmk, 1) * pitch if lmk else 0
        lm_bytes = 4096 * 8 + max(qcap, 1) * 48  # local_map_scratch_bytes(qcap)
        r = _run(exe, tmp_path, "block", [np.uint32([pitch, lmk, frames]), np.uint64([lm_bytes])])
        total, ring_begin, moved_begin, ring_end, contiguous, rows = (int(v) for v in r.take(np.uint64, 6))
        assert rows == N_BUFFERS and contiguous == 1
        bound, at, size, part = r.take(np.uint64, 4 * rows).reshape(rows, 4).astype(np.int64).T
        # every buffer where the walk put it, 256-aligned, inside the block, before the next one
        assert np.array_equal(bound, at) and not (at % 256).any() and (at + size <= total).all()
        assert (at[:-1] + size[:-1] <= at[1:]).all()
        # the ring: consecutive entries (one byte range up to alignment), the moved ones last
        ring = np.nonzero(part)[0]
        assert len(ring) == RING_BUFFERS and np.array_equal(ring, np.arange(ring[0], ring[0] + RING_BUFFERS))
        assert np.array_equal(at[ring[1:]], (at[ring[:-1]] + size[ring[:-1]] + 255) // 256 * 256)
        assert ring_begin == at[ring[0]] and ring_end == at[ring[-1]] + size[ring[-1]]
        moved = np.nonzero(part == 2)[0]
        assert moved_begin == at[moved[0]] and np.array_equal(moved, np.arange(moved[0], ring[-1] + 1))
        # the mirror's views at the device views' relative offsets
        rel = r.take(np.int64, 2 * RING_BUFFERS).reshape(RING_BUFFERS, 2)
        assert np.array_equal(rel[:, 0], rel[:, 1]) and np.array_equal(rel[:, 0], at[ring] - ring_begin)
        assert r.done()
