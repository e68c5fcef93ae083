"""Helpers of the BA dense-solve tests (test_ba_dense_reference.py, test_gpu_ba_large.py): graph
transformations that give the reduced camera system S an arbitrary block pattern, a plain fp64
reference of one Levenberg-Marquardt trial that shares nothing with either Schur implementation,
and the one-trial case tables with their tolerances.  Not a test module (nothing here is collected).

Tolerance: a backward-stable solve of S dx = rhs has the first-order forward error
cond2(S) * eps * |dx|, and the state x0 (+) dx carries eps * |state| of rounding of its own, so

    state_tol = K * eps * (cond2(S) * max|dx| + max|state|),   K = 4.

The CPU oracle sits between 0.001x and 0.17x of the K = 1 value on every case below (DESIGN.md,
"One-trial accuracy of the dense solve"); K = 4 leaves the GPU's other summation order and its FMA
contraction about 20x the reference's own error.

Tethers (TCASES).  Transform tethers have analytic Jacobians and are held to state_tol as it
stands.  Distance and rotation tethers are linearised, by specification, with an fp64 central
difference of step 1e-9, whose rounding noise (eps |e| / 1e-9, 1e-7 relative for a distance tether)
moves the solution by far more than state_tol and differs between two correct implementations.
Their reference is therefore built from a Richardson-extrapolated Jacobian (`hp`) and the tolerance is

    state_tol + F * d_fd,

d_fd the state distance between the `hp` reference and the one built from the oracle's own 1e-9
quotient, F = 4 x (the largest distance of FD_SAMPLES, independent fp64 roundings of that quotient,
from the `hp` reference) / d_fd, measured on the CPU and frozen in FD_F (fd_sample_ratios,
test_ba_dense_reference.py; the figures are in DESIGN.md).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from mageslam_amd import synth

EPS = float(np.finfo(np.float64).eps)
TOL_K = 4.0
MAX_ERR = 1e12  # maxErrorSquare of the one-trial cases: no edge is ever removed


# ------------------------------------------------------------------------------------------
# graph transformations
# ------------------------------------------------------------------------------------------
def permute_cameras(g, perm):
    """Relabel the cameras of `g`: old index i becomes perm[i].  Same geometry, but S takes the
    block pattern of the permutation and the fixed cameras land at arbitrary indices."""
    perm = np.asarray(perm, np.int64)
    assert sorted(perm.tolist()) == list(range(len(g.pos)))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))  # new index j holds old camera inv[j]
    return dataclasses.replace(
        g, pos=g.pos[inv].copy(), rot=g.rot[inv].copy(), intr=g.intr[inv].copy(), fixed=g.fixed[inv].copy(),
        true_rot=g.true_rot[inv].copy(), true_pos=g.true_pos[inv].copy(), cam=perm[g.cam].astype(np.uint32),
        points=g.points.copy(), uv=g.uv.copy(), pt=g.pt.copy(), info=g.info.copy())


def join_graphs(g1, g2):
    """g1 followed by g2 with camera and point offsets: two disconnected components, so the coupling
    block of S is exactly zero and g2's fixed cameras sit between free ones."""
    nc, npt = len(g1.pos), len(g1.points)
    cat = lambda f: np.concatenate([getattr(g1, f), getattr(g2, f)])  # noqa: E731
    return dataclasses.replace(
        g1, pos=cat("pos"), rot=cat("rot"), intr=cat("intr"), fixed=cat("fixed"), points=cat("points"), uv=cat("uv"),
        info=cat("info"), true_points=cat("true_points"), true_pos=cat("true_pos"), true_rot=cat("true_rot"),
        cam=np.concatenate([g1.cam, g2.cam + nc]).astype(np.uint32),
        pt=np.concatenate([g1.pt, g2.pt + npt]).astype(np.uint32))


def append_edges(g, src, uv_noise, rng):
    """`g` with copies of the edges `src` appended, their observations moved by N(0, uv_noise) px."""
    src = np.asarray(src, np.int64)
    uv = g.uv[src] + rng.normal(0, uv_noise, (len(src), 2)).astype(np.float32)
    return dataclasses.replace(g, cam=np.concatenate([g.cam, g.cam[src]]), pt=np.concatenate([g.pt, g.pt[src]]),
                               info=np.concatenate([g.info, g.info[src]]), uv=np.concatenate([g.uv, uv]))


def keep_edges(g, keep):
    """`g` with only the edges flagged in `keep`."""
    return dataclasses.replace(g, cam=g.cam[keep], pt=g.pt[keep], info=g.info[keep], uv=g.uv[keep])


# ------------------------------------------------------------------------------------------
# tethers: construction and linearisation
# ------------------------------------------------------------------------------------------
def _empty(stride):
    return (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, stride), np.float32), np.zeros(0, np.float32))


def make_tethers(g, distance=(), rotation=(), transform=()):
    """Tethers measured on the true poses of `g`.  Each entry is (cam1, cam2, weight) or, for a
    transform tether, (cam1, cam2, weight, offset) with `offset` added to the measured translation.
    Without an offset the k-th transform measurement is moved by 2 mm along axis k % 3 and the k-th
    distance by +-1 %, so that no tether is satisfied exactly at the true poses."""
    R, t = g.true_rot, g.true_pos
    u32 = lambda v: np.asarray(v, np.uint32)  # noqa: E731
    f32 = lambda v: np.asarray(v, np.float32)  # noqa: E731
    dist = rot = tr = None
    if distance:
        d = [np.linalg.norm(t[b] - t[a]) * (1 + 0.01 * (-1) ** k) for k, (a, b, _) in enumerate(distance)]
        dist = (u32([p[0] for p in distance]), u32([p[1] for p in distance]), f32(d), f32([p[2] for p in distance]))
    if rotation:
        q = [synth.quat_from_rot(R[a].T @ R[b]) for a, b, _ in rotation]
        rot = (u32([p[0] for p in rotation]), u32([p[1] for p in rotation]), f32(q), f32([p[2] for p in rotation]))
    if transform:
        p7 = []
        for k, p in enumerate(transform):
            a, b = p[0], p[1]
            off = np.asarray(p[3], np.float64) if len(p) > 3 else 0.002 * np.eye(3)[k % 3]
            Rc = R[b] @ R[a].T
            p7.append(np.concatenate([t[b] - Rc @ t[a] + off, synth.quat_from_rot(Rc)]))
        tr = (u32([p[0] for p in transform]), u32([p[1] for p in transform]), f32(p7), f32([p[2] for p in transform]))
    return synth.Tethers(distance=dist or _empty(1), rotation=rot or _empty(4), transform=tr or _empty(7))


def tether_count(tethers):
    return 0 if tethers is None else sum(len(tt[0]) for tt in (tethers.distance, tethers.rotation, tethers.transform))


def make_oracle(g, tethers=None, points_fixed=False):
    from oracle import oracle as O

    ob = O.BundlerOracle(points_fixed)
    ob.set_graph(g)
    if tethers is not None:
        for kind, tt in enumerate((tethers.distance, tethers.rotation, tethers.transform)):
            ob.set_tethers(kind, *tt)
    return ob


def _qmul(a, b):
    """Hamilton product of quaternions stored x, y, z, w."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def tether_error_numpy(kind, qt1, qt2, param, weight):
    """The distance (kind 0) and rotation (kind 1) tether errors restated in numpy on the fp64
    state rows (q xyzw, t) of the two cameras: (d - |t2 - t1|) w and the angle between
    rot(T1^-1 T2) and the measured quaternion, times w.  Another rounding of the oracle's expression."""
    w = float(np.float32(weight))
    if kind == 0:
        return (float(np.float32(param)) - np.linalg.norm(qt2[4:] - qt1[4:])) * w
    q1c = qt1[:4] * np.array([-1.0, -1.0, -1.0, 1.0])
    rel = _qmul(q1c, qt2[:4])
    rel = rel / np.linalg.norm(rel)
    m = np.asarray(param, np.float32).astype(np.float64) * np.array([-1.0, -1.0, -1.0, 1.0])
    d = _qmul(rel, m)
    return 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3])) * w


@dataclasses.dataclass
class TetherBlock:
    """The linearisation of one active tether: e (dim), J1 / J2 (dim x 6) with respect to camera
    c1 / c2, information om * I.  `scale` multiplies the information (1 for a tether, which is
    never robustified), `transpose12` swaps the off-diagonal block and `h12` = False leaves it out:
    the three exist for the mutation checks only."""
    index: int
    kind: int
    c1: int
    c2: int
    om: float
    e: np.ndarray
    J1: np.ndarray
    J2: np.ndarray
    scale: float = 1.0
    transpose12: bool = False
    h12: bool = True


FD_DELTA = 1e-9  # the central-difference step of the distance / rotation Jacobians (g2o's)
HP_STEP = 1e-5  # Richardson: (4 D(h) - D(2h)) / 3 with D the central difference
FD_SAMPLES = ("oracle", "numpy", "chain", "chain-swapped")


def _fd_jacobian(ob, g, tethers, i, kind, c, scheme):
    """d error / d camera c (1 x 6) of distance / rotation tether i at the initial state.
      hp             Richardson extrapolation of central differences of the oracle's error at
                     HP_STEP and 2 HP_STEP, each from the restored initial state
      numpy          the FD_DELTA quotient of tether_error_numpy on the perturbed oracle state
      chain          the FD_DELTA quotient of the oracle's error with the camera moved +d, -2d, +d
                     in place (the evaluation points carry the rounding of the chained updates)
      chain-swapped  the same with -d, +2d, -d
    """
    def restore():
        ob.set_cameras(g.pos, g.rot_colmajor, g.intr, g.fixed)

    def err_at(u):
        restore()
        ob.perturb_camera(c, u)
        return float(ob.tether_linearization(i)[0][0])

    J = np.zeros((1, 6))
    tt = (tethers.distance, tethers.rotation)[kind]
    k = i - (0 if kind == 0 else len(tethers.distance[0]))
    for dd in range(6):
        u = np.zeros(6)
        if scheme == "hp":
            D = []
            for h in (HP_STEP, 2 * HP_STEP):
                u[dd] = h
                ep = err_at(u)
                em = err_at(-u)
                D.append((ep - em) / (2 * h))
            J[0, dd] = (4 * D[0] - D[1]) / 3
        elif scheme == "numpy":
            e = []
            for s in (1.0, -1.0):
                u[dd] = s * FD_DELTA
                restore()
                ob.perturb_camera(c, u)
                qt = ob.state()[0]
                e.append(tether_error_numpy(kind, qt[int(tt[0][k])], qt[int(tt[1][k])], tt[2][k], tt[3][k]))
            J[0, dd] = (e[0] - e[1]) / (2 * FD_DELTA)
        else:
            s = 1.0 if scheme == "chain" else -1.0
            restore()
            u[dd] = s * FD_DELTA
            ob.perturb_camera(c, u)
            e1 = float(ob.tether_linearization(i)[0][0])
            ob.perturb_camera(c, -2 * u)
            e2 = float(ob.tether_linearization(i)[0][0])
            J[0, dd] = s * (e1 - e2) / (2 * FD_DELTA)
    restore()
    return J


def tether_blocks(g, tethers, points_fixed=False, jac="oracle"):
    """TetherBlock of every active tether (not both cameras fixed) at the initial state, in
    distance, rotation, transform order.  `jac` chooses the Jacobians of the distance and rotation
    tethers: 'oracle' (its own FD_DELTA quotient) or a scheme of _fd_jacobian; transform tethers
    always carry the oracle's analytic adjoints.  Jacobians of fixed cameras are left zero."""
    if tether_count(tethers) == 0:
        return []
    ob = make_oracle(g, tethers, points_fixed)
    kinds = [k for k, tt in enumerate((tethers.distance, tethers.rotation, tethers.transform)) for _ in tt[0]]
    flat = [(int(a), int(b), float(w)) for tt in (tethers.distance, tethers.rotation, tethers.transform)
            for a, b, w in zip(tt[0], tt[1], tt[3])]
    blocks = []
    for i, (kind, (c1, c2, w)) in enumerate(zip(kinds, flat)):
        e, J1, J2 = ob.tether_linearization(i)
        active = not (g.fixed[c1] and g.fixed[c2])
        assert (len(e) > 0) == active  # inactive exactly if both cameras are fixed
        if not active:
            continue
        J1, J2 = J1.copy(), J2.copy()
        if kind < 2 and jac != "oracle":
            if not g.fixed[c1]:
                J1 = _fd_jacobian(ob, g, tethers, i, kind, c1, jac)
            if not g.fixed[c2]:
                J2 = _fd_jacobian(ob, g, tethers, i, kind, c2, jac)
        if g.fixed[c1]:
            J1[:] = 0
        if g.fixed[c2]:
            J2[:] = 0
        blocks.append(TetherBlock(i, kind, c1, c2, w if kind == 2 else 1.0, e.copy(), J1, J2))
    return blocks


# ------------------------------------------------------------------------------------------
# the dense reference of one LM trial
# ------------------------------------------------------------------------------------------
def dense_system(g, huber, tethers=None, points_fixed=False, jac="oracle", mutate=None):
    """The full unreduced normal equations of `g` at its initial state in float64.  The oracle only
    supplies each edge's and each tether's error and Jacobians.  Returns (H, b, cams, pts, robust):
    H without the damping, the camera / point indices of the unknowns (6 per camera, then 3 per
    point; no points with `points_fixed`) and the per-edge flag 'in Huber's linear zone' of the
    active edges.  An edge is active unless its camera and its point are both fixed; the unknown
    cameras are the free ones with an active edge or an active tether.  Tethers add
    J_v^T Om J_v on the diagonal block of each free camera, J_1^T Om J_2 (and its transpose) when
    both are free and -J_v^T Om e to b, and are never robustified.  `mutate(blocks)` may alter the
    tether blocks before they are added (mutation checks)."""
    ob = make_oracle(g, None, points_fixed)
    cam = g.cam.astype(np.int64)
    pt = g.pt.astype(np.int64)
    active = np.ones(len(cam), bool) if not points_fixed else g.fixed[cam] == 0
    cam, pt = cam[active], pt[active]
    idx = np.flatnonzero(active)
    E = len(idx)
    err = np.zeros((E, 2))
    jpt = np.zeros((E, 2, 3))
    jp = np.zeros((E, 2, 6))
    for k, e in enumerate(idx):
        err[k], jpt[k], jp[k] = ob.edge_linearization(int(e))
    delta = float(np.float32(huber))
    info = g.info.astype(np.float64)[active]
    chi2 = info * (err ** 2).sum(1)
    robust = chi2 > delta * delta
    w = info * np.where(robust, delta / np.sqrt(np.where(robust, chi2, 1.0)), 1.0)

    blocks = tether_blocks(g, tethers, points_fixed, jac)
    if mutate is not None:
        mutate(blocks)
    seen = np.zeros(len(g.pos), bool)
    seen[cam] = True
    for t in blocks:
        seen[[t.c1, t.c2]] = True
    cams = np.flatnonzero(seen & (g.fixed == 0))
    pts = np.zeros(0, np.int64) if points_fixed else np.unique(pt)
    hc = np.full(len(g.pos), -1, np.int64)
    hc[cams] = np.arange(len(cams))
    hp = np.full(len(g.points), -1, np.int64)
    hp[pts] = np.arange(len(pts))
    n = 6 * len(cams) + 3 * len(pts)
    H = np.zeros((n, n))
    b = np.zeros(n)

    def add(rows, cols, blks):
        np.add.at(H, (rows[:, :, None], cols[:, None, :]), blks)

    f = hc[cam] >= 0
    crow = 6 * hc[cam[f]][:, None] + np.arange(6)
    wf = w[f]
    add(crow, crow, wf[:, None, None] * np.einsum("eki,ekj->eij", jp[f], jp[f]))
    np.add.at(b, crow, -wf[:, None] * np.einsum("eki,ek->ei", jp[f], err[f]))
    if not points_fixed:
        po = 6 * len(cams) + 3 * hp[pt]
        prow = po[:, None] + np.arange(3)
        add(prow, prow, w[:, None, None] * np.einsum("eki,ekj->eij", jpt, jpt))
        np.add.at(b, prow, -w[:, None] * np.einsum("eki,ek->ei", jpt, err))
        cross = wf[:, None, None] * np.einsum("eki,ekj->eij", jp[f], jpt[f])
        add(crow, prow[f], cross)
        add(prow[f], crow, cross.transpose(0, 2, 1))

    for t in blocks:
        om = t.om * t.scale
        h1, h2 = hc[t.c1], hc[t.c2]
        for h, J in ((h1, t.J1), (h2, t.J2)):
            if h >= 0:
                s = slice(6 * h, 6 * h + 6)
                H[s, s] += om * (J.T @ J)
                b[s] -= om * (J.T @ t.e)
        if h1 >= 0 and h2 >= 0 and t.h12:
            B = om * (t.J1.T @ t.J2)
            if t.transpose12:
                B = B.T
            H[6 * h1:6 * h1 + 6, 6 * h2:6 * h2 + 6] += B
            H[6 * h2:6 * h2 + 6, 6 * h1:6 * h1 + 6] += B.T
    return H, b, cams, pts, robust


def solve_refined(A, b, rounds=2):
    """np.linalg.solve followed by iterative refinement with the residual in np.longdouble."""
    x = np.linalg.solve(A, b)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(rounds):
        r = (bl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(A, r)
    return x


def apply_update(g, cams, pts, x, tethers=None, points_fixed=False):
    """x0 (+) x through the oracle's own exponential update; the fp64 state (qt, xyz)."""
    ob = make_oracle(g, tethers, points_fixed)
    for h, c in enumerate(cams):
        ob.perturb_camera(int(c), x[6 * h:6 * h + 6])
    o = 6 * len(cams)
    for h, p in enumerate(pts):
        ob.perturb_point(int(p), x[o + 3 * h:o + 3 * h + 3])
    return ob.state()


@dataclasses.dataclass
class DenseStep:
    qt: np.ndarray  # (C, 7) predicted state after the trial
    xyz: np.ndarray  # (P, 3)
    x: np.ndarray  # the update: 6 per free camera, then 3 per point
    cond_S: float  # cond2 of the reduced camera system
    cams: np.ndarray  # camera index of each 6-block of x
    pts: np.ndarray  # point index of each 3-block of x
    robust_frac: float  # share of (active) edges in Huber's linear zone at the initial state


def dense_lm_step(g, lam, huber, tethers=None, points_fixed=False, jac="oracle", mutate=None) -> DenseStep:
    """One LM trial of `g` from its initial state with damping `lam` and Huber width `huber` (both
    rounded to float32, as the C ABI receives them): (H + lam I) x = b over all 6 free + 3 P
    unknowns at once, no Schur complement.  cond_S is that of S = Hpp - Hpl Hll^-1 Hpl^T formed
    from the same damped blocks; with `points_fixed` there are no point unknowns and S is the damped
    camera system itself."""
    H, b, cams, pts, robust = dense_system(g, huber, tethers, points_fixed, jac, mutate)
    A = H + float(np.float32(lam)) * np.eye(len(b))
    x = solve_refined(A, b)
    nc = 6 * len(cams)
    S = A[:nc, :nc] - A[:nc, nc:] @ np.linalg.solve(A[nc:, nc:], A[nc:, :nc]) if len(pts) else A
    qt, xyz = apply_update(g, cams, pts, x, tethers, points_fixed)
    return DenseStep(qt, xyz, x, float(np.linalg.cond(S)), cams, pts, float(robust.mean()))


def state_tol(x, cond_S, state, k=TOL_K):
    qt, xyz = state
    return k * EPS * (cond_S * np.abs(x).max() + max(np.abs(qt).max(), np.abs(xyz).max()))


def state_diff(a, b):
    """Maximum absolute difference of two (qt, xyz) states; q and -q are the same rotation."""
    qa, pa = a
    qb, pb = b
    s = np.where(np.sum(qa[:, :4] * qb[:, :4], axis=1) < 0, -1.0, 1.0)[:, None]
    return max(np.abs(qa[:, :4] - s * qb[:, :4]).max(), np.abs(qa[:, 4:] - qb[:, 4:]).max(), np.abs(pa - pb).max())


# ------------------------------------------------------------------------------------------
# the one-trial cases
# ------------------------------------------------------------------------------------------
NO_HUBER = 1e6  # no edge robustified


def banded(free, points=None):
    cams = free + 2
    return synth.ba_graph(cameras=cams, fixed_cameras=2, points=max(5 * cams, 60) if points is None else points,
                          obs_per_point=min(cams, 8), seed=100 + free, outlier_frac=0)


def huber_graph(free):
    cams = free + 2
    return synth.ba_graph(cameras=cams, fixed_cameras=2, points=5 * cams, obs_per_point=8, seed=400 + free,
                          noise_px=1.0, outlier_frac=0.03)


def permuted(free, kind, points_per_camera=5):
    """`kind` 'rand': a random relabelling; 'rev': the reversal (fixed cameras last)."""
    cams = free + 3
    g = synth.ba_graph(cameras=cams, fixed_cameras=3, points=points_per_camera * cams, obs_per_point=8,
                       seed=200 + free, outlier_frac=0)
    perm = np.random.default_rng(200 + free).permutation(cams) if kind == "rand" else np.arange(cams)[::-1]
    return permute_cameras(g, perm)


def two_components(cams2, seed2):
    part = lambda c, s: synth.ba_graph(cameras=c, fixed_cameras=2, points=5 * c, obs_per_point=8, seed=s)  # noqa: E731
    return join_graphs(part(22, 301), part(cams2, seed2))


def _cases():
    c = {}
    for free in (1, 2, 8, 16, 40, 41, 48, 96):
        for lam in (1.0, 1e-3) if free in (40, 41, 96) else (1.0,):
            c[f"banded-{free}-lam{lam:g}"] = (functools.partial(banded, free), lam, NO_HUBER)
    for free in (11, 40, 48, 96):
        for lam in (1.0, 1e-2) if free == 48 else (1.0,):
            c[f"huber-{free}-lam{lam:g}"] = (functools.partial(huber_graph, free), lam, 1.8)
    for free in (40, 48):
        for kind in ("rand", "rev"):
            c[f"permuted-{kind}-{free}"] = (functools.partial(permuted, free, kind), 1.0, NO_HUBER)
    c["components-20+20"] = (functools.partial(two_components, 22, 302), 1.0, NO_HUBER)
    c["components-20+28"] = (functools.partial(two_components, 30, 303), 1.0, NO_HUBER)
    return c


CASES = _cases()  # id -> (graph builder, lambda, huber width)
CASE_IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def case(cid):
    """(graph, lam, huber, DenseStep) of one case; computed once per process, treat as read-only."""
    build, lam, huber = CASES[cid]
    g = build()
    return g, lam, huber, dense_lm_step(g, lam, huber)


def oracle_one_trial(g, lam, huber, tethers=None, points_fixed=False):
    """A fresh oracle after one step([huber], MAX_ERR) at damping lam: (oracle, outliers)."""
    ob = make_oracle(g, tethers, points_fixed)
    ob.set_lambda(lam)
    _, out = ob.step([huber], MAX_ERR)
    return ob, out


def mutated_reference(g, d: DenseStep, rel=1e-7):
    """The dense reference's state with the largest camera component of x scaled by 1 + rel: the
    'slightly wrong dx' that Levenberg-Marquardt forgives and the one-trial comparison must not."""
    x = d.x.copy()
    i = int(np.argmax(np.abs(x[:6 * len(d.cams)])))
    x[i] *= 1.0 + rel
    return apply_update(g, d.cams, d.pts, x)


# ------------------------------------------------------------------------------------------
# the one-trial cases with tethers, fixed points and odd edge lists
# ------------------------------------------------------------------------------------------
def base12(seed=500, points=120):
    """12 cameras, 0-2 fixed, 3-11 free; every point seen by 8 consecutive cameras."""
    return synth.ba_graph(cameras=12, fixed_cameras=3, points=points, obs_per_point=8, seed=seed, outlier_frac=0)


# tr-mixed: (4,7) listed c1 < c2; (9,5) listed c1 > c2 (the transposed H12); (6,10) and (10,6)
# on one pair in both orders (their H12 must sum); (1,8) fixed first, (11,2) fixed second; (0,2)
# fixed-fixed (inactive).  Indices into the transform set:
TR_MIXED = ((4, 7, 50.0), (9, 5, 40.0), (6, 10, 50.0), (10, 6, 30.0), (1, 8, 50.0), (11, 2, 60.0), (0, 2, 50.0))
TR_MIXED_REVERSED, TR_MIXED_DOUBLED_SECOND = 1, 3


def _tr_mixed():
    g = base12()
    return g, make_tethers(g, transform=TR_MIXED)


def _tr_shared():
    g = base12(501)
    assert np.intersect1d(g.pt[g.cam == 5], g.pt[g.cam == 6]).size > 20
    return g, make_tethers(g, transform=((5, 6, 50.0),))


def _tr_no_shared():
    part = lambda c, f, s: synth.ba_graph(cameras=c, fixed_cameras=f, points=60, obs_per_point=4, seed=s, outlier_frac=0)  # noqa: E731
    g = join_graphs(part(6, 2, 502), part(6, 1, 503))  # fixed: 0, 1 and 6
    return g, make_tethers(g, transform=((3, 9, 50.0), (10, 4, 40.0)))


def _tr_tether_only():
    from tests.test_gpu_ba import tethered_extra_camera

    g = tethered_extra_camera()
    n = len(g.pos)
    t = synth.Tethers(distance=_empty(1), rotation=_empty(4),
                      transform=(np.array([n - 2], np.uint32), np.array([n - 1], np.uint32),
                                 g.extra_tether[None, :], np.array([50.0], np.float32)))
    return g, t


# the first tether of the two Huber cases is off by `x` metres, chosen so that its chi2 lies just
# above the Huber width squared (sqrt(chi2) 1.81 against 1.8, 0.926 against 0.9): an implementation
# that robustified tethers would weigh it down by 0.7 and 3 %
def huber_tethers(g, x):
    return make_tethers(g, transform=((4, 9, 50.0, (x, 0.0, 0.0)), (11, 6, 50.0), (0, 7, 50.0), (12, 1, 40.0), (0, 1, 50.0)))


def _tr_huber():
    g = huber_graph(11)
    return g, huber_tethers(g, 0.266)


def _tr_40_corner():
    g = banded(40)
    return g, make_tethers(g, transform=((2, len(g.pos) - 1, 50.0, (0.0, 0.0, 0.0)),))


def _tr_41():
    g = banded(41)
    return g, make_tethers(g, transform=((2, 42, 50.0), (30, 9, 40.0)))


PF_TETHERS = ((4, 7, 50.0), (9, 5, 40.0), (1, 8, 50.0), (11, 2, 60.0), (0, 2, 50.0))


def _pf_plain():
    return base12(504), None


def _pf_tr():
    g = base12(505)
    return g, make_tethers(g, transform=PF_TETHERS)


def _pf_huber():
    g = huber_graph(11)
    return g, huber_tethers(g, 0.14)


def _dup_observation():
    g = base12(506)
    rng = np.random.default_rng(4)
    return append_edges(g, rng.choice(np.flatnonzero(g.fixed[g.cam] == 0), 20, replace=False), 0.3, rng), None


def _long_run_point():
    g = base12(507)
    rng = np.random.default_rng(5)
    extra = np.concatenate([rng.choice(np.flatnonzero(g.pt == p), 70, replace=True) for p in (7, 93)])
    return append_edges(g, extra, 0.3, rng), None


FIXED_ONLY_POINTS, SINGLE_POINTS = 3, 3


def _fixed_only_and_single():
    """Three points keep only their edges to the fixed cameras 0-2, three others one edge each (to
    a free camera)."""
    g = base12(508)
    first = np.array([g.cam[g.pt == p].min() for p in range(len(g.points))])
    fixed_only = np.flatnonzero(first == 0)[:FIXED_ONLY_POINTS]  # seen by cameras 0..7
    single = np.flatnonzero(first >= 3)[:SINGLE_POINTS]
    assert len(fixed_only) == FIXED_ONLY_POINTS and len(single) == SINGLE_POINTS
    keep = np.ones(len(g.cam), bool)
    keep[np.isin(g.pt, fixed_only) & (g.cam > 2)] = False
    for k, p in enumerate(single):
        e = np.flatnonzero(g.pt == p)
        keep[e] = False
        keep[e[2 * k + 1]] = True
    g = keep_edges(g, keep)
    g.fixed_only, g.single = fixed_only, single
    return g, None


# every finite-difference case has free-free pairs in both orders, a free-fixed and a fixed-fixed pair
def _dist():
    g = base12(509)
    return g, make_tethers(g, distance=((3, 6, 50.0), (8, 4, 50.0), (5, 9, 40.0), (1, 7, 50.0), (10, 2, 50.0), (0, 1, 50.0)))


def _rot():
    g = base12(510)
    return g, make_tethers(g, rotation=((3, 6, 10.0), (8, 4, 10.0), (5, 9, 8.0), (1, 7, 10.0), (10, 2, 10.0), (0, 1, 10.0)))


def _all_kinds_tethers(g):
    return make_tethers(g, distance=((3, 6, 50.0), (8, 4, 50.0), (1, 7, 50.0), (0, 1, 50.0)),
                        rotation=((5, 9, 10.0), (11, 4, 10.0), (10, 2, 10.0), (2, 0, 10.0)),
                        transform=((4, 7, 50.0), (9, 5, 40.0), (0, 8, 50.0), (1, 2, 50.0)))


def _all_kinds():
    g = base12(511)
    return g, _all_kinds_tethers(g)


def _all_kinds_pf():
    g = base12(512)
    return g, _all_kinds_tethers(g)


def _all_kinds_41():
    g = banded(41)
    return g, make_tethers(g, distance=((5, 20, 50.0), (30, 8, 50.0), (0, 12, 50.0), (0, 1, 50.0)),
                           rotation=((3, 40, 10.0), (22, 7, 10.0), (15, 1, 10.0), (1, 0, 10.0)),
                           transform=((2, 42, 50.0), (35, 10, 40.0), (6, 0, 50.0)))


@dataclasses.dataclass(frozen=True)
class TCase:
    build: object  # () -> (graph, Tethers or None)
    lam: float = 1.0
    huber: float = NO_HUBER
    points_fixed: bool = False
    fd: bool = False  # has distance / rotation tethers: hp reference, state_tol + F d_fd


TCASES = {
    "tr-mixed": TCase(_tr_mixed),
    "tr-no-shared-points": TCase(_tr_no_shared),
    "tr-shared-points": TCase(_tr_shared),
    "tr-tether-only-camera": TCase(_tr_tether_only),
    "tr-huber": TCase(_tr_huber, huber=1.8),
    "tr-40-corner": TCase(_tr_40_corner),
    "tr-41": TCase(_tr_41),
    "pf-plain": TCase(_pf_plain, points_fixed=True),
    "pf-tr": TCase(_pf_tr, points_fixed=True),
    "pf-huber": TCase(_pf_huber, huber=0.9, points_fixed=True),
    "dup-observation": TCase(_dup_observation),
    "long-run-point": TCase(_long_run_point),
    "fixed-only-and-single": TCase(_fixed_only_and_single),
    "dist": TCase(_dist, fd=True),
    "rot": TCase(_rot, fd=True),
    "all-kinds": TCase(_all_kinds, fd=True),
    "all-kinds-41": TCase(_all_kinds_41, fd=True),
    "all-kinds-pf": TCase(_all_kinds_pf, points_fixed=True, fd=True),
}
TCASE_IDS = list(TCASES)
FD_CASE_IDS = [c for c in TCASE_IDS if TCASES[c].fd]

# F of the finite-difference cases: 4 x max over FD_SAMPLES of (distance from the hp reference) /
# d_fd, measured by fd_sample_ratios on the CPU and rounded up (DESIGN.md has the samples).
FD_F = {"dist": 8.96, "rot": 4.0, "all-kinds": 4.77, "all-kinds-41": 4.01, "all-kinds-pf": 7.4}


@dataclasses.dataclass
class TCaseData:
    g: object
    tethers: object
    lam: float
    huber: float
    points_fixed: bool
    d: DenseStep  # the reference (hp Jacobians in a finite-difference case)
    tol: float  # state_tol, plus F d_fd in a finite-difference case
    tight: float  # state_tol alone
    d_fd: float  # 0 unless a finite-difference case

    @property
    def ref(self):
        return self.d.qt, self.d.xyz

    def dense(self, **kw):
        """Another dense reference of this case (jac=..., mutate=..., tethers=...)."""
        kw.setdefault("tethers", self.tethers)
        return dense_lm_step(self.g, self.lam, self.huber, points_fixed=self.points_fixed, **kw)


@functools.lru_cache(maxsize=None)
def tcase(cid) -> TCaseData:
    """The graph, tethers, reference and tolerance of one TCASES entry; computed once per process,
    treat as read-only."""
    c = TCASES[cid]
    g, t = c.build()
    d = dense_lm_step(g, c.lam, c.huber, t, c.points_fixed, "hp" if c.fd else "oracle")
    tight = state_tol(d.x, d.cond_S, (d.qt, d.xyz))
    d_fd = 0.0
    if c.fd:
        o = dense_lm_step(g, c.lam, c.huber, t, c.points_fixed, "oracle")
        d_fd = state_diff((o.qt, o.xyz), (d.qt, d.xyz))
    return TCaseData(g, t, c.lam, c.huber, c.points_fixed, d, tight + (FD_F[cid] * d_fd if c.fd else 0.0), tight, d_fd)


def fd_sample_ratios(cid):
    """{sample: distance of the dense reference built with that rounding of the FD_DELTA quotient
    from the hp reference, in units of d_fd} of a finite-difference case.  F = 4 x the largest."""
    t = tcase(cid)
    out = {}
    for s in FD_SAMPLES:
        o = t.dense(jac=s)
        out[s] = state_diff((o.qt, o.xyz), t.ref) / t.d_fd
    return out
