"""Helpers of the pose-only BA tests (test_pose_reference.py, test_gpu_pose.py): a plain fp64 NumPy
reference of pose-only StepBundleAdjustment written from the algorithm (the header of
mageslam_amd/csrc/pose.hip) that shares no code with oracle/ba_oracle.c or the kernel, input
transformations that drive a synth.PoseBatch into the Levenberg-Marquardt branches the stock
generator never reaches (rejected trials, failed solves, points behind the camera or passing
through its plane, per-problem intrinsics), the case table, and the comparison helpers.  Not a test
module (nothing is collected).

Decisions and fragility.  Every accept / reject and every outlier flag is a comparison of two fp64
numbers; the reference records how close each one came to flipping:

    m_rho  min over successfully solved trials of |currentChi - tempChi| / |currentChi|
    m_ss   min over edges of |ss - maxErrorSquare| / maxErrorSquare at the post-pass
    m_z    min over edges of |z| at the current pose

A problem with any margin below FRAGILE = 1e-9 may legitimately decide differently under another
rounding; it is left out of the decision comparisons, and at most MAX_FRAGILE_SHARE of a case's
problems may be fragile (asserted on the reference alone in test_pose_reference.py).

One-trial tolerance.  A backward-stable solve of (H + lambda I) x = b has the forward error
cond2(H + lambda I) eps |x|, and the pose exp(x) * T carries eps |pose| of its own:

    tol = K eps (cond2(H + lambda I) max|x| + max(1, max|t|))

with K = 4 for the CPU oracle and K = 256 for the kernel, whose Cholesky takes v_rsq_f64 plus one
Newton step (about 1e-14 = 45 eps relative, a backward error of the factor).
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from mageslam_amd import synth

EPS = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
FRAGILE = 1e-9
MAX_FRAGILE_SHARE = 0.02
K_ORACLE = 4.0
K_GPU = 256.0
MULTI_FLOOR = 1e-11  # multi-step pose tolerance: max(MULTI_FLOOR, MULTI_FACTOR * d_oracle(case))
MULTI_FACTOR = 100.0
NO_OUTLIERS = 1e12  # maxErrorSquare of the one-trial cases


# ------------------------------------------------------------------------------------------
# input transformations
# ------------------------------------------------------------------------------------------
def _problem_of_edge(obs_start):
    return np.repeat(np.arange(len(obs_start) - 1), np.diff(obs_start.astype(np.int64)))


def perturb(pb, deg, metres, seed):
    """Initial rotations left-multiplied by synth._rot of N(0, deg) per axis, N(0, metres) on pos."""
    rng = np.random.default_rng(seed)
    K = len(pb.pos)
    ang = np.deg2rad(rng.normal(0, deg, (K, 3)))
    dp = rng.normal(0, metres, (K, 3))
    r9 = np.empty((K, 9))
    for k in range(K):
        R0 = pb.r9[k].astype(np.float64).reshape(3, 3).T
        r9[k] = (synth._rot(*ang[k]) @ R0).T.reshape(9)
    return dataclasses.replace(pb, r9=r9.astype(np.float32), pos=(pb.pos.astype(np.float64) + dp).astype(np.float32))


def behind(pb, frac, seed):
    """ceil(frac * n) points of each problem mirrored through the true camera centre: the point
    projects to the same pixel and lies behind the camera."""
    rng = np.random.default_rng(seed)
    pts = pb.points.astype(np.float64).copy()
    for k in range(len(pb.pos)):
        s, e = int(pb.obs_start[k]), int(pb.obs_start[k + 1])
        n = e - s
        if n == 0:
            continue
        sel = s + rng.choice(n, size=int(math.ceil(frac * n)), replace=False)
        R, t = pb.true_rot[k], pb.true_pos[k]
        xc = pts[sel] @ R.T + t
        pts[sel] = (-xc - t) @ R
    return dataclasses.replace(pb, points=pts.astype(np.float32))


def vary_intrinsics(pb, seed):
    """Per problem a in U(0.5, 1.5), cx' in U(500, 800), cy' in U(250, 450): uv' = a (uv - c) + c',
    f' = a f.  The same geometry seen through another camera."""
    rng = np.random.default_rng(seed)
    K = len(pb.pos)
    a = rng.uniform(0.5, 1.5, K)
    c2 = np.stack([rng.uniform(500, 800, K), rng.uniform(250, 450, K)], axis=1)
    intr = pb.intr.astype(np.float64)
    pe = _problem_of_edge(pb.obs_start)
    uv = a[pe, None] * (pb.uv.astype(np.float64) - intr[pe, :2]) + c2[pe]
    intr2 = np.concatenate([c2, a[:, None] * intr[:, 2:]], axis=1)
    return dataclasses.replace(pb, uv=uv.astype(np.float32), intr=intr2.astype(np.float32))


GRAZING_INFO = 1e-15


def grazing(pb, frac, seed):
    """ceil(frac * n) observations of each problem replaced by points 5 to 50 mm in front of or
    behind the true camera plane and up to 3 m off the axis, observed without noise and weighted
    GRAZING_INFO, so that they hardly enter the normal equations.  A pose change of a fraction of a
    degree moves such a point through the camera plane: its cheirality at the first pose, at the
    pose before the last accepted trial and at the final pose differ, which nothing else in these
    cases achieves (Levenberg-Marquardt does not carry a weighted point through z = 0, where its
    error is singular).  Use with a maxErrorSquare that keeps them (NO_OUTLIERS)."""
    rng = np.random.default_rng(seed)
    pts, uv = pb.points.astype(np.float64).copy(), pb.uv.astype(np.float64).copy()
    info = pb.info.astype(np.float64).copy()
    for k in range(len(pb.pos)):
        s, e = int(pb.obs_start[k]), int(pb.obs_start[k + 1])
        n = e - s
        if n == 0:
            continue
        m = int(math.ceil(frac * n))
        sel = s + rng.choice(n, size=m, replace=False)
        xc = np.stack([rng.uniform(-3, 3, m), rng.uniform(-2, 2, m),
                       rng.uniform(0.005, 0.05, m) * rng.choice([-1.0, 1.0], m)], axis=1)
        R, t = pb.true_rot[k], pb.true_pos[k]
        pts[sel] = (xc - t) @ R
        cx, cy, f = (float(v) for v in pb.intr[k, :3])
        uv[sel] = f * xc[:, :2] / xc[:, 2:3] + np.array([cx, cy])
        info[sel] = GRAZING_INFO
    return dataclasses.replace(pb, points=pts.astype(np.float32), uv=uv.astype(np.float32), info=info.astype(np.float32))


def zero_info(pb):
    return dataclasses.replace(pb, info=np.zeros_like(pb.info, dtype=np.float32))


def concat(batches):
    """One batch holding the problems of all `batches` in order."""
    cat = lambda f: np.concatenate([getattr(b, f) for b in batches])  # noqa: E731
    counts = np.concatenate([np.diff(b.obs_start.astype(np.int64)) for b in batches])
    obs_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return dataclasses.replace(batches[0], pos=cat("pos"), r9=cat("r9"), intr=cat("intr"), obs_start=obs_start,
                               points=cat("points"), uv=cat("uv"), info=cat("info"), true_pos=cat("true_pos"),
                               true_rot=cat("true_rot"))


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def _quat_f32(r9):
    """Rotation (float32, column-major) -> quaternion (x, y, z, w) in float32 arithmetic, normalised
    in float32: what SetCameraPose does before the state continues in double."""
    f = np.float32
    m = np.asarray(r9, np.float32).reshape(3, 3).T  # m[r, c]
    q = [f(0)] * 4
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > f(0):
        s = np.sqrt(tr + f(1))
        q[3] = f(0.5) * s
        s = f(0.5) / s
        q[0] = (m[2, 1] - m[1, 2]) * s
        q[1] = (m[0, 2] - m[2, 0]) * s
        q[2] = (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + f(1))
        q[i] = f(0.5) * s
        s = f(0.5) / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    out = np.array([x / n for x in q])
    assert out.dtype == np.float32
    return out


def _normalized(q):
    q = -q if q[3] < 0 else q
    return q / math.sqrt(float(q @ q))


def _rotmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def oplus(q, t, x):
    """exp(x) * T for x = (omega, upsilon).  Below |omega| = 1e-5 the exponential is the truncated
    series R = V = I + [omega] + [omega]^2 converted to a quaternion, as the algorithm states it;
    above, the closed forms (the rotation's quaternion directly from the half angle)."""
    w, v = x[:3], x[3:]
    th = math.sqrt(float(w @ w))
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    O2 = O @ O
    if th < 1e-5:
        R = np.eye(3) + O + O2
        V = R
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        assert tr > 0
        s = math.sqrt(tr + 1.0)
        eq = np.array([(R[2, 1] - R[1, 2]) * 0.5 / s, (R[0, 2] - R[2, 0]) * 0.5 / s, (R[1, 0] - R[0, 1]) * 0.5 / s,
                       0.5 * s])
    else:
        sh = math.sin(0.5 * th)
        b = 2 * sh * sh / (th * th)  # (1 - cos th) / th^2 without the cancellation
        c = (th - math.sin(th)) / (th * th * th)
        V = np.eye(3) + b * O + c * O2
        eq = np.concatenate([w * (sh / th), [math.cos(0.5 * th)]])
    eq = _normalized(eq)
    return _normalized(_qmul(eq, q)), V @ v + _rotmat(eq) @ t


def _linearise(q, t, X, uv, info, f, cx, cy, huber):
    """H (6x6), b (6), robust chi2, and per edge |e|^2 and the depth, at pose (q, t)."""
    xc = X @ _rotmat(q).T + t
    z = xc[:, 2]
    with np.errstate(all="ignore"):
        xi, yi = xc[:, 0] / z, xc[:, 1] / z
        e = uv - np.stack([f * xi + cx, f * yi + cy], axis=1)
        ss = (e * e).sum(1)
        chi2 = info * ss
        inl = chi2 <= huber * huber
        sq = np.sqrt(chi2)
        rho0 = np.where(inl, chi2, 2 * sq * huber - huber * huber)
        rho1 = np.where(inl, 1.0, huber / np.where(inl, 1.0, sq))
        fi = f / z
        zero = np.zeros_like(z)
        J = np.stack([np.stack([xi * yi * f, -(1 + xi * xi) * f, yi * f, -fi, zero, xi * fi], axis=1),
                      np.stack([(1 + yi * yi) * f, -xi * yi * f, -xi * f, zero, -fi, yi * fi], axis=1)], axis=1)
        wgt = rho1 * info
        H = np.einsum("e,eki,ekj->ij", wgt, J, J)
        b = -np.einsum("e,eki,ek->i", wgt, J, e)
    return H, b, float(rho0.sum()), ss, z


def _solve(A, b):
    """(ok, x): ok as a Cholesky factorisation decides it (every pivot positive); x by LU with two
    rounds of refinement on a long-double residual."""
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, None
    x = np.linalg.solve(A, b)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(2):
        x = x + np.linalg.solve(A, (bl - Al @ x.astype(np.longdouble)).astype(np.float64))
    return True, x


@dataclasses.dataclass
class PoseRef:
    q: np.ndarray  # (K, 4) fp64 state (x, y, z, w)
    t: np.ndarray  # (K, 3)
    outlier: np.ndarray  # (E,) u8
    mean_sq: np.ndarray  # (K,) fp64, NaN where no edge is kept
    stats: np.ndarray  # (K, 2) u32 iterations, trials
    m_rho: np.ndarray  # (K,) the three decision margins
    m_ss: np.ndarray
    m_z: np.ndarray
    cheir_only: np.ndarray  # (E,) bool: flagged by z <= 0 alone (ss <= maxErrorSquare)
    front_moved: np.ndarray  # (E,) bool: ss <= maxErrorSquare and sign(z) differs between first and final pose
    front_moved_last: np.ndarray  # (E,) bool: the same between the final pose and the accepted one before it
    failed_solve: np.ndarray  # (K,) bool: some trial's Cholesky failed
    last_accepted: np.ndarray  # (K,) bool: the last evaluated trial was accepted (True if none ran)
    edge_problem: np.ndarray  # (E,) problem of each observation
    # the last successfully solved trial (the only one in a one-trial case)
    x: np.ndarray  # (K, 6), NaN if none
    cond: np.ndarray  # (K,) cond2(H + lambda I)
    q_before: np.ndarray  # (K, 4) pose that trial started from
    t_before: np.ndarray

    @property
    def fragile(self):
        return (self.m_rho < FRAGILE) | (self.m_ss < FRAGILE) | (self.m_z < FRAGILE)

    @property
    def qt7(self):
        return np.concatenate([self.q, self.t], axis=1)


def _reference_problem(r9, pos, intr, X, uv, info, nsteps, huber, maxe):
    q = _normalized(_quat_f32(r9).astype(np.float64))
    t = np.asarray(pos, np.float32).astype(np.float64)
    cx, cy, f = (float(v) for v in intr[:3])
    E = len(X)
    x = np.zeros(6)
    ss_last = np.zeros(E)
    lam, ni = 0.0, 2.0
    iters = trials = 0
    m_rho = math.inf
    failed = False
    last_accepted = True
    rec = dict(x=np.full(6, np.nan), cond=math.nan, q_before=q, t_before=t)
    lin = None
    depth = lambda q, t: (X @ _rotmat(q).T + t)[:, 2] if E else np.zeros(0)  # noqa: E731
    z_first = z_prev = depth(q, t)
    with np.errstate(all="ignore"):
        for step in range(nsteps if E > 0 else 0):
            if step == 0:
                lin = _linearise(q, t, X, uv, info, f, cx, cy, huber)
                lam = 1e-5 * float(np.abs(np.diag(lin[0])).max())
                ni = 2.0
            H, b, current_chi = lin[0], lin[1], lin[2]
            rho, qmax = 0.0, 0
            while True:
                A = H + lam * np.eye(6)
                ok, xs = _solve(A, b)
                if ok:
                    x = xs
                    rec = dict(x=x, cond=float(np.linalg.cond(A)), q_before=q, t_before=t)
                else:
                    failed = True
                tq, tt = oplus(q, t, x)
                scale = float(x @ (lam * x + b)) + 1e-3
                trial = _linearise(tq, tt, X, uv, info, f, cx, cy, huber)
                ss_last = trial[3]
                temp_chi = trial[2]
                if ok:
                    m = abs(current_chi - temp_chi)
                    m_rho = min(m_rho, m / abs(current_chi) if current_chi != 0 else (math.inf if m else 0.0))
                else:
                    temp_chi = DBL_MAX
                rho = float((np.float64(current_chi) - np.float64(temp_chi)) / np.float64(scale))
                trials += 1
                last_accepted = rho > 0 and math.isfinite(temp_chi)
                if last_accepted:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    z_prev = depth(q, t)
                    q, t, lin, current_chi = tq, tt, trial, temp_chi
                else:
                    lam *= ni
                    ni *= 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            iters += 1
            if qmax == 10 or rho == 0 or not math.isfinite(lam):
                break
    z = depth(q, t)
    small = ss_last <= maxe
    out = (z <= 0) | (ss_last > maxe)
    keep = ~out
    mean = float(ss_last[keep].mean()) if keep.any() else math.nan
    m_ss = float((np.abs(ss_last - maxe) / maxe).min()) if (E and maxe != 0) else math.inf
    m_z = float(np.abs(z).min()) if E else math.inf
    return dict(q=q, t=t, outlier=out.astype(np.uint8), mean_sq=mean, stats=(iters, trials), m_rho=m_rho, m_ss=m_ss,
                m_z=m_z, cheir_only=(z <= 0) & small, front_moved=((z_first > 0) != (z > 0)) & small,
                front_moved_last=((z_prev > 0) != (z > 0)) & small, failed_solve=failed, last_accepted=last_accepted,
                **rec)


def reference(pb, nsteps, huber, max_error_square) -> PoseRef:
    """Pose-only StepBundleAdjustment(nsteps x huber, max_error_square) of every problem of `pb`;
    the two widths rounded to float32 first, as the C ABI receives them."""
    huber = float(np.float32(huber))
    maxe = float(np.float32(max_error_square))
    K = len(pb.pos)
    X, uv, info = pb.points.astype(np.float64), pb.uv.astype(np.float64), pb.info.astype(np.float64)
    rs = []
    for k in range(K):
        s = slice(int(pb.obs_start[k]), int(pb.obs_start[k + 1]))
        rs.append(_reference_problem(pb.r9[k], pb.pos[k], pb.intr[k].astype(np.float64), X[s], uv[s], info[s], nsteps,
                                     huber, maxe))
    col = lambda n, **kw: np.array([r[n] for r in rs], **kw)  # noqa: E731
    cat = lambda n: np.concatenate([r[n] for r in rs]) if rs else np.zeros(0)  # noqa: E731
    return PoseRef(q=col("q"), t=col("t"), outlier=cat("outlier").astype(np.uint8), mean_sq=col("mean_sq"),
                   stats=col("stats", dtype=np.uint32).reshape(K, 2), m_rho=col("m_rho"), m_ss=col("m_ss"),
                   m_z=col("m_z"), cheir_only=cat("cheir_only").astype(bool), front_moved=cat("front_moved").astype(bool),
                   front_moved_last=cat("front_moved_last").astype(bool), failed_solve=col("failed_solve"),
                   last_accepted=col("last_accepted"), edge_problem=_problem_of_edge(pb.obs_start), x=col("x"),
                   cond=col("cond"), q_before=col("q_before"), t_before=col("t_before"))


def get_pose(q, t):
    """(pos (K, 3), r9 (K, 9) column-major) in float32 from the fp64 state, as GetPose converts it:
    t rounded, R of the normalised quaternion rounded."""
    q = q / np.sqrt((q * q).sum(1))[:, None]
    r9 = np.stack([_rotmat(qk).T.reshape(9) for qk in q]) if len(q) else np.zeros((0, 9))
    return t.astype(np.float32), r9.astype(np.float32)


def mutated_qt7(ref: PoseRef, rel=1e-7):
    """The one-trial reference with the largest component of every problem's x scaled by 1 + rel:
    the 'slightly wrong step' that Levenberg-Marquardt forgives and the comparison must not."""
    out = np.empty((len(ref.q), 7))
    for k in range(len(ref.q)):
        x = ref.x[k].copy()
        x[int(np.argmax(np.abs(x)))] *= 1.0 + rel
        q, t = oplus(ref.q_before[k], ref.t_before[k], x)
        out[k] = np.concatenate([q, t])
    return out


# ------------------------------------------------------------------------------------------
# comparisons
# ------------------------------------------------------------------------------------------
def pose_distance(qt7, ref: PoseRef):
    """Per problem: the largest absolute difference in q (sign-aligned) and in t."""
    qt7 = np.asarray(qt7, np.float64).reshape(-1, 7)
    s = np.where(np.sum(qt7[:, :4] * ref.q, axis=1) < 0, -1.0, 1.0)[:, None]
    return np.maximum(np.abs(s * qt7[:, :4] - ref.q).max(1), np.abs(qt7[:, 4:] - ref.t).max(1))


def check_decisions(got, ref: PoseRef):
    """`got` (a dict as OptimizeCameraPoses / oracle.pose_batch return it) takes every decision as
    the reference does on its non-fragile problems: stats, outlier flags and the NaN positions of
    mean_sq are equal."""
    ok = ~ref.fragile
    stats = np.asarray(got["stats"]).reshape(-1, 2)
    bad = np.flatnonzero(ok & (stats != ref.stats).any(1))
    assert len(bad) == 0, f"stats differ in problems {bad[:8]}: {stats[bad[:8]].tolist()} vs {ref.stats[bad[:8]].tolist()}"
    eok = ok[ref.edge_problem]
    outl = np.asarray(got["outlier"]).reshape(-1)
    assert outl.shape == ref.outlier.shape
    bad = np.flatnonzero(eok & (outl != ref.outlier))
    assert len(bad) == 0, f"{len(bad)} outlier flags differ, first in problems {np.unique(ref.edge_problem[bad])[:8]}"
    bad = np.flatnonzero(ok & (np.isnan(got["mean_sq"]) != np.isnan(ref.mean_sq)))
    assert len(bad) == 0, f"mean_sq NaN positions differ in problems {bad[:8]}"


def one_trial_tol(ref: PoseRef, k):
    """Per problem K eps (cond2(H + lambda I) max|x| + max(1, max|t|))."""
    return k * EPS * (ref.cond * np.abs(ref.x).max(1) + np.maximum(1.0, np.abs(ref.t).max(1)))


def _ulps32(got, want):
    """|got - want| in units of want's float32 spacing; 0 where both are NaN or equal."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    with np.errstate(all="ignore"):
        u = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return np.where((got == want) | (np.isnan(got) & np.isnan(want)), 0.0, u)


def check_outputs(got, cid, k_one_trial, label):
    """The whole comparison of one implementation's output `got` with the reference of case `cid`:
    decisions, float32 outputs to 2 ulp and the fp64 state to the case's tolerance (one-trial
    cases: one_trial_tol at k_one_trial; multi-step cases: multi_step_tol) on the non-fragile
    problems; on fragile ones only that the outputs are finite or NaN where the reference's are and
    that trials >= iterations.  Prints every figure before it asserts; returns them."""
    ref = case(cid)[4]
    ok = ~ref.fragile
    stats = np.asarray(got["stats"]).reshape(-1, 2)
    qt7 = np.asarray(got["qt7"]).reshape(-1, 7)
    one = cid in ONE_TRIAL_IDS
    tol = one_trial_tol(ref, k_one_trial) if one else np.full(len(ok), multi_step_tol(cid))
    dist = pose_distance(qt7, ref)
    pos32, r932 = get_pose(ref.q, ref.t)
    with np.errstate(all="ignore"):
        fig = dict(
            fragile=int((~ok).sum()),
            dist=float(dist[ok].max(initial=0.0)), ratio=float((dist / tol)[ok].max(initial=0.0)),
            mean_ulp=float(_ulps32(got["mean_sq"], ref.mean_sq.astype(np.float32))[ok].max(initial=0.0)),
            pos_ulp=float(_ulps32(got["pos"], pos32).max(1)[ok].max(initial=0.0)),
            r9_ulp=float(_ulps32(got["r9"], r932).max(1)[ok].max(initial=0.0)))
    if one:
        fig["ratio_k1"] = fig["ratio"] * k_one_trial
    print(f"{label} {cid}: " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()))
    check_decisions(got, ref)
    assert np.isfinite(qt7).all()
    assert np.array_equal(np.isnan(got["mean_sq"]), np.isnan(ref.mean_sq))
    assert np.array_equal(np.isfinite(got["pos"]), np.isfinite(pos32))
    assert np.array_equal(np.isfinite(got["r9"]), np.isfinite(r932))
    assert (stats[:, 1] >= stats[:, 0]).all()
    assert fig["ratio"] <= 1.0, f"fp64 state {fig['dist']:.3g} from the reference, {fig['ratio']:.3g} x the tolerance"
    assert fig["mean_ulp"] <= 2 and fig["pos_ulp"] <= 2 and fig["r9_ulp"] <= 2, fig
    return fig


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
SEED_PERTURB, SEED_BEHIND, SEED_INTR, SEED_GRAZING = 5, 7, 9, 11


def _far(problems=256, obs=48):
    return perturb(synth.pose_batch(problems=problems, obs=obs), 45, 2.0, SEED_PERTURB)


def _count(n):
    pb = synth.pose_batch(problems=3, obs=n, vary=False)
    return behind(perturb(pb, 25, 1.0, SEED_PERTURB), 0.1, SEED_BEHIND)


def _mixed():
    parts = [synth.pose_batch(problems=1, obs=n, vary=False, seed=synth.BA_SEED + 10 + i)
             for i, n in enumerate((0, 1, 257, 2048, 2049))]
    return behind(concat(parts), 0.1, SEED_BEHIND)


def _cases():
    c = {
        "far-3": (_far, 3, 4.0, 36.0),
        "far-behind-4": (lambda: behind(_far(), 0.15, SEED_BEHIND), 4, 0.9, 4.5 ** 2),
        "mid-intr": (lambda: vary_intrinsics(perturb(synth.pose_batch(problems=64, obs=48), 25, 1.0, SEED_PERTURB),
                                             SEED_INTR), 3, 4.0, 36.0),
        "zero-info-behind": (lambda: behind(zero_info(synth.pose_batch(problems=256, obs=48)), 0.15, SEED_BEHIND),
                             3, 4.0, 36.0),
        "huber-0": (lambda: synth.pose_batch(problems=64, obs=60), 3, 0.0, 36.0),
        "maxe-0": (lambda: perturb(synth.pose_batch(problems=64, obs=60), 10, 0.5, SEED_PERTURB), 3, 4.0, 0.0),
    }
    for n in (1, 2, 3, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 2305):
        c[f"count-{n}"] = (functools.partial(_count, n), 3, 4.0, 36.0)
    c["mixed"] = (_mixed, 3, 4.0, 36.0)
    c["many"] = (lambda: perturb(synth.pose_batch(problems=520, obs=8), 10, 0.5, SEED_PERTURB), 3, 4.0, 36.0)
    # the cheirality bits of the kernel's post-pass (front of the last pass against front_cur): many
    # kept edges change sides between the first, the second-last and the final pose
    c["grazing-2"] = (lambda: grazing(synth.pose_batch(problems=64, obs=48), 0.25, SEED_GRAZING), 2, 4.0, NO_OUTLIERS)
    c["one-trial-grazing"] = (lambda: grazing(synth.pose_batch(problems=64, obs=48), 0.25, SEED_GRAZING), 1, 4.0,
                              NO_OUTLIERS)
    c["one-trial-benign"] =(lambda: synth.pose_batch(problems=64, obs=48), 1, 4.0, NO_OUTLIERS)
    c["one-trial-far"] = (lambda: _far(problems=64), 1, 0.9, NO_OUTLIERS)
    for n in (1, 2, 3):
        c[f"one-trial-obs{n}"] = (
            lambda n=n: perturb(synth.pose_batch(problems=32, obs=n, vary=False), 10, 0.5, SEED_PERTURB), 1, 4.0,
            NO_OUTLIERS)
    return c


CASES = _cases()  # id -> (builder, nsteps, huber, maxErrorSquare)
CASE_IDS = list(CASES)
ONE_TRIAL_IDS = [c for c in CASE_IDS if c.startswith("one-trial-")]
MULTI_STEP_IDS = [c for c in CASE_IDS if c not in ONE_TRIAL_IDS]
BEHIND_IDS = ["far-behind-4", "zero-info-behind", "mixed"] + [c for c in CASE_IDS if c.startswith("count-")]


@functools.lru_cache(maxsize=None)
def case(cid):
    """(batch, nsteps, huber, maxErrorSquare, PoseRef) of one case; computed once per process,
    treat as read-only."""
    build, nsteps, huber, maxe = CASES[cid]
    pb = build()
    return pb, nsteps, huber, maxe, reference(pb, nsteps, huber, maxe)


@functools.lru_cache(maxsize=None)
def oracle_run(cid):
    """The CPU oracle's output of one case; computed once per process, treat as read-only."""
    from oracle import oracle as O

    pb, nsteps, huber, maxe, _ = case(cid)
    return O.pose_batch(pb, nsteps, huber, maxe)


def d_oracle(cid):
    """The oracle's pose distance from the reference over the non-fragile problems of a case."""
    ref = case(cid)[4]
    d = pose_distance(oracle_run(cid)["qt7"], ref)[~ref.fragile]
    return float(d.max()) if len(d) else 0.0


def multi_step_tol(cid):
    return max(MULTI_FLOOR, MULTI_FACTOR * d_oracle(cid))
