"""The CPU oracle's pose-only StepBundleAdjustment against an independent formulation: the plain
fp64 NumPy reference of tests/pose_cases.py, on inputs that reach the Levenberg-Marquardt branches
synth.pose_batch alone never does (rejected trials, failed solves, the qmax == 10 exit, points
behind the camera, per-problem intrinsics).  No GPU needed; test_gpu_pose.py runs the same
comparison on the kernel.  The coverage assertions here are made on the reference alone and keep
the case table from rotting: a case that no longer reaches its branch fails here, not silently.
"""
import numpy as np
import pytest

from mageslam_amd import synth
from tests import pose_cases as P

# cap on the oracle's own distance from the reference in the multi-step cases.  The GPU tolerance is
# derived from it (100 x), so this keeps that tolerance at or below 1e-7, a thousand times tighter
# than test_gpu_ba's POSE_TOL, whatever a future oracle does.  Measured: 3e-11 at most.
D_ORACLE_CAP = 1e-9


@pytest.mark.parametrize("cid", P.CASE_IDS)
def test_oracle_matches_reference(oracle, cid):
    """Decisions equal, float32 outputs within 2 ulp, fp64 state within K = 4 of the one-trial unit
    (one-trial cases) or within the multi-step tolerance, which for the oracle itself is trivially
    met and is capped instead."""
    o = P.oracle_run(cid)
    print(f"{cid}: d_oracle {P.d_oracle(cid):.3g}")
    assert P.d_oracle(cid) <= D_ORACLE_CAP
    P.check_outputs(o, cid, P.K_ORACLE, "oracle")


@pytest.mark.parametrize("cid", P.CASE_IDS)
def test_fragile_share(cid):
    ref = P.case(cid)[4]
    n = int(ref.fragile.sum())
    print(f"{cid}: {n} of {len(ref.fragile)} problems fragile")
    assert n <= P.MAX_FRAGILE_SHARE * len(ref.fragile)


def _rejected(ref):
    return int((ref.stats[:, 1] > ref.stats[:, 0]).sum())


def test_cases_reach_their_branches():
    for cid in ("far-3", "far-behind-4"):
        assert _rejected(P.case(cid)[4]) >= 10, cid
    assert _rejected(P.case("mid-intr")[4]) >= 1
    for cid in ("zero-info-behind", "huber-0"):
        ref = P.case(cid)[4]
        assert np.array_equal(ref.stats, np.tile(np.array([1, 10], np.uint32), (len(ref.stats), 1))), cid
        # ten failed solves, the last evaluated trial rejected: the 30 / 31 sums of the kernel
        assert ref.failed_solve.all() and not ref.last_accepted.any(), cid
    for cid in P.BEHIND_IDS:
        assert P.case(cid)[4].cheir_only.any(), cid
    ref = P.case("maxe-0")[4]
    assert np.isnan(ref.mean_sq).all() and ref.outlier.all()
    # kept edges that change sides of the camera plane between the first and the final pose (a
    # front_cur that is not refreshed on accept) and between the last two accepted poses (the sums
    # of the "rejected" outcome taken for an accepted last trial), in many problems
    for cid, first, last in (("grazing-2", 50, 5), ("one-trial-grazing", 50, 50)):
        ref = P.case(cid)[4]
        assert ref.front_moved.sum() >= first and ref.front_moved_last.sum() >= last, cid
        assert len(np.unique(ref.edge_problem[ref.front_moved])) >= 16, cid
        assert not ref.outlier.all() and not np.isnan(ref.mean_sq).any(), cid
    # staged and unstaged workgroups in one launch, and a problem without observations
    counts = np.diff(P.case("mixed")[0].obs_start.astype(np.int64))
    assert counts.tolist() == [0, 1, 257, 2048, 2049]
    assert P.case("mixed")[4].stats[0].tolist() == [0, 0] and np.isnan(P.case("mixed")[4].mean_sq[0])
    assert len(P.case("many")[0].pos) >= 512
    # per-problem intrinsics really differ
    assert len(np.unique(P.case("mid-intr")[0].intr, axis=0)) == 64
    # the perturbed starts reach Eigen's non-positive-trace branch of the float32 conversion
    r9 = P.case("far-3")[0].r9
    assert (r9[:, 0] + r9[:, 4] + r9[:, 8] <= 0).any()


@pytest.mark.parametrize("cid", P.ONE_TRIAL_IDS)
def test_one_trial_cases_take_one_accepted_step(cid):
    """The one-trial tolerance describes exp(x) * T0 for the one solve that was accepted: one
    iteration, no failed solve, the last trial accepted (rejected trials before it leave T0)."""
    pb, _, _, _, ref = P.case(cid)
    assert (ref.stats[:, 0] == 1).all() and ref.last_accepted.all() and not ref.failed_solve.any()
    assert np.isfinite(ref.cond).all() and np.isfinite(ref.x).all()
    q0 = np.stack([P._normalized(P._quat_f32(r).astype(np.float64)) for r in pb.r9])
    assert np.array_equal(ref.q_before, q0) and np.array_equal(ref.t_before, pb.pos.astype(np.float64))
    assert np.abs(ref.x).max(1).min() > 1e-4  # every camera really moves


@pytest.mark.parametrize("cid", P.ONE_TRIAL_IDS)
def test_comparison_rejects_a_slightly_wrong_step(cid):
    """Mutation check: the reference with the largest component of x scaled by 1 + 1e-7 must miss
    the one-trial tolerance at the GPU's K = 256 in every problem, while test_gpu_ba's 1e-4 accepts
    it.  A case where it does not is too ill conditioned to test anything."""
    ref = P.case(cid)[4]
    d = P.pose_distance(P.mutated_qt7(ref), ref)
    ratio = d / P.one_trial_tol(ref, P.K_GPU)
    print(f"{cid}: cond up to {ref.cond.max():.3g}, mutation at {ratio.min():.3g} .. {ratio.max():.3g} x the K = 256 bound")
    assert d.max() < 1e-4
    assert (ratio > 1).all()


def _copy(o):
    return {k: v.copy() for k, v in o.items()}


def test_comparison_rejects_a_flipped_decision(oracle):
    cid = "far-behind-4"
    ref = P.case(cid)[4]
    o = P.oracle_run(cid)
    P.check_decisions(o, ref)
    flip = _copy(o)
    flip["outlier"][len(flip["outlier"]) // 2] ^= 1
    with pytest.raises(AssertionError, match="outlier"):
        P.check_decisions(flip, ref)
    bump = _copy(o)
    bump["stats"][7, 1] += 1
    with pytest.raises(AssertionError, match="stats"):
        P.check_decisions(bump, ref)
    nan = _copy(o)
    k = int(np.flatnonzero(~np.isnan(o["mean_sq"]))[0])
    nan["mean_sq"][k] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        P.check_decisions(nan, ref)
    # and the value checks: one float32 output 3 ulp away, one fp64 component 1e-8 away
    off = _copy(o)
    off["pos"][3, 1] = np.nextafter(np.nextafter(np.nextafter(off["pos"][3, 1], np.float32(np.inf)), np.float32(np.inf)),
                                    np.float32(np.inf))
    with pytest.raises(AssertionError):
        P.check_outputs(off, cid, P.K_ORACLE, "mutated")
    off = _copy(o)
    off["qt7"][3, 5] += 1e-8
    with pytest.raises(AssertionError, match="tolerance"):
        P.check_outputs(off, cid, P.K_ORACLE, "mutated")


def test_input_transformations():
    pb = synth.pose_batch(problems=5, obs=30)
    pe = P._problem_of_edge(pb.obs_start)

    def project(b, R, t):
        xc = np.einsum("eij,ej->ei", R[pe], b.points.astype(np.float64)) + t[pe]
        f, c = b.intr[pe, 2:3].astype(np.float64), b.intr[pe, :2].astype(np.float64)
        return f * xc[:, :2] / xc[:, 2:3] + c, xc[:, 2]

    uv0, z0 = project(pb, pb.true_rot, pb.true_pos)
    assert (z0 > 0).all()
    bh = P.behind(pb, 0.2, 3)
    uv1, z1 = project(bh, pb.true_rot, pb.true_pos)
    moved = (bh.points != pb.points).any(1)
    assert np.array_equal(np.bincount(pe[moved], minlength=5), np.ceil(0.2 * np.diff(pb.obs_start.astype(np.int64))))
    assert (z1[moved] < 0).all() and np.array_equal(z1[~moved], z0[~moved])
    assert np.abs(uv1 - uv0).max() < 1e-2  # the same pixel (float32 points)
    vi = P.vary_intrinsics(pb, 4)
    uv2, _ = project(vi, pb.true_rot, pb.true_pos)
    a = vi.intr[:, 2].astype(np.float64) / pb.intr[:, 2]
    # the residuals scale with the focal length: the same geometry through another camera
    assert np.allclose(uv2 - vi.uv, a[pe, None] * (uv0 - pb.uv), atol=2e-3)
    assert (vi.intr[:, 2] == vi.intr[:, 3]).all() and len(np.unique(vi.intr[:, 0])) == 5
    pt = P.perturb(pb, 20, 0.5, 6)
    for k in range(5):
        R = pt.r9[k].astype(np.float64).reshape(3, 3).T
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6
    rot = lambda b: b.r9.reshape(-1, 3, 3).transpose(0, 2, 1).astype(np.float64)  # noqa: E731
    trace = np.einsum("kij,kij->k", rot(pt), rot(pb))  # tr(R1 R0^T)
    assert np.arccos(np.clip((trace - 1) / 2, -1, 1)).min() > np.deg2rad(2) and np.abs(pt.pos - pb.pos).max() > 0.1
    zi = P.zero_info(pb)
    assert zi.info.dtype == np.float32 and not zi.info.any() and zi.uv is pb.uv
    gz = P.grazing(pb, 0.25, 8)
    uv3, z3 = project(gz, pb.true_rot, pb.true_pos)
    moved = gz.info == np.float32(P.GRAZING_INFO)
    assert np.array_equal(np.bincount(pe[moved], minlength=5), np.ceil(0.25 * np.diff(pb.obs_start.astype(np.int64))))
    assert (np.abs(z3[moved]) > 0.004).all() and (np.abs(z3[moved]) < 0.051).all()
    assert (z3[moved] < 0).any() and (z3[moved] > 0).any()
    assert np.array_equal(gz.points[~moved], pb.points[~moved]) and np.array_equal(gz.uv[~moved], pb.uv[~moved])
    for b in (bh, vi, pt, zi, gz):
        assert all(getattr(b, f).dtype == np.float32 for f in ("pos", "r9", "intr", "points", "uv", "info"))
    cc = P.concat([pb, bh])
    assert len(cc.pos) == 10 and cc.obs_start[-1] == 2 * pb.obs_start[-1] and cc.obs_start.dtype == np.uint32


def test_pose_distance_aligns_quaternion_signs():
    ref = P.case("one-trial-obs3")[4]
    qt = ref.qt7
    qt[1, :4] *= -1
    assert P.pose_distance(qt, ref).max() == 0.0
    qt[2, 5] += 1e-9
    assert abs(P.pose_distance(qt, ref)[2] - 1e-9) < 1e-15
