"""The monocular map initialisation's plain C++ twin (mage_mono_init_two_view_host, the CPU backend
the kernels are byte-compared with in test_gpu_mono_init.py) against independent formulations, no
GPU: (i) the sampler against a Python set with integers and float32 compares, exactly; (ii) every
traced essential matrix against its defining constraints in fp64, and an fp64 solve by another
route whose real solutions must all be present; (iii) every traced score against fp64; (iv) the
decision logic from the twin's own traced numbers, exactly; (v) the selected pose against the
scene's truth and the case table's verdicts.  The tolerances are the measured figures of
tests/mono_init_cases.py; each test prints what it measures."""
import numpy as np
import pytest

from mageslam_amd import mono
from tests import mono_init_cases as mc

CASES = [c for c in mc.cases()]
RAN = [c for c in CASES if c.expect not in (mono.FEW_MATCHES,)]
# The solver and score comparisons need a well-posed two-view problem.  Without a baseline (pure
# rotation) every [t]x R is a solution, and with a baseline of 1/40 of the depth nearly so: the
# solutions of a sample lie on a near-continuum, the fp64 formulation is itself unstable there, and
# which of them a float32 elimination returns is free.  Those two scenes are checked for sampling,
# decision logic, verdict and kernel parity only.
SOLVED = [c for c in RAN if c.name not in ("clustered", "tiny_baseline", "pure_rotation")]
_HOST = {}


def host(c):
    if c.name not in _HOST:
        _HOST[c.name] = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=c.matches,
                                                    backend="host", want_trace=True)
    return _HOST[c.name]


@pytest.mark.parametrize("c", RAN, ids=lambda c: c.name)
def test_sampling(c):
    """(i) FindPossiblePoses' sampler (:196-249): the indices per iteration, exactly."""
    p0, p1 = mc.match_points(c)
    ref = mc.sample_reference(p0, p1, c.settings.ransac_iterations_for_models, c.settings.min_pixel_spread)
    got = host(c).trace["indices"]
    assert np.array_equal(got, ref)
    if c.name == "clustered":
        assert np.all(got == -1)
    if c.name == "eight":
        assert np.all(got >= 0)  # 100 tries always find 5 of 8 when nothing is too close


def _solver_figures(c):
    """Worst residual of a traced E, worst distance of an fp64 solution from the traced set, the
    fragile share: over the case's hypotheses."""
    tr = host(c).trace
    p0, p1 = mc.match_points(c)
    worst_e = worst_root = 0.0
    fragile = hyps = 0
    missing = []
    for it in range(len(tr["indices"])):
        idx = tr["indices"][it]
        if idx[0] < 0:
            assert tr["candidates"][it] == 0
            continue
        hyps += 1
        q1, q2 = mc.normalise(p0[idx], mc.INTR[:4]), mc.normalise(p1[idx], mc.INTR[:4])
        k = int(tr["candidates"][it])
        Es = tr["E"][it, :k].astype(np.float64)
        assert np.all(tr["E"][it, k:] == 0)
        sols, roots, every, amp = mc.five_point_fp64(q1, q2)
        for E in Es:
            assert abs(np.linalg.norm(E) - 1) < 4 * mc.EPS32
            worst_e = max(worst_e, mc.essential_residual(E, q1, q2) / (mc.EPS32 * amp))
        if mc.fragile_hypothesis(roots, every):
            fragile += 1
            continue
        if len(sols) != k:
            missing.append((it, len(sols), k))
            continue
        for S in sols:
            d = min(min(np.abs(E - S).max(), np.abs(E + S).max()) for E in Es)
            worst_root = max(worst_root, d / (mc.EPS32 * amp))
    return worst_e, worst_root, fragile, hyps, missing


@pytest.mark.parametrize("c", SOLVED, ids=lambda c: c.name)
def test_solver(c):
    """(ii) the five-point solver (ComputeEssential.cpp:357-514): every traced E satisfies its
    constraints and every real solution of the fp64 formulation is among them, outside the fragile
    hypotheses.  Both figures are ratios to eps32 times the hypothesis's amplification (see
    mono_init_cases.five_point_fp64).  Measured: residual 1.5-192.2 (outliers128 the worst), solution
    distance 2.8-114.6 (clean128), fragile 0-2 of 90."""
    worst_e, worst_root, fragile, hyps, missing = _solver_figures(c)
    print(f"{c.name}: residual ratio {worst_e:.1f}, fp64 solution distance ratio {worst_root:.1f}, "
          f"fragile {fragile}/{hyps}, count mismatches {missing}")
    assert hyps > 0
    assert fragile <= mc.MAX_FRAGILE_SHARE * hyps
    assert not missing
    assert worst_e <= mc.K_TOL_E
    assert worst_root <= mc.K_TOL_ROOT


@pytest.mark.parametrize("c", SOLVED, ids=lambda c: c.name)
def test_scores(c):
    """(iii) ScoreFundamentalMatrix (:279-322) per traced candidate, re-evaluated in fp64 on the
    traced float32 E: the inlier count equal up to the matches within FRAGILE of the threshold (at
    most MAX_FRAGILE_SHARE of all), the in-order float sum within the measured bound where no match
    is unsure."""
    tr = host(c).trace
    s = c.settings
    p0, p1 = mc.match_points(c)
    n = len(p0)
    f = np.float32
    thr = float(f(s.fundamental_transfer_error_threshold))
    worst = 0.0
    fragile = total = 0
    for it in range(len(tr["indices"])):
        for r in range(int(tr["candidates"][it])):
            inl, margin, t12, t21, bound = mc.score_fp64(tr["E"][it, r], p0, p1, mc.INTR, thr)
            unsure = margin <= mc.FRAGILE
            total += n
            fragile += int(unsure.sum())
            sure = inl & ~unsure
            count = int(tr["inliers"][it, r])
            assert sure.sum() <= count <= sure.sum() + unsure.sum(), (c.name, it, r)
            if unsure.any():
                continue  # the sum depends on which of the unsure matches were taken
            gated = count >= s.min_scoring_inliers and f(count) / f(n) > f(s.min_inlier_percentage)
            if not gated:
                assert tr["score"][it, r] == 0
                continue
            ref = float(t12[inl].sum() + t21[inl].sum())
            scale = float(np.abs(t12[inl]).sum() + np.abs(t21[inl]).sum() + bound[inl].sum())
            worst = max(worst, abs(float(tr["score"][it, r]) - ref) / (mc.EPS32 * scale))
    print(f"{c.name}: score error {worst:.2f} eps32 (sum |terms| + bound), unsure matches {fragile}/{total}")
    assert fragile <= mc.MAX_FRAGILE_SHARE * total
    assert worst <= mc.K_TOL_SUM


@pytest.mark.parametrize("c", RAN, ids=lambda c: c.name)
def test_decision_logic(c):
    """(iv) exact, from the twin's own traced numbers: the winner is the earliest maximum among the
    consistent candidates; FindCorrectPose's verdict follows from its per-pose scores, counts and
    medians; the records are the accepted matches in match order."""
    h = host(c)
    tr, res, s = h.trace, h.result, c.settings
    score, ok = tr["score"].reshape(-1), tr["cheirality"].reshape(-1).astype(bool)
    elig = ok & (score > 0)
    if not elig.any():
        assert h.verdict == mono.NO_HYPOTHESIS and res["win_iteration"] == -1
        return
    best = score[elig].max()
    slot = int(np.flatnonzero(elig & (score == best))[0])
    assert (res["win_iteration"], res["win_root"]) == (slot // 10, slot % 10)
    assert res["win_score"] == best
    assert np.array_equal(res["win_indices"], tr["indices"][slot // 10])
    # the sequential rule of :263-269 gives the same
    run, win = np.float32(0), -1
    for k in range(len(score)):
        if score[k] > run and ok[k]:
            run, win = score[k], k
    assert win == slot
    # FindCorrectPose's bookkeeping (:435-472)
    n = len(c.matches)
    flags, cs, cc, med = res["cand_flags"], res["cand_score"], res["cand_count"], res["cand_median"]
    sel, sel_score, nxt = -1, np.float32(0), np.float32(0)
    for p in range(4):
        if flags[p] & mono.POSE_TWISTED:
            assert cs[p] == 0 and cc[p] == 0
            continue
        enough = cc[p] >= s.min_scoring_inliers and np.float32(cc[p]) / np.float32(n) > np.float32(s.min_inlier_percentage)
        assert bool(flags[p] & mono.POSE_ENOUGH) == bool(enough)
        if not enough:
            continue
        assert bool(flags[p] & mono.POSE_MEDIAN_OK) == bool(med[p] <= np.float32(s.max_parallax_3d_median_distance))
        if not flags[p] & mono.POSE_MEDIAN_OK:
            continue
        if sel == -1 or cs[p] > sel_score:
            nxt, sel_score, sel = sel_score, cs[p], p
        else:
            nxt = max(nxt, cs[p])
    assert res["selected_pose"] == sel and res["next_best_score"] == nxt
    if sel_score <= 0:
        verdict = mono.NO_VALID_POSE
    elif (sel_score - nxt) / sel_score < np.float32(s.min_candidate_pose_disimilarity):
        verdict = mono.TOO_SIMILAR
    else:
        # the selected pose's world-space position z, C = -(R^T t), as make_frame sums it in float32
        f = np.float32
        rt, t = res["cand_r9"][9 * sel + 6: 9 * sel + 9], res["cand_pos3"][3 * sel: 3 * sel + 3]
        cz = -f(f(f(f(0) + f(rt[0] * t[0])) + f(rt[1] * t[1])) + f(rt[2] * t[2]))
        verdict = mono.Z_BIASED if abs(cz) > f(s.max_pose_contribution_z) else mono.OK
    assert h.verdict == verdict
    if verdict != mono.OK:
        assert len(h.points) == 0 and np.array_equal(h.r9[1], np.eye(3).reshape(-1))
        return
    assert np.array_equal(h.pos3[1], res["cand_pos3"][3 * sel: 3 * sel + 3])
    assert np.array_equal(h.r9[1], res["cand_r9"][9 * sel: 9 * sel + 9])
    # the records: accepted matches in match order, count and median as reported
    pts = h.points
    assert len(pts) == cc[sel]
    pos = {(int(m["query_idx"]), int(m["train_idx"])): k for k, m in enumerate(c.matches)}
    order = [pos[(int(p["query_idx"]), int(p["train_idx"]))] for p in pts]
    assert order == sorted(order) and len(set(order)) == len(order)
    assert np.array_equal(pts["distance"], c.matches["distance"][order])
    assert med[sel] == np.sort(pts["position"][:, 2])[len(pts) // 2]
    # the bundle adjustment's inputs: frame-major, as the stereo stage lays them out
    k = len(pts)
    assert np.array_equal(h.ba_points, pts["position"])
    assert np.array_equal(h.ba_cam, np.repeat([0, 1], k)) and np.array_equal(h.ba_pt, np.tile(np.arange(k), 2))
    a, b = c.kp0[pts["query_idx"]], c.kp1[pts["train_idx"]]
    assert np.array_equal(h.ba_uv, np.concatenate([np.stack([a["x"], a["y"]], 1), np.stack([b["x"], b["y"]], 1)]))
    x = np.float32(2.5)
    assert np.all(h.ba_info == np.float32(1) - np.float32(1) / (x * x))


def test_verdicts_and_ground_truth():
    """(v) every expected verdict of the case table; on the clean cases that end in OK every match
    is within the scoring threshold and the selected pose is the scene's, within the measured
    angle."""
    worst = 0.0
    seen = set()
    for c in CASES:
        h = host(c)
        seen.add(h.verdict)
        assert h.status == 0
        if c.expect is not None:
            assert h.verdict == c.expect, (c.name, mono.VERDICT_NAMES[h.verdict])
        if not (c.clean and c.expect == mono.OK):
            continue
        res = h.result
        assert h.trace["inliers"][res["win_iteration"], res["win_root"]] == len(c.matches), c.name
        assert len(h.points) == len(c.matches), c.name
        R = h.r9[1].reshape(3, 3).T
        a_r = mc.rotation_angle_deg(R, c.R)
        a_t = mc.angle_deg(h.pos3[1], c.t)
        print(f"{c.name}: rotation {a_r:.4f} deg, translation direction {a_t:.4f} deg")
        worst = max(worst, a_r, a_t)
        assert abs(np.linalg.norm(h.pos3[1]) - 1) < 1e-5 or res["selected_pose"] == 2
    print(f"worst angle {worst:.4f} deg")
    assert worst <= mc.ANGLE_TOL
    assert {mono.OK, mono.FEW_MATCHES, mono.NO_HYPOTHESIS, mono.NO_VALID_POSE, mono.Z_BIASED} <= seen


def test_over_limit_and_bad_index():
    c = mc.over_limit_case()
    h = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=c.matches, backend="host")
    assert h.status == mono.STATUS_OVER_LIMIT and len(h.points) == 0
    c = mc.case("clean64")
    bad = c.matches.copy()
    bad["train_idx"][5] = len(c.kp1)
    h = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=bad, backend="host")
    assert h.status == mono.STATUS_BAD_INDEX and len(h.points) == 0


def test_settings_are_checked():
    from mageslam_amd._lib import MageError

    c = mc.case("clean64")
    for bad in (dict(ransac_iterations_for_models=257), dict(ransac_iterations_for_models=0),
                dict(min_feature_matches=4), dict(min_pixel_spread=-1.0)):
        s = mono.MonoMapInitializationSettings(**bad)
        with pytest.raises(MageError):
            mono.initialize_with_frames(s, mc.INTR, c.kp0, c.kp1, matches=c.matches, backend="host")
    cs = mono.MonoMapInitializationSettings().to_c()
    cs.struct_size -= 4
    with pytest.raises(MageError):
        mono.initialize_with_frames(cs, mc.INTR, c.kp0, c.kp1, matches=c.matches, backend="host")
