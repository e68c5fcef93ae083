"""mage_reloc_pnp_host (the plain C++ twin of the relocalisation PnP kernels) against the fp64 NumPy
formulation of tests/reloc_pnp_cases.py: the sampler, RANSACUpdateNumIters, the per-hypothesis poses,
the inlier rule, the decisions, the noise-free pose and the adaptive loop's replay.  No GPU."""
import math

import numpy as np
import pytest

from mageslam_amd import _lib, reloc
from mageslam_amd._lib import ptr
from tests import reloc_pnp_cases as rc


def test_verdicts_are_the_cases_purpose():
    want = {"n4": reloc.NO_MODEL, "n5": reloc.OK, "n6": reloc.OK, "mix40_i2": reloc.OK, "mix40_i65": reloc.OK,
            "half300": reloc.OK, "clean40": reloc.OK, "behind60": reloc.OK, "few_inliers": reloc.FEW_INLIERS,
            "few_matches": reloc.FEW_MATCHES}
    for name in rc.NAMES:
        h = rc.twin(name)
        assert h.status == 0 and h.verdict == want[name], name
    # the update ends half300 early, and mix40_i65's 65 iterations are not all run either
    assert int(rc.twin("half300").result["iterations_run"]) < 256
    assert int(rc.twin("n5").result["iterations_run"]) == 1
    # behind60: the filter removes the true points behind the camera, and only those
    c, h = rc.case("behind60"), rc.twin("behind60")
    assert c.behind.sum() == 6 and set(h.inliers) == set(np.flatnonzero(~c.behind))
    assert int(h.result["n_inliers"]) == 60 and int(h.result["n_in_front"]) == 54


@pytest.mark.parametrize("name", rc.RANSAC_NAMES)
def test_sampler(name):
    f, h = rc.formulate(name), rc.twin(name)
    assert np.array_equal(h.trace["indices"], f.indices)


def test_update_num_iters_grid():
    L = _lib.load()
    cases = 0
    for conf in (0.6, 0.9, 0.99):
        for n in range(6, 513):
            out = np.zeros(n + 1, np.int32)
            _lib.check(L.mage_debug_reloc_pnp_update(conf, n, 256, ptr(out)))
            want = [rc.update_num_iters(conf, (n - g) / n, 5, 256) for g in range(5, n + 1)]
            assert out[5:].tolist() == want, (conf, n)
            cases += len(want)
    assert cases == 3 * sum(n - 4 for n in range(6, 513))


def hypotheses(name):
    """(iteration, the formulation's hypothesis) for every sampled iteration, and the fragile share."""
    f = rc.formulate(name)
    hyp = [(it, h) for it, h in enumerate(f.hyp) if h is not None]
    return hyp, sum(h.fragile for _, h in hyp) / len(hyp)


@pytest.mark.parametrize("name", rc.RANSAC_NAMES)
def test_hypothesis_poses(name):
    c, T = rc.case(name), rc.twin(name).trace
    pw, uv = rc.correspondences(c)
    hyp, share = hypotheses(name)
    print(f"{name}: fragile share {share:.4f}")
    assert share <= 0.05
    worst = exact = 0.0
    cx, cy, fx, fy = (float(a) for a in rc.INTR)
    for it, h in hyp:
        if T["solved"][it]:
            # what the twin reports is a pose, and its chosen start's error is that pose's error
            R, t = T["R"][it], T["t"][it]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-9) and abs(np.linalg.det(R) - 1) < 1e-9
            X = pw[T["indices"][it]] @ R.T + t
            q = uv[T["indices"][it]]
            e = np.hypot(q[:, 0] - (cx + fx * X[:, 0] / X[:, 2]), q[:, 1] - (cy + fy * X[:, 1] / X[:, 2])).sum()
            errs = T["err"][it][T["err"][it] >= 0]
            assert abs(errs.min() - e) <= 1e-9 * max(e, 1.0)
        if h.fragile:
            continue
        assert T["solved"][it], (name, it)
        fig = rc.pose_figure(T["R"][it], T["t"][it], h.R, h.t)
        worst = max(worst, fig)
        if h.err.min() < 1e-3:
            exact = max(exact, fig)
    print(f"{name}: worst pose figure {worst:.3g}, over exact-fit samples {exact:.3g}")
    assert worst <= 4 * rc.POSE_FIGURE
    assert exact <= 4 * rc.EXACT_FIT_FIGURE


@pytest.mark.parametrize("name", rc.RANSAC_NAMES)
def test_inlier_rule(name):
    """The twin's counts against the formulation's rule on the twin's own poses (the two differ in the
    poses of outlier-ridden samples, which says nothing about the rule), and the winner's set."""
    c, h = rc.case(name), rc.twin(name)
    T = h.trace
    pw, uv = rc.correspondences(c)
    thr = c.settings.max_bundle_pnp_reprojection_error
    n = len(c.matches)
    for it in range(c.settings.ransac_iterations):
        if not T["solved"][it] or n == 5:
            continue
        mask, e64 = rc.inlier_mask(T["R"][it], T["t"][it], rc.INTR, pw, uv, thr)
        doubt = int((np.abs(e64 - thr * thr) <= 1e-4 * thr * thr).sum())
        assert abs(int(T["inliers"][it]) - int(mask.sum())) <= doubt, (name, it)
    f = rc.formulate(name)
    if f.win >= 0 and int(h.result["win_iteration"]) == f.win:
        sure = np.abs(f.err64[f.win] - thr * thr) > 1e-4 * thr * thr if n > 5 else np.ones(n, bool)
        got = np.zeros(n, bool)
        got[h.inliers] = True
        front = np.zeros(n, bool)
        front[f.kept] = True
        assert np.array_equal(got[sure], front[sure])


def test_decisions():
    left_out = 0
    for name in rc.NAMES:
        f, h = rc.formulate(name), rc.twin(name)
        r = h.result
        if f.hyp is not None and f.win >= 0:
            # a tie through a fragile hypothesis: the winner or the runner-up is fragile and their counts are equal
            order = np.argsort(-f.counts, kind="stable")
            second = int(order[1]) if len(order) > 1 else f.win
            if f.counts[second] == f.counts[f.win] and (f.hyp[f.win].fragile or f.hyp[second].fragile):
                left_out += 1
                continue
        assert h.verdict == f.verdict, name
        assert int(r["win_iteration"]) == f.win and int(r["iterations"]) == f.niters, name
        assert int(r["iterations_run"]) == f.run and int(r["n_in_front"]) == f.n_in_front, name
        if f.kept is not None:
            assert np.array_equal(h.inliers, f.kept), name
            assert np.array_equal(r["win_indices"], f.indices[f.win]), name
    assert left_out == 0


def test_noise_free_pose():
    c, h = rc.case("clean40"), rc.twin("clean40")
    fig = rc.pose_figure(h.r9.reshape(3, 3).T.astype(np.float64), h.pos3.astype(np.float64), c.R, c.t)
    print(f"clean40: winner against the true pose {fig:.3g}")
    assert fig <= 4 * rc.NOISE_FREE_FIGURE
    assert len(h.inliers) == 40 and np.array_equal(h.points3, c.map_xyzi[c.matches["query_idx"], :3])
    assert np.array_equal(h.info, c.map_xyzi[c.matches["query_idx"], 3])
    assert np.array_equal(h.uv[:, 0], c.kp["x"][c.matches["train_idx"]])


def loop(solved, counts, n, conf, sequential):
    out = np.zeros(4, np.int32)
    _lib.check(_lib.load().mage_debug_reloc_pnp_loop(ptr(np.asarray(solved, np.int32)), ptr(np.asarray(counts, np.uint32)),
                                                     len(counts), n, conf, int(sequential), ptr(out)))
    return out.tolist()


def py_loop(solved, counts, n, conf):
    niters, best, win, it = len(counts), 0, -1, 0
    while it < niters:
        if solved[it] and counts[it] > max(best, 4):
            best, win = counts[it], it
            niters = rc.update_num_iters(conf, (n - best) / n, 5, niters)
        it += 1
    return [win, best, niters, it]


@pytest.mark.parametrize("counts, solved", [
    ([7, 7, 7, 7], None),                       # ties: the first wins
    ([6, 9, 9, 3], None),                       # a later equal count does not replace
    ([4, 4, 4], None),                          # a count of exactly 4 is no model
    ([4, 5, 4], None),
    ([30, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 40], None),  # the update stops the loop before a better later hypothesis
    ([12, 40, 3], [0, 1, 1]),                   # an unsolved sample is passed over
    ([40] + [0] * 9, None),                     # every match an inlier: niters drops to 0
    ([5, 6, 7, 8, 9, 10, 11, 12], None),        # every iteration improves
    ([0] * 16, [0] * 16),
])
def test_replay_equals_sequential_loop(counts, solved):
    solved = [1] * len(counts) if solved is None else solved
    for conf in (0.6, 0.99):
        a, b = loop(solved, counts, 40, conf, False), loop(solved, counts, 40, conf, True)
        assert a == b == py_loop(solved, counts, 40, conf), (counts, conf)
    assert loop([1, 1, 1, 1], [7, 7, 7, 7], 40, 0.6, False)[0] == 0
    assert loop([1] * 3, [4, 4, 4], 40, 0.6, False)[0] == -1
    assert loop([1] * 13, [30, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 40], 40, 0.6, False)[:2] == [0, 30]


def test_replay_on_random_sequences():
    rng = np.random.default_rng(5)
    for _ in range(200):
        k = int(rng.integers(1, 257))
        n = int(rng.integers(6, 400))
        counts = rng.integers(0, n + 1, k).tolist()
        solved = (rng.random(k) > 0.2).astype(int).tolist()
        assert loop(solved, counts, n, 0.9, False) == loop(solved, counts, n, 0.9, True) == py_loop(solved, counts, n, 0.9)
