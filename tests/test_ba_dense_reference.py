"""The CPU oracle's Schur complement and dense solve against an independent formulation: one
Levenberg-Marquardt trial of every case of tests/ba_cases.py, solved as the full unreduced system
(H + lambda I) x = b in float64 with iterative refinement (ba_cases.dense_lm_step), must predict the
oracle's state to within state_tol = 4 eps (cond2(S) max|dx| + max|state|).  No GPU needed; the GPU
runs the same comparison in test_gpu_ba_large.py, and the preconditions asserted here (the trial is
accepted, nothing is removed, the Huber cases really are robustified) are what keeps that test from
passing for the wrong reason.
"""
import numpy as np
import pytest

from tests import ba_cases as B
from tests.test_gpu_ba import compare


@pytest.mark.parametrize("cid", B.CASE_IDS)
def test_oracle_matches_dense_reference(cid):
    g, lam, huber, d = B.case(cid)
    ob, out = B.oracle_one_trial(g, lam, huber)
    st = ob.stats()
    # the state is x0 (+) dx only if the one trial was accepted and nothing left the graph
    assert st["iterations"] == 1 and st["trials"] == 1 and st["rejected"] == 0
    assert len(out) == 0
    free = int((g.fixed == 0).sum())
    assert len(d.cams) == free and len(d.pts) == len(g.points)  # every free camera and point is in the system
    if huber < B.NO_HUBER:
        assert d.robust_frac > 0.5
    else:
        assert d.robust_frac == 0.0
    ref = (d.qt, d.xyz)
    diff, tol = B.state_diff(ob.state(), ref), B.state_tol(d.x, d.cond_S, ref)
    print(f"{cid}: cond(S) {d.cond_S:.3g} tol {tol:.3g} oracle-dense {diff:.3g} ratio to K=1 {B.TOL_K * diff / tol:.4f}")
    assert diff <= tol
    assert np.abs(d.x[:6 * free]).max() > 1e-4  # the cameras really move: the comparison is not of x0 with x0


class _State:
    """A fixed (qt, xyz) state behind the .state() that test_gpu_ba.compare reads."""

    def __init__(self, s):
        self._s = s

    def state(self):
        return self._s


# The cases in which the (1 + 1e-7) mutation lies inside state_tol, with the measured
# state_diff / state_tol.  The bound is 4 eps cond2(S) max|dx| with the maximum over all unknowns,
# so a relative change d of one camera component c is visible only if
# d > 4 eps cond2(S) max|dx| / |dx_c|: with d = 1e-7 never above cond2(S) = 1.1e8 (the two 96-camera
# banded cases), and below that not where a point moves much further than the mutated camera
# component (max|dx| / |dx_c| between 4 and 17 in the other four).  No choice of component helps
# the first two, so "fails in every case" cannot hold for the K = 4 formula; every other case is
# asserted.
MUTATION_1E7_INSIDE = {
    "banded-96-lam1": 0.57, "banded-96-lam0.001": 0.021, "huber-48-lam0.01": 0.33, "huber-96-lam1": 0.41,
    "permuted-rand-40": 0.49, "permuted-rev-40": 0.49,
}


@pytest.mark.parametrize("cid", B.CASE_IDS)
def test_comparison_rejects_a_slightly_wrong_dx(cid):
    """Mutation check of the one-trial comparison: a reference whose dx has its largest camera
    component scaled by (1 + rel) must miss state_tol, while test_gpu_ba.compare (poses at 1e-4)
    accepts it.  rel = 1e-7 is asserted in the 16 cases where it is detectable (state_diff /
    state_tol between 1.77 and 1650) and shown to lie inside the bound in the 6 of
    MUTATION_1E7_INSIDE; rel = 1e-5 is asserted in all 22."""
    g, lam, huber, d = B.case(cid)
    ob, _ = B.oracle_one_trial(g, lam, huber)
    so = ob.state()
    tol = B.state_tol(d.x, d.cond_S, (d.qt, d.xyz))
    for rel in (1e-7, 1e-5):
        mut = B.mutated_reference(g, d, rel)
        compare(_State(so), _State(mut))  # the old net accepts the mutated reference
        ratio = B.state_diff(so, mut) / tol
        if rel == 1e-7 and cid in MUTATION_1E7_INSIDE:
            assert ratio < 1 and abs(ratio / MUTATION_1E7_INSIDE[cid] - 1) < 0.05, ratio
        else:
            assert ratio > 1, (rel, ratio, d.cond_S)


def test_graph_transformations():
    g = B.banded(8)
    perm = np.random.default_rng(1).permutation(len(g.pos))
    gp = B.permute_cameras(g, perm)
    assert np.array_equal(gp.pos[perm], g.pos) and np.array_equal(gp.fixed[perm], g.fixed)
    assert np.array_equal(gp.rot[gp.cam], g.rot[g.cam]) and np.array_equal(gp.true_pos[gp.cam], g.true_pos[g.cam])
    assert np.array_equal(gp.uv, g.uv) and np.array_equal(gp.pt, g.pt)
    j = B.join_graphs(g, gp)
    assert len(j.pos) == 2 * len(g.pos) and len(j.points) == 2 * len(g.points) and len(j.cam) == 2 * len(g.cam)
    second = j.cam >= len(g.pos)
    assert np.array_equal(second, j.pt >= len(g.points))  # no edge joins the components
    assert np.array_equal(j.pos[j.cam[second]], gp.pos[gp.cam])
    # the permuted cases scatter the fixed cameras; the joined ones put them between free ones
    for cid in ("permuted-rand-40", "permuted-rand-48", "components-20+20"):
        fixed = np.flatnonzero(B.case(cid)[0].fixed)
        assert fixed.max() > len(fixed)


def test_state_diff_aligns_quaternion_signs():
    g, _, _, d = B.case("banded-2-lam1")
    qt = d.qt.copy()
    qt[1, :4] *= -1
    assert B.state_diff((qt, d.xyz), (d.qt, d.xyz)) == 0.0
    qt[2, 5] += 1e-9
    assert abs(B.state_diff((qt, d.xyz), (d.qt, d.xyz)) - 1e-9) < 1e-15
