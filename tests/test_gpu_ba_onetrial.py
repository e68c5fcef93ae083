"""GPU: one Levenberg-Marquardt trial of local BA with tethers, with fixed points and on edge
lists with code paths of their own, against the dense fp64 reference of tests/ba_cases.py (TCASES).

Transform tethers (analytic Jacobians), points_fixed and the plain-graph cases are held to
state_tol = 4 eps (cond2(S) max|dx| + max|state|), the tolerance of
test_gpu_ba_large.test_one_trial_matches_dense_reference.  Cases with distance or rotation tethers,
whose Jacobians are 1e-9 difference quotients by specification, are held to state_tol + F d_fd
against a reference with Richardson-extrapolated Jacobians (ba_cases' docstring).  The CPU side of
the comparison, its preconditions and the mutations it rejects are in test_ba_dense_reference.py.
"""
import numpy as np
import pytest

from mageslam_amd import bundler
from tests import ba_cases as B

pytestmark = pytest.mark.gpu


def gpu_instance(t):
    gb = bundler.BundlerLib(bundler.BundlerParameters(t.points_fixed))
    gb.set_graph(t.g)
    if t.tethers is not None:
        gb.set_tethers(t.tethers)
    return gb


@pytest.mark.parametrize("cid", B.TCASE_IDS)
def test_one_trial_matches_dense_reference(gpu, cid):
    t = B.tcase(cid)
    gb = gpu_instance(t)
    s0 = B.make_oracle(t.g, t.tethers, t.points_fixed).state()
    assert B.state_diff(gb.state(), s0) <= 4 * B.EPS * max(np.abs(s0[0]).max(), np.abs(s0[1]).max())
    gb.SetCurrentLambda(t.lam)
    _, out = gb.step([t.huber], B.MAX_ERR)
    diff = B.state_diff(gb.state(), t.ref)
    print(f"{cid}: cond(S) {t.d.cond_S:.3g} state_tol {t.tight:.3g} d_fd {t.d_fd:.3g} tol {t.tol:.3g} "
          f"gpu-dense {diff:.3g} ratio to tol {diff / t.tol:.4f}"
          + (f" ratio to d_fd {diff / t.d_fd:.3f}" if t.d_fd else f" ratio to K=1 {B.TOL_K * diff / t.tol:.4f}"))
    st = gb.stats()
    assert st["iterations"] == 1 and st["trials"] == 1 and st["rejected"] == 0
    assert len(out) == 0
    assert diff <= t.tol


@pytest.mark.parametrize("cid", ["tr-mixed", "all-kinds"])
def test_two_runs_agree_bitwise(gpu, cid):
    """The tether blocks are added without floating-point atomics: two fresh instances give the
    same bits after three steps."""
    t = B.tcase(cid)
    runs = []
    for _ in range(2):
        gb = gpu_instance(t)
        outs = [gb.step([1.8], 7.25 * 0.9025 ** k)[1] for k in range(3)]
        runs.append((gb.state(), outs))
    (sa, oa), (sb, ob) = runs
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
    assert gb.stats()["iterations"] == 3
