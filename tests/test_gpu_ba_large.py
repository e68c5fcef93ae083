"""GPU: local BA's two dense solvers (chol_tiles up to 40 free cameras, cholesky_solve from 41 to
96) at fp64 accuracy and above 240 unknowns.

(a) One Levenberg-Marquardt trial against the dense reference of tests/ba_cases.py within
    state_tol = 4 eps (cond2(S) max|dx| + max|state|): 1 to 96 free cameras, both sides of the 40/41
    kernel switch, block counts without padding rows, Huber-weighted systems, scattered and
    block-diagonal S, fixed cameras between free ones.  The CPU side of the same comparison and
    its preconditions are in test_ba_dense_reference.py; the same trial with tethers, fixed
    points and odd edge lists is in test_gpu_ba_onetrial.py.
(b) The in-place solver (np > 240: S cleared per trial, factored in place) over several steps with
    rejected trials, speculative linearisation, outlier removal, a camera leaving the system, and one
    instance crossing the switch in both directions; envelope fill from a far off-band block.
(c) The 96-camera limit and the instance's recovery from it.
(d) Bitwise run-to-run determinism on a scattered S for both solvers.
"""
import numpy as np
import pytest

from mageslam_amd import _lib, bundler, synth
from tests import ba_cases as B
from tests.test_gpu_ba import _empty, compare, run_pair

pytestmark = pytest.mark.gpu


# ---- (a) one trial against the dense reference ----------------------------------------------
@pytest.mark.parametrize("cid", B.CASE_IDS)
def test_one_trial_matches_dense_reference(gpu, cid):
    from oracle import oracle as O

    g, lam, huber, d = B.case(cid)
    gb = bundler.BundlerLib()
    gb.set_graph(g)
    ob = O.BundlerOracle()
    ob.set_graph(g)
    s0 = ob.state()
    # the same float32 inputs become the same fp64 state (quaternion of the rotation matrix included)
    assert B.state_diff(gb.state(), s0) <= 4 * B.EPS * max(np.abs(s0[0]).max(), np.abs(s0[1]).max())
    gb.SetCurrentLambda(lam)
    _, out = gb.step([huber], B.MAX_ERR)
    ref = (d.qt, d.xyz)
    diff, tol = B.state_diff(gb.state(), ref), B.state_tol(d.x, d.cond_S, ref)
    print(f"{cid}: cond(S) {d.cond_S:.3g} tol {tol:.3g} gpu-dense {diff:.3g} ratio to K=1 {B.TOL_K * diff / tol:.4f}")
    st = gb.stats()
    assert st["iterations"] == 1 and st["trials"] == 1 and st["rejected"] == 0
    assert len(out) == 0
    assert diff <= tol


# ---- (b) the in-place path over several steps -----------------------------------------------
def same_counts(gb, ob):
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]
    return so


def run_pair_on(monkeypatch, gb, ob, g, steps, **kw):
    """test_gpu_ba.run_pair itself on the existing instances gb / ob: its two constructors hand
    them out for the duration of the call."""
    from oracle import oracle as O

    with monkeypatch.context() as m:
        m.setattr(bundler, "BundlerLib", lambda *a, **k: gb)
        m.setattr(O, "BundlerOracle", lambda *a, **k: ob)
        return run_pair(g, steps, **kw)


@pytest.mark.parametrize("free", [41, 64, 96])
def test_in_place_solver_sizes(gpu, free):
    """np = 256, 384 and 576 (the LDS panel's limit), 3 default steps."""
    g = synth.ba_graph(cameras=free + 2, points=25 * (free + 2), obs_per_point=8, fixed_cameras=2)
    gb, ob = run_pair(g, 3)
    compare(gb, ob)
    same_counts(gb, ob)


@pytest.mark.parametrize("spec", ["1", "0"])
def test_in_place_rejected_trials(gpu, monkeypatch, spec):
    """test_gpu_ba.test_rejected_trials at 48 free cameras: every rejected trial leaves a factor in S
    that the next trial's clear must remove before the Schur products land (with and without the
    speculative linearisation queued behind the decision)."""
    monkeypatch.setenv("MAGE_BA_SPEC_LIN", spec)
    g = synth.ba_graph(cameras=50, points=1200, obs_per_point=8, fixed_cameras=2, seed=5, noise_px=8.0,
                       outlier_frac=0.05)
    gb, ob = run_pair(g, 5, lam=1e-6)
    compare(gb, ob)
    so = same_counts(gb, ob)
    assert so["trials"] > so["iterations"]
    assert abs(gb.GetCurrentLambda() - ob.get_lambda()) <= 1e-3 * abs(ob.get_lambda())


def test_in_place_reference_schedule(gpu):
    """test_gpu_ba.test_reference_schedule_windows' loop at 48 free cameras: edges leave on most calls
    (incremental removal and the lambda re-initialisation after it) on the in-place path."""
    from oracle import oracle as O

    g = synth.ba_graph(cameras=50, points=1200, obs_per_point=8, fixed_cameras=2, seed=11)
    gb = bundler.BundlerLib()
    ob = O.BundlerOracle()
    lam_g = lam_o = None
    removed = 0
    for w in range(2):
        gb.set_graph(g)
        ob.set_graph(g)
        if lam_g is not None:
            gb.SetCurrentLambda(lam_g)
            ob.set_lambda(lam_o)
        me = np.float32(7.25)
        for it in range(8):
            ms_g, out_g = gb.step([1.8], float(me))
            ms_o, out_o = ob.step([1.8], float(me))
            assert np.array_equal(out_g, out_o), f"window {w}: outliers differ at call {it}"
            assert abs(ms_g - ms_o) <= 1e-4 * max(1.0, abs(ms_o)), (w, it, ms_g, ms_o)
            removed += len(out_o)
            me = np.float32(me * np.float32(0.95) * np.float32(0.95))
        compare(gb, ob)
        same_counts(gb, ob)
        lam_g, lam_o = max(gb.GetCurrentLambda(), 1e-3), max(ob.get_lambda(), 1e-3)
        assert abs(lam_g - lam_o) <= 1e-3 * lam_o
    assert removed > 16


def test_camera_leaves_across_the_switch(gpu):
    """41 free cameras, one of which loses every observation at the first call: the system is
    re-initialised with 40 and the solver changes from cholesky_solve to chol_tiles mid-run."""
    from oracle import oracle as O

    g = synth.ba_graph(cameras=43, points=1000, obs_per_point=8, fixed_cameras=2, seed=5)
    rng = np.random.default_rng(3)
    m = g.cam == 20
    g.uv[m] += rng.choice(np.float32([-40.0, 40.0]), size=(int(m.sum()), 2))
    probe = O.BundlerOracle()
    probe.set_graph(g)
    _, first = probe.step([1.8], 9.0)
    assert np.isin(np.flatnonzero(m), first).all()  # camera 20 is gone after the first call
    gb, ob = run_pair(g, 5, max_err=9.0)
    compare(gb, ob)
    same_counts(gb, ob)


def test_one_instance_across_the_switch(gpu, monkeypatch):
    """40 free -> 41 free -> 9 free on one instance: buffers, the tile table and the per-trial clear
    follow the solver in both directions.  An instance keeps its camera count (a second allocation
    is MAGE_EINVAL, as the reference's AllocateCameras asserts), so every graph has 43 cameras and
    the free count comes from the number of fixed ones; the last has the 9 free cameras of
    test_small_graph's 12-camera graph.  Point and edge counts change with each graph."""
    from oracle import oracle as O

    gb = bundler.BundlerLib()
    ob = O.BundlerOracle()
    for free, kw in ((40, dict(points=1050, fixed_cameras=3, seed=61)), (41, dict(points=1075, fixed_cameras=2, seed=62)),
                     (9, dict(points=400, fixed_cameras=34, seed=1))):
        g = synth.ba_graph(cameras=43, obs_per_point=8, **kw)
        assert len(np.unique(g.cam[g.fixed[g.cam] == 0])) == free
        run_pair_on(monkeypatch, gb, ob, g, 2)
        compare(gb, ob)
        same_counts(gb, ob)


def test_tile_envelope_fill_from_a_far_block(gpu):
    """40 free cameras in a band plus one transform tether between the first and the last free
    camera: a block in the corner of S, so the symbolic-fill envelope of chol_tile_table covers
    the last block row entirely while the band alone would not."""
    g = B.banded(40, points=25 * 42)
    a, b = 2, len(g.pos) - 1
    Rc = g.true_rot[b] @ g.true_rot[a].T
    tc = g.true_pos[b] - Rc @ g.true_pos[a]
    p7 = np.concatenate([tc, synth.quat_from_rot(Rc)]).astype(np.float32)
    t = synth.Tethers(distance=_empty(1), rotation=_empty(4),
                      transform=(np.array([a], np.uint32), np.array([b], np.uint32), p7[None, :],
                                 np.array([50.0], np.float32)))
    gb, ob = run_pair(g, 4, tethers=t)
    compare(gb, ob)
    same_counts(gb, ob)


# ---- (c) the limit ----------------------------------------------------------------------------
def test_more_than_96_free_cameras_is_refused(gpu, monkeypatch):
    """97 free observed cameras: MAGE_EUNSUPPORTED naming the limit, and the instance works again
    on a smaller graph.  (The camera count may change here, from 99 to 12, although an instance
    otherwise keeps it, see test_one_instance_across_the_switch: mage_ba_set_cameras refuses another
    count only once the state is on the device, and the refusal returns from the initialisation
    before the state is uploaded.)  The device initialisation runs with nb = 97 > nbm = 96 before
    the host refuses; every use of a block index there is covered:
      init_scan      camblk[x] / s_camblk[x] with x < nb <= C (both hold C entries); s_rc cleared
                     for h < nbm only.
      init_camcsr    'if (h >= nbm) h = -1' before rc[h] is counted.
      sc_bitmaps     grid of nbm + 1 workgroups: rows h < nbm of A / R (nbm rows allocated), the
                     last workgroup writes F; 'h >= hdr[0]' returns for unused rows.
      sc_pair_counts grid nbm x nbm; 'nb > gridDim.x' returns before cnt[a nb + b] (nbm^2 ints).
      init_pcache    camh[c] with c < C only.
    """
    from oracle import oracle as O

    g = synth.ba_graph(cameras=99, fixed_cameras=2, points=5 * 99, obs_per_point=8, seed=97)
    assert len(np.unique(g.cam[g.fixed[g.cam] == 0])) == 97
    gb = bundler.BundlerLib()
    gb.set_graph(g)
    with pytest.raises(_lib.MageError) as ei:
        gb.step([1.8], 7.25)
    assert ei.value.status == _lib.MAGE_EUNSUPPORTED
    assert "96 free cameras" in str(ei.value)
    assert "96 free cameras" in _lib.load().mage_last_error().decode()
    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=1)  # test_small_graph's
    ob = O.BundlerOracle()
    run_pair_on(monkeypatch, gb, ob, g, 5)
    compare(gb, ob)
    same_counts(gb, ob)


# ---- (d) determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rand", "rev"])
@pytest.mark.parametrize("free", [40, 48])
def test_two_runs_agree_bitwise(gpu, free, kind):
    """No floating-point atomics in the BA kernels: two fresh instances give the same bits (the check
    that caught two lanes storing one diagonal entry of S), on a scattered and on a reversed S and
    both solvers."""
    g = B.permuted(free, kind, points_per_camera=25)
    runs = []
    for _ in range(2):
        gb = bundler.BundlerLib()
        gb.set_graph(g)
        outs = [gb.step([1.8], 7.25 * 0.9025 ** k)[1] for k in range(3)]
        runs.append((gb.state(), outs))
    (sa, oa), (sb, ob_) = runs
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob_))
    assert gb.stats()["iterations"] == 3  # the three steps really ran
