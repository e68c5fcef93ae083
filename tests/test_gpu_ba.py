"""GPU parity: BundlerLib (local BA) through the C-ABI vs the fp64 CPU oracle.

Tolerance (north star): pose parity within 1e-4 — translation max-abs difference and rotation
angle between the quaternions both < 1e-4 — identical outlier sets (same order), mean squared
error within 1e-4 relative.  Parity unpinned against g2o itself.
"""
import numpy as np
import pytest

from mageslam_amd import bundler, synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4


def quat_angle(qa, qb):
    d = np.abs(np.sum(qa * qb, axis=1)).clip(0, 1)
    return 2 * np.arccos(d)


def compare(gb, ob, tol=POSE_TOL):
    qg, pg = gb.state()
    qo, po = ob.state()
    assert np.abs(qg[:, 4:] - qo[:, 4:]).max() < tol
    assert quat_angle(qg[:, :4], qo[:, :4]).max() < tol
    assert np.abs(pg - po).max() < 10 * tol


def run_pair(g, steps, huber=1.8, max_err=7.25, scale=0.95, points_fixed=False, lam=None, nsteps=1,
             tethers=None):
    gb = bundler.BundlerLib(bundler.BundlerParameters(points_fixed))
    gb.set_graph(g)
    from oracle import oracle as O

    ob = O.BundlerOracle(points_fixed)
    ob.set_graph(g)
    if tethers is not None:
        gb.set_tethers(tethers)
        for kind, tt in enumerate((tethers.distance, tethers.rotation, tethers.transform)):
            ob.set_tethers(kind, *tt)
    if lam is not None:
        gb.SetCurrentLambda(lam)
        ob.set_lambda(lam)
    me = max_err
    for it in range(steps):
        ms_g, out_g = gb.step([huber] * nsteps, me)
        ms_o, out_o = ob.step([huber] * nsteps, me)
        assert np.array_equal(out_g, out_o), f"outliers differ at iteration {it}"
        if np.isnan(ms_o):
            assert np.isnan(ms_g)
        else:
            assert abs(ms_g - ms_o) <= 1e-4 * max(1.0, abs(ms_o)), (it, ms_g, ms_o)
        me *= scale * scale
    return gb, ob


def test_small_graph(gpu):
    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=1)
    gb, ob = run_pair(g, 5)
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]
    assert abs(gb.GetCurrentLambda() - ob.get_lambda()) <= 1e-3 * abs(ob.get_lambda())


def test_c3_graph(gpu):
    g = synth.ba_graph()  # 50 KF x 5000 pts x 20 obs
    gb, ob = run_pair(g, 6)
    compare(gb, ob)


@pytest.mark.parametrize("spec", ["1", "0"])
def test_rejected_trials(gpu, monkeypatch, spec):
    """Small lambda + noisy observations: many LM trials are rejected (pop, lambda *= ni), which
    exercises the device-side decision and the speculative linearisation after a rejection (the
    unchanged state with the new lambda, the trial's errors kept) against the oracle; spec = 0 runs
    the host-only path (MAGE_BA_SPEC_LIN=0)."""
    monkeypatch.setenv("MAGE_BA_SPEC_LIN", spec)
    # (seed 5, 8 px noise: chi2 stays far above roundoff, so every accept/reject is decisive; a graph
    # that converges to chi2 ~ 1e-25 decides its late trials on roundoff and the counts differ)
    g = synth.ba_graph(cameras=12, points=300, obs_per_point=8, fixed_cameras=3, seed=5, noise_px=8.0,
                       outlier_frac=0.05)
    gb, ob = run_pair(g, 5, lam=1e-6)
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]
    assert so["trials"] > so["iterations"]  # rejections happened
    assert abs(gb.GetCurrentLambda() - ob.get_lambda()) <= 1e-3 * abs(ob.get_lambda())


def test_multi_step_and_user_lambda(gpu):
    g = synth.ba_graph(cameras=20, points=1500, obs_per_point=10, fixed_cameras=5, seed=7)
    gb, ob = run_pair(g, 3, nsteps=3, lam=0.01)
    compare(gb, ob)


def test_pose_only(gpu):
    # TrackLocalMap::OptimizeCameraPose style: points fixed, one free camera
    g = synth.ba_graph(cameras=6, points=500, obs_per_point=6, fixed_cameras=5, seed=3)
    gb, ob = run_pair(g, 3, huber=0.9, max_err=4.5 ** 2, points_fixed=True)
    compare(gb, ob)


def test_all_fixed_is_useless(gpu):
    g = synth.ba_graph(cameras=6, points=200, obs_per_point=6, fixed_cameras=6, seed=3)
    gb, ob = run_pair(g, 1, points_fixed=True)
    assert gb.stats()["iterations"] == 0


def test_reference_facade_setters(gpu):
    # the per-index setters of the reference API produce the same problem as the bulk path
    g = synth.ba_graph(cameras=8, points=200, obs_per_point=5, fixed_cameras=2, seed=9)
    b = bundler.BundlerLib()
    b.AllocateCameras(len(g.pos))
    for i in range(len(g.pos)):
        b.SetCameraPose(i, g.pos[i], g.rot[i], g.intr[i], bool(g.fixed[i]))
    b.AllocateMapPoints(len(g.points))
    for i in range(len(g.points)):
        b.SetMapPoint(i, g.points[i])
    b.AllocateObservations(len(g.cam))
    for i in range(len(g.cam)):
        b.SetObservation(i, g.uv[i], int(g.cam[i]), int(g.pt[i]), float(g.info[i]))
    outl = []
    ms = b.StepBundleAdjustment([1.8], 7.25, outl)
    c = bundler.BundlerLib()
    c.set_graph(g)
    ms2, out2 = c.step([1.8], 7.25)
    assert ms == ms2 and outl == list(out2)
    pos, R = b.GetPose(3)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-5)


def test_repeated_setters_before_a_step(gpu):
    """Setters called several times before a step (small copies are queued until the step):
    a growing buffer, then the same size with other data, must give exactly the last call's
    problem (queued copies into a freed or re-queued destination)."""
    import dataclasses

    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=1)
    half = len(g.cam) // 2
    g_half = dataclasses.replace(g, uv=g.uv[:half], cam=g.cam[:half], pt=g.pt[:half], info=g.info[:half])
    rng = np.random.default_rng(5)
    g_other = dataclasses.replace(g, uv=(g.uv + rng.normal(0, 3, g.uv.shape)).astype(g.uv.dtype),
                                  points=(g.points + 0.05).astype(g.points.dtype),
                                  pos=(g.pos + 0.01).astype(g.pos.dtype))
    b = bundler.BundlerLib()
    for gg in (g_half, g_other, g):  # grow, then same size with different data
        b.set_graph(gg)
        b._upload()
    ref = bundler.BundlerLib()
    ref.set_graph(g)
    for _ in range(3):
        ms_b, out_b = b.step([1.8], 7.25)
        ms_r, out_r = ref.step([1.8], 7.25)
        assert ms_b == ms_r and np.array_equal(out_b, out_r)
    qb, pb = b.state()
    qr, pr = ref.state()
    assert np.array_equal(qb, qr) and np.array_equal(pb, pr)


def test_tethers(gpu):
    # distance / rotation / transform tethers (BundlerLib.cpp:22-88, 311-350), incl. an inactive
    # fixed-fixed pair and tethers to fixed cameras
    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=1)
    gb, ob = run_pair(g, 5, tethers=synth.ba_tethers(g))
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]
    assert abs(sg["chi2"] - so["chi2"]) <= 1e-6 * abs(so["chi2"])


def test_tethers_c3_and_pose_only(gpu):
    g = synth.ba_graph()
    gb, ob = run_pair(g, 4, tethers=synth.ba_tethers(g, count=8))
    compare(gb, ob)
    g = synth.ba_graph(cameras=6, points=500, obs_per_point=6, fixed_cameras=4, seed=3)
    gb, ob = run_pair(g, 3, huber=0.9, max_err=4.5 ** 2, points_fixed=True, tethers=synth.ba_tethers(g, count=2))
    compare(gb, ob)


def test_tether_only_camera(gpu):
    # a free camera without observations joins the system through its transform tether
    g = tethered_extra_camera()
    t = synth.Tethers(distance=_empty(1), rotation=_empty(4),
                      transform=(np.array([len(g.pos) - 2], np.uint32), np.array([len(g.pos) - 1], np.uint32),
                                 g.extra_tether[None, :], np.array([50.0], np.float32)))
    gb, ob = run_pair(g, 4, tethers=t)
    compare(gb, ob)


def test_tether_argument_errors(gpu):
    from mageslam_amd import _lib

    g = synth.ba_graph(cameras=6, points=100, obs_per_point=4, fixed_cameras=2, seed=5)
    b = bundler.BundlerLib()
    b.set_graph(g)
    b._upload()
    L = _lib.load()
    one = np.array([1], np.uint32)
    p = np.ones(7, np.float32)
    w = np.ones(1, np.float32)
    assert L.mage_ba_set_tethers(b._h, 0, 1, _lib.ptr(one), _lib.ptr(one), _lib.ptr(p), _lib.ptr(w)) == _lib.MAGE_EINVAL
    big = np.array([99], np.uint32)
    assert L.mage_ba_set_tethers(b._h, 2, 1, _lib.ptr(one), _lib.ptr(big), _lib.ptr(p), _lib.ptr(w)) == _lib.MAGE_EINVAL
    assert L.mage_ba_set_tethers(b._h, 3, 0, None, None, None, None) == _lib.MAGE_EINVAL


def _empty(stride):
    return (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, stride), np.float32), np.zeros(0, np.float32))


def tethered_extra_camera():
    """C = 10 graph plus one unobserved camera near the last one (see test_tether_only_camera)."""
    g = synth.ba_graph(cameras=10, points=300, obs_per_point=6, fixed_cameras=3, seed=11)
    R, t = g.true_rot[-1], g.true_pos[-1]
    Rx = synth._rot(0.02) @ R
    tx = t + np.array([0.1, 0.0, 0.0])
    Rc = Rx @ R.T
    tc = tx - Rc @ t
    import dataclasses

    g2 = dataclasses.replace(
        g, pos=np.vstack([g.pos, (tx + 0.01).astype(np.float32)]),
        rot=np.concatenate([g.rot, (synth._rot(0.025) @ R)[None].astype(np.float32)]),
        intr=np.vstack([g.intr, g.intr[-1:]]), fixed=np.append(g.fixed, 0).astype(np.uint8),
        true_rot=np.concatenate([g.true_rot, Rx[None]]), true_pos=np.vstack([g.true_pos, tx]))
    g2.extra_tether = np.concatenate([tc, synth.quat_from_rot(Rc)]).astype(np.float32)
    return g2


@pytest.mark.parametrize("problems,obs", [(96, 500), (600, 200), (4, 2500)])  # the < 512 / >= 512 problems launch branches (256 threads each), > 2048 obs (not staged)
@pytest.mark.parametrize("steps,huber,maxe", [(3, 4.0, 36.0), (4, 0.9, 4.5 ** 2)])
def test_pose_batch_matches_per_frame_oracle(gpu, steps, huber, maxe, problems, obs):
    """Batched OptimizeCameraPose (TrackLocalMap.cpp:96-140 settings: 3 x 4.0 / 6^2, then
    4 x 0.9 / 4.5^2) vs a fresh oracle BundlerLib per frame."""
    from oracle import oracle as O

    pb = synth.pose_batch(problems=problems, obs=obs)
    g = bundler.OptimizeCameraPoses(pb, steps, maxe, huber)
    o = O.pose_batch(pb, steps, huber, maxe)
    assert np.array_equal(g["stats"], o["stats"])
    assert np.array_equal(g["outlier"], o["outlier"])
    assert np.abs(g["qt7"][:, 4:] - o["qt7"][:, 4:]).max() < POSE_TOL
    assert quat_angle(g["qt7"][:, :4], o["qt7"][:, :4]).max() < POSE_TOL
    assert np.allclose(g["mean_sq"], o["mean_sq"], rtol=1e-4)
    assert np.abs(g["pos"] - o["pos"]).max() < 1e-4 and np.abs(g["r9"] - o["r9"]).max() < 1e-4


def test_pose_batch_edges_and_single_problem_path(gpu):
    """Zero-observation problems (useless optimizer: NaN mean), a one-observation problem, zero
    steps (post-pass only), and agreement with the general BundlerLib path (ArePointsFixed)."""
    from oracle import oracle as O

    pb = synth.pose_batch(problems=6, obs=40, vary=False)
    counts = np.diff(pb.obs_start.astype(np.int64))
    counts[1] = 0
    counts[3] = 1
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    sel = np.concatenate([np.arange(pb.obs_start[k], pb.obs_start[k] + counts[k]) for k in range(6)]).astype(int)
    import dataclasses

    pb2 = dataclasses.replace(pb, obs_start=starts, points=pb.points[sel], uv=pb.uv[sel], info=pb.info[sel])
    for steps in (0, 3):
        g = bundler.OptimizeCameraPoses(pb2, steps, 36.0, 4.0)
        o = O.pose_batch(pb2, steps, 4.0, 36.0)
        assert np.array_equal(g["outlier"], o["outlier"]) and np.array_equal(g["stats"], o["stats"])
        assert np.isnan(g["mean_sq"][1]) and np.isnan(o["mean_sq"][1])
        ok = ~np.isnan(o["mean_sq"])
        assert np.allclose(g["mean_sq"][ok], o["mean_sq"][ok], rtol=1e-4)
        assert np.abs(g["qt7"] - o["qt7"]).max() < POSE_TOL
    # the same problem through the general C-ABI BundlerLib (points fixed) gives the same pose
    k = 0
    s = slice(int(pb.obs_start[k]), int(pb.obs_start[k + 1]))
    b = bundler.BundlerLib(bundler.BundlerParameters(True))
    b.AllocateCameras(1)
    b.SetCameraPose(0, pb.pos[k], pb.r9[k].reshape(3, 3).T, pb.intr[k], False)
    n = s.stop - s.start
    b.AllocateMapPoints(n)
    b.AllocateObservations(n)
    for i in range(n):
        b.SetMapPoint(i, pb.points[s][i])
        b.SetObservation(i, pb.uv[s][i], 0, i, float(pb.info[s][i]))
    outl = []
    ms = b.StepBundleAdjustment([4.0] * 3, 36.0, outl)
    g = bundler.OptimizeCameraPoses(pb, 3, 36.0, 4.0)
    qt, _ = b.state()
    assert np.abs(qt[0, 4:] - g["qt7"][0, 4:]).max() < POSE_TOL
    assert list(np.nonzero(g["outlier"][s])[0]) == outl
    assert abs(ms - g["mean_sq"][0]) <= 1e-4 * abs(ms)


def test_reference_schedule_windows(gpu):
    """BundleAdjustTask::Impl::Iterate's schedule (BundleAdjust.cpp:380-404): maxErrorSquare starts
    at the non-squared MaxOutlierError and shrinks by 0.95^2 per call, so edges are removed on most
    calls (removal re-initialises lambda at the next Step); the second window is seeded with the
    first one's lambda (PersistLambda, MappingWorker.cpp:272-293) — both lambda paths after removals."""
    from oracle import oracle as O

    g = synth.ba_graph(cameras=20, points=1500, obs_per_point=10, fixed_cameras=5, seed=11)
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
        sg, so = gb.stats(), ob.stats()
        assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]
        lam_g, lam_o = max(gb.GetCurrentLambda(), 1e-3), max(ob.get_lambda(), 1e-3)
        assert abs(lam_g - lam_o) <= 1e-3 * lam_o
    assert removed > 16  # the decaying threshold really removes edges call after call


def test_removals_drop_points_and_cameras(gpu):
    """Outlier removal that empties points (they leave the system with their last edge) and a whole
    free camera (the block numbering is rebuilt: full re-initialisation), then keeps stepping."""
    from oracle import oracle as O

    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=5)
    rng = np.random.default_rng(3)
    # offsets no pose or point can absorb: every observation of free camera 6 and of point 17
    # becomes an outlier
    for m, d in ((g.cam == 6, 40.0), (g.pt == 17, 25.0)):
        g.uv[m] += rng.choice(np.float32([-d, d]), size=(int(m.sum()), 2))
    gb, ob = run_pair(g, 5, max_err=9.0)
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]


def test_camera_observing_a_point_twice(gpu):
    """A camera with two observations of the same point (the reference API allows it): the Schur
    product lists take the general per-point path (both orders of the same-camera pair) instead of
    the cameras' point bit sets; same outliers, counts and poses as the oracle."""
    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=21)
    rng = np.random.default_rng(4)
    dup = rng.choice(np.flatnonzero(g.fixed[g.cam] == 0), 60, replace=False)
    for f in ("cam", "pt", "info"):
        setattr(g, f, np.concatenate([getattr(g, f), getattr(g, f)[dup]]))
    g.uv = np.concatenate([g.uv, g.uv[dup] + rng.normal(0, 0.3, (60, 2)).astype(np.float32)])
    gb, ob = run_pair(g, 4)
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]


def test_point_with_more_than_64_observations(gpu):
    """Points observed by more edges than one wave holds (device initialisation's long-run path of
    the point CSR: init_psort), here 70 extra observations of two points spread over the cameras
    and appended at the end of the edge list; same outliers, counts and poses as the oracle."""
    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=22)
    rng = np.random.default_rng(5)
    extra = []
    for p in (7, 123):
        src = np.flatnonzero(g.pt == p)
        extra.append(rng.choice(src, 70, replace=True))
    extra = np.concatenate(extra)
    for f in ("cam", "pt", "info"):
        setattr(g, f, np.concatenate([getattr(g, f), getattr(g, f)[extra]]))
    g.uv = np.concatenate([g.uv, g.uv[extra] + rng.normal(0, 0.3, (len(extra), 2)).astype(np.float32)])
    gb, ob = run_pair(g, 4)
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]


@pytest.mark.parametrize("free", [2, 3, 11, 21, 27, 38])
def test_dense_solve_block_counts(gpu, free):
    """chol_tiles at several block counts (np = 16, 32, 80, 128, 176, 240 -> 1 to 15 block steps:
    the factor wave's chain, the staged tiles and the TRSM-phase counter at every depth); same
    outliers, counts and poses as the oracle."""
    g = synth.ba_graph(cameras=free + 2, points=60 * (free + 2), obs_per_point=min(free + 2, 8), fixed_cameras=2,
                       seed=30 + free)
    gb, ob = run_pair(g, 3)
    compare(gb, ob)
    sg, so = gb.stats(), ob.stats()
    assert sg["iterations"] == so["iterations"] and sg["trials"] == so["trials"]


def test_get_pose_point_outputs_match_fp64_state(gpu):
    """GetPose / GetPoint after a step (UpdateData's reads) come from the device-written float
    outputs once the caller reads between steps; they equal BundlerLib.cpp:457-471 evaluated on
    the fp64 state (t and R of the normalised quaternion cast to float, points cast to float)."""
    g = synth.ba_graph(cameras=12, points=400, obs_per_point=8, fixed_cameras=3, seed=1)
    b = bundler.BundlerLib()
    b.set_graph(g)
    for _ in range(4):
        b.step([1.8], 7.25)
        pos, r9 = b.poses()
        xyz = b.points()
        qt, p = b.state()
        q0, q1, q2, q3 = (qt[:, k].copy() for k in range(4))
        nn = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3)
        q0, q1, q2, q3 = q0 / nn, q1 / nn, q2 / nn, q3 / nn
        tx, ty, tz = 2 * q0, 2 * q1, 2 * q2
        twx, twy, twz = tx * q3, ty * q3, tz * q3
        txx, txy, txz = tx * q0, ty * q0, tz * q0
        tyy, tyz, tzz = ty * q1, tz * q1, tz * q2
        R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
                      txz - twy, tyz + twx, 1 - (txx + tyy)], 1).reshape(-1, 3, 3)
        assert np.array_equal(pos, qt[:, 4:].astype(np.float32))
        assert np.array_equal(r9.reshape(-1, 3, 3), R.transpose(0, 2, 1).astype(np.float32))
        assert np.array_equal(xyz, p.astype(np.float32))


def test_more_cameras_than_lds_sort_counters(gpu):
    # > CS_MAX_KEYS (12288) cameras: the camera-CSR counting sort takes its multi-pass digit path.
    # The graph's cameras are the C3-like problem's plus 12300 fixed, unobserved ones interleaved
    # before them, so the active edges' camera keys span the whole range.
    import dataclasses
    g = synth.ba_graph(cameras=24, points=1200, obs_per_point=8, fixed_cameras=6, seed=21)
    extra = 12300
    n = len(g.pos) + extra
    rng = np.random.default_rng(5)
    slots = np.sort(rng.choice(n, len(g.pos), replace=False))  # where the real cameras land
    def spread(a, fill):
        out = np.repeat(fill[None], n, axis=0).astype(a.dtype)
        out[slots] = a
        return out
    g2 = dataclasses.replace(
        g, pos=spread(g.pos, g.pos[0]), rot=spread(g.rot, g.rot[0]), intr=spread(g.intr, g.intr[0]),
        fixed=spread(g.fixed, np.uint8(1)), cam=slots[g.cam].astype(np.uint32),
        true_pos=spread(g.true_pos, g.true_pos[0]), true_rot=spread(g.true_rot, g.true_rot[0]))
    assert len(g2.pos) > 12288
    gb, ob = run_pair(g2, 3)
    compare(gb, ob)


def test_block_cache_trim_and_reuse(gpu):
    """Destroyed BundlerLib instances retire their blocks into the library's cache (common.hpp);
    mage_pool_trim frees them for real, and later instances allocate afresh with unchanged results."""
    from mageslam_amd import _lib

    g = synth.ba_graph(cameras=8, points=200, obs_per_point=6, fixed_cameras=2, seed=5)
    first = None
    for rnd in range(3):
        gb, ob = run_pair(g, 2)
        compare(gb, ob)
        res = gb.state()
        if first is None:
            first = res
        else:
            assert np.array_equal(first[0], res[0]) and np.array_equal(first[1], res[1])
        del gb
        import gc

        gc.collect()
        freed = _lib.load().mage_pool_trim(-1)
        if rnd == 0:
            assert freed > 0  # the destroyed instance's device / host blocks were cached
    assert _lib.load().mage_pool_trim(-1) == 0
