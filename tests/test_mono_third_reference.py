"""mage_mono_init_third_frame_host (the plain C++ twin of the third-frame kernels and the CPU backend)
against the oracle's literal single-query loop (oracle/orb_oracle.c oracle_local_map_match, one
query at a time) for the matching, the independent fp64 formulation of tests/mono_third_cases.py for
the midpoint pose, the projection and the behind verdicts, and a direct Python restatement of
MapInitialization.cpp:829-838 fed oracle.pose_batch's outlier flags for the finish half.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mageslam_amd import _lib, mono
from tests import mono_third_cases as tc

CASES = list(tc.cases())
RUN = [n for n in CASES if tc.case(n).expect_status == 0]
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host():
    """name -> the twin's ThirdFrame without outlier flags (it stops after the first gate)."""
    return {n: mono.locate_third_frame(*c.args(), backend="host") for n, c in tc.cases().items()}


_finish_cache = {}


def finish(host, name):
    """(oracle.pose_batch's output or None, the twin fed its flags) of one case, computed once."""
    if name not in _finish_cache:
        from oracle import oracle as O

        c, h = tc.case(name), host[name]
        if h.verdict == mono.M3_FEW_MATCHES:
            _finish_cache[name] = (None, mono.locate_third_frame(*c.args(), backend="host", outlier=np.zeros(0, np.uint8),
                                                                 opt_pos3=np.zeros(3), opt_r9=np.zeros(9)))
        else:
            s = c.settings
            o = O.pose_batch(tc.pose_batch_of(h, c), s.extra_frame_bundle_adjustment_steps, s.extra_frame_huber_width,
                             float(np.float32(s.extra_frame_max_outlier_error) * np.float32(s.extra_frame_max_outlier_error)))
            _finish_cache[name] = (o, mono.locate_third_frame(*c.args(), backend="host", outlier=o["outlier"],
                                                              opt_pos3=o["pos"][0], opt_r9=o["r9"][0],
                                                              mean_sq=float(o["mean_sq"][0])))
    return _finish_cache[name]


def oracle_point(c, xy, i, mask):
    """Map point i at float32 position xy against `mask` (not changed): each query alone through the
    oracle's single-query RadiusMatch, then :766-798.  -> (keypoint or -1, verdict byte, the two
    queries' matches, their Hamming distances or None)."""
    from oracle import oracle as O

    s = c.settings
    res, dist = [], []
    for desc, idx, maxd, mind in ((c.desc0, c.idx0, s.extra_frame_max_hamming_distance, s.extra_frame_min_hamming_difference),
                                  (c.desc1, c.idx1, s.five_point_max_hamming_distance, s.five_point_min_hamming_difference)):
        r, _ = O.local_map_match(np.asarray(xy, np.float32).reshape(1, 2), [0], desc[[int(idx[i])]], None, c.kp2, c.desc2,
                                 mask.copy(), s.extra_frame_search_radius, maxd, mind)
        res.append(int(r[0]))
        dist.append(O.hamming(desc[int(idx[i])], c.desc2[int(r[0])]) if r[0] >= 0 else None)
    ref_t, cur_t = res
    if cur_t >= 0 and ref_t >= 0:
        take, ver = (cur_t, mono.M3_PT_FRAME1) if dist[1] < dist[0] else (ref_t, mono.M3_PT_FRAME0)
    elif cur_t >= 0:
        take, ver = cur_t, mono.M3_PT_FRAME1
    elif ref_t >= 0:
        take, ver = ref_t, mono.M3_PT_FRAME0
    else:
        take, ver = -1, mono.M3_PT_NO_MATCH
    return take, ver, res, dist


def python_loop(c, h):
    """:723-799 with the oracle's single-query RadiusMatch, fed the twin's own float32 positions:
    -> (keypoints, verdict bytes, final mask, per point and query the match's distance or -1)."""
    mask = np.ones(len(c.kp2), np.uint8)
    n = len(c.points)
    key, ver, dist = np.full(n, -1, np.int32), np.zeros(n, np.uint8), np.full((n, 2), -1, np.int32)
    behind = h.point_verdict == mono.M3_PT_BEHIND
    for i in range(n):
        if behind[i]:
            ver[i] = mono.M3_PT_BEHIND
            continue
        key[i], ver[i], _, d = oracle_point(c, h.proj[i], i, mask)
        dist[i] = [-1 if x is None else x for x in d]
        if key[i] >= 0:
            mask[key[i]] = 0
    return key, ver, mask.astype(bool), dist


@pytest.mark.parametrize("name", RUN)
def test_matching_equals_oracle_loop(host, name):
    c, h = tc.case(name), host[name]
    key, ver, mask, dist = python_loop(c, h)
    assert np.array_equal(h.keypoint, key), name
    assert np.array_equal(h.point_verdict, ver), name
    assert np.array_equal(h.mask, mask), name
    # where a query matched, its reported best distance is the Hamming distance of that match; a
    # behind point reports none
    matched = dist >= 0
    assert np.array_equal(h.dist[matched], dist[matched]), name
    assert (h.dist[ver == mono.M3_PT_BEHIND] == -1).all(), name
    r = h.result
    assert int(r["n_points"]) == len(c.points) and int(r["n_behind"]) == int((ver == mono.M3_PT_BEHIND).sum())
    assert int(r["n_matched"]) == int((key >= 0).sum()) == int(r["n_associated"]) and int(r["n_outliers"]) == 0
    assert h.verdict == (mono.M3_FEW_MATCHES if len(c.points) == 0 or
                         np.float32(r["n_matched"]) / np.float32(len(c.points)) <
                         np.float32(c.settings.min_third_frame_match_percentage) else mono.M3_OK)
    # the bundle adjustment's inputs: the matched points in point order with their keypoints' positions
    m = np.nonzero(key >= 0)[0]
    assert h.ba_points.tobytes() == c.points[m].tobytes()
    assert np.array_equal(h.ba_uv, np.stack([c.kp2["x"][key[m]], c.kp2["y"][key[m]]], 1).reshape(-1, 2))
    assert (h.ba_info == np.float32(1 - 1 / np.float32(2.5) ** 2)).all()


def test_projection_within_tolerance(host):
    """The float32 projection through the float32 midpoint pose against fp64 through the geodesic
    midpoint, within K_TOL eps32 (|px - cx| + |cx| + fx |X - C| / |depth|) over every point whose
    depth is not fragile.  Prints the worst ratio, the basis of K_TOL."""
    worst, at, n = 0.0, None, 0
    for name in RUN:
        ref, h = tc.reference(name), host[name]
        ok = ref.margin >= tc.FRAGILE
        if not ok.any():
            continue
        rx = np.abs(h.proj[ok, 0] - ref.x[ok]) / (tc.EPS32 * ref.xscale[ok])
        ry = np.abs(h.proj[ok, 1] - ref.y[ok]) / (tc.EPS32 * ref.yscale[ok])
        w = max(float(rx.max()), float(ry.max()))
        if w > worst:
            worst, at = w, name
        n += int(ok.sum())
    print(f"worst projection error / (eps32 scale) over {n} points: {worst:.3f} ({at})")
    assert worst <= tc.K_TOL
    assert n >= 700


@pytest.mark.parametrize("name", RUN)
def test_behind_verdicts_equal_fp64(host, name):
    ref, h = tc.reference(name), host[name]
    assert ref.share <= tc.MAX_FRAGILE_SHARE, ref.share
    keep = ref.margin >= tc.FRAGILE
    assert np.array_equal((h.point_verdict == mono.M3_PT_BEHIND)[keep], (ref.depth < 0)[keep])
    # only the deliberate depth-0 point is fragile anywhere
    assert int((~keep).sum()) == (1 if name == "rot_same" else 0)


def test_depth_zero_passes(host):
    """`Distance < 0` lets a depth of exactly zero through; ProjectUndistorted then divides by 1."""
    c, h = tc.case("rot_same"), host["rot_same"]
    i = int(np.argmin(np.abs(tc.reference("rot_same").depth)))
    assert c.points[i, 2] == 0 and h.point_verdict[i] == mono.M3_PT_NO_MATCH
    f = np.float32
    assert tuple(c.points[i]) == (f(0.8), f(0.2), f(0)) and tuple(h.pos3) == (f(-0.5), f(0), f(0))
    assert tuple(h.proj[i]) == ((f(0.8) + f(-0.5)) * f(500) + f(320), f(0.2) * f(500) + f(240))


def test_midpoint_pose(host):
    """The rotation within ANGLE_TOL of the geodesic midpoint (prints the worst angle, its basis); the
    centre exact: one float add and one halving per component of the two float32 centres."""
    worst, at = 0.0, None
    for name in RUN:
        c, ref, h = tc.case(name), tc.reference(name), host[name]
        Rw = h.r9.astype(np.float64).reshape(3, 3)  # column-major view R = row-major world R
        a = tc.rotation_angle(ref.Rm, Rw)
        if a > worst:
            worst, at = a, name
        assert abs(np.linalg.det(Rw) - 1) < 1e-5
        # the centre: C = -(R^T t) per frame in float32, then (C0 + C1) / 2; the pose's t = R (-C)
        f = np.float32
        C = []
        for k in range(2):
            r, t = c.r9[k], c.pos3[k]
            C.append([-((f(0) + r[3 * i] * t[0]) + r[3 * i + 1] * t[1] + r[3 * i + 2] * t[2]) for i in range(3)])
        mid = np.array([(C[0][i] + C[1][i]) / f(2) for i in range(3)], np.float32)
        back = -(Rw @ h.pos3.astype(np.float64))
        assert np.abs(back - mid).max() <= 4 * tc.EPS32 * max(1.0, np.abs(mid).max()), name
        assert np.abs(mid - ref.Cm).max() <= 4 * tc.EPS32 * max(1.0, np.abs(ref.Cm).max()), name
    print(f"worst midpoint rotation angle: {worst:.3e} rad ({at})")
    assert worst <= tc.ANGLE_TOL
    # the three rotation shapes the closed-form slerp has to cover
    q = {n: [_quat(tc.case(n).r9[k]) for k in range(2)] for n in ("rot_neg_dot", "rot_same", "rot120", "rot_small_w")}
    assert q["rot_neg_dot"][0] @ q["rot_neg_dot"][1] < -0.1
    assert np.array_equal(tc.case("rot_same").r9[0], tc.case("rot_same").r9[1])
    R0, R1 = tc.case("rot120").Rw
    assert abs(np.degrees(tc.rotation_angle(R0, R1)) - 120) < 2
    assert min(abs(q["rot_small_w"][k][3]) for k in range(2)) < 0.2  # the trace <= 0 branch of the conversion


def _quat(r9):
    from tests.pose_cases import _quat_f32

    return _quat_f32(r9).astype(np.float64)


def restate_finish(c, h, outlier):
    """:829-838 and the outputs, directly: -> (verdict, n_outliers, n_associated, keypoints, verdicts, obs)."""
    key, ver = h.keypoint.copy(), h.point_verdict.copy()
    n = len(c.points)
    pct = np.float32(c.settings.min_third_frame_match_percentage)
    verdict = h.verdict
    nout = 0
    if verdict == mono.M3_OK:
        m = np.nonzero(key >= 0)[0]
        for j in np.nonzero(outlier)[0]:
            key[m[j]] = -1
            ver[m[j]] = mono.M3_PT_CULLED
            nout += 1
        if np.float32((key >= 0).sum()) / np.float32(n) < pct:
            verdict = mono.M3_FEW_AFTER_CULL
    left = np.nonzero(key >= 0)[0]
    uv = np.stack([c.kp2["x"][key[left]], c.kp2["y"][key[left]]], 1).reshape(-1, 2)
    return verdict, nout, len(left), key, ver, (uv, left.astype(np.uint32))


@pytest.mark.parametrize("name", tc.FINISH_CASES)
def test_finish_half(host, name):
    c, h = tc.case(name), host[name]
    o, g = finish(host, name)
    verdict, nout, na, key, ver, (uv, pt) = restate_finish(c, h, o["outlier"] if o else None)
    r = g.result
    assert (g.verdict, int(r["n_outliers"]), int(r["n_associated"])) == (verdict, nout, na)
    assert int(r["n_matched"]) == int(h.result["n_matched"]) and int(r["n_behind"]) == int(h.result["n_behind"])
    assert np.array_equal(g.keypoint, key) and np.array_equal(g.point_verdict, ver)
    assert np.array_equal(g.obs_uv, uv) and np.array_equal(g.obs_pt, pt)
    assert (g.obs_cam == c.cam_index).all() and (g.obs_info == np.float32(1 - 1 / np.float32(2.5) ** 2)).all()
    assert len(g.obs_cam) == na
    # untouched by the finish half
    assert g.dist.tobytes() == h.dist.tobytes() and np.array_equal(g.mask, h.mask) and g.proj.tobytes() == h.proj.tobytes()
    assert g.pos3.tobytes() == h.pos3.tobytes() and g.r9.tobytes() == h.r9.tobytes()
    if o is None:
        assert not g.opt_r9.any() and float(r["mean_sq"]) == 0
    else:
        assert g.opt_pos3.tobytes() == o["pos"][0].tobytes() and g.opt_r9.tobytes() == o["r9"][0].tobytes()


def test_decoys_are_culled(host):
    """Keypoints 20 px from where their point projects are matched (the radius is 40) and culled by the
    bundle adjustment at 8 px; in cull_tips that tips the second gate."""
    for name, verdict in (("decoys", mono.M3_OK), ("cull_tips", mono.M3_FEW_AFTER_CULL)):
        c, h = tc.case(name), host[name]
        o, g = finish(host, name)
        assert h.verdict == mono.M3_OK and g.verdict == verdict
        decoys = [i for i in range(len(c.points)) if (i, 0) in c.kp_of and
                  np.hypot(c.kp2["x"][c.kp_of[(i, 0)]] - h.proj[i, 0], c.kp2["y"][c.kp_of[(i, 0)]] - h.proj[i, 1]) > 15]
        assert len(decoys) == 3
        assert sorted(np.nonzero(g.point_verdict == mono.M3_PT_CULLED)[0].tolist()) == decoys


def test_rules(host):
    c, h = tc.case("rules"), host["rules"]
    k, v, d = h.keypoint, h.point_verdict, h.dist
    K = c.kp_of
    assert (k[0], k[1]) == (K[(0, 0)], K[(0, 1)])           # the later point falls back
    assert tuple(d[1]) == (12, 12)
    assert k[2] == K[(2, 0)] and k[3] == -1 and v[3] == mono.M3_PT_NO_MATCH and tuple(d[3]) == (-1, -1)
    assert k[4] == K[(4, 0)] and v[4] == mono.M3_PT_FRAME0 and tuple(d[4]) == (6, 6)   # equal: frame 0's
    assert k[5] == K[(5, 1)] and v[5] == mono.M3_PT_FRAME1 and tuple(d[5]) == (9, 5)   # strictly better
    assert k[6] == K[(6, 0)] and v[6] == mono.M3_PT_FRAME0 and tuple(d[6]) == (10, -1)
    assert k[7] == K[(7, 0)] and v[7] == mono.M3_PT_FRAME1 and tuple(d[7]) == (-1, 10)
    assert k[8] == K[(8, 1)] and c.kp2["octave"][K[(8, 0)]] == 1 and tuple(d[8]) == (8, 8)  # octave 1 ignored
    assert K[(9, 0)] < K[(9, 1)] and k[9] == -1 and tuple(d[9]) == (7, 7)  # 8 then 7: the ratio test fails for both
    assert k[10] == -1 and tuple(d[10]) == (-1, -1)          # outside the box
    assert h.mask[K[(8, 0)]] and not h.mask[K[(0, 1)]]


def test_bags_differ(host):
    """With the two matcher bags swapped every specified point of the bags case decides differently."""
    c, h = tc.case("bags"), host["bags"]
    s = c.settings
    sw = tc.settings(extra_frame_max_hamming_distance=s.five_point_max_hamming_distance,
                     extra_frame_min_hamming_difference=s.five_point_min_hamming_difference,
                     five_point_max_hamming_distance=s.extra_frame_max_hamming_distance,
                     five_point_min_hamming_difference=s.extra_frame_min_hamming_difference)
    g = mono.locate_third_frame(sw, *c.args()[1:], backend="host")
    assert [int(x) for x in h.point_verdict[:5]] == [mono.M3_PT_FRAME1, mono.M3_PT_FRAME1, mono.M3_PT_FRAME0,
                                                     mono.M3_PT_FRAME1, mono.M3_PT_FRAME0]
    assert (h.point_verdict[:5] != g.point_verdict[:5]).all()
    assert np.array_equal(h.point_verdict[5:], g.point_verdict[5:])


def test_contention_under_different_bags(host):
    """bags_blob: a point whose outcome turns on a keypoint that the point before it took and that is a
    candidate of its query 1 alone (beyond query 0's maximal distance, within query 1's), while query 0
    has nothing left: only a resolver that looks for earlier marks among both queries' candidates sees
    the conflict."""
    from oracle import oracle as O

    c, h = tc.case("bags_blob"), host["bags_blob"]
    s = c.settings
    assert (s.extra_frame_max_hamming_distance, s.extra_frame_min_hamming_difference,
            s.five_point_max_hamming_distance, s.five_point_min_hamming_difference) == (25, 0, 35, 3)
    mask = np.ones(len(c.kp2), np.uint8)
    seen = 0
    for i in range(1, len(c.points)):
        if h.keypoint[i - 1] < 0:
            break
        before = mask.copy()               # the state the point before i saw
        mask[h.keypoint[i - 1]] = 0
        t = int(h.keypoint[i - 1])
        d0 = O.hamming(c.desc0[int(c.idx0[i])], c.desc2[t])
        d1 = O.hamming(c.desc1[int(c.idx1[i])], c.desc2[t])
        stale = oracle_point(c, h.proj[i], i, before)
        fresh = oracle_point(c, h.proj[i], i, mask)
        assert fresh[0] == h.keypoint[i]
        if d0 > 25 and d1 <= 35 and fresh[2][0] < 0 and stale[0] != fresh[0]:
            seen += 1
    assert seen >= 2, seen
    assert set(h.point_verdict.tolist()) == {mono.M3_PT_FRAME0, mono.M3_PT_FRAME1, mono.M3_PT_NO_MATCH}


def test_pose_fragile_cases_are_the_listed_ones(host):
    """Of the cases that reach the bundle adjustment, the fp64 reference of tests/pose_cases.py is
    fragile exactly on tc.POSE_FRAGILE, and there only through the accept / reject margin: the outlier
    and cheirality margins are wide everywhere, so the outlier flags are compared in every case."""
    from tests import pose_cases as P

    fragile, ran = [], 0
    for name in RUN:
        c, h = tc.case(name), host[name]
        if h.verdict != mono.M3_OK or int(h.result["n_matched"]) == 0:
            continue
        s = c.settings
        ref = P.reference(tc.pose_batch_of(h, c), s.extra_frame_bundle_adjustment_steps, s.extra_frame_huber_width,
                          float(np.float32(s.extra_frame_max_outlier_error) * np.float32(s.extra_frame_max_outlier_error)))
        ran += 1
        assert ref.m_ss[0] >= 1e-3 and ref.m_z[0] >= 1.0, (name, ref.m_ss[0], ref.m_z[0])
        if ref.fragile[0]:
            fragile.append(name)
    assert sorted(fragile) == sorted(tc.POSE_FRAGILE), fragile
    assert ran >= 19 and len(fragile) <= 2


def test_coverage(host):
    point, frame = set(), set()
    for name in tc.FINISH_CASES:
        g = finish(host, name)[1]
        point |= set(g.point_verdict.tolist())
        frame.add(g.verdict)
    assert point == {0, 1, 2, 3, 4} and frame == {mono.M3_OK, mono.M3_FEW_MATCHES, mono.M3_FEW_AFTER_CULL}
    cs = tc.cases()
    assert [len(cs[n].points) for n in ("n0", "n1", "n63", "n64", "n65", "n257")] == [0, 1, 63, 64, 65, 257]
    assert [len(cs[n].kp2) for n in ("kp0", "kp1", "kp4096", "kp4097")] == [0, 1, 4096, 4097]
    assert (host["kp4096"].keypoint >= 2048).any()
    # the gates: exactly at the threshold passes, one short fails
    assert host["gate_exact"].verdict == mono.M3_OK and int(host["gate_exact"].result["n_matched"]) == 5
    assert host["gate_short"].verdict == mono.M3_FEW_MATCHES and int(host["gate_short"].result["n_matched"]) == 4
    assert host["n0"].verdict == mono.M3_FEW_MATCHES
    # the blob: far more candidates than a point can keep, and most points contend
    b = host["blob"]
    assert int(b.result["n_matched"]) == 40 and (b.point_verdict == mono.M3_PT_NO_MATCH).sum() == 60
    assert (b.dist[:40] >= 0).all()


def test_limits_and_bad_indices(host):
    for name, status in (("kp4097", mono.M3_STATUS_OVER_LIMIT), ("bad_idx0", mono.M3_STATUS_BAD_INDEX),
                         ("bad_idx1", mono.M3_STATUS_BAD_INDEX)):
        h = host[name]
        r = h.result
        assert h.status == status == tc.case(name).expect_status and int(r["n_points"]) == len(tc.case(name).points)
        rest = np.frombuffer(r.tobytes(), np.uint32).copy()
        rest[[1, 2]] = 0
        assert not rest.any() and len(h.keypoint) == 0 and len(h.obs_uv) == 0
    c = tc.case("n1")
    big = np.zeros((4097, 3), np.float32)
    h = mono.locate_third_frame(c.settings, tc.INTR, c.pos3, c.r9, big, np.zeros(4097, np.int32), np.zeros(4097, np.int32),
                                c.desc0, c.desc1, c.kp2, c.desc2, backend="host")
    assert h.status == mono.M3_STATUS_OVER_LIMIT


def test_argument_checks():
    c = tc.case("n1")

    def status_of(cs):
        with pytest.raises(_lib.MageError) as e:
            mono.locate_third_frame(cs, *c.args()[1:], backend="host")
        return e.value.status

    bad = c.settings.to_c()
    bad.struct_size = ctypes.sizeof(bad) + 4
    assert status_of(bad) == _lib.MAGE_EINVAL
    bad = c.settings.to_c()
    bad.extra_frame_max_hamming_distance = 257
    assert status_of(bad) == _lib.MAGE_EINVAL
    bad = c.settings.to_c()
    bad.extra_frame_search_radius = float("nan")
    assert status_of(bad) == _lib.MAGE_EINVAL


def test_struct_layout():
    assert _lib.M3_RESULT_DTYPE.itemsize == 128
    assert [_lib.M3_RESULT_DTYPE.fields[f][1] for f in ("verdict", "mean_sq", "pos3", "r9", "opt_pos3", "opt_r9")] == [
        0, 28, 32, 44, 80, 92]
    n, off = mono.third_scratch_layout(5, 300)
    assert list(off) == list(mono.M3_SCRATCH_ARRAYS) and all(o % 256 == 0 for o in off.values()) and n % 256 == 0
    assert off["ba_count"] - off["obs_start"] >= 4 * 6 and n - off["mean_sq"] >= 4 * 5


def test_host_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/cpp/mono_third_host_check.cpp: the twin's translation unit in a stand-alone program (its
    own main, no library, no GPU, nothing loaded into Python) built with -fsanitize=address,undefined,
    fed the limit cases (bad indices, 0 / 1 / 4096 / 4097 keypoints) with every output buffer exactly
    as long as its count."""
    src = ROOT / "tests" / "cpp" / "mono_third_host_check.cpp"
    csrc = ROOT / "mageslam_amd" / "csrc"
    out = tmp_path / "mono_third_host_check_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", f"-I{csrc}", f"-I{ROOT / 'include'}", str(src), "-o", str(out)], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)
    assert "6 cases" in r.stdout
