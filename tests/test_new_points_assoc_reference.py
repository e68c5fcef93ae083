"""mage_new_points_associate_host (the plain C++ twin of the association kernel and the CPU backend)
against the independent fp64 formulation of tests/new_points_assoc_cases.py for the projection, gate
and octave, against the oracle's literal sequential loop (oracle/orb_oracle.c
oracle_local_map_match) for the matching, and mapping.new_map_points_creation against a plain Python
double loop.  No GPU."""
import ctypes

import numpy as np
import pytest

from mageslam_amd import _lib, mapping
from tests import new_points_assoc_cases as ac

CASES = list(ac.cases())


@pytest.fixture(scope="module")
def host():
    """name -> (records, verdicts, masks, status) of the twin, computed once."""
    return {n: mapping.new_points_associate(*c.args(), backend="host") for n, c in ac.cases().items()}


@pytest.mark.parametrize("name", CASES)
def test_fragile_share(name):
    ref = ac.reference(name)
    assert ref.share <= ac.MAX_FRAGILE_SHARE, ref.share


@pytest.mark.parametrize("name", CASES)
def test_host_verdicts_equal_fp64(host, name):
    c, ref = ac.cases()[name], ac.reference(name)
    rec, v, masks, status = host[name]
    assert status == ref.status
    got = v.astype(int)
    got[got == ac.ASSOCIATED] = ac.NO_MATCH  # the fp64 side stops before the descriptor search
    got[v == 0xFF] = -1                      # untouched: a keyframe over the limit
    keep = ref.margin >= ac.FRAGILE
    assert np.array_equal(got[keep], ref.verdict[keep])
    searched = keep & (ref.verdict == ac.NO_MATCH)
    assert np.array_equal(rec["octave"][searched], ref.octave[searched])
    # fields the reference had not computed are 0 / -1
    early = np.isin(v, [ac.SAME_FRAME, ac.BAD_INDEX, 0xFF])
    assert (rec["x"][early] == 0).all() and (rec["y"][early] == 0).all()
    assert (rec["octave"][np.isin(v, [ac.SAME_FRAME, ac.BAD_INDEX, ac.BEHIND, ac.BORDER_OUT, ac.ANGLE, ac.DISTANCE,
                                     0xFF])] == 0).all()
    assert (rec["keypoint"][v != ac.ASSOCIATED] == -1).all() and (rec["keypoint"][v == ac.ASSOCIATED] >= 0).all()
    for k, kf in enumerate(c.kfs):
        if len(kf.kp) > 4096:  # the column, its records and its mask are left alone
            assert (v[:, k] == 0xFF).all() and np.array_equal(masks[k], kf.mask)


def test_projection_within_tolerance(host):
    """The float32 projection against fp64 within K_TOL eps32 (|px - cx| + |cx| + fx |X - C| / depth),
    over every projected pair whose depth is not fragile.  Prints the worst ratio, the basis of K_TOL."""
    worst, n = 0.0, 0
    for name in CASES:
        ref, (rec, v, _, _) = ac.reference(name), host[name]
        ok = ~np.isnan(ref.x) & (ref.margin >= ac.FRAGILE)
        if not ok.any():
            continue
        rx = np.abs(rec["x"][ok] - ref.x[ok]) / (ac.EPS32 * ref.xscale[ok])
        ry = np.abs(rec["y"][ok] - ref.y[ok]) / (ac.EPS32 * ref.yscale[ok])
        worst = max(worst, float(rx.max()), float(ry.max()))
        n += int(ok.sum())
        assert max(rx.max(), ry.max()) <= ac.K_TOL, (name, rx.max(), ry.max())
    print(f"worst projection error / (eps32 scale) over {n} pairs: {worst:.3f}")
    assert n >= 1500


def oracle_column(c, rec, v, k, mask=None):
    """Keyframe k through the oracle's sequential loop: the twin's own (x, y, octave) of the points
    that passed the gate, in point order, Ki's descriptors, the starting mask with the claims cleared.
    -> (point indices, keypoints, final mask)."""
    from oracle import oracle as O

    kf = c.kfs[k]
    passed = np.nonzero(np.isin(v[:, k], [ac.ASSOCIATED, ac.NO_MATCH]))[0]
    qpos = np.stack([rec["x"][passed, k], rec["y"][passed, k]], axis=1).astype(np.float32).reshape(-1, 2)
    qdesc = c.ki_desc[c.points["ki_index"][passed].astype(np.int64)].reshape(-1, 32)
    res, m = O.local_map_match(qpos, rec["octave"][passed, k], qdesc, None, kf.kp, kf.desc,
                               ac.start_mask(c, k) if mask is None else mask, c.assoc.search_radius,
                               c.assoc.max_hamming_distance, c.assoc.min_hamming_difference)
    return passed, res, m


@pytest.mark.parametrize("name", CASES)
def test_matching_equals_oracle_loop(host, name):
    c = ac.cases()[name]
    rec, v, masks, _ = host[name]
    for k, kf in enumerate(c.kfs):
        if len(kf.kp) > 4096:
            continue
        passed, res, m = oracle_column(c, rec, v, k)
        assert np.array_equal(rec["keypoint"][passed, k], res), (name, k)
        assert np.array_equal(masks[k], m.astype(bool)), (name, k)


def test_coverage(host):
    hist = np.zeros(9, int)
    for name in CASES:
        v = host[name][1]
        hist += np.bincount(v[v != 0xFF].ravel(), minlength=9)
    assert (hist > 0).all(), hist
    cs = ac.cases()
    assert {cs[n].assoc.min_hamming_difference for n in CASES} >= {0, 1, 3}
    assert max(len(c.kfs) for c in cs.values()) > 8
    assert [len(cs[n].points) for n in ("empty", "n1", "n64", "n65", "n257")] == [0, 1, 64, 65, 257]
    assert any(k.slot == -1 for k in cs["base"].kfs) and not cs["base"].kfs[-1].mask.any()
    assert (host["base"][1][:, -1] != ac.ASSOCIATED).all()       # a keyframe with every keypoint associated
    assert any(not k.mask.all() for k in cs["contend"].kfs)     # keypoints associated before the call
    assert len(cs["kp4096"].kfs[1].kp) == 4096 and len(cs["kp4097"].kfs[1].kp) == 4097
    assert (host["kp4096"][0]["keypoint"][:, 1] == 4095).any()  # the last keypoint is reached
    assert host["kp4097"][3] == 1 and host["kp4096"][3] == 0
    assert len(set(cs["octaves3"].kfs[2].kp["octave"].tolist())) >= 3
    # a search box with far more candidates than points can keep
    c = cs["blob"]
    rec, v, _, _ = host["blob"]
    kp = c.kfs[0].kp
    inbox = [(np.abs(kp["x"] - rec["x"][p, 0]) <= c.assoc.search_radius) &
             (np.abs(kp["y"] - rec["y"][p, 0]) <= c.assoc.search_radius) & (kp["octave"] == rec["octave"][p, 0])
             for p in range(100)]
    assert np.median([b.sum() for b in inbox]) >= 30 and (v[:, 0] == ac.ASSOCIATED).sum() >= 30
    # the kernel's kept list of 8 exactly full, and its first overflow
    for n, size in (("blob8", 8), ("blob9", 9)):
        assert (ac.start_candidates(cs[n], host[n][0], host[n][1], 0) == size).any()


def test_order_matters(host):
    """In the contend case several points want one keypoint (each point alone, against the starting
    mask, would take it), and a keypoint claimed by CreateInitialAssociations would be the match of
    another point if the claim were not cleared first."""
    c = ac.cases()["contend"]
    rec, v, masks, _ = host["contend"]
    from oracle import oracle as O

    contested, claimed_best = 0, 0
    for k, kf in enumerate(c.kfs):
        passed = np.nonzero(np.isin(v[:, k], [ac.ASSOCIATED, ac.NO_MATCH]))[0]
        alone = []
        for p in passed:
            res, _ = O.local_map_match(np.array([[rec["x"][p, k], rec["y"][p, k]]], np.float32), rec["octave"][[p], k],
                                       c.ki_desc[[int(c.points["ki_index"][p])]], None, kf.kp, kf.desc,
                                       ac.start_mask(c, k), c.assoc.search_radius, c.assoc.max_hamming_distance,
                                       c.assoc.min_hamming_difference)
            alone.append(int(res[0]))
        alone = np.array(alone)
        want, cnt = np.unique(alone[alone >= 0], return_counts=True)
        contested += int((cnt >= 2).sum())
        assert not np.array_equal(alone, rec["keypoint"][passed, k]) or (cnt < 2).all()
        if kf.slot >= 0:  # the same loop with the claims left in the mask
            _, res, _ = oracle_column(c, rec, v, k, mask=kf.mask.astype(np.uint8))
            claims = set(int(pt["kc_index"]) for pt in c.points if int(pt["kc_slot"]) == kf.slot)
            claimed_best += sum(1 for t in res if int(t) in claims)
    assert contested >= 10, contested
    assert claimed_best >= 5, claimed_best


def test_over_limit_leaves_other_keyframes_alone(host):
    c = ac.cases()["kp4097"]
    rec, v, masks, status = host["kp4097"]
    a = list(c.args())
    for i in range(4, 11):
        a[i] = [a[i][0], a[i][2]]
    rec2, v2, masks2, status2 = mapping.new_points_associate(*a, backend="host")
    assert status == 1 and status2 == 0
    assert rec[:, [0, 2]].tobytes() == rec2.tobytes() and np.array_equal(v[:, [0, 2]], v2)
    assert np.array_equal(masks[0], masks2[0]) and np.array_equal(masks[2], masks2[1])
    assert (rec["keypoint"][:, 1] == -1).all() and (rec["x"][:, 1] == 0).all() and (rec["octave"][:, 1] == 0).all()


def test_composition():
    """new_map_points_creation(backend="host") on a scene of the existing generator equals
    create_initial_associations followed by a plain Python double loop (points outer, keyframes
    inner) that calls oracle.local_map_match one point at a time."""
    from oracle import oracle as O

    ki, cov, matcher, s, a = ac.composition_scene()
    ki_desc = ki.descriptors
    got = mapping.new_map_points_creation(ki, cov, s, a, backend="host", matcher=matcher)
    init = mapping.create_initial_associations(ki, cov, s, backend="host", matcher=matcher)
    assert got.initial.points.tobytes() == init.points.tobytes() and len(init.points) > 20
    order = mapping.sort_covisible(ki, cov)
    assert sorted(order) == [0, 1, 2] and init.frames == order[:2]
    masks = []
    for i in order:
        m = (~cov[i].associated).astype(np.uint8)
        if i in init.frames:
            m[init.kc_associated[init.frames.index(i)]] = 0
        masks.append(m)
    expect = []
    for pi, pt in enumerate(init.points):
        kfs = [(-1, int(pt["ki_index"])), (init.frames[int(pt["kc_slot"])], int(pt["kc_index"]))]
        for k, i in enumerate(order):
            if i == init.frames[int(pt["kc_slot"])]:
                continue
            r = got.local.records[pi, k]
            if got.local.verdicts[pi, k] not in (ac.ASSOCIATED, ac.NO_MATCH):
                continue
            res, masks[k] = O.local_map_match(np.array([[r["x"], r["y"]]], np.float32), [int(r["octave"])],
                                              ki_desc[[int(pt["ki_index"])]], None, cov[i].keypoints, cov[i].descriptors,
                                              masks[k], a.search_radius, a.max_hamming_distance, a.min_hamming_difference)
            if res[0] >= 0:
                kfs.append((i, int(res[0])))
        expect.append(kfs)
    assert [m.keyframes for m in got.points] == expect
    gained = sum(1 for m in got.points if len(m.keyframes) >= 3)
    assert gained >= len(got.points) // 2, (gained, len(got.points))
    for k in range(3):
        assert np.array_equal(got.local.masks[k], masks[k].astype(bool))
    assert all(m.keyframes[0][0] == -1 for m in got.points)


def test_argument_checks():
    c = ac.cases()["bad_index"]

    def status_of(args):
        with pytest.raises(_lib.MageError) as e:
            mapping.new_points_associate(*args, backend="host")
        return e.value.status

    a = list(c.args())
    bad = c.assoc.to_c()
    bad.struct_size = ctypes.sizeof(bad) + 4
    assert status_of([a[0], bad] + a[2:]) == _lib.MAGE_EINVAL
    bad = c.assoc.to_c()
    bad.max_hamming_distance = 257
    assert status_of([a[0], bad] + a[2:]) == _lib.MAGE_EINVAL
    bad = c.settings.to_c()
    bad.num_levels = 9
    assert status_of([bad] + a[1:]) == _lib.MAGE_EINVAL
    b = list(a)
    b[9] = [8] + list(a[9][1:])
    assert status_of(b) == _lib.MAGE_EINVAL  # kf_slot out of [-1, 7]
    assert b"" != _lib.load().mage_last_error()


def test_struct_layouts():
    assert ctypes.sizeof(_lib.NewPointsAssocSettingsC) == 24
    assert _lib.NewPointsAssocSettingsC.struct_size.offset == 0
    assert _lib.NA_DTYPE.itemsize == 16
    assert [_lib.NA_DTYPE.fields[f][1] for f in ("x", "y", "octave", "keypoint")] == [0, 4, 8, 12]
    s = mapping.NewPointsAssociationSettings()
    assert (s.search_radius, s.max_keyframe_angle_degrees, s.max_hamming_distance, s.min_hamming_difference) == (
        11.8816156, 60.0, 30, 1)
    assert (mapping.NA_ASSOCIATED, mapping.NA_SAME_FRAME, mapping.NA_BEHIND, mapping.NA_BORDER, mapping.NA_ANGLE,
            mapping.NA_DISTANCE, mapping.NA_OCTAVE, mapping.NA_NO_MATCH, mapping.NA_BAD_INDEX) == tuple(range(9))
