"""The frames of tests/orb_select_cases.py reach the select_kernel branches they are meant for.

CPU only: every condition is computed from the oracle and the NumPy restatement of the retain
counts, so test_gpu_orb_select.py cannot pass because a case quietly stopped reaching its branch.
(n0, cut, K) are the candidate count, the retain cut and the retained count of orb_select_cases.
"""
import numpy as np
import pytest

from tests import orb_select_cases as sc


def counts(name):
    x, y, s = sc.candidates(sc.frame(name))
    return x, y, s, sc.retain(s, sc.nfeatures(name))


def test_helper_agrees_with_oracle_on_raster_path(oracle):
    # fewer candidates than NumFeatures: the oracle returns every candidate in raster order
    img = sc.dots(640, 480, 20, 20)
    x, y, s = sc.candidates(img)
    st, kp, _ = oracle.orb_detect(img, oracle.default_settings(2000))
    assert st == 0 and len(kp) == len(s) == 31 * 23
    assert np.array_equal(kp["x"], x.astype(np.float32)) and np.array_equal(kp["y"], y.astype(np.float32))
    assert np.array_equal(kp["response"], s.astype(np.float32))
    assert sc.retain(s, 2000) == (len(s), 0, len(s))


def test_retain_rule_small_histogram():
    # 10 x 50, 10 x 40, 30 x 20, N = 15, factor 1.5 (maxNum 22), strength 0.9: suffix >= 15 first at 40,
    # lower = (int)(40.f * 0.9f) = 36 (the f32 product rounds to 36.0), suffix >= 22 only below lower
    s = np.array([50] * 10 + [40] * 10 + [20] * 30)
    assert sc.retain(s, 15) == (50, 36, 20)
    # five more at 37: suffix >= 22 is reached at 37 >= lower
    assert sc.retain(np.array([50] * 10 + [40] * 10 + [37] * 5 + [20] * 30), 15) == (55, 37, 25)
    # 2000 x 99: lower = (int)(99.f * 0.9f) = 89, not 90
    assert sc.retain(np.array([99] * 2000 + [89] * 1500 + [50] * 10), 2000) == (3510, 89, 3500)
    assert sc.retain(s, 50) == (50, 0, 50)
    assert sc.retain(np.array([3] * 40), 15, t=4) == (40, 4, 0)


def test_ties(oracle):
    _, _, s, (n0, cut, K) = counts("ties")
    N = sc.nfeatures("ties")
    assert len(np.unique(s)) == 1 and s[0] == 99  # one response: the order is the tie rules alone
    assert (n0, cut, K) == (len(s), 99, len(s)) and N < K <= sc.KMAX and K > sc.KMAX - 256
    kp, _ = sc.expected_case("ties")
    assert len(kp) == N and (kp["response"] == 99).all()


def test_kmax_edge(oracle):
    _, _, s, (n0, cut, K) = counts("kmax")
    assert K == sc.KMAX == n0 and len(np.unique(s)) == 1
    _, _, s1, (n1, cut1, K1) = counts("kmax+1")
    assert K1 == sc.KMAX + 1 == n1 and cut1 == cut
    for name in ("kmax", "kmax+1"):
        assert len(sc.expected_case(name)[0]) == sc.nfeatures(name)


def test_mixed(oracle):
    _, _, s, (n0, cut, K) = counts("mixed")
    N = sc.nfeatures("mixed")
    assert sorted(np.unique(s)) == [69, 119] and cut == 69 and K == n0 == len(s) and N < K <= sc.KMAX
    strong = int((s == 119).sum())
    assert 0 < strong < N  # the strong items alone do not fill the output
    kp, _ = sc.expected_case("mixed")
    r, c = np.unique(kp["response"], return_counts=True)
    # every strong item is kept (nothing is stronger: r = gmax); the rest of the output are weak
    # items, ranked by their distance to a strong one
    assert list(r) == [69, 119] and c[1] == strong and c[0] == N - strong
    assert (kp["response"][:strong] == 119).all()


@pytest.mark.parametrize("name,flat,spread", [("row", "y", "x"), ("col", "x", "y")])
def test_degenerate_extent(oracle, name, flat, spread):
    x, y, s, (n0, cut, K) = counts(name)
    N = sc.nfeatures(name)
    assert n0 == K == 315 and N < K  # ANMS on
    p = {"x": x, "y": y}
    assert p[flat].min() == p[flat].max() and p[spread].max() - p[spread].min() > 32  # area 0: gmax == 0
    kp, _ = sc.expected_case(name)
    assert len(kp) == N


@pytest.mark.parametrize("name,axis", [("thin_w", "x"), ("thin_h", "y")])
def test_thin_frames(oracle, name, axis):
    img = sc.frame(name)
    assert max(img.shape) == 4095
    _, _, s, (n0, cut, K) = counts(name)
    N = sc.nfeatures(name)
    assert n0 > N and N <= K <= sc.KMAX  # ANMS on
    kp, _ = sc.expected_case(name)
    assert len(kp) == N and (kp[axis] >= 4000).any()  # coordinates that need all 12 bits


def test_hd(oracle):
    img = sc.frame("hd")
    h, w = img.shape
    T = sc.tiles(w, h)
    assert T == 576 and 4 * T > 2 * sc.SEL_THREADS  # for_each_cand's tail runs more than once per thread
    _, _, s, (n0, cut, K) = counts("hd")
    N = sc.nfeatures("hd")
    assert n0 > N and N <= K <= sc.KMAX and cut > 4
    assert len(sc.expected_case("hd")[0]) == N


def test_cap_in_level(oracle):
    full, _ = sc.expected_case("cap_in_level", **sc.PYRAMID)
    per_level = np.bincount(full["octave"], minlength=4)
    assert (per_level > 0).all() and len(full) == sc.nfeatures("cap_in_level")
    for cap in sc.CAP_IN_LEVEL:
        kp, _ = sc.expected_case("cap_in_level", cap=cap, **sc.PYRAMID)
        got = np.bincount(kp["octave"], minlength=4)
        assert len(kp) == cap
        assert got[0] == per_level[0] and 0 < got[1] < per_level[1]  # the capacity ends inside level 1
        assert got[2] == 0 and got[3] == 0  # and leaves the later levels empty


def test_redo_frames(oracle):
    frames = sc.redo_frames()
    assert len(frames) == sc.REDO_FRAMES > 2 * sc.REDO_WORKGROUPS  # some workgroup runs three frames
    for f in frames:
        _, _, s = sc.candidates(f)
        n0, cut, K = sc.retain(s, sc.REDO_N)
        assert n0 > sc.REDO_N and sc.REDO_N <= K <= sc.KMAX
        # at the forced gate no more than N candidates are left: select sends the frame to the redo list
        assert (s >= sc.REDO_GATE).sum() <= sc.REDO_N
    # as a pyramid every level adds keypoints, so the redo loop appends behind a non-zero base
    for i, f in enumerate(frames):
        kp, _ = sc.expected(("redo", i), f, sc.PYRAMID3, sc.REDO_N)
        assert (np.bincount(kp["octave"], minlength=3) > 0).all()
    mixed = sc.redo_frames(blank=True)
    assert len(sc.REDO_BLANK) == 12 > sc.REDO_WORKGROUPS
    for i in sc.REDO_BLANK:
        assert (mixed[i] == 128).all() and len(sc.candidates(mixed[i])[2]) == 0
    rest = [i for i in range(sc.REDO_FRAMES) if i not in sc.REDO_BLANK]
    assert all(np.array_equal(mixed[i], frames[i]) for i in rest)


def test_cells_frame_takes_anms(oracle):
    # ST_CELLS is raised inside the ANMS branch only
    _, _, s, (n0, cut, K) = counts("cells")
    N = sc.nfeatures("cells")
    assert n0 > N and N <= K <= sc.KMAX
    assert 128 * 64 > 4096 >= 64 * 64
