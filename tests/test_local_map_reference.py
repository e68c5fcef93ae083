"""The oracle's local-map loop (oracle/orb_oracle.c oracle_local_map_match), the reference of
mage_local_map_match and of its twins (new-point association, the third frame of the monocular map
initialisation, relocalisation), pinned on the CPU: against local_map_cases.loop_reference, an
independent order-free formulation of the rule in include/mage_hot.h, on scenes where hidden
keypoints, the starting mask and the order of the points decide results, and against hand-written
known answers.  The conditions that keep those scenes from being vacuous are asserted here, on
loop_reference alone; test_gpu_localmap.py runs the same scenes on the GPU.

With the hide ignored in a copy of the oracle (`hidden` never set), 16 of this module's 25 tests
fail: the comparison on every G scene and on every blob combination, the known answers and the mask
edge scenes; the floors, the blocks and the signed-zero sets (no hides) pass."""
import numpy as np
import pytest

import local_map_cases as L

# scene -> floors: results that differ from the run without hides, points whose hidden keypoint a
# later point takes, hidden-only-start-candidate, hidden with > 9 start candidates, with exactly 9
FLOORS = {"G1": dict(differ=50, later=15, only=60), "G2": dict(differ=30, later=30, over9=50, exact9=20),
          "G3": dict(differ=15), "G4": dict(differ=150, later=50), "G5": dict(differ=15, later=4)}


def oracle_run(oracle, s, hide, radius, md, mdiff):
    o, om = oracle.local_map_match(s.qp, s.qo, s.qd, hide, s.tk, s.td, s.mask.astype(np.uint8), radius, md, mdiff)
    return o, om.astype(bool)


def assert_oracle_is_reference(oracle, s, hide, radius, md, mdiff, ref=None):
    r, rm = ref if ref is not None else L.loop_reference(s.qp, s.qo, s.qd, hide, s.tk, s.td, s.mask, radius, md, mdiff)[:2]
    o, om = oracle_run(oracle, s, hide, radius, md, mdiff)
    assert np.array_equal(o, r), np.flatnonzero(o != r)[:10]
    assert np.array_equal(om, rm), np.flatnonzero(om != rm)[:10]
    return r


@pytest.mark.parametrize("name", list(L.G_SCENES))
def test_grid_scene_floors(name):
    """The scene is not vacuous, by loop_reference alone: hides change results, hidden keypoints go
    to later points, the starting mask covers hidden keypoints, keypoint 0 is hidden somewhere."""
    s = L.g_scene(name)
    c = L.hide_counts(s)
    print(name, c)
    for key, floor in FLOORS[name].items():
        assert c[key] >= floor, (key, c[key], floor)
    assert c["assoc"] >= 0.10
    assert c["hide0"] >= 1
    if name == "G2":  # the kernel's own count (starting mask, the hidden keypoint left out) reaches both paths
        assert c["kept_over"] >= 10 and c["kept_full"] >= 10
    # the first result that differs belongs to a point whose hidden keypoint was still unassociated
    first = int(np.flatnonzero(s.ref != s.ref_nohide)[0])
    assert s.hide[first] >= 0 and s.diag.hide_avail[first]
    assert s.diag.hide_best.any()
    assert not ((s.ref == s.hide) & (s.hide >= 0)).any()  # no point takes its own hidden keypoint


@pytest.mark.parametrize("name", list(L.G_SCENES))
def test_oracle_is_loop_reference_grid(oracle, name):
    s = L.g_scene(name)
    assert_oracle_is_reference(oracle, s, s.hide, s.radius, s.md, s.mdiff, ref=(s.ref, s.ref_mask))
    no_hide = assert_oracle_is_reference(oracle, s, None, s.radius, s.md, s.mdiff)
    assert np.array_equal(no_hide, s.ref_nohide)
    all_none = np.full(len(s.hide), -1, np.int32)  # an array of -1 is no hide
    o, _ = oracle_run(oracle, s, all_none, s.radius, s.md, s.mdiff)
    assert np.array_equal(o, s.ref_nohide)


@pytest.mark.parametrize("mdiff", L.BLOB_MDIFFS)
@pytest.mark.parametrize("blob", L.BLOBS)
def test_oracle_is_loop_reference_blob(oracle, blob, mdiff):
    """The blob of test_local_map_match_conflicts_and_overflow without hides and with hide[q] =
    q % blob on even q: at least 2 results differ, and no point takes its own hidden keypoint."""
    s = L.blob_scene(blob)
    plain = assert_oracle_is_reference(oracle, s, None, L.BLOB_RADIUS, L.BLOB_MD, mdiff)
    r, _, diag = L.loop_reference(s.qp, s.qo, s.qd, s.hide, s.tk, s.td, s.mask, L.BLOB_RADIUS, L.BLOB_MD, mdiff)
    assert (r != plain).sum() >= 2
    assert ((r == s.hide) & (s.hide >= 0)).sum() == 0
    assert_oracle_is_reference(oracle, s, s.hide, L.BLOB_RADIUS, L.BLOB_MD, mdiff)
    first = diag.ncand[0] + (1 if s.hide[0] >= 0 else 0)  # point 0 sees the whole blob
    assert first == blob if blob < 40 else first > 8


def test_oracle_is_loop_reference_blocks(oracle):
    s = L.blocks_scene()
    r = assert_oracle_is_reference(oracle, s, None, L.BLOCKS_RADIUS, L.BLOCKS_MD, L.BLOCKS_MDIFF)
    first, middle, third = (r[i:i + 1024] for i in (0, 1024, 2048))
    assert (first >= 0).sum() >= 300
    assert (middle >= 0).sum() == 0
    assert 1 <= (third >= 0).sum() < (first >= 0).sum()
    assert not np.isin(third[third >= 0], first[first >= 0]).any()  # keypoints that the first block left


@pytest.mark.parametrize("radius", L.SIGNED_ZERO_RADII)
def test_oracle_is_loop_reference_signed_zero(oracle, radius):
    s = L.signed_zero_sets(radius)
    for md, mdiff in L.SIGNED_ZERO_SETTINGS:
        r = assert_oracle_is_reference(oracle, s, None, radius, md, mdiff)
        assert (s.tk["y"][r[r >= 0]] == 0).any()


def test_local_map_match_known_answers(oracle):
    """Hand-written answers (local_map_cases.known_answers: every expected value is a literal there),
    on the oracle and on loop_reference."""
    seen = set()
    for c in L.known_answers():
        o, om = oracle_run(oracle, c, c.hide, c.radius, c.md, c.mdiff)
        assert list(o) == c.result, (c.name, list(o))
        assert list(om) == [bool(v) for v in c.final_mask], c.name
        r, rm, _ = L.loop_reference(c.qp, c.qo, c.qd, c.hide, c.tk, c.td, c.mask, c.radius, c.md, c.mdiff)
        assert list(r) == c.result and np.array_equal(rm, om), c.name
        seen.add(c.name)
    assert len(seen) == 21


def test_mask_edge_scenes(oracle):
    for nt in L.MASK_EDGE_NT:
        c = L.mask_edge_scene(nt)
        o, om = oracle_run(oracle, c, c.hide, c.radius, c.md, c.mdiff)
        assert np.array_equal(o, c.result) and np.array_equal(om, c.final_mask), nt
        assert c.mask[nt - 1] and o[nt - 1] == -1 and om[nt - 1]
