"""TrackLocalMap's per-map-point matching (TrackLocalMap.cpp:175-256; mage_local_map_match) against
the oracle's literal sequential loop (oracle/orb_oracle.c oracle_local_map_match): identical
results and final masks.  The GPU resolves the points 64 at a time with conflict restarts, so the
cases below force what makes the sequential order matter: many points competing for the same
keypoints (duplicate map points), hidden keypoints of pose-estimation outliers, keypoints already
associated at the start, dense clusters that overflow a point's kept candidates, several octaves."""
import numpy as np
import pytest

import local_map_cases as L
from mageslam_amd import matcher
from mageslam_amd._lib import KP_DTYPE, MAGE_EINVAL, MAGE_EUNSUPPORTED, MageError

pytestmark = pytest.mark.gpu


def frame(rng, n, w=1280, h=720, octaves=1, cluster=None):
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.uniform(0, w, n).astype(np.float32)
    kp["y"] = rng.uniform(0, h, n).astype(np.float32)
    if cluster:  # a dense blob: more than 8 candidates inside one 16 x 16 box
        c = cluster
        kp["x"][:c] = np.float32(640) + rng.uniform(-6, 6, c).astype(np.float32)
        kp["y"][:c] = np.float32(360) + rng.uniform(-6, 6, c).astype(np.float32)
    kp["octave"] = rng.integers(0, octaves, n)
    kp["size"] = 15
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return kp, desc


def queries(rng, kp, desc, nq, dup=3, noise_bits=0.04, jitter=3.0):
    """Map points near keypoints, each physical point repeated `dup` times (different keyframes)."""
    base = rng.integers(0, len(kp), nq // dup + 1)
    src = np.repeat(base, dup)[:nq]
    pos = np.stack([kp["x"][src], kp["y"][src]], 1) + rng.uniform(-jitter, jitter, (nq, 2)).astype(np.float32)
    flip = (rng.random((nq, 256)) < noise_bits)
    bits = np.unpackbits(desc[src], axis=1) ^ flip
    qd = np.packbits(bits.astype(np.uint8), axis=1)
    return pos.astype(np.float32), kp["octave"][src].astype(np.int32), qd, src


def run_both(qp, qo, qd, kp, desc, mask, hide=None, radius=8.0, md=30, mdiff=1):
    from oracle import oracle as O

    g, gm = matcher.LocalMapMatch(qp, qo, qd, kp, desc, mask, radius, md, mdiff, queryHidden=hide)
    o, om = O.local_map_match(qp, qo, qd, hide, kp, desc, mask.astype(np.uint8), radius, md, mdiff)
    return g, gm, o, om.astype(bool)


@pytest.mark.parametrize("seed,nt,nq,dup,octaves", [(0, 2000, 3000, 3, 1), (1, 4096, 8000, 4, 1), (2, 500, 2000, 6, 2),
                                                    (3, 2000, 64, 2, 1), (4, 2000, 65, 1, 1), (5, 3000, 6000, 2, 3)])
def test_local_map_match_matches_oracle(gpu, seed, nt, nq, dup, octaves):
    rng = np.random.default_rng(seed)
    kp, desc = frame(rng, nt, octaves=octaves)
    qp, qo, qd, src = queries(rng, kp, desc, nq, dup=dup)
    mask = rng.random(nt) < 0.7  # 30 % already associated by the pose-estimation matches
    hide = np.where(rng.random(nq) < 0.2, rng.integers(0, nt, nq), -1).astype(np.int32)
    g, gm, o, om = run_both(qp, qo, qd, kp, desc, mask, hide)
    assert np.array_equal(g, o)
    assert np.array_equal(gm, om)
    assert (o >= 0).sum() > nq // (4 * dup)  # the case really associates keypoints


def start_candidates(qp, qo, qd, kp, desc, radius, md):
    """Per query, the keypoints it can be offered when every keypoint is unassociated: inside the f32
    box, the query's octave, Hamming distance <= md."""
    r = np.float32(radius)
    x, y = kp["x"][None], kp["y"][None]
    box = (x >= qp[:, :1] - r) & (x <= qp[:, :1] + r) & (y >= qp[:, 1:] - r) & (y <= qp[:, 1:] + r)
    d = np.unpackbits(qd[:, None] ^ desc[None], axis=2).sum(2)
    return (box & (kp["octave"][None] == qo[:, None]) & (d <= md)).sum(1)


@pytest.mark.parametrize("blob", [8, 9, 40])
def test_local_map_match_conflicts_and_overflow(gpu, blob):
    """A dense blob of keypoints with near-identical descriptors inside one search box and map points
    all projecting into it, so that each success changes the next points' results.  40 keypoints and
    200 points: every point sees > 8 candidates (overflow rescans).  8 and 9 keypoints and 70 points
    (two 64-lane rounds): the kept list exactly full, and the first overflow; there the descriptors
    are spread wider, so that the points still take keypoints at minHammingDifference 3."""
    rng = np.random.default_rng(7)
    nq, kflip, qflip = (200, 0.05, 0.03) if blob == 40 else (70, 0.3, 0.1)
    kp, desc = frame(rng, 1000, cluster=blob)
    desc[:blob] = desc[0] ^ (rng.random((blob, 32)) < kflip).astype(np.uint8)
    qp = np.float32([640, 360]) + rng.uniform(-2, 2, (nq, 2)).astype(np.float32)
    qo = np.zeros(nq, np.int32)
    qd = np.repeat(desc[:1], nq, 0) ^ (rng.random((nq, 32)) < qflip).astype(np.uint8)
    cand = start_candidates(qp, qo, qd, kp, desc, 8.0, 30)
    assert (cand == blob).any() if blob < 40 else (cand > 8).all(), np.bincount(cand)
    for mdiff in (0, 1, 3):
        g, gm, o, om = run_both(qp, qo, qd, kp, desc, np.ones(1000, bool), None, 8.0, 30, mdiff)
        assert np.array_equal(g, o) and np.array_equal(gm, om), mdiff
    assert (o >= 0).sum() >= 5


def test_local_map_match_edges(gpu):
    rng = np.random.default_rng(9)
    kp, desc = frame(rng, 300)
    qp, qo, qd, _ = queries(rng, kp, desc, 100)
    # nothing available, empty target set, empty query set, radius 0, maxDist -1
    g, gm, o, om = run_both(qp, qo, qd, kp, desc, np.zeros(300, bool))
    assert (g == -1).all() and np.array_equal(g, o)
    g, _ = matcher.LocalMapMatch(qp, qo, qd, kp[:0], desc[:0], np.zeros(0, bool))
    assert (g == -1).all()
    g, gm = matcher.LocalMapMatch(qp[:0], qo[:0], qd[:0], kp, desc, np.ones(300, bool))
    assert len(g) == 0 and gm.all()
    for radius, md in ((0.0, 30), (8.0, -1), (30.0, 256)):
        g, gm, o, om = run_both(qp, qo, qd, kp, desc, np.ones(300, bool), None, radius, md, 1)
        assert np.array_equal(g, o) and np.array_equal(gm, om), (radius, md)


# ------------------------- hidden keypoints and masks that decide ---------------------------------
# The scenes of local_map_cases.py (its docstring says which kernel path each reaches);
# test_local_map_reference.py asserts on the CPU that hides, masks and order decide results in them.


def both_scene(s, hide, radius, md, mdiff):
    return run_both(s.qp, s.qo, s.qd, s.tk, s.td, s.mask, hide, radius, md, mdiff)


def assert_scene(s, hide, radius, md, mdiff, what=None):
    g, gm, o, om = both_scene(s, hide, radius, md, mdiff)
    assert np.array_equal(g, o), (what, np.flatnonzero(g != o)[:10])
    assert np.array_equal(gm, om), (what, np.flatnonzero(gm != om)[:10])
    return g, gm


@pytest.mark.parametrize("name", list(L.G_SCENES))
def test_local_map_match_hidden_grid(gpu, name):
    s = L.g_scene(name)
    g, gm = assert_scene(s, s.hide, s.radius, s.md, s.mdiff)
    assert np.array_equal(g, s.ref) and np.array_equal(gm, s.ref_mask)  # the independent formulation's too
    if name == "G2":  # again: the same bytes
        g2, gm2 = matcher.LocalMapMatch(s.qp, s.qo, s.qd, s.tk, s.td, s.mask, s.radius, s.md, s.mdiff, queryHidden=s.hide)
        assert g2.tobytes() == g.tobytes() and gm2.tobytes() == gm.tobytes()


@pytest.mark.parametrize("blob", L.BLOBS)
def test_local_map_match_hidden_blob(gpu, blob):
    """The blob of test_local_map_match_conflicts_and_overflow with hide[q] = q % blob on even q: with
    9 keypoints a hide leaves a kept list of exactly 8, with 40 only the rescan honours the hide."""
    s = L.blob_scene(blob)
    for mdiff in L.BLOB_MDIFFS:
        g, gm = assert_scene(s, s.hide, L.BLOB_RADIUS, L.BLOB_MD, mdiff, mdiff)
        assert ((g == s.hide) & (s.hide >= 0)).sum() == 0
        if blob == 40:
            g2, gm2 = matcher.LocalMapMatch(s.qp, s.qo, s.qd, s.tk, s.td, s.mask, L.BLOB_RADIUS, L.BLOB_MD, mdiff,
                                            queryHidden=s.hide)
            assert g2.tobytes() == g.tobytes() and gm2.tobytes() == gm.tobytes()


def test_local_map_match_blocks(gpu):
    """Three 1024-point blocks of lm_resolve_kernel, the middle one without a single candidate."""
    s = L.blocks_scene()
    g, _ = assert_scene(s, None, L.BLOCKS_RADIUS, L.BLOCKS_MD, L.BLOCKS_MDIFF)
    assert (g[1024:2048] == -1).all() and (g[:1024] >= 0).sum() > (g[2048:] >= 0).sum() >= 1


def test_local_map_match_known_answers(gpu):
    """The hand-written answers of local_map_cases.known_answers, the 4096-keypoint / distance-256
    packing extremes and the non-finite positions among them."""
    for c in L.known_answers():
        g, gm = assert_scene(c, c.hide, c.radius, c.md, c.mdiff, c.name)
        assert list(g) == c.result and list(gm) == [bool(v) for v in c.final_mask], (c.name, list(g))


def test_radius_match_packing_extremes(gpu):
    """radius.hip packs d << 12 | t and t << 9 | d as ordered_take.hpp does: keypoints 0 and 4095 at
    distance 256, keypoint 0 masked out."""
    from oracle import oracle as O

    c = L.packing_extremes(0, True)
    qk = L.keypoints(c.qp[:, 0], c.qp[:, 1])
    tmask = np.ones(len(c.tk), bool)
    tmask[0] = False
    for mask, train in ((tmask, 4095), (None, 0)):
        o = O.radius_match(qk, c.qd, c.tk, c.td, c.radius, tmask=None if mask is None else mask.astype(np.uint8),
                           max_distance=256, min_difference=0)
        g = matcher.RadiusMatch(qk, c.qd, c.tk, c.td, c.radius, maxHammingDist=256, minHammingDifference=0,
                                targetKeypointsMask=mask)
        assert [(int(m["query_idx"]), int(m["train_idx"]), float(m["distance"])) for m in o] == [(0, train, 256.0)]
        assert g.tobytes() == o.tobytes(), (g, o)


@pytest.mark.parametrize("nt", L.MASK_EDGE_NT)
def test_local_map_match_mask_word_edges(gpu, nt):
    """One point per keypoint around the 32-bit mask word edges, every second keypoint associated at
    the start, the last keypoint hidden from the point aimed at it: its bit survives."""
    c = L.mask_edge_scene(nt)
    g, gm = assert_scene(c, c.hide, c.radius, c.md, c.mdiff)
    assert np.array_equal(g, c.result) and np.array_equal(gm, c.final_mask)


def test_local_map_match_limits(gpu):
    rng = np.random.default_rng(3)
    kp, desc = frame(rng, 4097)
    qp, qo, qd, _ = queries(rng, kp, desc, 10)
    with pytest.raises(MageError) as e:
        matcher.LocalMapMatch(qp, qo, qd, kp, desc, np.ones(4097, bool))
    assert e.value.status == MAGE_EUNSUPPORTED
    for md in (257, -2):
        with pytest.raises(MageError) as e:
            matcher.LocalMapMatch(qp, qo, qd, kp[:100], desc[:100], np.ones(100, bool), maxHammingDist=md)
        assert e.value.status == MAGE_EINVAL
    g, gm, o, om = run_both(qp, qo, qd, kp[:4096], desc[:4096], np.ones(4096, bool))  # the largest frame passes
    assert np.array_equal(g, o) and np.array_equal(gm, om)
