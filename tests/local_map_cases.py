"""Helpers of the local-map matching tests (test_local_map_reference.py on the CPU,
test_gpu_localmap.py on the GPU): an independent formulation of mage_local_map_match's rule and the
scenes in which a point's hidden keypoint, the starting mask and the order of the points decide
results.  Not a test module (nothing is collected).

loop_reference is written from the rule in include/mage_hot.h (mage_local_map_match) in its
order-free form and shares no code with oracle/orb_oracle.c: per point, the candidates are the
keypoints that are available, not hidden, inside the f32 box, of the point's octave and within
maxHammingDist; best = min (distance, index); second = min(maxHammingDist + 1, the smallest distance
among candidates with an index below the best's); the point takes the best when second - best >
minHammingDifference.

Which path of mageslam_amd/csrc/localmap.hip a scene reaches, with the counts loop_reference gives for
the chosen seeds (test_local_map_reference.py asserts floors far below them, on loop_reference alone).
"differ" = results that differ from the run without hides; "later" = points whose hidden keypoint is
the result of a later point; "assoc" = share of hidden keypoints already associated at the start;
"kept > 8" / "kept == 8" = points with a hide whose candidates under the starting mask, the hidden one
left out, overflow lm_cand_kernel's kept list (lm_resolve_kernel rescans the band through scan_band) /
fill it exactly.

    scene    nq    nt  r, md, mdiff  seed  hidden  differ  later  assoc  other
    G1     2500   800  1.5,  30, 1      1     284     151     42   33 %  hidden is the only start candidate: 240
    G2     2500   800  3.0, 256, 0      1     988      78     77   28 %  hidden and > 9 start candidates: 173, exactly 9: 108, most 15;
                                                                         kept > 8: 22, kept == 8: 43
    G3     2500   800  0.5,   8, 2      2      58      25      0   50 %
    G4     3000  4096  1.5,  30, 1      7     949     515    143   27 %  three 1024-point blocks of lm_resolve_kernel, every mask word
    G5      700   300  3.0,  30, 1      4     113      58     14   28 %  one block, a ragged last 64-lane round

G1 (at most 5 start candidates per point): the kept list, where lm_cand_kernel alone honours the hide.
G2 (maxHammingDist 256: every box keypoint of the octave is a candidate): kept lists of exactly 8 and
the overflow rescan with a hide.  G3: radius 0.5 and minHammingDifference 2, boxes of two grid cells.
Every scene has a point with hide == 0.  At a point's turn its hidden keypoint was still unassociated
and ahead of every other candidate in 137 (G1), 26 (G2), 26 (G3), 400 (G4) and 49 (G5) points.

    blob_scene(8 / 9 / 40), hide[q] = q % blob on even q, minHammingDifference 0 / 1 / 3:
        results that differ from the run without hides
                 mdiff 0  mdiff 1  mdiff 3
        blob 8        5        5        5     kept lists of 7 (with a hide) and 8
        blob 9        4        7        3     a hide leaves a kept list of exactly 8; without one, the first overflow
        blob 40      11        4        5     39 or 40 candidates: the hide is honoured only by the rescan
        no point takes its own hidden keypoint

    blocks_scene(): 3072 points = three blocks of lm_resolve_kernel; the first takes 513 keypoints,
        the middle one (an octave no keypoint has) compacts to nothing, the third (the first again)
        takes 12 keypoints that the first left.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from mageslam_amd._lib import KP_DTYPE
from match_cases import POPCOUNT, radius_sets

ROW_CHUNK = 256  # rows of the (point, keypoint) candidate matrix held at a time


def start_candidates(qpos, qoct, qdesc, tkp, tdesc, radius, md):
    """Per point, the keypoints it can be offered when every keypoint is unassociated: inside the f32
    box (>= p - r, <= p + r, r and both edges in float32), the point's octave, distance <= md.
    -> a list of (ascending keypoint indices, their distances), one entry per point.  The matrix is
    formed ROW_CHUNK points at a time and distances are computed for the box pairs only."""
    qpos = np.asarray(qpos, np.float32).reshape(-1, 2)
    qoct = np.asarray(qoct, np.int64)
    r = np.float32(radius)
    x, y, o = tkp["x"][None], tkp["y"][None], tkp["octave"].astype(np.int64)[None]
    out = []
    for i0 in range(0, len(qpos), ROW_CHUNK):
        p = qpos[i0:i0 + ROW_CHUNK]
        x0, x1 = (p[:, :1] - r).astype(np.float32), (p[:, :1] + r).astype(np.float32)
        y0, y1 = (p[:, 1:] - r).astype(np.float32), (p[:, 1:] + r).astype(np.float32)
        box = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (o == qoct[i0:i0 + ROW_CHUNK, None])
        for k in range(len(p)):
            idx = np.flatnonzero(box[k])
            d = POPCOUNT[tdesc[idx] ^ qdesc[i0 + k][None]].sum(1, dtype=np.int64)
            keep = d <= md
            out.append((idx[keep], d[keep]))
    return out


def loop_reference(qpos, qoct, qdesc, hide, tkp, tdesc, mask, radius, md, mdiff):
    """The per-point loop in its order-free form (see the module docstring).
    -> (result (nq,) int32, final mask (nt,) bool, diagnostics) with, per point: `ncand` the number
    of candidates at the point's turn, `hide_avail` whether its hidden keypoint was still
    unassociated at its turn, `hide_best` whether that keypoint was then a candidate but for the
    hide and ahead of every other one in (distance, index)."""
    nq = len(np.asarray(qpos).reshape(-1, 2))
    hide = np.full(nq, -1, np.int64) if hide is None else np.asarray(hide, np.int64)
    avail = np.array(mask, bool).reshape(len(tkp)).copy()
    start = start_candidates(qpos, qoct, qdesc, tkp, tdesc, radius, md)
    result = np.full(nq, -1, np.int32)
    diag = SimpleNamespace(ncand=np.zeros(nq, np.int64), hide_avail=np.zeros(nq, bool), hide_best=np.zeros(nq, bool))
    for q, (idx, d) in enumerate(start):
        h = int(hide[q])
        free = avail[idx]
        cand = [(int(dd), int(t)) for t, dd, f in zip(idx, d, free) if f and t != h]
        diag.ncand[q] = len(cand)
        if h >= 0:
            diag.hide_avail[q] = avail[h]
            mine = [(int(dd), int(t)) for t, dd, f in zip(idx, d, free) if f and t == h]
            diag.hide_best[q] = bool(mine) and (not cand or mine[0] < min(cand))
        if not cand:
            continue
        best, tb = min(cand)
        second = min([md + 1] + [dd for dd, t in cand if t < tb])
        if second - best > mdiff:
            result[q] = tb
            avail[tb] = False
    return result, avail, diag


def frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return SimpleNamespace(**arrays)


# name -> (seed, nq, nt, radius, maxHammingDist, minHammingDifference)
G_SCENES = {"G1": (1, 2500, 800, 1.5, 30, 1), "G2": (1, 2500, 800, 3.0, 256, 0), "G3": (2, 2500, 800, 0.5, 8, 2),
            "G4": (7, 3000, 4096, 1.5, 30, 1), "G5": (4, 700, 300, 3.0, 30, 1)}


def grid_scene(seed, nq, nt, radius=1.5, md=30):
    """match_cases.radius_sets' construction (targets on the integer 60 x 40 grid, queries at x + 0.5,
    two octaves, a palette of 6 descriptors with 2 % noise on the targets) as a local-map problem: a
    starting mask with 70 % available, drawn independently of everything else, and per point with
    probability 0.4 a hide drawn uniformly from the point's start candidates at (radius, md),
    whatever their mask bits; -1 otherwise and for a point without start candidates."""
    rng = np.random.default_rng(seed)
    qk, qd, tk, td, _ = radius_sets(nq, nt, rng)
    qp = np.stack([qk["x"], qk["y"]], 1).astype(np.float32)
    qo = qk["octave"].astype(np.int32)
    mask = rng.random(nt) < 0.7
    wants, pick = rng.random(nq) < 0.4, rng.random(nq)
    start = start_candidates(qp, qo, qd, tk, td, radius, md)
    hide = np.full(nq, -1, np.int32)
    for q, (idx, _) in enumerate(start):
        if wants[q] and len(idx):
            hide[q] = idx[int(pick[q] * len(idx))]
    nstart = np.array([len(idx) for idx, _ in start])
    return frozen(qp=qp, qo=qo, qd=qd, hide=hide, tk=tk, td=td, mask=mask, nstart=nstart)


@functools.lru_cache(maxsize=None)
def g_scene(name):
    """Scene `name` of G_SCENES with its settings, loop_reference's outcome with the hides (`ref`,
    `ref_mask`, `diag`) and without them (`ref_nohide`), computed once and read-only."""
    seed, nq, nt, radius, md, mdiff = G_SCENES[name]
    s = grid_scene(seed, nq, nt, radius, md)
    s.radius, s.md, s.mdiff = radius, md, mdiff
    s.ref, s.ref_mask, s.diag = loop_reference(s.qp, s.qo, s.qd, s.hide, s.tk, s.td, s.mask, radius, md, mdiff)
    s.ref_nohide, _, _ = loop_reference(s.qp, s.qo, s.qd, None, s.tk, s.td, s.mask, radius, md, mdiff)
    for a in (s.ref, s.ref_mask, s.ref_nohide):
        a.setflags(write=False)
    return s


def hide_counts(s):
    """The counts of the module docstring's table for a scene with `ref` / `ref_nohide`."""
    hid = s.hide >= 0
    taken_at = np.full(len(s.tk), -1, np.int64)  # a keypoint is taken once at the most
    taken_at[s.ref[s.ref >= 0]] = np.flatnonzero(s.ref >= 0)
    later = hid & (taken_at[np.where(hid, s.hide, 0)] > np.arange(len(s.hide)))
    kept = np.zeros(len(s.hide), np.int64)  # lm_cand_kernel's count: starting mask, the hidden one left out
    for q, (idx, _) in enumerate(start_candidates(s.qp, s.qo, s.qd, s.tk, s.td, s.radius, s.md)):
        kept[q] = (s.mask[idx] & (idx != s.hide[q])).sum()
    return dict(hidden=int(hid.sum()), differ=int((s.ref != s.ref_nohide).sum()), later=int(later.sum()),
                assoc=float((~s.mask[s.hide[hid]]).mean()), hide0=int((s.hide == 0).sum()),
                only=int((hid & (s.nstart == 1)).sum()), over9=int((hid & (s.nstart > 9)).sum()),
                exact9=int((hid & (s.nstart == 9)).sum()), most=int(s.nstart.max()),
                kept_over=int((hid & (kept > 8)).sum()), kept_full=int((hid & (kept == 8)).sum()))


def frame(rng, n, w=1280, h=720, octaves=1, cluster=None):
    """test_gpu_localmap.py's frame generator, draw for draw."""
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.uniform(0, w, n).astype(np.float32)
    kp["y"] = rng.uniform(0, h, n).astype(np.float32)
    if cluster:
        c = cluster
        kp["x"][:c] = np.float32(640) + rng.uniform(-6, 6, c).astype(np.float32)
        kp["y"][:c] = np.float32(360) + rng.uniform(-6, 6, c).astype(np.float32)
    kp["octave"] = rng.integers(0, octaves, n)
    kp["size"] = 15
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return kp, desc


BLOBS = (8, 9, 40)
BLOB_MDIFFS = (0, 1, 3)
BLOB_RADIUS, BLOB_MD = 8.0, 30


@functools.lru_cache(maxsize=None)
def blob_scene(blob):
    """The generator of test_local_map_match_conflicts_and_overflow (same seed, flips and counts: a
    blob of near-identical keypoints inside one search box, every point projecting into it, full
    mask) plus hide[q] = q % blob for even q and -1 otherwise."""
    rng = np.random.default_rng(7)
    nq, kflip, qflip = (200, 0.05, 0.03) if blob == 40 else (70, 0.3, 0.1)
    tk, td = frame(rng, 1000, cluster=blob)
    td[:blob] = td[0] ^ (rng.random((blob, 32)) < kflip).astype(np.uint8)
    qp = np.float32([640, 360]) + rng.uniform(-2, 2, (nq, 2)).astype(np.float32)
    qo = np.zeros(nq, np.int32)
    qd = np.repeat(td[:1], nq, 0) ^ (rng.random((nq, 32)) < qflip).astype(np.uint8)
    q = np.arange(nq)
    hide = np.where(q % 2 == 0, q % blob, -1).astype(np.int32)
    return frozen(qp=qp, qo=qo, qd=qd, hide=hide, tk=tk, td=td, mask=np.ones(1000, bool))


BLOCKS_RADIUS, BLOCKS_MD, BLOCKS_MDIFF = 8.0, 30, 0


@functools.lru_cache(maxsize=None)
def blocks_scene():
    """3072 points, three 1024-point blocks of lm_resolve_kernel, against a 320 x 240 frame of 700
    keypoints whose descriptors come from a palette of 8 with 3 % noise, so that a box holds
    runners-up.  Points 0..1023 are noisy copies of 600 of the keypoints, points 2048..3071 are the
    same points again, and points 1024..2047 carry octave 5, which no keypoint has: that block
    compacts to nothing.  Full mask."""
    rng = np.random.default_rng(31)
    nt, n = 700, 1024
    tk, _ = frame(rng, nt, w=320, h=240)
    pal = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    td = np.packbits(np.unpackbits(pal[rng.integers(0, 8, nt)], axis=1) ^ (rng.random((nt, 256)) < 0.03), axis=1)
    src = rng.permutation(nt)[:600][rng.integers(0, 600, n)]
    pos = np.stack([tk["x"][src], tk["y"][src]], 1) + rng.uniform(-3, 3, (n, 2)).astype(np.float32)
    qd1 = np.packbits(np.unpackbits(td[src], axis=1) ^ (rng.random((n, 256)) < 0.02), axis=1)
    qp = np.concatenate([pos, pos, pos]).astype(np.float32)
    qd = np.concatenate([qd1, qd1, qd1])
    qo = np.concatenate([np.zeros(n), np.full(n, 5), np.zeros(n)]).astype(np.int32)
    return frozen(qp=qp, qo=qo, qd=qd, hide=None, tk=tk, td=td, mask=np.ones(nt, bool))


def signed_zero_sets(radius):
    """test_gpu_match_paths.py::test_signed_zero_band_sets' sets, draw for draw, as a local-map
    problem (full mask, no hides): targets with y in {-2, -1, -0.0, +0.0, 1, 2}, queries whose band
    edges land on both zeros.  The settings are SIGNED_ZERO_SETTINGS."""
    rng = np.random.default_rng(17)
    ys = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], np.float32)
    nt, nq = 200, 96
    tk = np.zeros(nt, KP_DTYPE)
    tk["x"] = rng.integers(0, 6, nt).astype(np.float32)
    tk["y"] = ys[rng.integers(0, 6, nt)]
    tk["octave"] = rng.integers(0, 2, nt)
    pal = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    td = pal[rng.integers(0, 6, nt)] ^ (rng.random((nt, 32)) < 0.02).astype(np.uint8)
    qk = np.zeros(nq, KP_DTYPE)
    qk["x"] = rng.integers(0, 6, nq).astype(np.float32)
    qy = np.array([radius, -radius, -0.0, 0.0, 1.0, -2.0], np.float32)
    qk["y"] = qy[np.arange(nq) % 6]
    qk["octave"] = rng.integers(0, 2, nq)
    qd = pal[rng.integers(0, 6, nq)]
    return frozen(qp=np.stack([qk["x"], qk["y"]], 1), qo=qk["octave"].astype(np.int32), qd=qd, hide=None, tk=tk, td=td,
                  mask=np.ones(nt, bool))


SIGNED_ZERO_RADII = (0.0, 1.0, 2.0)
SIGNED_ZERO_SETTINGS = ((256, 0), (30, 1), (8, 2))


# ------------------------- hand-written known answers ---------------------------------------------


def desc_at(d):
    """A descriptor at Hamming distance d from the all-zero one."""
    bits = np.zeros(256, np.uint8)
    bits[:d] = 1
    return np.packbits(bits)


def keypoints(xs, ys, octs=0):
    k = np.zeros(len(xs), KP_DTYPE)
    k["x"], k["y"], k["octave"] = xs, ys, octs
    return k


def micro(name, txy, tdist, result, final_mask, *, toct=0, qxy=((10.0, 10.0),), qoct=0, hide=None, mask=None,
          radius=5.0, md=30, mdiff=1):
    """One known answer: keypoints at txy with descriptors at distance tdist from the all-zero
    descriptor every point carries; `result` and `final_mask` are the expected outcome."""
    nt, nq = len(txy), len(qxy)
    txy = np.asarray(txy, np.float32).reshape(nt, 2)
    return SimpleNamespace(
        name=name, qp=np.asarray(qxy, np.float32).reshape(nq, 2), qo=np.full(nq, qoct, np.int32),
        qd=np.zeros((nq, 32), np.uint8), hide=None if hide is None else np.asarray(hide, np.int32),
        tk=keypoints(txy[:, 0], txy[:, 1], toct), td=np.stack([desc_at(d) for d in tdist]),
        mask=np.ones(nt, bool) if mask is None else np.asarray(mask, bool), radius=radius, md=md, mdiff=mdiff,
        result=list(result), final_mask=list(final_mask))


def packing_extremes(mdiff, first_available):
    """4096 keypoints with keypoints 0 and 4095 at the point's position carrying all-ones descriptors
    (distance 256, the largest, at the smallest and the largest index), the others far away."""
    nt = 4096
    tk = keypoints(np.full(nt, 500.0), np.full(nt, 500.0))
    tk["x"][[0, nt - 1]] = tk["y"][[0, nt - 1]] = 10.0
    td = np.zeros((nt, 32), np.uint8)
    td[[0, nt - 1]] = 255
    mask = np.ones(nt, bool)
    mask[0] = first_available
    return SimpleNamespace(qp=np.float32([[10, 10]]), qo=np.zeros(1, np.int32), qd=np.zeros((1, 32), np.uint8), hide=None,
                           tk=tk, td=td, mask=mask, radius=1.0, md=256, mdiff=mdiff)


def known_answers():
    """The micro-cases; every expected value is a literal.  A = keypoint 0, B = keypoint 1, both at
    the point's position unless stated; the point is at (10, 10), radius 5, md 30, mdiff 1."""
    at, far = (10.0, 10.0), (100.0, 100.0)
    nan, inf = float("nan"), float("inf")
    cases = [
        # A at distance 5, B at 0: B is the best and the second is A's 5; with B hidden A is alone and
        # its second is md + 1 = 31; with A hidden B is alone
        micro("d5_d0", [at, at], [5, 0], [1], [1, 0]),
        micro("d5_d0_hide_B", [at, at], [5, 0], [0], [0, 1], hide=[1]),
        micro("d5_d0_hide_A", [at, at], [5, 0], [1], [1, 0], hide=[0]),
        # 3 and 2: 3 - 2 is not > 1; hiding A leaves B alone; swapped, A is the best and the first seen,
        # so its second is 31
        micro("d3_d2", [at, at], [3, 2], [-1], [1, 1]),
        micro("d3_d2_hide_A", [at, at], [3, 2], [1], [1, 0], hide=[0]),
        micro("d2_d3", [at, at], [2, 3], [0], [0, 1]),
        # the hidden keypoint (2) is the only candidate of three identical points and the first hides
        # it: the second takes it, the third finds it gone
        micro("only_candidate", [far, far, at], [0, 0, 4], [-1, 2, -1], [1, 1, 0], qxy=(at, at, at), hide=[2, -1, -1]),
        # the hidden keypoint is associated at the start: as without the hide, and it stays associated
        micro("hidden_associated", [at, at], [5, 0], [0], [0, 0], hide=[1], mask=[1, 0]),
        micro("hidden_associated_nohide", [at, at], [5, 0], [0], [0, 0], mask=[1, 0]),
        # hides that cannot matter: keypoint 2 in another octave, keypoint 3 outside the box
        micro("hide_other_octave", [at, at, at, far], [5, 0, 0, 0], [1], [1, 0, 1, 1], toct=[0, 0, 1, 0], hide=[2]),
        micro("hide_outside_box", [at, at, at, far], [5, 0, 0, 0], [1], [1, 0, 1, 1], toct=[0, 0, 1, 0], hide=[3]),
        micro("hide_none", [at, at, at, far], [5, 0, 0, 0], [1], [1, 0, 1, 1], toct=[0, 0, 1, 0], hide=[-1]),
        # hide = 0 where keypoint 0 is the best: not taken; taken without the hide
        micro("hide_zero", [at, at], [0, 5], [1], [1, 0], hide=[0]),
        micro("hide_zero_off", [at, at], [0, 5], [0], [0, 1], hide=[-1]),
        # the box is inclusive on all four edges and exclusive one float beyond them
        micro("box_edges", [(5.0, 10.0), (15.0, 10.0), (10.0, 5.0), (10.0, 15.0)], [0, 1, 2, 3], [0, 1, 2, 3, -1],
              [0, 0, 0, 0], qxy=(at, at, at, at, at), mdiff=0),
        micro("box_beyond", [(np.nextafter(np.float32(5), np.float32(0)), 10.0), (np.nextafter(np.float32(15), np.float32(99)), 10.0),
                             (10.0, np.nextafter(np.float32(5), np.float32(0))), (10.0, np.nextafter(np.float32(15), np.float32(99)))],
              [0, 1, 2, 3], [-1], [1, 1, 1, 1], mdiff=0),
        # a NaN, +inf or -inf coordinate on either axis: no match for that point, and the finite point
        # after it takes its own keypoint (keypoint i at (20 i, 10))
        micro("non_finite", [(20.0 * i, 10.0) for i in range(6)], [0] * 6, [-1, 0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5], [0] * 6,
              qxy=((nan, 10.0), (0.0, 10.0), (20.0, nan), (20.0, 10.0), (inf, 10.0), (40.0, 10.0), (60.0, inf), (60.0, 10.0),
                   (-inf, 10.0), (80.0, 10.0), (100.0, -inf), (100.0, 10.0))),
    ]
    # 256 at indices 0 and 4095: mdiff 0 takes the lower index (second = 257); with keypoint 0
    # associated 4095 is alone; 257 - 256 is not > 1
    for name, mdiff, first, res in (("pack_0", 0, True, 0), ("pack_4095", 0, False, 4095), ("pack_mdiff1", 1, True, -1),
                                    ("pack_4095_mdiff1", 1, False, -1)):
        c = packing_extremes(mdiff, first)
        c.name, c.result = name, [res]
        fm = c.mask.copy()
        if res >= 0:
            fm[res] = False
        c.final_mask = list(fm)
        cases.append(c)
    return cases


def mask_edge_scene(nt):
    """One point per keypoint, keypoint i at (100 i, 50) with its own random descriptor; the keypoints
    nt - 1, nt - 3, ... are available at the start; the point aimed at keypoint nt - 1 hides it.
    -> scene with the expected `result` and `final_mask`."""
    rng = np.random.default_rng(nt)
    tk = keypoints(100.0 * np.arange(nt), np.full(nt, 50.0))
    td = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    i = np.arange(nt)
    mask = (nt - 1 - i) % 2 == 0
    hide = np.where(i == nt - 1, nt - 1, -1).astype(np.int32)
    result = np.where(mask & (i != nt - 1), i, -1).astype(np.int32)
    return SimpleNamespace(qp=np.stack([tk["x"], tk["y"]], 1), qo=np.zeros(nt, np.int32), qd=td.copy(), hide=hide, tk=tk, td=td,
                           mask=mask, radius=8.0, md=30, mdiff=1, result=result, final_mask=i == nt - 1)


MASK_EDGE_NT = (1, 31, 32, 33, 63, 64, 65)
