"""Helpers of the matcher tests (test_match_reference.py, test_gpu_match_paths.py, test_gpu_bow.py):
descriptor and keypoint generators that put results where the kernels' paths differ, an independent
NumPy formulation of the two-way Match, and the canary check of the batched entry points' output
regions.  Not a test module (nothing is collected).

Which body of match_kernel (mageslam_amd/csrc/match.hip) a pair takes, from its B count nb, maxDist
and minDiff (DESIGN.md has the same table with the tests that reach each body):

    fp4 kernel               maxDist < 128, minDiff >= 1 and the B pitch (or the host count) <= 2048
    Keys16 resident          nb <= 2048, maxDist < 128, otherwise
    Keys32<false> resident   2048 < nb <= 2560, maxDist < 128
    Keys32<false> streaming  nb > 2560, maxDist < 128
    Keys32<true>  (PADMASK)  maxDist >= 128; resident for nb <= 2560, streaming above
"""
from __future__ import annotations

import numpy as np

from mageslam_amd._lib import DM_DTYPE, KP_DTYPE

CANARY = 0xA5

# (maxDist, minDiff): the packed-key bodies (Keys16, Keys32<false>, the fp4 kernel) and PADMASK
SETTINGS_PACKED = [(30, 0), (64, 0), (127, 0), (30, 1), (127, 2)]
SETTINGS_PADMASK = [(128, 1), (200, 0), (256, 0), (255, 3)]
SETTINGS = SETTINGS_PACKED + SETTINGS_PADMASK

# (radius, maxDist, minDiff) of the RadiusMatch cases
RADIUS_SETTINGS = [(1.5, 30, 1), (3.0, 256, 0), (0.5, 8, 2)]


def dm_bytes(m) -> np.ndarray:
    return np.ascontiguousarray(m).view(np.uint8).reshape(-1)


def match_sets(na: int, nb: int, seed: int):
    """A (na, 32) and B (nb, 32): B rows are noisy copies of random A rows (the flip mask is the AND
    of three random bytes, ~32 differing bits, so many pairs lie within 30..127); all-zero and all-one
    rows on both sides give the distances 0 and 256; duplicated B rows give exact ties, at the start
    and in the last (ragged) 32-column tile."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (max(na, nb), 32), dtype=np.uint8)
    base[:2] = 0
    base[2:4] = 255
    A = base[:na].copy()
    flip = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    flip &= rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    flip &= rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    B = base[rng.integers(0, na, nb)] ^ flip
    k = min(4, na, nb)
    B[:k] = A[:k]
    if nb >= 16:
        B[8:12] = B[12:16]
    if nb >= 40:
        B[nb - 8:nb - 4] = B[nb - 4:]
    return A, B


def radius_sets(nq: int, nt: int, rng, shift_y: float = 0.0):
    """The generator of test_radius_match_ties: targets on an integer 60 x 40 grid, queries at
    x + 0.5, two octaves, a palette of 6 descriptors with 2 % bit noise on the targets, so that exact
    ties are everywhere; plus position overrides qpos = query position + {-1, 0, 1} per axis.
    shift_y moves every y (shift_y = -20: half of them negative).
    -> (query keypoints, query descriptors, target keypoints, target descriptors, qpos)."""
    tk = np.zeros(nt, KP_DTYPE)
    qk = np.zeros(nq, KP_DTYPE)
    tk["x"] = rng.integers(0, 60, nt).astype(np.float32)
    tk["y"] = rng.integers(0, 40, nt).astype(np.float32)
    tk["octave"] = rng.integers(0, 2, nt)
    qk["x"] = rng.integers(0, 60, nq).astype(np.float32) + 0.5
    qk["y"] = rng.integers(0, 40, nq).astype(np.float32)
    qk["octave"] = rng.integers(0, 2, nq)
    tk["y"] += np.float32(shift_y)
    qk["y"] += np.float32(shift_y)
    pal = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    td = pal[rng.integers(0, 6, nt)] ^ (rng.random((nt, 32)) < 0.02).astype(np.uint8)
    qd = pal[rng.integers(0, 6, nq)]
    qpos = np.stack([qk["x"] + rng.integers(-1, 2, nq), qk["y"] + rng.integers(-1, 2, nq)], 1).astype(np.float32)
    return qk, qd, tk, td, qpos


POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def hamming_matrix(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """(na, nb) int32 Hamming distances through a 256-entry popcount table."""
    D = np.empty((len(A), len(B)), np.int32)
    step = max(1, (1 << 21) // max(len(B), 1))  # ~64 MiB of xor bytes per block at the most
    for i in range(0, len(A), step):
        D[i:i + step] = POPCOUNT[A[i:i + step, None] ^ B[None]].sum(2, dtype=np.int32)
    return D


def _best_per_row(D: np.ndarray, max_dist: int, min_diff: int):
    """Per row of D: the candidates are the entries <= max_dist; the best is the lowest distance, then
    the lowest index; the row is rejected (-1) with no candidate, or with more than one when
    second - best < min_diff."""
    far = 1 << 20
    Dm = np.where(D <= max_dist, D, far)
    best = Dm.argmin(1)
    d0 = Dm.min(1)
    cnt = (D <= max_dist).sum(1)
    d1 = np.partition(Dm, 1, axis=1)[:, 1] if D.shape[1] > 1 else np.full(len(D), far)
    ok = (cnt > 0) & ~((cnt > 1) & (d1 - d0 < min_diff))
    return np.where(ok, best, -1), d0


def numpy_match(A: np.ndarray, B: np.ndarray, max_dist: int, min_diff: int) -> np.ndarray:
    """Two-way Match in NumPy, written from the rule and sharing no code with the oracle."""
    if len(A) == 0 or len(B) == 0:
        return np.zeros(0, DM_DTYPE)
    D = hamming_matrix(A, B)
    fwd, fd = _best_per_row(D, max_dist, min_diff)
    bwd, _ = _best_per_row(D.T, max_dist, min_diff)
    rows = [i for i in range(len(A)) if fwd[i] >= 0 and bwd[fwd[i]] == i]
    out = np.zeros(len(rows), DM_DTYPE)
    out["query_idx"] = rows
    out["train_idx"] = fwd[rows]
    out["img_idx"] = -1
    out["distance"] = fd[rows]
    return out


def assert_regions(out_h: np.ndarray, n_h: np.ndarray, cap: int, expected, what=""):
    """out_h: (pairs, cap * 16) bytes copied back from a buffer prefilled with CANARY; n_h: the
    reported counts; expected[p]: the full oracle result of pair p.  Pair p's count is the full
    count, its region holds the first min(count, cap) records and every byte after them is still
    CANARY."""
    assert out_h.shape == (len(expected), cap * 16)
    for p, o in enumerate(expected):
        assert int(n_h[p]) == len(o), (what, p, int(n_h[p]), len(o))
        w = 16 * min(len(o), cap)
        assert np.array_equal(out_h[p, :w], dm_bytes(o)[:w]), (what, p)
        assert (out_h[p, w:] == CANARY).all(), (what, p, "bytes past the results were written")
