"""The fp4 matcher's column flush and its operand expansion (expand32_fp4, or the lookup table of
MAGE_FP4_LUT, which replaces it byte by byte) in mageslam_amd/csrc/match.hip, byte for byte
against oracle.match; no tolerances.  Every call takes the fp4 body (maxDist < 128, minDiff >= 1,
nb <= 2048), through matcher.Match and through match_batch_device with a B pitch <= 2048.

In the kernel a wave owns 128 A rows per pass (wave slot = row // 128), a column flush serves 64 of
them (the 6-bit row code: group = row // 64), and within a 32-row tile lanes 0-31 hold the rows
with (row % 8) < 4, lanes 32-63 the others.  Both half-waves push their own (best, second) of a
column into the workgroup's state with LDS atomics, so the cases put a column's two closest rows
into the same half, into opposite halves, into neighbouring flush groups and into neighbouring
waves, in both orders, at distances (d, d), (d, d + 1), (d, d + 2): the column is accepted or
rejected by minDiff on exactly the pair of keys the flush has to keep.

A scenario is one (A, B) pair: B is random (its columns ~128 bits apart), A is random except for
the rows that compete for one target column, which are that column with k bits flipped.  The
scenarios of one parametrisation form one batched call and are also matched one by one through
Match.  The conditions against vacuous passes are asserted on the oracle's output per
parametrisation: at least one accepted match, and (except where every row ties) at least one match
that minDiff = 0 would give and the parametrisation's minDiff rejects."""
import functools

import numpy as np
import pytest

from match_cases import CANARY, assert_regions, dm_bytes
from mageslam_amd import matcher

pytestmark = pytest.mark.gpu

D0 = 6          # best distance of the competing rows (maxDist = 30)
GAPS = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0)]  # (first row, second row) distance above D0


def flipped(desc, k, rng):
    """desc (32 bytes) with k distinct random bits flipped."""
    out = desc.copy()
    for bit in rng.choice(256, size=k, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def scenario(na, nb, col, rows_dists, rng):
    """Random A (na, 32) and B (nb, 32); A[row] = B[col] with dist bits flipped for every
    (row, dist) of rows_dists."""
    A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    for row, dist in rows_dists:
        A[row] = flipped(B[col], dist, rng)
    return A, B


def pair_scenarios(na, nb, row_pairs, seed):
    """One scenario per (row pair, gap): the two rows compete for one column (cycling over the
    first, the last and a middle column)."""
    rng = np.random.default_rng(seed)
    cols = sorted({0, nb - 1, nb // 2})
    out = []
    for n, (ra, rb) in enumerate(row_pairs):
        for ga, gb in GAPS:
            out.append(scenario(na, nb, cols[(n + ga + 2 * gb) % len(cols)], [(ra, D0 + ga), (rb, D0 + gb)], rng))
    return out


def run_batch(scen, md, mdiff):
    """One match_batch_device call over the scenarios (pitch = the largest count, at most 2048 B
    rows: the fp4 kernel); the rows above a pair's counts hold random bytes.
    -> (out bytes (pairs, cap * 16), counts)."""
    import torch

    pairs = len(scen)
    a_rows = max(len(a) for a, _ in scen)
    b_rows = max(len(b) for _, b in scen)
    assert b_rows <= 2048
    rng = np.random.default_rng(7)
    A = rng.integers(0, 256, (pairs, a_rows, 32), dtype=np.uint8)
    B = rng.integers(0, 256, (pairs, b_rows, 32), dtype=np.uint8)
    for p, (a, b) in enumerate(scen):
        A[p, : len(a)] = a
        B[p, : len(b)] = b
    tA, tB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    na = torch.tensor([len(a) for a, _ in scen], dtype=torch.int32, device="cuda")
    nb = torch.tensor([len(b) for _, b in scen], dtype=torch.int32, device="cuda")
    out = torch.full((pairs, a_rows * 16), CANARY, dtype=torch.uint8, device="cuda")
    nout = torch.full((pairs,), -1, dtype=torch.int32, device="cuda")
    matcher.match_batch_device(tA, a_rows * 32, na, tB, b_rows * 32, nb, pairs, md, mdiff, out, a_rows, nout)
    torch.cuda.synchronize()
    return out.cpu().numpy(), nout.cpu().numpy(), a_rows


def pairs_of(m):
    return set(zip(m["query_idx"].tolist(), m["train_idx"].tolist()))


def check(oracle, scen, md, mdiff):
    exp = [oracle.match(a, b, max_distance=md, min_difference=mdiff) for a, b in scen]
    loose = [oracle.match(a, b, max_distance=md, min_difference=0) for a, b in scen]
    assert sum(len(e) for e in exp) > 0, "no accepted match in the oracle's result"
    rejected = sum(len(pairs_of(l) - pairs_of(e)) for l, e in zip(loose, exp))
    assert rejected > 0, "nothing rejected by minDiff in the oracle's result"
    out, n, cap = run_batch(scen, md, mdiff)
    assert_regions(out, n, cap, exp, (md, mdiff))
    for p, ((a, b), e) in enumerate(zip(scen, exp)):
        g = matcher.Match(a, b, maxHammingDist=md, minHammingDifference=mdiff)
        assert len(g) == len(e) and np.array_equal(dm_bytes(g), dm_bytes(e)), (p, md, mdiff, len(g), len(e))


# ------------------------- best and runner-up in opposite half-waves ------------------------------

# rows 0-3: lanes 0-31, rows 4-7: lanes 32-63; opposite halves, then the same half, in both row orders
# (and, with GAPS, both distance orders)
HALF_PAIRS = [(0, 4), (4, 0), (3, 4), (2, 7), (7, 1), (3, 7), (0, 1), (1, 3), (5, 6), (7, 4)]


@pytest.mark.parametrize("mdiff", [1, 2])
@pytest.mark.parametrize("nb", [1, 32, 33])
def test_opposite_half_waves(gpu, oracle, nb, mdiff):
    """na = 8.  (d, d) is the index tie (rejected, both orders of the lower index's half); (d, d + 1)
    passes minDiff 1 only, (d, d + 2) both."""
    check(oracle, pair_scenarios(8, nb, HALF_PAIRS, 1000 + nb), 30, mdiff)


# ------------------------- flush group and wave edges --------------------------------------------

EDGE_PAIRS = [(63, 64), (64, 63), (59, 63), (60, 63), (62, 64), (0, 64), (127, 128), (128, 127), (124, 128),
              (63, 127), (64, 128), (192, 256), (255, 256), (127, 256), (0, -1), (-1, 63)]


@pytest.mark.parametrize("mdiff", [1, 2])
@pytest.mark.parametrize("nb", [32, 33, 129])
@pytest.mark.parametrize("na", [64, 65, 128, 129, 257])
def test_flush_group_and_wave_edges(gpu, oracle, na, nb, mdiff):
    """The competing rows on either side of rows 63 / 64 (two flushes of one wave) and 127 / 128 (two
    waves), and the last row (alone in its group or wave at na = 65, 129, 257) against an earlier one."""
    row_pairs = [(ra % na, rb % na) for ra, rb in EDGE_PAIRS if max(ra, rb) < na and ra % na != rb % na]
    assert len(row_pairs) >= 2
    check(oracle, pair_scenarios(na, nb, row_pairs, 2000 + 7 * na + nb), 30, mdiff)


# ------------------------- many contributors to one column ---------------------------------------


@pytest.mark.parametrize("na", [64, 200])
def test_many_contributors(gpu, oracle, na):
    """Every A row is B[0] or B[0] with D0 / D0 + 1 bits flipped, minDiff 1: all rows tie (exact
    copies, and distinct rows at one distance) -> column 0 rejected, nothing matches; one strict
    winner at D0 among na - 1 rows at D0 + 1, at the first row, the last, both sides of 63 / 64 and
    of 127 / 128 -> exactly that row matches."""
    rng = np.random.default_rng(3000 + na)
    nb = 33
    scen = []
    for dist in (0, D0):
        scen.append(scenario(na, nb, 0, [(r, dist) for r in range(na)], rng))
    n_ties = len(scen)
    winners = [w for w in (0, 4, 63, 64, 127, 128, na - 1) if w < na]
    for w in winners:
        scen.append(scenario(na, nb, 0, [(r, D0 if r == w else D0 + 1) for r in range(na)], rng))
    exp = [oracle.match(a, b, max_distance=30, min_difference=1) for a, b in scen]
    assert all(len(e) == 0 for e in exp[:n_ties])
    assert [e["query_idx"].tolist() for e in exp[n_ties:]] == [[w] for w in winners]
    check(oracle, scen, 30, 1)


# ------------------------- every table entry -----------------------------------------------------


@functools.lru_cache(maxsize=None)
def table_sets():
    """A, B (256, 32) in which every byte value occurs in every byte position of a dword, on both
    sides.  Column c of B is a permutation of 0..255 over the rows (so B's rows look random, ~128
    bits apart).  A[i] = B[s(i)] ^ mask, s(i) = i for i < 200 and i - 200 above (56 columns get two
    candidate rows, 56 none), the mask one of four fixed 32-byte patterns of 10, 11, 12 and 40 set
    bits: columns with two rows at (10, 10) and (10, 11) are rejected by minDiff 1 / 2, the others
    match."""
    rng = np.random.default_rng(4000)
    B = np.stack([rng.permutation(256) for _ in range(32)], 1).astype(np.uint8)
    masks = np.stack([flipped(np.zeros(32, np.uint8), k, rng) for k in (10, 11, 12, 40)])
    src = np.where(np.arange(256) < 200, np.arange(256), np.arange(256) - 200)
    A = B[src] ^ masks[rng.integers(0, 4, 256)]
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def covers_all_bytes(M):
    """Every value 0..255 occurs in every byte position (0..3) of a dword."""
    return all(len(np.unique(M[:, q::4])) == 256 for q in range(4))


@pytest.mark.parametrize("mdiff", [1, 2])
def test_every_table_entry(gpu, oracle, mdiff):
    """na = nb = 256, maxDist = 127: pair 0 is the covering set, pair 1 its bitwise complement (the
    same distances, every table entry again at the mirrored index)."""
    A, B = table_sets()
    assert covers_all_bytes(A) and covers_all_bytes(B)
    scen = [(A, B), (~A, ~B)]
    assert covers_all_bytes(scen[1][0]) and covers_all_bytes(scen[1][1])
    check(oracle, scen, 127, mdiff)
