"""The fp4 matcher's tile pipeline (MAGE_FP4_PIPE in mageslam_amd/csrc/match.hip), byte for byte
against oracle.match; no tolerances.  Every call takes the fp4 body (maxDist < 128, minDiff >= 1, a B
pitch <= 2048) through match_batch_device, with the library as built: the cases hold for either
setting of the switch.

With the switch on, a wave walks the 16 (column tile, row tile) tiles of a 128-column stage as one
stream: the MFMAs of tile n + 1 run under the fold of tile n on a second accumulator, the B operands
of the next column tile are read a tile ahead into a second register set, the next stage's fill runs
under the stage's first tile, the stream drains at the stage barrier, and behind a ragged column
edge a tile is issued and dropped.  A wave owns rows [128 w, 128 w + 128) of a pass
of 1024 rows; a row tile is 32 rows, a column tile 32 columns.

Shapes: every nb of NBS against the smallest and the largest na, every na of NAS against the
smallest and the largest nb, and 2000 x 2000, all in one batched call per setting (unequal counts
in one launch); a batch of three pairs with an empty one in the middle.  The pairs are match_sets'
(noisy copies, all-zero / all-one rows, duplicated B rows = exact ties at the start and in the last,
ragged column tile).

Planted cases: B and A random (~128 bits apart) but for rows / columns that compete at distances
(d, d), (d, d + 1), (d + 1, d), (d, d + 2):
  * two rows for one column, the rows in row tiles n and n + 1 of one wave for n = 0, 1, 2, in tile 3
    of one wave and tile 0 of the next, and on both sides of the pass edge (rows 1023 / 1024);
  * two columns for one row, the columns on both sides of a column-tile edge and of the stage edge
    (127 / 128: the last tile before the drain and the first after it), the row in row tile 3 (the
    stage's last tile), 0 (its first) and 2.
(d, d) is an exact tie, which minDiff >= 1 rejects.  The conditions against vacuous passes are
asserted on the oracle's output: at least one accepted match per call, and for every planted
scenario that the planting decides it: with a tie the oracle at minDiff = 0 gives a match of the
planted row or column that minDiff = 1 rejects, without a tie minDiff = 1 accepts the closer one."""
import functools

import numpy as np
import pytest

from match_cases import CANARY, assert_regions, match_sets
from mageslam_amd import matcher

pytestmark = pytest.mark.gpu

NBS = [1, 31, 32, 33, 127, 128, 129, 257, 2047, 2048]
NAS = [1, 32, 33, 127, 128, 129, 1023, 1024, 1025, 2000]
SETTINGS = [(30, 1), (127, 1)]
D0 = 6
GAPS = [(0, 0), (0, 1), (1, 0), (0, 2)]


def edge_shapes():
    """(na, nb) along the four edges of NAS x NBS, plus 2000 x 2000."""
    s = [(na, nb) for na in (NAS[0], NAS[-1]) for nb in NBS]
    s += [(na, nb) for nb in (NBS[0], NBS[-1]) for na in NAS if (na, nb) not in s]
    return s + [(2000, 2000)]


def flipped(desc, k, rng):
    out = desc.copy()
    for bit in rng.choice(256, size=k, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def run_batch(scen, md, mdiff):
    """One match_batch_device call over the scenarios; the rows above a pair's counts hold random
    bytes.  -> (out bytes (pairs, cap * 16), counts, cap)."""
    import torch

    pairs = len(scen)
    a_rows = max(1, max(len(a) for a, _ in scen))
    b_rows = max(1, max(len(b) for _, b in scen))
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


def check(oracle, scen, md, mdiff, plants=None):
    """plants[p] = (candidate (row, column) pairs of scenario p, the one the planting makes win or
    None for a tie)."""
    exp = [oracle.match(a, b, max_distance=md, min_difference=mdiff) for a, b in scen]
    assert sum(len(e) for e in exp) > 0, "no accepted match in the oracle's result"
    for p, (cand, win) in enumerate(plants or []):
        got = pairs_of(exp[p])
        if win is None:
            loose = pairs_of(oracle.match(*scen[p], max_distance=md, min_difference=0))
            assert not (got & cand) and (loose - got) & cand, (p, "the planted tie is not what minDiff rejects")
        else:
            assert win in got and not (got & (cand - {win})), (p, "the planted winner is not matched")
    out, n, cap = run_batch(scen, md, mdiff)
    assert_regions(out, n, cap, exp, (md, mdiff))
    return exp


# ------------------------- shapes ----------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def shape_scenarios():
    return [match_sets(na, nb, 9000 + 3 * na + nb) for na, nb in edge_shapes()]


@pytest.mark.parametrize("md,mdiff", SETTINGS)
def test_edge_shapes(gpu, oracle, md, mdiff):
    """One tile, the column-tile edge, the stage edge (128 columns), a wave's row tiles partly
    inactive, the pass edge (1024 rows), and the full size."""
    assert len(edge_shapes()) == 37
    check(oracle, shape_scenarios(), md, mdiff)


@pytest.mark.parametrize("md,mdiff", SETTINGS)
def test_unequal_batch_with_empty_pair(gpu, oracle, md, mdiff):
    """Three pairs of unequal counts; the middle one has no A rows, then no B rows, then neither."""
    first, last = match_sets(300, 257, 9101), match_sets(129, 2047, 9102)
    z = np.zeros((0, 32), np.uint8)
    for empty in ((z, first[1]), (first[0], z), (z, z)):
        exp = check(oracle, [first, empty, last], md, mdiff)
        assert len(exp[1]) == 0 and len(exp[0]) > 0 and len(exp[2]) > 0


# ------------------------- planted competitions --------------------------------------------------

# (first row, second row): row tiles 0|1, 1|2, 2|3 of wave 0, both orders; tile 3 of wave 0 | tile 0 of
# wave 1; the same tiles of wave 1
ROW_PAIRS = [(5, 40), (40, 5), (40, 70), (70, 40), (70, 100), (100, 70), (127, 128), (128, 127), (100, 130),
             (128 + 70, 128 + 100), (128 + 31, 128 + 32)]
# the same across the pass edge and in the second pass (rows 1024 + ...)
ROW_PAIRS_2 = [(1023, 1024), (1024, 1023), (1000, 1030), (1024 + 70, 1024 + 100), (1024 + 100, 1024 + 70), (70, 1024 + 70)]
# (first column, second column): column-tile edges inside a stage, the stage edge, far apart
COL_PAIRS = [(31, 32), (32, 31), (95, 96), (126, 127), (127, 128), (128, 127), (100, 130), (0, 256), (255, 256)]
ROWS = [100, 3, 70, 128 + 96]  # row tile 3 (the stage's last tile), 0 (its first), 2, and wave 1's tile 3


def column_scenarios(na, nb, row_pairs, seed):
    """Per (row pair, gap): the two rows are copies of one column with D0 + gap bits flipped."""
    rng = np.random.default_rng(seed)
    cols = sorted({0, 31, 32, 127, 128, nb - 1})
    out, plants = [], []
    for n, (ra, rb) in enumerate(row_pairs):
        for ga, gb in GAPS:
            A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
            B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
            col = cols[(n + ga + 2 * gb) % len(cols)]
            A[ra] = flipped(B[col], D0 + ga, rng)
            A[rb] = flipped(B[col], D0 + gb, rng)
            out.append((A, B))
            plants.append(({(ra, col), (rb, col)}, None if ga == gb else (ra, col) if ga < gb else (rb, col)))
    return out, plants


def row_scenarios(na, nb, col_pairs, rows, seed):
    """Per (column pair, row, gap): the two columns are copies of one row with D0 + gap bits flipped."""
    rng = np.random.default_rng(seed)
    out, plants = [], []
    for ca, cb in col_pairs:
        for row in rows:
            for ga, gb in GAPS:
                A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
                B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
                B[ca] = flipped(A[row], D0 + ga, rng)
                B[cb] = flipped(A[row], D0 + gb, rng)
                out.append((A, B))
                plants.append(({(row, ca), (row, cb)}, None if ga == gb else (row, ca) if ga < gb else (row, cb)))
    return out, plants


@pytest.mark.parametrize("md,mdiff", SETTINGS)
@pytest.mark.parametrize("nb", [129, 257])
def test_rows_in_consecutive_tiles(gpu, oracle, nb, md, mdiff):
    """A column's best and runner-up rows in consecutive tiles of the stream (na = 257: two full
    waves and one row of a third)."""
    scen, plants = column_scenarios(257, nb, ROW_PAIRS, 9200 + nb)
    check(oracle, scen, md, mdiff, plants)


@pytest.mark.parametrize("md,mdiff", SETTINGS)
def test_rows_across_the_pass_edge(gpu, oracle, md, mdiff):
    """The same on both sides of row 1024 and in the second pass (na = 1153: its first wave and one
    row of the next), nb = 129: a full stage and a stage of one column."""
    scen, plants = column_scenarios(1153, 129, ROW_PAIRS_2, 9300)
    check(oracle, scen, md, mdiff, plants)


@pytest.mark.parametrize("md,mdiff", SETTINGS)
def test_columns_across_tile_and_stage_edges(gpu, oracle, md, mdiff):
    """A row's best and runner-up columns on both sides of a column-tile edge and of the stage edge
    (na = nb = 257)."""
    scen, plants = row_scenarios(257, 257, COL_PAIRS, ROWS, 9400)
    check(oracle, scen, md, mdiff, plants)
