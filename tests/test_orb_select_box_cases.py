"""The frames of tests/orb_select_box_cases.py have the properties they exist for.

CPU only: every condition comes from the oracle's score map and the NumPy restatement of the ANMS
search, so test_gpu_orb_select_box.py cannot pass because a case quietly stopped reaching the edge
of the box rule it is meant for.  On every ANMS case the box rule's minimum is also compared with
the brute-force minimum over all items.
"""
import numpy as np
import pytest

from tests import orb_select_box_cases as bc
from tests import orb_select_cases as sc


def cell(q, i):
    return int(q.cell_x(q.x[i])), int(q.cell_y(q.y[i]))


def assert_box_is_exact(q):
    # cells of at least sqrt(mcd2) pixels: the box rule, the reference's ring loop and the brute-force
    # minimum agree on every item
    assert not q.thin
    got, _ = bc.box_min(q)
    assert np.array_equal(got, bc.brute_min(q))
    assert np.array_equal(got, bc.ring_min(q))


def test_isqrt_below():
    assert [bc.isqrt_below(g) for g in (-3, 0, 1, 2, 4, 5, 100, 101, 121, 122)] == [-1, -1, 0, 1, 1, 2, 9, 10, 10, 11]
    for g in (2**24 - 1, 2**24, 2**24 + 1, 4095 * 4095):
        r = bc.isqrt_below(g)
        assert r * r < g <= (r + 1) * (r + 1)


def test_box_edge_sweep(oracle):
    assert bc.frame("lattice").shape == (bc.LATTICE_H, bc.LATTICE_W)
    qs = [bc.search("lattice", N) for N in bc.BOX_EDGE_N]
    assert all(q is not None for q in qs)  # every N takes the ANMS path
    assert sorted(np.unique(qs[0].s)) == [69, 119]  # two strengths, the weak ones below the strong / rob
    # gmax on both sides of the neighbour distances 11^2 and 10^2 + 11^2, with 121 and 122
    # themselves; above 10^2 only (N stays below the 616 candidates, so gmax stays above 101)
    gmaxs = [q.gmax for q in qs]
    assert min(gmaxs) > 100
    for d2 in (121, 221):
        assert any(g <= d2 for g in gmaxs) and any(g > d2 for g in gmaxs)
    assert 121 in gmaxs and 122 in gmaxs
    edge = diff_cell = 0
    outside = np.zeros(4, bool)
    shrunk = 0
    for q in qs:
        assert_box_is_exact(q)
        e = bc.edge_items(q)
        edge += len(e)
        diff_cell += sum(cell(q, i) != cell(q, o) for i, o in e)
        minX, maxX, minY, maxY = q.bbox
        outside |= [(q.x - q.r < minX).any(), (q.x + q.r > maxX).any(), (q.y - q.r < minY).any(), (q.y + q.r > maxY).any()]
        shrunk += int((bc.box_min(q, q.r - 1)[0] != bc.brute_min(q)).sum())
    assert edge > 0  # an only stronger neighbour below gmax at exactly |dx| = r or |dy| = r
    assert diff_cell > 0  # ... in another cell than the item
    assert outside.all()  # x - r, x + r, y - r, y + r each leave the bounding box for some item
    assert shrunk > 0  # a radius of r - 1 misses a neighbour that decides


@pytest.mark.parametrize("name,N", bc.RING_CASES)
def test_former_ring_path(oracle, name, N):
    assert bc.frame(name).shape == (bc.H, bc.W) and 50 <= N <= 100
    q = bc.search(name, N)
    assert q is not None
    assert 16 * q.mcd2 < q.gmax  # the square of whole rings ended at D = 5: the ring loop ran here
    x0, x1, y0, y1 = bc.box_bounds(q)
    assert max((x1 - x0 + 1).max(), (y1 - y0 + 1).max()) >= 7
    assert_box_is_exact(q)


@pytest.mark.parametrize("cells", bc.GRIDS)
def test_cell_grids(oracle, cells):
    q = bc.search("grids", bc.GRIDS_N, cells)
    assert q is not None and q.r > 0
    assert cells[0] * cells[1] <= 4096
    x0, x1, y0, y1 = bc.box_bounds(q)
    if cells == (1, 1):
        assert (x1 == 0).all() and (y1 == 0).all()  # one cell holds every item
    else:
        assert (x1 > x0).any() and (y1 > y0).any()  # boxes over more than one cell column and row
    assert_box_is_exact(q)


@pytest.mark.parametrize("name,N,cells,gmax,r,thin", [c + v for c, v in zip(bc.DEGENERATE, ((0, -1, True), (0, -1, True), (1, 0, True), (1, 0, False)))])
def test_degenerate_gmax(oracle, name, N, cells, gmax, r, thin):
    q = bc.search(name, N, cells)
    assert q is not None and q.K >= N
    assert (q.gmax, q.r, q.thin) == (gmax, r, thin)
    minX, maxX, minY, maxY = q.bbox
    if name == "row":
        assert minY == maxY and maxX - minX > 32
    elif name == "col":
        assert minX == maxX and maxY - minY > 32
    else:
        assert q.K == bc.GMAX1_K and (maxX - minX) * (maxY - minY) >= N
        x, y, s = sc.candidates(bc.frame(name))
        assert len(s) > q.K  # the weaker lattice: more candidates than N
    # nothing below gmax by either walk: the order is strength and raster alone
    assert (bc.brute_min(q) == gmax).all() and (bc.ring_min(q) == gmax).all() and (bc.box_min(q)[0] == gmax).all()
    assert len(bc.expected(name, N, num_cells_x=cells[0], num_cells_y=cells[1])[0]) == N


def test_thin_frame(oracle):
    # cells thinner than a pixel: the reference's loop stops before a nearer stronger item, so its
    # result is not the nearest-stronger minimum the box rule gives, and the kernel must follow it
    name, N = bc.THIN
    assert bc.frame(name).shape[1] == bc.W
    q = bc.search(name, N)
    assert q is not None and q.thin and q.mcd2 == 1 and q.gmax > 16
    ring, brute = bc.ring_min(q), bc.brute_min(q)
    assert (ring >= brute).all() and (ring > brute).any()
    assert np.array_equal(bc.box_min(q)[0], brute)
    assert len(bc.expected(name, N)[0]) == N


def test_batch_frames(oracle):
    assert bc.BATCHES[0] == bc.BATCHES[1][::-1] and set(bc.BATCHES[0]) == {"small_lattice", "noise", "plain"}
    for name in bc.BATCHES[0]:
        assert bc.frame(name).shape == (bc.H, bc.W)
    lat, noise, plain = (bc.search(n, bc.BATCH_N) for n in ("small_lattice", "noise", "plain"))
    assert lat is not None and noise is not None and plain is not None
    # a case-1 frame: a deciding neighbour in the last column or row of the box, in another cell,
    # and lost at r - 1
    e = bc.edge_items(lat)
    assert e and any(cell(lat, i) != cell(lat, o) for i, o in e)
    assert (bc.box_min(lat, lat.r - 1)[0] != bc.brute_min(lat)).any()
    assert ("noise", bc.BATCH_N) in bc.RING_CASES  # a case-2 frame (test_former_ring_path)
    # the three frames differ in every per-frame value a workgroup keeps
    assert len({q.gmax for q in (lat, noise, plain)}) == 3 and len({q.bbox for q in (lat, noise, plain)}) == 3
    assert len({q.r for q in (lat, noise)}) == 2
    for q in (lat, noise, plain):
        assert_box_is_exact(q)


def test_pyramid_frame(oracle):
    assert bc.PYRAMID_N in bc.BOX_EDGE_N
    kp, _ = bc.expected("lattice", bc.PYRAMID_N, **bc.PYRAMID)
    assert (np.bincount(kp["octave"], minlength=4)[:2] > 0).all()  # levels append behind level 0
