"""Frames of the box-search tests (test_orb_select_box_cases.py, test_gpu_orb_select_box.py) and a
NumPy restatement of what select_kernel's ANMS search (mageslam_amd/csrc/orb.hip) decides on them.
Not a test module (nothing is collected); nothing here touches the GPU.

The search gives every retained item min(gmax, d^2 to the nearest stronger item).  Only items with
d^2 < gmax can matter, so the kernel reads the cells [cell(x - r), cell(x + r)] x [cell(y - r),
cell(y + r)], r the largest integer with r^2 < gmax and the coordinates clamped to the bounding box
of the retained items.  The cases put items, neighbours and gmax on the edges of that rule:

    gmax   (int)((maxX - minX) (maxY - minY) / N), N the NumFeatures of the level
    r      the largest integer with r^2 < gmax (-1 when gmax <= 0: nothing is visited)
    mcd2   min((maxX - minX) / numCellsX, (maxY - minY) / numCellsY, at least 1)^2: the reference's
           ring d lies at least (d - 1) sqrt(mcd2) away, so with 16 mcd2 < gmax its ring loop runs
           past ring 4
    thin   (maxX - minX) / numCellsX or (maxY - minY) / numCellsY is 0: the "at least 1" above is
           then more than a cell really spans, the reference's loop can stop before a nearer
           stronger item, and the kernel walks the rings as the reference does instead
    stronger  o is stronger than i when f32(s_o) > f32(s_i) * rob + 0.002, rob the robustness factor
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from mageslam_amd import synth
from tests import orb_select_cases as sc

W, H = 640, 480  # every batch frame
LATTICE_W, LATTICE_H = 320, 240
PYRAMID = sc.PYRAMID


def lattice(w=LATTICE_W, h=LATTICE_H):
    """One dot in six at 220, the rest at 170, 11 x 10 pixels apart."""
    return sc.dots(w, h, 11, 10, val=sc.mixed_val)


def on_canvas(img, w=W, h=H, bg=100):
    """img in the top left corner of a flat w x h frame (the dots keep their coordinates)."""
    out = np.full((h, w), bg, np.uint8)
    out[: img.shape[0], : img.shape[1]] = img
    return out


def row_frame():
    return sc.dots(W, 64, 4, 1000, y0=30)


def col_frame():
    return sc.dots(64, H, 1000, 4, x0=30)


GMAX1_K = 41  # strong dots of gmax1_frame = its NumFeatures


def gmax1_frame():
    """21 dots 4 pixels apart on one row and 20 between them on the next, all at 220: a bounding box
    of 80 x 1 around 41 items.  A weaker lattice below them brings the candidates above N = 41."""
    img = np.full((240, 320), 100, np.uint8)
    img[30, 20:101:4] = 220
    img[31, 22:99:4] = 220
    img[60:, :] = sc.dots(320, 180, 16, 16, val=170)
    return img


# The box-edge sweep is the lattice at these NumFeatures: gmax = 222, 143, 122, 121, 110, 101, across
# the lattice's squared neighbour distances 10^2 + 11^2, 11^2 and 10^2.
BOX_EDGE_N = (280, 435, 510, 515, 565, 615)
BATCH_N = 63  # one NumFeatures for a small lattice, the noise frame and a plain frame
_FRAMES = {
    "lattice": lattice,
    "small_lattice": lambda: on_canvas(lattice(110, 120)),
    "noise": lambda: sc.noise(W, H, 7),
    "textured": lambda: synth.frame(3, W, H),
    "grids": lambda: synth.frame(2, W, H),
    "row": row_frame,
    "col": col_frame,
    "gmax1": gmax1_frame,
    "plain": lambda: synth.frame(1, W, H),
    "thin": lambda: sc.noise(W, 40, 3),
}
RING_CASES = (("noise", 50), ("textured", 50), ("noise", BATCH_N))
GRIDS = ((1, 1), (7, 3), (64, 64))
GRIDS_N = 1000
# (frame, NumFeatures, cell grid): gmax = 0 twice, gmax = 1 over thin cells (the ring walk) and over
# one cell (the box rule at r = 0)
DEGENERATE = (("row", 50, (32, 32)), ("col", 50, (32, 32)), ("gmax1", GMAX1_K, (32, 32)), ("gmax1", GMAX1_K, (1, 1)))
THIN = ("thin", 100)  # a bounding box 26 pixels high under 32 cell rows
BATCHES = (("small_lattice", "noise", "plain"), ("plain", "noise", "small_lattice"))
PYRAMID_N = 565


@functools.lru_cache(maxsize=None)
def frame(name):
    img = np.ascontiguousarray(_FRAMES[name]())
    img.setflags(write=False)
    return img


def expected(name, nfeat, **settings_kw):
    return sc.expected(("box", name), frame(name), settings_kw, nfeat)


def isqrt_below(g):
    """The largest integer r with r^2 < g, -1 when there is none."""
    if g <= 0:
        return -1
    r = int(np.sqrt(float(g)))
    while r * r >= g:
        r -= 1
    while (r + 1) * (r + 1) < g:
        r += 1
    return r


@functools.lru_cache(maxsize=None)
def search(name, N, cells=(32, 32), t=4, strong=20, min_r=1.1, max_r=2.0):
    """The ANMS search of level 0 restated: the retained items, the frame's constants and, per item,
    the squared distances to its stronger items.  None when the level does not take the ANMS path."""
    x, y, s = sc.candidates(frame(name), t)
    n0, cut, K = sc.retain(s, N, t)
    if n0 <= N or K < N:
        return None
    keep = s >= cut
    x, y, s = x[keep].astype(np.int64), y[keep].astype(np.int64), s[keep].astype(np.int64)
    minX, maxX, minY, maxY = int(x.min()), int(x.max()), int(y.min()), int(y.max())
    numX, numY = cells
    gmax = int(float(maxX - minX) * float(maxY - minY) / float(N))
    r = isqrt_below(gmax)
    dx, dy = max((maxX - minX) // numX, 1), max((maxY - minY) // numY, 1)
    mcd2 = min(dx, dy) ** 2
    f = np.float32
    val = min(f(strong) - f(t), max(f(0), f(int(s.min())) - f(t)))
    rob = f(max_r) - f(f(val / f(strong - t)) * max(f(0), f(max_r) - f(min_r)))
    sth = f(s.astype(f) * rob) + f(0.002)
    stronger = s.astype(f)[None, :] > sth[:, None]  # [i, o]
    ddx, ddy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    d2 = ddx * ddx + ddy * ddy
    cell_x = lambda v: (np.clip(v, minX, maxX) - minX) * numX // (maxX + 1 - minX)
    cell_y = lambda v: (np.clip(v, minY, maxY) - minY) * numY // (maxY + 1 - minY)
    thin = (maxX - minX) // numX == 0 or (maxY - minY) // numY == 0
    return SimpleNamespace(x=x, y=y, s=s, K=len(x), N=N, gmax=gmax, r=r, mcd2=mcd2, thin=thin, numX=numX, numY=numY,
                           bbox=(minX, maxX, minY, maxY), stronger=stronger, ddx=ddx, ddy=ddy, d2=d2,
                           cell_x=cell_x, cell_y=cell_y)


def brute_min(q):
    """min(gmax, d^2 to the nearest stronger item) over all items."""
    d = np.where(q.stronger, q.d2, np.iinfo(np.int64).max)
    return np.minimum(d.min(axis=1), q.gmax)


def ring_min(q):
    """The reference's loop (OpenCVModified.cpp:266-326): ring d of cells around the item's cell is
    read while max(0, d - 1)^2 mcd2 is below the running minimum."""
    cx, cy = q.cell_x(q.x), q.cell_y(q.y)
    ring = np.maximum(np.abs(cx[:, None] - cx[None, :]), np.abs(cy[:, None] - cy[None, :]))
    out = np.full(q.K, q.gmax, np.int64)
    for i in range(q.K):
        m, d = q.gmax, 0
        while max(0, d - 1) ** 2 * q.mcd2 < m:
            hit = q.d2[i][q.stronger[i] & (ring[i] == d)]
            if len(hit):
                m = min(m, int(hit.min()))
            d += 1
        out[i] = m
    return out


def box_bounds(q, radius=None):
    r = q.r if radius is None else radius
    return q.cell_x(q.x - r), q.cell_x(q.x + r), q.cell_y(q.y - r), q.cell_y(q.y + r)


def box_min(q, radius=None):
    """The same minimum over the items of the cells the box rule reads (all cells of radius r), and
    the number of items visited per item."""
    r = q.r if radius is None else radius
    out = np.full(q.K, q.gmax, np.int64)
    if r < 0:
        return out, np.zeros(q.K, np.int64)
    x0, x1, y0, y1 = box_bounds(q, r)
    cx, cy = q.cell_x(q.x), q.cell_y(q.y)
    inside = ((cx[None, :] >= x0[:, None]) & (cx[None, :] <= x1[:, None]) &
              (cy[None, :] >= y0[:, None]) & (cy[None, :] <= y1[:, None]))
    d = np.where(inside & q.stronger, q.d2, np.iinfo(np.int64).max)
    return np.minimum(d.min(axis=1), q.gmax), inside.sum(axis=1)


def edge_items(q):
    """(i, o): item i has exactly one stronger item o with d^2 < gmax, and it sits at |dx| = r or
    |dy| = r, the last column or row of the box."""
    below = q.stronger & (q.d2 < q.gmax)
    out = []
    for i in np.nonzero(below.sum(axis=1) == 1)[0]:
        o = int(np.nonzero(below[i])[0][0])
        if abs(q.ddx[i, o]) == q.r or abs(q.ddy[i, o]) == q.r:
            out.append((int(i), o))
    return out
