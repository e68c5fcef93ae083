"""load_tile's plan for the FAST image tile, checked on the host (no GPU).

mage_debug_fast_tile_plan runs the arithmetic the kernels share (csrc/fast_tile_plan.hpp): for
every tile of a frame, which bytes each thread loads and where they land.  Every load must lie
inside an in-frame row's [row, row + w) (the plan never reads pitch padding, so it stays inside
[0, h * stride) as well), and the assembled 136 x 38 tile must equal the reflect-101 window."""
import ctypes as C

import numpy as np
import pytest

TW, TH, LW, LH = 120, 30, 136, 38

# (w, h, stride)
SHAPES = [(300, 100, 300), (304, 101, 304), (297, 99, 304), (250, 70, 256), (136, 38, 136), (128, 30, 128),
          (640, 480, 640), (1280, 720, 1280)]
GENERIC = [(40, 40, 40), (16, 16, 16), (7, 7, 8), (301, 99, 301)]


@pytest.fixture(scope="module")
def lib():
    from mageslam_amd import _lib, build

    build.build()
    return _lib.load()


def plan(lib, img, w, h, stride, tx, ty):
    path = C.c_int32(-1)
    loads = np.full((LH, 9, 2), -1, np.int32)
    tile = np.zeros((LH, LW), np.uint8)
    st = lib.mage_debug_fast_tile_plan(img.ctypes.data_as(C.c_void_p), w, h, stride, tx, ty, C.byref(path),
                                       loads.ctypes.data_as(C.c_void_p), tile.ctypes.data_as(C.c_void_p))
    assert st == 0
    return path.value, loads, tile


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * n - 2)
    return np.where(i >= n, 2 * n - 2 - i, i)


def window(img, w, h, tx, ty):
    ys = reflect101(np.arange(ty * TH - 4, ty * TH - 4 + LH), h)
    xs = reflect101(np.arange(tx * TW - 8, tx * TW - 8 + LW), w)
    return img[ys][:, xs]


def tiles(w, h):
    return [(tx, ty) for ty in range((h + TH - 1) // TH) for tx in range((w + TW - 1) // TW)]


@pytest.mark.parametrize("w,h,stride", SHAPES)
def test_plan_stays_in_frame_and_builds_the_window(lib, w, h, stride):
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, stride), dtype=np.uint8)
    paths = set()
    for tx, ty in tiles(w, h):
        path, loads, tile = plan(lib, img, w, h, stride, tx, ty)
        gx0, gy0 = tx * TW - 8, ty * TH - 4
        interior = gx0 >= 0 and gx0 + LW <= w and gy0 >= 0 and gy0 + LH <= h
        # rows that do not start 8-byte aligned (300 x 100) keep the generic loop, as (301, 99, 301) below
        assert path == (0 if stride % 8 else 1 if interior else 2), (tx, ty, path)
        paths.add(path)
        if path == 0:
            assert np.all(loads == -1)
            continue
        off, nb = loads[..., 0].astype(np.int64), loads[..., 1].astype(np.int64)
        assert np.all((nb == 16) | (nb == 8))
        row, col = off // stride, off % stride
        # (a) inside the allocation, and inside one in-frame row's pixels (no pitch padding)
        assert off.min() >= 0 and (off + nb).max() <= h * stride, (tx, ty)
        assert np.all((row >= 0) & (row < h) & (col + nb <= w)), (tx, ty)
        # rows are the reflected window rows
        assert np.array_equal(row, np.broadcast_to(reflect101(np.arange(gy0, gy0 + LH), h)[:, None], row.shape))
        # (b) all 136 x 38 bytes
        assert np.array_equal(tile, window(img[:, :w], w, h, tx, ty)), (tx, ty)
    assert 2 in paths or stride % 8


@pytest.mark.parametrize("w,h,stride", GENERIC)
def test_small_or_unaligned_frames_take_the_generic_loop(lib, w, h, stride):
    img = np.zeros((h, stride), np.uint8)
    for tx, ty in tiles(w, h):
        path, loads, _ = plan(lib, img, w, h, stride, tx, ty)
        assert path == 0 and np.all(loads == -1), (tx, ty)


def test_numpy_reflection_matches_single_bounce_cases():
    assert reflect101(np.array([-8, -1, 0, 1279, 1280, 1327]), 1280).tolist() == [8, 1, 0, 1279, 1278, 1231]
    assert reflect101(np.array([-4, 40, 77]), 40).tolist() == [4, 38, 1]
