"""Helpers of the undistortion tests (test_image_reference.py, test_gpu_image_paths.py): named
calibrations that put output tiles on every path of remap_linear_kernel (mageslam_amd/csrc/image.hip),
an independent NumPy formulation of cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8UC1, the tile
classification of remap_boxes_kernel, and the canary check of strided destinations.  Not a test
module (nothing is collected).

remap_reference is written from DESIGN.md ("undistortion") and shares no code with the oracle:

    X = round_half_even(float32(u) * float32(32)), Y likewise; a product that is NaN, +-inf or
        outside [-2^31, 2^31) gives INT_MIN (the "integer indefinite" of the x86 conversions)
    sx = clip(X >> 5, -32768, 32767), sy likewise; fraction index (X & 31, Y & 31)
    weights (32-ty)(32-tx)*32, (32-ty)tx*32, ty(32-tx)*32, ty*tx*32; index (0, 0): (32767, 0, 0, 1)
    a tap outside the frame contributes 0; result (sum + 2^14) >> 15 clipped to 0..255

Which path a 64 x 16 output tile takes, from the bounding box of its in-range source taps (x0
aligned down to 4, width padded up to a multiple of 4):

    EMPTY     no tap in range: every pixel is 0
    STAGED    width * height <= 8192: the box is staged in LDS
    FALLBACK  larger: taps are read from global memory
"""
from __future__ import annotations

import numpy as np

CANARY = 0xA5
INT_MIN = -(1 << 31)
TILE_W, TILE_H, BOX_BYTES = 64, 16, 8192
EMPTY, STAGED, FALLBACK = 0, 1, 2

MILD = [-0.2, 0.05, 0.001, -0.0005, 0.01]


def _case(w, h, f, dist, cx=None, cy=None):
    return {"w": w, "h": h, "kd": (float(f), float(f), w * 0.5 if cx is None else cx, h * 0.5 if cy is None else cy),
            "dist": list(dist)}


# name -> size, distorted intrinsics (fx, fy, cx, cy) and distortion.  The undistorted principal
# point is the image centre (mage_undistorter_create).
CASES = {
    # k1 = 6 at fx = 100: the frame's border maps far outside (empty tiles), the centre tiles
    # gather the whole source (fallback), the ring between them is staged
    "zoom": _case(384, 192, 100, [6, 0, 0, 0, 0], 193.5, 95.25),
    # the radial polynomial turns over inside the frame: the map folds back on itself
    "fold": _case(320, 192, 50, [-0.4, 0.05, 0, 0, 0], 161.25, 96.5),
    # every quantity a power of two: u * 32 = 32 j + 1/2 and v * 32 = 32 i - 1/2, exactly
    "ties": _case(96, 40, 64, [], 48 + 1 / 64, 20 - 1 / 64),
    # 1 + k4 r^2 = 0 on r^2 = 1/4, reached exactly 64 pixels left / right / above / below the centre
    "pole_inf": _case(320, 192, 128, [0.1, 0, 0, 0, 0, -4, 0, 0], 160.25, 96.5),
    # numerator and denominator vanish together there: 0 / 0
    "pole_nan": _case(320, 192, 128, [-4, 0, 0, 0, 0, -4, 0, 0], 160.25, 96.5),
}
POLE_PIXELS = [(32, 160), (96, 96), (96, 224), (160, 160)]  # (row, col) of the pole cases
SIZES = [(1, 1), (2, 2), (3, 5), (63, 15), (64, 16), (65, 17), (132, 40)]
for _w, _h in SIZES:
    CASES[f"size_{_w}x{_h}"] = _case(_w, _h, max(_w, _h, 8), MILD, _w * 0.5 + 0.3, _h * 0.5 - 0.2)
SIZE_CASES = [f"size_{w}x{h}" for w, h in SIZES]
POLE_CASES = ["pole_inf", "pole_nan"]
ALL_CASES = list(CASES)


def source(name: str, frames: int = 1, seed: int = 0) -> np.ndarray:
    """(frames, h, w) uniform random uint8, every frame different; the pole cases get
    src[0, 0] = 255, the value a NaN entry converted to 0 would show."""
    c = CASES[name]
    rng = np.random.default_rng([seed, c["w"], c["h"]])
    s = rng.integers(0, 256, (frames, c["h"], c["w"]), dtype=np.uint8)
    if name in POLE_CASES:
        s[:, 0, 0] = 255
    return s


_ORACLE_MAPS: dict = {}


def oracle_maps(O, name: str):
    """(mapx, mapy) of a case from the CPU oracle, computed once."""
    if name not in _ORACLE_MAPS:
        c = CASES[name]
        _, mx, my, _ = O.undistort_image(np.zeros((c["h"], c["w"]), np.uint8), c["kd"], np.float32(c["dist"]))
        mx.setflags(write=False)
        my.setflags(write=False)
        _ORACLE_MAPS[name] = (mx, my)
    return _ORACLE_MAPS[name]


def expected(O, name: str, frames: np.ndarray) -> np.ndarray:
    """remap_reference of every frame on the oracle's maps, after checking that the oracle's own
    remap gives the same bytes."""
    c = CASES[name]
    mx, my = oracle_maps(O, name)
    ref = np.stack([remap_reference(f, mx, my) for f in frames])
    for f, r in zip(frames, ref):
        assert np.array_equal(O.undistort_image(f, c["kd"], np.float32(c["dist"]))[0], r), (name, "oracle != reference")
    ref.setflags(write=False)
    return ref


def fixed_point(u, half_away: bool = False, nan_to_zero: bool = False) -> np.ndarray:
    """cvRound(float32(u) * 32) as int64 values of an int32."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (np.asarray(u, np.float32) * np.float32(32)).astype(np.float64)
    ok = np.isfinite(p) & (p >= -2.0 ** 31) & (p < 2.0 ** 31)
    q = np.where(ok, p, 0.0)
    r = np.sign(q) * np.floor(np.abs(q) + 0.5) if half_away else np.rint(q)
    X = np.where(ok, r.astype(np.int64), INT_MIN)
    if nan_to_zero:
        X = np.where(np.isnan(p), 0, X)
    return X


def _taps(X, Y, w, h):
    """Integer positions of the 4 taps (order 00, 01, 10, 11) and which lie in the frame."""
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    xs = np.stack([sx, sx + 1, sx, sx + 1])
    ys = np.stack([sy, sy, sy + 1, sy + 1])
    return xs, ys, (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)


def _remap(src, mapx, mapy, half_away=False, bias=1 << 14, replicate=False, nan_to_zero=False):
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    X = fixed_point(mapx, half_away, nan_to_zero)
    Y = fixed_point(mapy, half_away, nan_to_zero)
    tx, ty = X & 31, Y & 31
    wts = np.stack([(32 - ty) * (32 - tx) * 32, (32 - ty) * tx * 32, ty * (32 - tx) * 32, ty * tx * 32])
    origin = (tx | ty) == 0
    wts[0][origin] = 32767
    wts[3][origin] = 1
    xs, ys, inside = _taps(X, Y, w, h)
    vals = src[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)].astype(np.int64)
    if not replicate:
        vals *= inside
    return np.clip(((vals * wts).sum(0) + bias) >> 15, 0, 255).astype(np.uint8)


def remap_reference(src, mapx, mapy) -> np.ndarray:
    """cv::remap(src, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT 0) of one 8UC1 frame."""
    return _remap(src, mapx, mapy)


# Wrong variants of remap_reference and the case whose inputs must tell each from the right one.
MUTANTS = {
    "half_away": ("ties", lambda s, mx, my: _remap(s, mx, my, half_away=True)),
    "no_bias": ("zoom", lambda s, mx, my: _remap(s, mx, my, bias=0)),
    "replicate": ("fold", lambda s, mx, my: _remap(s, mx, my, replicate=True)),
    "nan_to_zero": ("pole_nan", lambda s, mx, my: _remap(s, mx, my, nan_to_zero=True)),
}


def half_way_fraction(mapx, mapy) -> float:
    """Of the entries whose 2x2 block touches the frame, the share with u * 32 and v * 32 both
    exactly half-way between two integers."""
    h, w = mapx.shape
    _, _, inside = _taps(fixed_point(mapx), fixed_point(mapy), w, h)
    sel = inside.any(0)
    px = np.float32(mapx[sel]) * np.float32(32)
    py = np.float32(mapy[sel]) * np.float32(32)
    tie = (np.abs(px - np.floor(px)) == 0.5) & (np.abs(py - np.floor(py)) == 0.5)
    return float(tie.mean()) if sel.any() else 0.0


def tile_kinds(mapx, mapy, w: int, h: int) -> np.ndarray:
    """(tile rows, tile columns) of EMPTY / STAGED / FALLBACK by the rule of remap_boxes_kernel."""
    xs, ys, inside = _taps(fixed_point(mapx), fixed_point(mapy), w, h)
    big = 1 << 20
    lo_x = np.where(inside, xs, big).min(0)
    hi_x = np.where(inside, xs, -big).max(0)
    lo_y = np.where(inside, ys, big).min(0)
    hi_y = np.where(inside, ys, -big).max(0)
    nty, ntx = -(-h // TILE_H), -(-w // TILE_W)

    def per_tile(a, fill, red):
        p = np.full((nty * TILE_H, ntx * TILE_W), fill, np.int64)
        p[:h, :w] = a
        return red(red(p.reshape(nty, TILE_H, ntx, TILE_W), 3), 1)

    x0, x1 = per_tile(lo_x, big, np.min), per_tile(hi_x, -big, np.max)
    y0, y1 = per_tile(lo_y, big, np.min), per_tile(hi_y, -big, np.max)
    xa = x0 & ~3
    wp = ((x1 + 1 - xa) + 3) & ~3
    hh = y1 - y0 + 1
    return np.where(x1 < x0, EMPTY, np.where(wp * hh <= BOX_BYTES, STAGED, FALLBACK))


def tile_pixels(kinds: np.ndarray, kind: int, w: int, h: int) -> np.ndarray:
    """(h, w) mask of the pixels whose tile is of that kind."""
    return np.repeat(np.repeat(kinds == kind, TILE_H, 0), TILE_W, 1)[:h, :w]


def frame_index(base: int, stride: int, pitch: int, w: int, h: int, batch: int) -> np.ndarray:
    """(batch, h, w) byte offsets of the pixels of a strided batch that starts at byte `base`."""
    f = np.arange(batch, dtype=np.int64)[:, None, None]
    r = np.arange(h, dtype=np.int64)[None, :, None]
    c = np.arange(w, dtype=np.int64)[None, None, :]
    return base + f * pitch + r * stride + c


def assert_canary(buf: np.ndarray, base: int, stride: int, pitch: int, w: int, h: int, batch: int, what=""):
    """buf: every byte of a destination allocated with slack and prefilled with CANARY, copied back.
    Each byte outside [row * stride, row * stride + w) of every frame, the bytes before the first
    frame and after the last included, is still CANARY."""
    flat = np.asarray(buf, np.uint8).reshape(-1)
    idx = frame_index(base, stride, pitch, w, h, batch)
    assert idx.min() >= 0 and idx.max() < flat.size, (what, "the frames do not fit the buffer")
    assert base > 0 and idx.max() + 1 < flat.size, (what, "no canary bytes before or after the frames")
    untouched = np.ones(flat.size, bool)
    untouched[idx.reshape(-1)] = False
    bad = np.flatnonzero(untouched & (flat != CANARY))
    assert bad.size == 0, (what, "bytes outside the frames were written", bad[:8].tolist())
