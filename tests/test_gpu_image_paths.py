"""GPU parity of frame undistortion on every path of remap_linear_kernel (mageslam_amd/csrc/image.hip):
staged, global-fallback and empty tiles, the dword and byte staging loads and stores, both LDS
buffers, batches past one grid slice of 64 frames, ragged sizes, exact rounding ties and non-finite
map entries.

Bit-exact against image_cases.remap_reference on the oracle's maps (which test_image_reference.py
pins to the oracle's own remap, and image_cases.expected checks again for every frame used here).
Which path a tile took is read off the device's maps with image_cases.tile_kinds.  Destinations are
prefilled with a canary and checked byte for byte outside the frames; source padding is 255.
"""
import ctypes as C

import numpy as np
import pytest

import image_cases as ic
from mageslam_amd import _lib, image
from mageslam_amd._lib import MAGE_EINVAL, MAGE_OK, Calibration, ptr

pytestmark = pytest.mark.gpu

D_BASE = 16  # canary bytes in front of the first destination frame (keeps its dword alignment)
SLACK = 64


@pytest.fixture(scope="module")
def und(gpu):
    """name -> Undistorter of that case, created once."""
    made = {}

    def get(name):
        if name not in made:
            c = ic.CASES[name]
            made[name] = image.Undistorter(Calibration.make(*c["kd"], c["dist"]), c["w"], c["h"])
        return made[name]

    yield get
    for u in made.values():
        u.close()


@pytest.fixture(scope="module")
def want(oracle):
    """(name, frames) -> (source frames, expected frames), computed once and read-only."""
    made = {}

    def get(name, frames):
        if (name, frames) not in made:
            src = ic.source(name, frames)
            src.setflags(write=False)
            made[name, frames] = (src, ic.expected(oracle, name, src))
        return made[name, frames]

    return get


def run_device(u, frames, s_stride=None, s_pitch=None, s_base=0, d_stride=None, d_pitch=None, d_base=D_BASE, what=""):
    """Undistorts (B, h, w) host frames through mage_undistort_image_batch_device with the given
    layout (strides and pitches in bytes, bases as byte offsets into the allocations); checks the
    canary around the destination frames and returns them as (B, h, w)."""
    import torch

    B, h, w = frames.shape
    s_stride = s_stride or w
    s_pitch = s_pitch or s_stride * h
    d_stride = d_stride or w
    d_pitch = d_pitch or d_stride * h
    src_h = np.full(s_base + B * s_pitch + SLACK, 255, np.uint8)
    src_h[ic.frame_index(s_base, s_stride, s_pitch, w, h, B)] = frames
    src = torch.from_numpy(src_h).cuda()
    dst = torch.full((d_base + B * d_pitch + SLACK,), ic.CANARY, dtype=torch.uint8, device="cuda")
    u.batch_device(src.data_ptr() + s_base, s_stride, s_pitch, dst.data_ptr() + d_base, d_stride, d_pitch, B)
    torch.cuda.synchronize()
    dst_h = dst.cpu().numpy()
    assert np.array_equal(src.cpu().numpy(), src_h), (what, "the source was written")
    ic.assert_canary(dst_h, d_base, d_stride, d_pitch, w, h, B, what)
    return dst_h[ic.frame_index(d_base, d_stride, d_pitch, w, h, B)]


def assert_frames(got, ref, what):
    assert got.shape == ref.shape, what
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (what, len(bad), "pixels differ; first (frame, row, col):", bad[:6].tolist())


@pytest.mark.parametrize("name", ic.ALL_CASES)
def test_maps_equal_oracle(und, oracle, name):
    """Float bits of both maps; a NaN only has to be a NaN at the same place (sign and payload of an
    invalid operation's result differ between x86 and the GPU)."""
    gx, gy = und(name).maps()
    for g, o in zip((gx, gy), ic.oracle_maps(oracle, name)):
        nan = np.isnan(o)
        assert np.array_equal(np.isnan(g), nan), name
        assert np.array_equal(g.view(np.uint32)[~nan], o.view(np.uint32)[~nan]), name


@pytest.mark.parametrize("name,kinds", [("zoom", (ic.EMPTY, ic.STAGED, ic.FALLBACK)), ("fold", (ic.STAGED, ic.FALLBACK))])
def test_tile_kinds(und, want, name, kinds):
    c = ic.CASES[name]
    u = und(name)
    k = ic.tile_kinds(*u.maps(), c["w"], c["h"])
    for kind in kinds:
        assert (k == kind).sum() >= 1, (name, "no tile of kind", kind)
    src, ref = want(name, 3)
    got = run_device(u, src, what=name)
    assert_frames(got, ref, name)
    for kind in kinds:  # each class on its own: a missing one must not hide in the whole image
        m = ic.tile_pixels(k, kind, c["w"], c["h"])
        assert m.any() and np.array_equal(got[:, m], ref[:, m]), (name, kind)
    if ic.EMPTY in kinds:
        assert not got[:, ic.tile_pixels(k, ic.EMPTY, c["w"], c["h"])].any()
    assert ref[:, ic.tile_pixels(k, ic.FALLBACK, c["w"], c["h"])].any()  # fallback tiles carry image content


@pytest.mark.parametrize("batch", [1, 2, 3, 64, 65, 130])
def test_batch_counts(und, want, batch):
    """Grid slices of 64 frames (blockIdx.z 0..2) and both LDS buffers; every frame is different."""
    src, ref = want("size_132x40", 130)
    assert len({f.tobytes() for f in src}) == 130
    assert_frames(run_device(und("size_132x40"), src[:batch], what=batch), ref[:batch], batch)


def _layouts(w, h):
    """Named (source / destination) layouts: keyword arguments of run_device."""
    return {
        "a_aligned_padded": dict(s_stride=w + 4, s_pitch=(w + 4) * h + 8, d_stride=w + 4),
        "b_odd_src_stride": dict(s_stride=w + 3),
        "c_src_base_1": dict(s_base=1),
        "d_odd_src_pitch": dict(s_pitch=w * h + 1),
        "e_dst_stride_base_1": dict(d_stride=w + 1, d_base=D_BASE + 1),
        "e_dst_stride_base_2": dict(d_stride=w + 1, d_base=D_BASE + 2),
        "f_dst_pitch": dict(d_pitch=w * h + 40),
    }


@pytest.mark.parametrize("layout", list(_layouts(4, 4)))
@pytest.mark.parametrize("name", ["size_132x40", "fold"])
def test_strides_and_alignment(und, want, name, layout):
    c = ic.CASES[name]
    src, ref = want(name, 3)
    got = run_device(und(name), src, what=(name, layout), **_layouts(c["w"], c["h"])[layout])
    assert_frames(got, ref, (name, layout))


def host_entry(u, img, s_pad=0, d_pad=0):
    """mage_undistort_image on numpy views of wider arrays (source padding 255, destination canary)."""
    h, w = img.shape
    src = np.full((h, w + s_pad), 255, np.uint8)
    src[:, :w] = img
    dst = np.full((h + 2, w + d_pad), ic.CANARY, np.uint8)
    st = _lib.load().mage_undistort_image(u._h, ptr(src), w + s_pad, ptr(dst[1:]), w + d_pad)
    assert st == MAGE_OK, _lib.load().mage_last_error()
    ic.assert_canary(dst, w + d_pad, w + d_pad, 0, w, h, 1, "host entry")
    return dst[1:h + 1, :w]


@pytest.mark.parametrize("name", ["size_132x40", "fold"])
def test_host_entry_strides(und, want, name):
    src, ref = want(name, 3)
    for s_pad, d_pad in ((5, 7), (0, 3), (4, 0)):
        assert_frames(host_entry(und(name), src[0], s_pad, d_pad), ref[0], (name, s_pad, d_pad))


@pytest.mark.parametrize("name", ic.SIZE_CASES)
def test_sizes(und, want, name):
    """Widths below a tile (and below one thread's 4 pixels), heights below a tile row, one past both."""
    src, ref = want(name, 130 if name == "size_132x40" else 2)
    u = und(name)
    assert_frames(u(src[0]), ref[0], (name, "host"))
    assert_frames(host_entry(u, src[1], 3, 1), ref[1], (name, "host strided"))
    assert_frames(run_device(u, src[:2], what=name), ref[:2], (name, "device"))


def test_rounding_ties(und, want):
    """u * 32 and v * 32 exactly half-way at every pixel: round half to even."""
    src, ref = want("ties", 2)
    u = und("ties")
    assert_frames(u(src[0]), ref[0], "host")
    assert_frames(run_device(u, src, what="ties"), ref, "device")


@pytest.mark.parametrize("name", ic.POLE_CASES)
def test_non_finite_map_entries(und, want, name):
    """A NaN or infinite entry is an outlier and is written 0 (never the pixel at (0, 0), here 255)."""
    src, ref = want(name, 2)
    u = und(name)
    gx, gy = u.maps()
    bad = ~(np.isfinite(gx) & np.isfinite(gy))
    assert sorted(map(tuple, np.argwhere(bad).tolist())) == ic.POLE_PIXELS
    got = run_device(u, src, what=name)
    assert (src[:, 0, 0] == 255).all()
    assert [int(got[f][p]) for f in range(2) for p in ic.POLE_PIXELS] == [0] * 8
    assert_frames(got, ref, name)
    assert_frames(u(src[0]), ref[0], (name, "host"))


def test_arguments(und, want):
    import torch

    lib = _lib.load()
    name = "size_132x40"
    w, h = ic.CASES[name]["w"], ic.CASES[name]["h"]
    u = und(name)
    src, ref = want(name, 130)
    img = np.ascontiguousarray(src[0])
    out = np.zeros_like(img)
    d_src = torch.from_numpy(src[:2].copy()).cuda()
    d_dst = torch.full((2, h, w), ic.CANARY, dtype=torch.uint8, device="cuda")
    n = w * h
    # a stride below the width, on either side
    assert lib.mage_undistort_image(u._h, ptr(img), w - 1, ptr(out), w) == MAGE_EINVAL
    assert lib.mage_undistort_image(u._h, ptr(img), w, ptr(out), w - 1) == MAGE_EINVAL
    assert lib.mage_undistort_image_batch_device(u._h, ptr(d_src), w - 1, n, ptr(d_dst), w, n, 2, None) == MAGE_EINVAL
    assert lib.mage_undistort_image_batch_device(u._h, ptr(d_src), w, n, ptr(d_dst), w - 1, n, 2, None) == MAGE_EINVAL
    # a pitch below one frame with batch 2
    assert lib.mage_undistort_image_batch_device(u._h, ptr(d_src), w, n - 1, ptr(d_dst), w, n, 2, None) == MAGE_EINVAL
    assert lib.mage_undistort_image_batch_device(u._h, ptr(d_src), w, n, ptr(d_dst), w, n - 1, 2, None) == MAGE_EINVAL
    torch.cuda.synchronize()
    assert (d_dst.cpu().numpy() == ic.CANARY).all() and not out.any()  # a refused call writes nothing
    # batch 0 with null pointers
    assert lib.mage_undistort_image_batch_device(u._h, None, w, n, None, w, n, 0, None) == MAGE_OK
    # a width of 32768, ndist = 3
    c = ic.CASES[name]
    hnd = C.c_void_p()
    cal = Calibration.make(*c["kd"], c["dist"])
    assert lib.mage_undistorter_create(C.byref(cal), 32768, 8, 0, C.byref(hnd), None) == MAGE_EINVAL and not hnd.value
    cal3 = Calibration.make(*c["kd"], c["dist"])
    cal3.ndist = 3
    assert lib.mage_undistorter_create(C.byref(cal3), w, h, 0, C.byref(hnd), None) == MAGE_EINVAL and not hnd.value
    # the refused calls leave the instance usable
    assert_frames(u(img), ref[0], "host after refusals")
    u.batch_device(d_src, w, n, d_dst, w, n, 2)
    torch.cuda.synchronize()
    assert_frames(d_dst.cpu().numpy(), ref[:2], "device after refusals")
