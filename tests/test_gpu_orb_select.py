"""GPU parity of select_kernel on the frames of tests/orb_select_cases.py: mass ties, the retained
count at and above KMAX, degenerate extents, frames up to 4095 pixels wide or high, a capacity
that ends inside a pyramid level, redo lists longer than the redo grid, and the status word.

Byte for byte against the CPU oracle, as tests/test_gpu_orb.py: 28-byte keypoints and 32-byte
descriptors, no tolerances.  tests/test_orb_select_cases.py checks on the CPU that each frame
reaches its branch.
"""
import numpy as np
import pytest

from mageslam_amd import orb
from mageslam_amd._lib import MAGE_ECAPACITY, MAGE_EUNSUPPORTED, MageError
from tests import orb_select_cases as sc

pytestmark = pytest.mark.gpu

PYRAMID = dict(nlevels=4, patchSize=31, useOrientation=True)
PYRAMID3 = dict(nlevels=3, patchSize=31, useOrientation=True)


def kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8)


def assert_exact(got, want, what):
    (kp, d), (okp, od) = got, want
    assert len(kp) == len(okp), what
    assert np.array_equal(kp_bytes(kp), kp_bytes(okp)), what
    assert np.array_equal(d, od), what


def run_batch(det, frames_np, cap):
    """One device batch; returns the per-frame (keypoint bytes, descriptors) without a status check."""
    import torch

    B, h, w = frames_np.shape
    frames = torch.from_numpy(np.array(frames_np, order="C")).cuda()  # a writable copy: the cases are read-only
    kp = torch.zeros((B, cap * 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    det.detect_and_compute_batch_device(frames, w, h, kp, desc, n, cap)
    torch.cuda.synchronize()
    kp_h, desc_h, n_h = kp.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()
    return [(kp_h[i, : 28 * n_h[i]], desc_h[i, : n_h[i]]) for i in range(B)]


def assert_batch_exact(outs, wants, what):
    assert len(outs) == len(wants)
    for i, ((kb, d), (okp, od)) in enumerate(zip(outs, wants)):
        assert len(kb) == 28 * len(okp), (what, i)
        assert np.array_equal(kb, kp_bytes(okp).reshape(-1)), (what, i)
        assert np.array_equal(d, od), (what, i)


# ------------------------- parity -------------------------


@pytest.mark.parametrize("name", sc.PARITY)
def test_single_image_matches_oracle(gpu, oracle, name):
    det = orb.OrbDetector(nfeatures=sc.nfeatures(name))
    want = sc.expected_case(name)
    assert len(want[0]) > 0
    assert_exact(det.DetectAndCompute(sc.frame(name)), want, name)


@pytest.mark.parametrize("name", sc.BATCH_PARITY)
def test_batch_with_plain_neighbour_matches_oracle(gpu, oracle, name):
    # the tie-heavy / large frame between two copies of an ordinary one: neither changes the other
    img = sc.frame(name)
    h, w = img.shape
    N = sc.nfeatures(name)
    plain = sc.plain(w, h)
    det = orb.OrbDetector(nfeatures=N)
    outs = run_batch(det, np.stack([plain, img, plain]), N)
    det.device_status()
    want_plain = sc.expected(("plain", w, h), plain, {}, N)
    assert_batch_exact(outs, [want_plain, sc.expected_case(name), want_plain], name)


# ------------------------- KMAX -------------------------


def test_kmax_overflow_single_image(gpu, oracle):
    det = orb.OrbDetector(nfeatures=sc.nfeatures("kmax+1"))
    with pytest.raises(MageError) as e:
        det.DetectAndCompute(sc.frame("kmax+1"))
    assert e.value.status == MAGE_ECAPACITY
    # the flag is per call here: the last size that fits succeeds on the same detector
    assert_exact(det.DetectAndCompute(sc.frame("kmax")), sc.expected_case("kmax"), "kmax after kmax+1")


def test_kmax_overflow_batch_is_sticky_until_reset(gpu, oracle):
    bad = sc.frame("kmax+1")
    h, w = bad.shape
    N = sc.nfeatures("kmax+1")
    a, b = sc.plain(w, h), sc.plain(w, h, 2)
    want_a, want_b = sc.expected(("plain", w, h), a, {}, N), sc.expected(("plain", w, h, 2), b, {}, N)
    det = orb.OrbDetector(nfeatures=N)
    outs = run_batch(det, np.stack([a, bad, b]), N)
    with pytest.raises(MageError) as e:
        det.device_status()
    assert e.value.status == MAGE_ECAPACITY
    # the frames around the overflowing one are untouched by it
    assert_batch_exact([outs[0], outs[2]], [want_a, want_b], "around kmax+1")
    with pytest.raises(MageError) as e:  # sticky
        det.device_status()
    assert e.value.status == MAGE_ECAPACITY
    outs = run_batch(det, np.stack([a, b]), N)
    with pytest.raises(MageError):  # a good batch does not clear it
        det.device_status()
    assert_batch_exact(outs, [want_a, want_b], "good batch, flag still set")
    det.reset_device_status()
    det.device_status()
    outs = run_batch(det, np.stack([a, sc.frame("kmax"), b]), N)
    det.device_status()
    assert_batch_exact(outs, [want_a, sc.expected_case("kmax"), want_b], "after reset")


# ------------------------- capacity ending inside a level -------------------------


@pytest.mark.parametrize("cap", sc.CAP_IN_LEVEL)
def test_capacity_inside_level_single(gpu, oracle, cap):
    det = orb.OrbDetector(nfeatures=sc.nfeatures("cap_in_level"), **PYRAMID)
    want = sc.expected_case("cap_in_level", cap=cap, **sc.PYRAMID)
    assert len(want[0]) == cap
    assert_exact(det.DetectAndCompute(sc.frame("cap_in_level"), capacity=cap), want, cap)


@pytest.mark.parametrize("cap", sc.CAP_IN_LEVEL)
def test_capacity_inside_level_batch(gpu, oracle, cap):
    from mageslam_amd import synth

    N = sc.nfeatures("cap_in_level")
    frames = np.stack([sc.frame("cap_in_level"), synth.frame(1, 640, 480), synth.frame(2, 640, 480)])
    wants = [sc.expected(("cap", i), f, sc.PYRAMID, N, cap) for i, f in enumerate(frames)]
    for kp, _ in wants:
        octaves = np.bincount(kp["octave"], minlength=4)
        assert len(kp) == cap and octaves[1] > 0 and octaves[2] == 0
    det = orb.OrbDetector(nfeatures=N, **PYRAMID)
    outs = run_batch(det, frames, cap)
    det.device_status()
    assert_batch_exact(outs, wants, cap)


# ------------------------- redo lists longer than the redo grid -------------------------


def test_redo_list_longer_than_grid(gpu, oracle):
    frames = sc.redo_frames()
    det = orb.OrbDetector(nfeatures=sc.REDO_N)
    det.set_fast_gate(sc.REDO_GATE)
    outs = run_batch(det, frames, sc.REDO_N)
    det.device_status()
    st = det.fast_gate_stats()
    print("redo20 single level:", st)
    assert st["last_gate"] == sc.REDO_GATE and st["last_redo"] == sc.REDO_FRAMES
    assert_batch_exact(outs, [sc.expected(("redo", i), f, {}, sc.REDO_N) for i, f in enumerate(frames)], "redo20")


def test_redo_list_longer_than_grid_pyramid(gpu, oracle):
    frames = sc.redo_frames()
    det = orb.OrbDetector(nfeatures=sc.REDO_N, **PYRAMID3)
    for l in range(3):
        det.set_fast_gate(sc.REDO_GATE, level=l)
    outs = run_batch(det, frames, sc.REDO_N)
    det.device_status()
    for l in range(3):
        st = det.fast_gate_stats(level=l)
        print("redo20 pyramid level", l, st)
        assert st["last_gate"] == sc.REDO_GATE and st["last_redo"] == sc.REDO_FRAMES, l
    wants = [sc.expected(("redo", i), f, sc.PYRAMID3, sc.REDO_N) for i, f in enumerate(frames)]
    assert_batch_exact(outs, wants, "redo20 pyramid")


def test_redo_list_mixed_with_blank_frames(gpu, oracle):
    frames = sc.redo_frames(blank=True)
    det = orb.OrbDetector(nfeatures=sc.REDO_N)
    det.set_fast_gate(sc.BLANK_GATE)
    outs = run_batch(det, frames, sc.REDO_N)
    det.device_status()
    st = det.fast_gate_stats()
    print("redo20 mixed list:", st)
    assert st["last_gate"] == sc.BLANK_GATE and st["last_redo"] >= len(sc.REDO_BLANK)
    plain = sc.redo_frames()
    wants = []
    for i, f in enumerate(frames):
        if i in sc.REDO_BLANK:
            wants.append(sc.expected("blank", f, {}, sc.REDO_N))
            assert len(wants[-1][0]) == 0
        else:
            wants.append(sc.expected(("redo", i), plain[i], {}, sc.REDO_N))
    assert_batch_exact(outs, wants, "mixed redo list")


# ------------------------- limits and the cell-count flag -------------------------


def test_frame_size_limits(gpu):
    det = orb.OrbDetector(nfeatures=100)
    for shape in ((16, 4096), (4096, 16)):
        with pytest.raises(MageError) as e:
            det.DetectAndCompute(np.full(shape, 128, np.uint8))
        assert e.value.status == MAGE_EUNSUPPORTED
    kp, d = det.DetectAndCompute(np.full((16, 4095), 128, np.uint8))
    assert len(kp) == 0 and d.shape == (0, 32)


def test_too_many_cells(gpu, oracle):
    img = sc.frame("cells")
    N = sc.nfeatures("cells")
    det = orb.OrbDetector(nfeatures=N, numCellsX=128, numCellsY=64)
    with pytest.raises(MageError) as e:
        det.DetectAndCompute(img)
    assert e.value.status == MAGE_EUNSUPPORTED
    det64 = orb.OrbDetector(nfeatures=N, numCellsX=64, numCellsY=64)
    assert_exact(det64.DetectAndCompute(img), sc.expected_case("cells", num_cells_x=64, num_cells_y=64), "64x64 cells")
