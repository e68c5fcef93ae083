"""GPU parity of select_kernel's box-pruned ANMS search on the frames of
tests/orb_select_box_cases.py: neighbours on the last row and column of the box, boxes that leave
the bounding box, boxes over seven and more cells (the frames that took the ring loop), 1x1 to
64x64 cell grids, gmax = 0 and 1, a bounding box narrower than the grid (where the reference's
ring order decides and the kernel walks the rings), batches whose frames differ in every per-frame
value, and the pyramid's append path.

Byte for byte against the CPU oracle, as tests/test_gpu_orb_select.py: 28-byte keypoints and
32-byte descriptors, no tolerances.  tests/test_orb_select_box_cases.py checks on the CPU that
each frame has its property.
"""
import numpy as np
import pytest

from mageslam_amd import orb
from tests import orb_select_box_cases as bc

pytestmark = pytest.mark.gpu

PYRAMID = dict(nlevels=4, patchSize=31, useOrientation=True)


def kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8)


def assert_exact(got, want, what):
    (kp, d), (okp, od) = got, want
    assert len(kp) == len(okp), what
    assert np.array_equal(kp_bytes(kp), kp_bytes(okp)), what
    assert np.array_equal(d, od), what


def run_batch(det, frames_np, cap):
    """One device batch: the per-frame (keypoint bytes, descriptors)."""
    import torch

    B, h, w = frames_np.shape
    frames = torch.from_numpy(np.array(frames_np, order="C")).cuda()  # a writable copy: the cases are read-only
    kp = torch.zeros((B, cap * 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    det.detect_and_compute_batch_device(frames, w, h, kp, desc, n, cap)
    torch.cuda.synchronize()
    det.device_status()
    kp_h, desc_h, n_h = kp.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()
    return [(kp_h[i, : 28 * n_h[i]], desc_h[i, : n_h[i]]) for i in range(B)]


def single(name, N, **det_kw):
    want = bc.expected(name, N, **{{"numCellsX": "num_cells_x", "numCellsY": "num_cells_y"}[k]: v for k, v in det_kw.items()})
    assert len(want[0]) == N
    assert_exact(orb.OrbDetector(nfeatures=N, **det_kw).DetectAndCompute(bc.frame(name)), want, (name, N, det_kw))


@pytest.mark.parametrize("N", bc.BOX_EDGE_N)
def test_box_edge(gpu, oracle, N):
    single("lattice", N)


@pytest.mark.parametrize("name,N", bc.RING_CASES)
def test_former_ring_path(gpu, oracle, name, N):
    single(name, N)


@pytest.mark.parametrize("cells", bc.GRIDS)
def test_cell_grids(gpu, oracle, cells):
    single("grids", bc.GRIDS_N, numCellsX=cells[0], numCellsY=cells[1])


@pytest.mark.parametrize("name,N,cells", bc.DEGENERATE)
def test_degenerate_gmax(gpu, oracle, name, N, cells):
    single(name, N, numCellsX=cells[0], numCellsY=cells[1])


def test_thin_frame(gpu, oracle):
    single(*bc.THIN)


@pytest.mark.parametrize("names", bc.BATCHES)
def test_batch(gpu, oracle, names):
    N = bc.BATCH_N
    det = orb.OrbDetector(nfeatures=N)
    outs = run_batch(det, np.stack([bc.frame(n) for n in names]), N)
    assert len(outs) == len(names)
    for i, (name, (kb, d)) in enumerate(zip(names, outs)):
        okp, od = bc.expected(name, N)
        assert len(okp) == N
        assert len(kb) == 28 * len(okp), (names, i)
        assert np.array_equal(kb, kp_bytes(okp).reshape(-1)), (names, i)
        assert np.array_equal(d, od), (names, i)


def test_pyramid(gpu, oracle):
    N = bc.PYRAMID_N
    want = bc.expected("lattice", N, **bc.PYRAMID)
    assert_exact(orb.OrbDetector(nfeatures=N, **PYRAMID).DetectAndCompute(bc.frame("lattice")), want, "pyramid")
