"""GPU: pose_ba_kernel (mage_ba_pose_batch / mage_ba_pose_batch_device) against the plain fp64
NumPy reference of tests/pose_cases.py, not against the oracle, on the cases that reach rejected
trials, failed solves, the qmax == 10 exit, the "last trial rejected" post-pass sums, points behind
the camera in staged and unstaged workgroups, per-problem intrinsics and both launch branches.
test_pose_reference.py asserts on the CPU that every case reaches its branch and that the oracle
passes the same comparison.

Tolerances (tests/pose_cases.py): decisions are equal on non-fragile problems; float32 outputs
within 2 ulp of the converted reference; the fp64 state within 256 eps (cond2(H + lambda I) max|x|
+ max(1, max|t|)) after one step, and within max(1e-11, 100 x the oracle's own distance from the
reference) after several.
"""
import numpy as np
import pytest

from mageslam_amd import bundler
from tests import pose_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", P.CASE_IDS)
def test_pose_kernel_matches_reference(gpu, cid):
    pb, nsteps, huber, maxe, _ = P.case(cid)
    g = bundler.OptimizeCameraPoses(pb, nsteps, maxe, huber)
    P.check_outputs(g, cid, P.K_GPU, "gpu")


CANARY = 0xA5


def _guarded(torch, shape, dtype, dev):
    """A device buffer of `shape` followed by 64 canary bytes: (view, whole byte buffer, bytes)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=dev)
    return raw[:n].view(dtype).view(*shape), raw, n


def test_device_entry_and_optional_outputs(gpu):
    """mage_ba_pose_batch_device on device tensors: byte-identical to the host entry; with the
    optional qt7_out and stats null the other outputs are unchanged; no output is written past
    its end."""
    import torch

    cid = "far-behind-4"
    pb, nsteps, huber, maxe, _ = P.case(cid)
    host = bundler.OptimizeCameraPoses(pb, nsteps, maxe, huber)
    K, E = len(pb.pos), int(pb.obs_start[-1])
    dev = "cuda:0"
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    ins = (T(pb.pos, np.float32), T(pb.r9, np.float32), T(pb.intr, np.float32), T(pb.obs_start.astype(np.int32), np.int32),
           T(pb.points, np.float32), T(pb.uv, np.float32), T(pb.info, np.float32))

    def run(optional):
        bufs = dict(pos=_guarded(torch, (K, 3), torch.float32, dev), r9=_guarded(torch, (K, 9), torch.float32, dev),
                    qt7=_guarded(torch, (K, 7), torch.float64, dev), outlier=_guarded(torch, (E,), torch.uint8, dev),
                    mean_sq=_guarded(torch, (K,), torch.float32, dev), stats=_guarded(torch, (K, 2), torch.int32, dev))
        v = {k: b[0] for k, b in bufs.items()}
        bundler.pose_batch_device(K, *ins, nsteps, huber, maxe, v["pos"], v["r9"], v["qt7"] if optional else None,
                                  v["outlier"], v["mean_sq"], v["stats"] if optional else None)
        torch.cuda.synchronize()
        out = {}
        for k, (view, raw, n) in bufs.items():
            whole = raw.cpu().numpy()
            assert (whole[n:] == CANARY).all(), f"{k}: written past its end"
            out[k] = (view.cpu().numpy(), whole[:n])
        return out

    full = run(True)
    for k in ("pos", "r9", "qt7", "outlier", "mean_sq"):
        assert full[k][0].tobytes() == np.ascontiguousarray(host[k]).tobytes(), k
    assert np.array_equal(full["stats"][0].astype(np.uint32), host["stats"])
    part = run(False)
    for k in ("pos", "r9", "outlier", "mean_sq"):
        assert part[k][0].tobytes() == full[k][0].tobytes(), k
    for k in ("qt7", "stats"):  # never handed to the library: still the fill pattern
        assert (part[k][1] == CANARY).all(), k


def test_pose_kernel_is_deterministic(gpu):
    """The kernel's reductions are fixed-order: two runs give bit-identical fp64 states."""
    pb, nsteps, huber, maxe, _ = P.case("far-3")
    a = bundler.OptimizeCameraPoses(pb, nsteps, maxe, huber)
    b = bundler.OptimizeCameraPoses(pb, nsteps, maxe, huber)
    assert a["qt7"].tobytes() == b["qt7"].tobytes()
    assert np.array_equal(a["stats"], b["stats"]) and np.array_equal(a["outlier"], b["outlier"])
