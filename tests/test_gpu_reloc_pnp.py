"""The relocalisation PnP kernels (mageslam_amd/csrc/reloc_pnp.hip) against their plain C++ twin
(mage_reloc_pnp_host, itself checked against an independent formulation in
test_reloc_pnp_reference.py): result records, inlier indices, obs_start, the compacted bundle
adjustment arrays, poses and the whole trace byte-identical — one problem at a time over the case
table of tests/reloc_pnp_cases.py, and every case in one batch with an over-limit and a bad-index
problem in the middle of it; and the pose bundle adjustment queued behind the stage on one stream."""
import dataclasses

import numpy as np
import pytest

from mageslam_amd import bundler, reloc
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, RP_RESULT_DTYPE
from tests import reloc_pnp_cases as rc

pytestmark = pytest.mark.gpu

FILL = 0xA5
FIELDS = ("verdict", "status", "pos3", "r9", "inliers", "points3", "uv", "info")


def same(g, h, what):
    assert g.result.tobytes() == h.result.tobytes(), (what, "result", g.result, h.result)
    for f in FIELDS:
        a, b = getattr(g, f), getattr(h, f)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, f)
        else:
            assert a == b, (what, f)
    assert (g.trace is None) == (h.trace is None), what
    if g.trace is not None:
        for f in g.trace.dtype.names:
            if f != "pad":
                assert g.trace[f].tobytes() == h.trace[f].tobytes(), (what, "trace", f)


@pytest.mark.parametrize("name", rc.NAMES)
def test_kernel_equals_host_twin(gpu, name):
    """The single-problem form, every case under its own settings."""
    c = rc.case(name)
    g = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, c.matches, backend="hip", want_trace=True)
    same(g, rc.twin(name), name)


def test_single_form_cap_and_bad_problems(gpu):
    c = rc.case("behind60")
    for cap in (0, 7):
        g = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, c.matches, backend="hip", cap=cap)
        h = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, c.matches, backend="host", cap=cap)
        same(g, h, f"cap {cap}")
        assert g.status == reloc.STATUS_OVER_CAP and len(g.inliers) == cap
    bad = c.matches.copy()
    bad["train_idx"][5] = len(c.kp)
    over = np.zeros(reloc.MAX_MATCHES + 1, DM_DTYPE)
    for mm, status in ((bad, reloc.STATUS_BAD_INDEX), (over, reloc.STATUS_OVER_LIMIT)):
        g = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, mm, backend="hip", want_trace=True)
        h = reloc.pnp_ransac(c.settings, rc.INTR, c.map_xyzi, c.kp, mm, backend="host", want_trace=True)
        same(g, h, status)
        assert g.status == status


class Batch:
    """Every case as one problem of a single launch under shared settings, at pitches larger than the
    counts, every output prefilled with 0xA5; problem 3 is over the match capacity and problem 6
    names a candidate keypoint with no map point."""

    OVER, BAD = 3, 6

    def __init__(self, settings):
        import torch

        self.settings = settings
        self._twins = None
        cs = [rc.case(n) for n in rc.NAMES]
        bad = dataclasses.replace(cs[4], matches=cs[4].matches.copy())
        bad.matches["query_idx"][7] = np.flatnonzero(bad.map_xyzi[:, 3] <= 0)[0]
        cs.insert(self.OVER, cs[5])
        cs.insert(self.BAD, bad)
        self.cs = cs
        P = self.P = len(cs)
        self.kf_pitch = max(len(c.map_xyzi) for c in cs) + 9
        self.kp_pitch = max(len(c.kp) for c in cs) + 3
        self.match_cap = max(len(c.matches) for c in cs) + 5
        self.cap = 100  # below half300's kept count
        self.iters = settings.ransac_iterations
        intr = np.tile(rc.INTR, (P, 1))
        mp = np.zeros((P, self.kf_pitch, 4), np.float32)
        kp = np.zeros((P, self.kp_pitch), KP_DTYPE)
        mm = np.zeros((P, self.match_cap), DM_DTYPE)
        n = np.zeros((2, P), np.uint32)
        for i, c in enumerate(cs):
            mp[i, : len(c.map_xyzi)] = c.map_xyzi
            kp[i, : len(c.kp)] = c.kp
            mm[i, : len(c.matches)] = c.matches
            n[:, i] = len(c.kp), len(c.matches)
        n[1, self.OVER] = self.match_cap + 1
        self.mp, self.n = mp, n
        dev = torch.device("cuda")
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        self.d = dict(intr=up(intr), mp=up(mp), kp=up(kp), mm=up(mm), n=up(n))
        self.tbytes = reloc.trace_bytes(self.iters)
        self.sizes = dict(result=RP_RESULT_DTYPE.itemsize * P, idx=4 * P * self.cap, obs_start=4 * (P + 1),
                          points3=12 * P * self.cap, uv=8 * P * self.cap, info=4 * P * self.cap, pos3=12 * P, r9=36 * P,
                          trace=self.tbytes * P,
                          scratch=reloc.scratch_bytes(self.iters, P, self.match_cap, True))

    def run(self, then=None):
        import torch

        o = {k: torch.full((v,), FILL, dtype=torch.uint8, device="cuda") for k, v in self.sizes.items()}
        P, d = self.P, self.d
        stream = torch.cuda.current_stream().cuda_stream
        reloc.pnp_ransac_batch_device(self.settings, P, d["intr"], d["mp"], self.kf_pitch, d["kp"], self.kp_pitch,
                                      d["n"].data_ptr(), d["mm"], self.match_cap, d["n"].data_ptr() + 4 * P, o["result"],
                                      o["idx"], self.cap, o["obs_start"], o["points3"], o["uv"], o["info"], o["pos3"],
                                      o["r9"], o["trace"], o["scratch"], stream)
        extra = then(o, stream) if then else None
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        return (out, extra) if then else out

    def twins(self):
        """Per problem the twin's outcome (its candidate the whole pitch, as the kernels see it), None
        for the over-capacity problem (the twin has no capacity)."""
        if self._twins is None:
            self._twins = self._run_twins()
        return self._twins

    def _run_twins(self):
        hs = []
        for i, c in enumerate(self.cs):
            hs.append(None if i == self.OVER else
                      reloc.pnp_ransac(self.settings, rc.INTR, self.mp[i], c.kp, c.matches, backend="host",
                                       want_trace=True, cap=self.cap))
        return hs


def check_batch(b, out, hs):
    P, cap = b.P, b.cap
    res = out["result"].view(RP_RESULT_DTYPE)
    idx = out["idx"].view(np.uint32).reshape(P, cap)
    start = out["obs_start"].view(np.uint32)
    points3, uv, info = out["points3"].view(np.float32), out["uv"].view(np.float32), out["info"].view(np.float32)
    trace = out["trace"].reshape(P, b.tbytes)
    at = 0
    for i, h in enumerate(hs):
        what = (i, b.cs[i].name)
        assert start[i] == at, what
        if h is None:
            want = np.zeros(1, RP_RESULT_DTYPE)
            want["status"], want["n_matches"], want["win_iteration"] = reloc.STATUS_OVER_LIMIT, b.match_cap + 1, -1
            want["win_indices"], want["r9"] = -1, np.eye(3, dtype=np.float32).reshape(9)
            assert res[i].tobytes() == want.tobytes(), what
            nk, nb, tr = 0, 0, None
            pos3, r9 = want["pos3"][0], want["r9"][0]
        else:
            assert res[i].tobytes() == h.result.tobytes(), (what, res[i], h.result)
            nk, nb, tr = len(h.inliers), len(h.points3), h.trace
            pos3, r9 = h.pos3, h.r9
            assert idx[i, :nk].tobytes() == h.inliers.tobytes(), what
            assert points3[3 * at:3 * (at + nb)].tobytes() == h.points3.tobytes(), what
            assert uv[2 * at:2 * (at + nb)].tobytes() == h.uv.tobytes(), what
            assert info[at:at + nb].tobytes() == h.info.tobytes(), what
        assert out["pos3"].view(np.float32)[3 * i:3 * i + 3].tobytes() == pos3.tobytes(), what
        assert out["r9"].view(np.float32)[9 * i:9 * i + 9].tobytes() == r9.tobytes(), what
        # nothing past the counts, and a problem that stopped early leaves its trace alone
        assert (idx[i, nk:].view(np.uint8) == FILL).all(), what
        if tr is None:
            assert (trace[i] == FILL).all(), what
        else:
            got = trace[i].view(tr.dtype)[0]
            for f in tr.dtype.names:  # an odd iteration count leaves four bytes of padding, which nobody writes
                if f != "pad":
                    assert got[f].tobytes() == tr[f].tobytes(), (what, "trace", f)
        at += nb
    assert start[P] == at
    for k, per in (("points3", 12), ("uv", 8), ("info", 4)):
        assert (out[k][per * at:] == FILL).all(), k
    return at


@pytest.fixture(scope="module")
def wide():
    """The gate at four matches and 65 iterations: every case runs its RANSAC, 65 crosses a workgroup."""
    return Batch(reloc.RelocalizationSettings(min_brute_force_correspondences=4, ransac_iterations=65))


def test_batch_equals_host_twin(gpu, wide):
    hs = wide.twins()
    verdicts = [None if h is None else (h.status, h.verdict) for h in hs]
    assert verdicts[wide.BAD] == (reloc.STATUS_BAD_INDEX, reloc.OK)
    assert (0, reloc.NO_MODEL) in verdicts and (0, reloc.FEW_INLIERS) in verdicts
    assert (reloc.STATUS_OVER_CAP, reloc.OK) in verdicts  # half300 keeps more than the capacity
    total = check_batch(wide, wide.run(), hs)
    assert total == sum(len(h.points3) for h in hs if h is not None) > 0
    # the neighbours of the bad problems are what they are on their own
    for i in (wide.OVER - 1, wide.OVER + 1, wide.BAD - 1, wide.BAD + 1):
        assert hs[i].status in (0, reloc.STATUS_OVER_CAP) and hs[i].trace is not None


def test_batch_default_settings(gpu):
    """MinBruteForceCorrespondences 20 and two iterations: the small cases stop at the gate."""
    b = Batch(reloc.RelocalizationSettings())
    hs = b.twins()
    assert sum(h is not None and h.verdict == reloc.FEW_MATCHES for h in hs) == 4
    check_batch(b, b.run(), hs)


def test_pose_bundle_adjustment_queued_behind(gpu, wide):
    """mage_ba_pose_batch_device on the stage's outputs, same stream, no host step: equal to the host
    path (the twin, then mage_ba_pose_batch on its arrays), byte for byte as the pose bundle
    adjustment's own device-entry test compares."""
    import torch

    s = wide.settings
    nsteps, huber = s.bundle_adjust_iterations, 1.8
    maxe = s.max_bundle_adjust_reprojection_error ** 2
    P, E = wide.P, wide.P * wide.cap

    def then(o, stream):
        f32 = lambda k: o[k].view(torch.float32)  # noqa: E731
        ba = dict(pos=torch.full((P, 3), -1.0, device="cuda"), r9=torch.full((P, 9), -1.0, device="cuda"),
                  outlier=torch.full((E,), FILL, dtype=torch.uint8, device="cuda"),
                  mean_sq=torch.full((P,), -1.0, device="cuda"))
        kw = reloc.pose_inputs(wide.d["intr"].view(torch.float32), o["obs_start"].view(torch.int32), f32("points3"),
                               f32("uv"), f32("info"), f32("pos3"), f32("r9"))
        bundler.pose_batch_device(P, nsteps=nsteps, huber=huber, max_error_square=maxe, pos3_out=ba["pos"],
                                  r9_out=ba["r9"], qt7_out=None, outlier=ba["outlier"], mean_sq=ba["mean_sq"],
                                  stream=stream, **kw)
        return ba

    out, ba = wide.run(then)
    hs = wide.twins()
    total = check_batch(wide, out, hs)

    class PoseBatch:
        pass

    pb = PoseBatch()
    ok = [h if h is not None else None for h in hs]
    eye = np.eye(3, dtype=np.float32).reshape(9)
    pb.pos = np.stack([h.pos3 if h is not None else np.zeros(3, np.float32) for h in ok])
    pb.r9 = np.stack([h.r9 if h is not None else eye for h in ok])
    pb.intr = np.tile(rc.INTR, (P, 1))
    counts = [0 if h is None else len(h.points3) for h in ok]
    pb.obs_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    cat = lambda f, w: np.concatenate([getattr(h, f).reshape(-1, w) for h in ok if h is not None])  # noqa: E731
    pb.points, pb.uv, pb.info = cat("points3", 3), cat("uv", 2), cat("info", 1).reshape(-1)
    assert int(pb.obs_start[-1]) == total
    host = bundler.OptimizeCameraPoses(pb, nsteps, maxe, huber)
    g = {k: v.cpu().numpy() for k, v in ba.items()}
    assert g["pos"].tobytes() == host["pos"].tobytes()
    assert g["r9"].tobytes() == host["r9"].tobytes()
    assert g["mean_sq"].tobytes() == host["mean_sq"].tobytes()
    assert g["outlier"][:total].tobytes() == host["outlier"].tobytes()
    assert (g["outlier"][total:] == FILL).all()
    # the bundle adjustment moved the OK problems' poses, and not far
    moved = [i for i, h in enumerate(ok) if h is not None and h.verdict == reloc.OK and len(h.points3) >= 6]
    assert moved and all(np.abs(g["pos"][i] - pb.pos[i]).max() < 0.5 for i in moved)
