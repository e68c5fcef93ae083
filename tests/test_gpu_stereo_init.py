"""The stereo-initialisation kernels (mageslam_amd/csrc/stereoinit.hip) against their plain C++ twin
(mage_stereo_init_triangulate_host, itself checked against fp64 in test_stereo_init_reference.py):
masks, counts, verdicts, the compacted records, the bundle adjustment's inputs and the status
byte-identical over the case table of tests/stereo_init_cases.py, with the matches given and with
the two-way matcher in the chain; and the batched entry with every case in one launch."""
import numpy as np
import pytest

from mageslam_amd import stereo
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, SP_DTYPE
from tests import stereo_init_cases as sc

pytestmark = pytest.mark.gpu

CASES = list(sc.cases())
FIELDS = ("mask0", "n_masked", "matches", "verdicts", "points", "ba_points", "ba_uv", "ba_cam", "ba_pt", "ba_info",
          "status")


def same(g, h, what):
    for f in FIELDS:
        a, b = getattr(g, f), getattr(h, f)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, f)
        else:
            assert a == b, (what, f)


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_host_twin(gpu, name):
    """The matches given to both sides."""
    c = sc.cases()[name]
    g = stereo.triangulate_points(c.settings, *c.args(), matches=c.matches, cap=c.cap, backend="gpu")
    same(g, sc.host_result(name), name)


@pytest.mark.parametrize("name", [n for n in CASES if sc.cases()[n].matcher])
def test_chain_with_the_matcher(gpu, name):
    """Mask, two-way match and triangulation in one call: the matcher finds the case's matches
    (queryIdx mapped back from the packed frame 0), the rest equals the twin fed with them."""
    c, h = sc.cases()[name], sc.host_result(name)
    g = stereo.triangulate_points(c.settings, *c.args(), desc0=c.desc0, desc1=c.desc1, cap=c.cap, backend="gpu")
    if h.status & stereo.STATUS_OVER_LIMIT:
        assert g.status == h.status and g.n_masked == 0 and len(g.matches) == 0 and len(g.points) == 0
        return
    assert g.matches.tobytes() == c.matches.tobytes()
    same(g, h, name)


class Batch:
    """Every case as one pair of a single launch, at pitches larger than the counts, all outputs
    prefilled with 0xA5; one more pair whose frame-0 count exceeds its pitch."""

    def __init__(self):
        import torch

        self.cs = [sc.cases()[n] for n in CASES if sc.cases()[n].matcher and sc.cases()[n].settings ==
                   stereo.StereoMapInitializationSettings()]
        P = self.P = len(self.cs) + 1
        self.pitch0 = max(len(c.kp0) for c in self.cs) + 37
        self.pitch1 = max(len(c.kp1) for c in self.cs) + 11
        self.match_cap = max(len(c.matches) for c in self.cs) + 5
        self.cap = 600  # below m2000's accepted count
        pose = np.zeros((P, 32), np.float32)
        crop = np.zeros((P, 4), np.int32)
        kp0, kp1 = np.zeros((P, self.pitch0), KP_DTYPE), np.zeros((P, self.pitch1), KP_DTYPE)
        d0, d1 = np.zeros((P, self.pitch0, 32), np.uint8), np.zeros((P, self.pitch1, 32), np.uint8)
        n = np.zeros((2, P), np.uint32)
        for i, c in enumerate(self.cs + [self.cs[0]]):
            pose[i] = np.concatenate([c.pos3.reshape(-1), c.r9.reshape(-1), c.intr4.reshape(-1)])
            crop[i] = c.crop
            kp0[i, : len(c.kp0)], kp1[i, : len(c.kp1)] = c.kp0, c.kp1
            d0[i, : len(c.kp0)], d1[i, : len(c.kp1)] = c.desc0, c.desc1
            n[:, i] = len(c.kp0), len(c.kp1)
        n[0, P - 1] = self.pitch0 + 1
        dev = torch.device("cuda")
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        self.pos3, self.r9, self.intr4 = up(pose[:, :6].copy()), up(pose[:, 6:24].copy()), up(pose[:, 24:].copy())
        self.crop, self.kp0, self.kp1, self.d0, self.d1, self.n = up(crop), up(kp0), up(kp1), up(d0), up(d1), up(n)
        self.sizes = dict(mask0=P * self.pitch0, n_masked=4 * P, matches=16 * P * self.match_cap, n_matches=4 * P,
                          verdict=P * self.match_cap, out=SP_DTYPE.itemsize * P * self.cap, n_out=4 * P,
                          ba_points=12 * P * self.cap, ba_uv=16 * P * self.cap, ba_cam=8 * P * self.cap,
                          ba_pt=8 * P * self.cap, ba_info=8 * P * self.cap, status=4 * P)
        self.scratch = torch.zeros(stereo.scratch_bytes(P, self.pitch0), dtype=torch.uint8, device=dev)

    def run(self):
        import torch

        o = {k: torch.full((v,), 0xA5, dtype=torch.uint8, device="cuda") for k, v in self.sizes.items()}
        stereo.triangulate_batch_device(
            self.cs[0].settings, self.P, self.pos3, self.r9, self.intr4, self.crop, self.kp0, self.d0, self.pitch0,
            self.n.data_ptr(), self.kp1, self.d1, self.pitch1, self.n.data_ptr() + 4 * self.P, o["mask0"], o["n_masked"],
            o["matches"], self.match_cap, o["n_matches"], o["verdict"], o["out"], self.cap, o["n_out"], o["ba_points"],
            o["ba_uv"], o["ba_cam"], o["ba_pt"], o["ba_info"], o["status"], self.scratch,
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def test_batch(gpu):
    b = Batch()
    o = b.run()
    again = b.run()
    for k in o:
        assert o[k].tobytes() == again[k].tobytes(), k
    P, cap, mc = b.P, b.cap, b.match_cap
    A5 = 0xA5
    n_masked, n_matches = o["n_masked"].view(np.uint32), o["n_matches"].view(np.uint32)
    n_out, status = o["n_out"].view(np.uint32), o["status"].view(np.uint32)
    mask0 = o["mask0"].reshape(P, b.pitch0)
    matches, verdict = o["matches"].view(DM_DTYPE).reshape(P, mc), o["verdict"].reshape(P, mc)
    out = o["out"].view(SP_DTYPE).reshape(P, cap)
    pts = o["ba_points"].view(np.float32).reshape(P, cap, 3)
    uv = o["ba_uv"].view(np.float32).reshape(P, 2 * cap, 2)
    cam, pt = o["ba_cam"].view(np.uint32).reshape(P, 2 * cap), o["ba_pt"].view(np.uint32).reshape(P, 2 * cap)
    info = o["ba_info"].view(np.float32).reshape(P, 2 * cap)
    untouched = lambda a: bool(np.all(a.view(np.uint8) == A5))  # noqa: E731
    over_cap_seen = 0
    for i, c in enumerate(b.cs):
        h = sc.host_result(c.name)
        what = c.name
        if h.status & stereo.STATUS_OVER_LIMIT:
            assert status[i] == stereo.STATUS_OVER_LIMIT and n_masked[i] == 0 and n_matches[i] == 0 and n_out[i] == 0
            assert untouched(mask0[i]) and untouched(verdict[i]) and untouched(out[i]) and untouched(uv[i]), what
            continue
        n0, nm = len(c.kp0), len(c.matches)
        assert n_masked[i] == h.n_masked and n_matches[i] == nm, what
        assert np.array_equal(mask0[i, :n0].astype(bool), h.mask0) and untouched(mask0[i, n0:]), what
        assert matches[i, :nm].tobytes() == c.matches.tobytes() and untouched(matches[i, nm:]), what
        assert np.array_equal(verdict[i, :nm], h.verdicts) and untouched(verdict[i, nm:]), what
        # this launch's cap is its own: the twin ran with the case's, so cut the twin's records or
        # take them from its verdicts
        accepted = int((h.verdicts == sc.ACCEPTED).sum())
        n = min(accepted, cap)
        assert n_out[i] == n, what
        expect_status = stereo.STATUS_OVER_CAP if accepted > cap else 0
        assert status[i] == expect_status, what
        over_cap_seen += accepted > cap
        full = h if len(h.points) >= n else stereo.triangulate_points(c.settings, *c.args(), matches=c.matches,
                                                                      cap=cap, backend="host")
        assert out[i, :n].tobytes() == full.points[:n].tobytes() and untouched(out[i, n:]), what
        assert pts[i, :n].tobytes() == full.points["position"][:n].tobytes() and untouched(pts[i, n:]), what
        q, t = full.points["query_idx"][:n], full.points["train_idx"][:n]
        xy = np.concatenate([np.stack([c.kp0["x"][q], c.kp0["y"][q]], 1), np.stack([c.kp1["x"][t], c.kp1["y"][t]], 1)])
        assert uv[i, : 2 * n].tobytes() == xy.astype(np.float32).tobytes() and untouched(uv[i, 2 * n:]), what
        assert np.array_equal(cam[i, : 2 * n], np.repeat([0, 1], n)) and untouched(cam[i, 2 * n:]), what
        assert np.array_equal(pt[i, : 2 * n], np.tile(np.arange(n), 2)) and untouched(pt[i, 2 * n:]), what
        assert np.all(info[i, : 2 * n] == full.ba_info[0] if n else True) and untouched(info[i, 2 * n:]), what
    assert over_cap_seen >= 1
    # the pair whose count exceeds its pitch: the status bit and nothing else
    i = P - 1
    assert status[i] == stereo.STATUS_OVER_LIMIT and n_masked[i] == 0 and n_matches[i] == 0 and n_out[i] == 0
    assert untouched(mask0[i]) and untouched(verdict[i]) and untouched(out[i]) and untouched(uv[i])
