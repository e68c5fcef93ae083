"""The monocular map initialisation kernels (mageslam_amd/csrc/monoinit.hip) against their plain C++
twin (mage_mono_init_two_view_host, itself checked against independent formulations in
test_mono_init_reference.py): the result record (verdict, poses, scores, winner, status), the
records, the bundle adjustment's inputs and the whole trace byte-identical over the case table of
tests/mono_init_cases.py with the matches given; the chain with the two-way matcher in front; and
the batched entry with every case in one launch."""
import numpy as np
import pytest

from mageslam_amd import matcher, mono
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, MI_RESULT_DTYPE, SP_DTYPE
from tests import mono_init_cases as mc

pytestmark = pytest.mark.gpu

ALL = list(mc.cases()) + [mc.over_limit_case()]
FIELDS = ("verdict", "status", "matches", "points", "ba_points", "ba_uv", "ba_cam", "ba_pt", "ba_info")
_HOST = {}


def host(c, matches=None):
    key = (c.name, matches is None)
    if key not in _HOST:
        _HOST[key] = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1,
                                                 matches=c.matches if matches is None else matches, backend="host",
                                                 want_trace=True)
    return _HOST[key]


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
            assert g.trace[f].tobytes() == h.trace[f].tobytes(), (what, "trace", f)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_kernel_equals_host_twin(gpu, c):
    """The matches given to both sides."""
    g = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=c.matches, backend="gpu",
                                    want_trace=True)
    h = host(c)
    same(g, h, c.name)
    assert g.status == c.expect_status
    if c.expect is not None and not c.expect_status:
        assert g.verdict == c.expect, mono.VERDICT_NAMES[g.verdict]


def test_chain_with_the_matcher(gpu):
    """Octave-0 masks, two-way match and the two-view stage in one call: the matcher's result equals
    mage_hamming_match with the octave-0 masks, the rest equals the twin fed with those matches."""
    c = mc.matcher_case()
    m0, m1 = mc.octave0_masks(c)
    expect = matcher.Match(c.desc0, c.desc1, m0, m1, c.settings.five_point_max_hamming_distance,
                           c.settings.five_point_min_hamming_difference)
    assert len(expect) == int(m0.sum()) == 128  # every octave-0 keypoint finds its partner
    g = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, desc0=c.desc0, desc1=c.desc1, backend="gpu",
                                    want_trace=True)
    assert g.matches.tobytes() == expect.tobytes()
    same(g, host(c, expect), c.name)
    assert g.verdict == mono.OK and len(g.points) == 128


class Batch:
    """Every case that runs on the default settings as one pair of a single launch, at pitches larger
    than the counts, all outputs prefilled with 0xA5; plus one pair over 4096 keypoints, and one
    whose frame-0 count exceeds its pitch."""

    def __init__(self):
        import torch

        default = mono.MonoMapInitializationSettings()
        self.cs = [c for c in mc.cases() if c.settings == default] + [mc.over_limit_case()]
        self.settings = default
        P = self.P = len(self.cs) + 1
        self.pitch0 = max(len(c.kp0) for c in self.cs) + 37
        self.pitch1 = max(len(c.kp1) for c in self.cs) + 11
        self.match_cap = max(len(c.matches) for c in self.cs) + 5
        self.cap = 600  # below clean2000's accepted count
        self.iters = default.ransac_iterations_for_models
        intr = np.tile(mc.INTR, (P, 1))
        kp0, kp1 = np.zeros((P, self.pitch0), KP_DTYPE), np.zeros((P, self.pitch1), KP_DTYPE)
        mm = np.zeros((P, self.match_cap), DM_DTYPE)
        n = np.zeros((3, P), np.uint32)
        for i, c in enumerate(self.cs + [self.cs[0]]):
            kp0[i, : len(c.kp0)], kp1[i, : len(c.kp1)] = c.kp0, c.kp1
            mm[i, : len(c.matches)] = c.matches
            n[:, i] = len(c.kp0), len(c.kp1), len(c.matches)
        n[0, P - 1] = self.pitch0 + 1
        self.matches_in = mm
        dev = torch.device("cuda")
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        self.intr, self.kp0, self.kp1, self.mm, self.n = up(intr), up(kp0), up(kp1), up(mm), up(n)
        self.tbytes = mono.trace_bytes(self.iters)
        self.sizes = dict(result=MI_RESULT_DTYPE.itemsize * P, out=SP_DTYPE.itemsize * P * self.cap,
                          ba_points=12 * P * self.cap, ba_uv=16 * P * self.cap, ba_cam=8 * P * self.cap,
                          ba_pt=8 * P * self.cap, ba_info=8 * P * self.cap, trace=self.tbytes * P)

    def run(self):
        import torch

        o = {k: torch.full((v,), 0xA5, dtype=torch.uint8, device="cuda") for k, v in self.sizes.items()}
        P = self.P
        mono.two_view_batch_device(
            self.settings, P, self.intr, self.kp0, None, self.pitch0, self.n.data_ptr(), self.kp1, None, self.pitch1,
            self.n.data_ptr() + 4 * P, self.mm, self.match_cap, self.n.data_ptr() + 8 * P, o["result"], o["out"],
            self.cap, o["ba_points"], o["ba_uv"], o["ba_cam"], o["ba_pt"], o["ba_info"], o["trace"], None,
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        o["matches"] = self.mm
        return {k: v.cpu().numpy() for k, v in o.items()}


def test_batch(gpu):
    b = Batch()
    o = b.run()
    again = b.run()
    for k in o:
        assert o[k].tobytes() == again[k].tobytes(), k
    P, cap = b.P, b.cap
    A5 = 0xA5
    assert o["matches"].tobytes() == b.matches_in.tobytes()  # given matches are inputs only
    result = o["result"].view(MI_RESULT_DTYPE)
    out = o["out"].view(SP_DTYPE).reshape(P, cap)
    pts = o["ba_points"].view(np.float32).reshape(P, cap, 3)
    uv = o["ba_uv"].view(np.float32).reshape(P, 2 * cap, 2)
    cam, pt = o["ba_cam"].view(np.uint32).reshape(P, 2 * cap), o["ba_pt"].view(np.uint32).reshape(P, 2 * cap)
    info = o["ba_info"].view(np.float32).reshape(P, 2 * cap)
    trace = o["trace"].reshape(P, b.tbytes)
    untouched = lambda a: bool(np.all(a.view(np.uint8) == A5))  # noqa: E731
    over_cap_seen = stopped_seen = 0
    for i, c in enumerate(b.cs):
        what = c.name
        # this launch's cap is its own: the twin runs with it
        h = mono.initialize_with_frames(c.settings, mc.INTR, c.kp0, c.kp1, matches=c.matches, cap=cap, backend="host",
                                        want_trace=True)
        assert result[i].tobytes() == h.result.tobytes(), (what, result[i], h.result)
        n = len(h.points)
        over_cap_seen += bool(h.status & mono.STATUS_OVER_CAP)
        assert out[i, :n].tobytes() == h.points.tobytes() and untouched(out[i, n:]), what
        assert pts[i, :n].tobytes() == h.ba_points.tobytes() and untouched(pts[i, n:]), what
        assert uv[i, : 2 * n].tobytes() == h.ba_uv.tobytes() and untouched(uv[i, 2 * n:]), what
        assert cam[i, : 2 * n].tobytes() == h.ba_cam.tobytes() and untouched(cam[i, 2 * n:]), what
        assert pt[i, : 2 * n].tobytes() == h.ba_pt.tobytes() and untouched(pt[i, 2 * n:]), what
        assert info[i, : 2 * n].tobytes() == h.ba_info.tobytes() and untouched(info[i, 2 * n:]), what
        if h.trace is None:  # over a limit or too few matches: the trace is left alone
            stopped_seen += 1
            assert untouched(trace[i]), what
        else:
            assert trace[i].tobytes() == h.trace.tobytes(), what
    assert over_cap_seen >= 1 and stopped_seen >= 2
    # the pair over 4096 keypoints and the pair whose count exceeds its pitch: the status bit in the
    # result record and nothing else, the neighbours as the twin has them (checked above)
    for i in (P - 2, P - 1):
        assert result[i]["status"] == mono.STATUS_OVER_LIMIT and result[i]["n_points"] == 0
        assert untouched(out[i]) and untouched(pts[i]) and untouched(uv[i]) and untouched(trace[i])
