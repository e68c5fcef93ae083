"""The loop-closure kernels (csrc/loopclose.hip) against the plain C++ twin, byte for byte: every case
of tests/loop_closure_cases.py through the synchronous entry, the batched device chain over problems
of differing counts, the status bits per problem, and the refresh alone."""
import numpy as np
import pytest

from mageslam_amd import _lib, loopclosure as lcm
from tests import loop_closure_cases as lc
from tests.test_loop_closure_reference import refresh_inputs

pytestmark = pytest.mark.gpu
CASES = list(lc.cases())
FIELDS = ("state", "obs", "sample_index", "closure", "closure_verdict", "connect", "connect_verdict", "ki_mask", "kf_modified",
          "counts")


@pytest.fixture(scope="module")
def host():
    return {n: lcm.cheap_loop_closure_and_connect(c.settings, c.problem, backend="host", prefill=0xA5)
            for n, c in lc.cases().items()}


@pytest.mark.parametrize("name", CASES)
def test_kernels_equal_twin(gpu, host, name):
    """Every output byte, the states and appended observations included; buffers start as 0xA5, so
    nothing past the counts is written by either side."""
    c, h = lc.cases()[name], host[name]
    g = lcm.cheap_loop_closure_and_connect(c.settings, c.problem, backend="hip", prefill=0xA5)
    assert (g.status, g.refused) == (h.status, h.refused)
    for f in FIELDS:
        assert np.ascontiguousarray(getattr(g, f)).tobytes() == np.ascontiguousarray(getattr(h, f)).tobytes(), f
    for a, b in zip(g.kf_masks, h.kf_masks):
        assert np.array_equal(a, b)


BATCH = ("base", "empty_map", "two_rounds", "below_min_keyframes", "obs_full", "many_kp", "levels2_kf4")


def batch_cases():
    """Problems of differing counts under one settings block and one observation pitch (12).  obs_full
    is rebuilt for that pitch: point 5 has 9 observations, and 9 + 1 + 3 keyframes do not fit.  The
    last problem has four keyframes."""
    cs = lc.cases()
    out = [cs[n] for n in BATCH[:-1]]
    p = out[4].problem
    state, obs = p.state.copy(), np.zeros((len(p.state), 12), _lib.MP_OBS_DTYPE)
    obs[:, :p.obs.shape[1]] = p.obs
    obs[5, :9], state["n_obs"][5] = obs[5, 0], 9
    out[4] = lc.Case("obs_full", out[4].settings, lc.dataclasses.replace(p, state=state, obs=obs))
    sc = lc.Scene(31, 130)
    out.append(sc.case("levels2_kf4", sc.ki(), sc.kfs(4)))
    return out


def test_batch_equals_per_problem_calls(gpu):
    import torch

    cs = batch_cases()
    s = cs[0].settings
    assert all(c.settings == s and c.problem.obs.shape[1] == 12 for c in cs)
    packed = lcm.pack_problems(s, [c.problem for c in cs], fill=0xA5)
    lcm.cheap_loop_closure_batch_device(s, packed)
    torch.cuda.synchronize()
    out = lcm.unpack_problems(packed)
    assert packed["kf_slots"] == 4 and packed["kf_pitch"] < 4097 and packed["obs_pitch"] == 12
    for i, c in enumerate(cs):
        p = c.problem
        h = lcm.cheap_loop_closure_and_connect(s, p, backend="host", prefill=0xA5)
        n, nkf, L = len(p.state), len(p.kfs), int(h.counts[0])
        assert out["d_counts"][i].tolist() == h.counts.tolist(), c.name
        assert int(out["d_status"][i]) == h.status, c.name
        assert out["d_sample_index"][i, :L].tobytes() == h.sample_index[:L].tobytes()
        assert out["d_closure"][i, :L].tobytes() == h.closure[:L].tobytes()
        assert out["d_closure_verdict"][i, :L].tobytes() == h.closure_verdict[:L].tobytes()
        assert np.ascontiguousarray(out["d_connect"][i, :L, :nkf]).tobytes() == np.ascontiguousarray(h.connect[:L]).tobytes()
        assert np.array_equal(out["d_connect_verdict"][i, :L, :nkf], h.connect_verdict[:L])
        assert out["d_state"][i, :n].tobytes() == h.state.tobytes(), c.name
        assert np.ascontiguousarray(out["d_obs"][i, :n]).tobytes() == h.obs.tobytes(), c.name
        if L:
            assert np.array_equal(out["d_kf_modified"][i, :nkf], h.kf_modified)
            if len(p.ki.kp) <= 4096:
                assert np.array_equal(out["d_ki_mask"][i, :len(p.ki.kp)], h.ki_mask)
        for k, kf in enumerate(p.kfs):  # a keyframe over the limit sent no mask: nothing to compare
            if len(kf.kp) <= 4096:
                assert np.array_equal(out["d_kf_mask"][i, k, :len(kf.kp)], h.kf_masks[k]), (c.name, k)
        # nothing past the counts
        assert (out["d_sample_index"][i, L:].view(np.uint8) == 0xA5).all() and (out["d_closure"][i, L:].view(np.uint8) == 0xA5).all()
        assert (out["d_closure_verdict"][i, L:] == 0xA5).all() and (out["d_connect"][i, L:].view(np.uint8) == 0xA5).all()
        assert (out["d_connect_verdict"][i, L:] == 0xA5).all() and (out["d_connect_verdict"][i, :, nkf:] == 0xA5).all()
        assert (out["d_kf_modified"][i, nkf if L else 0:] == 0xA5).all()
        assert (out["d_state"][i, n:].view(np.uint8) == 0xA5).all() and (out["d_obs"][i, n:].view(np.uint8) == 0xA5).all()
    status = out["d_status"].tolist()
    assert status[BATCH.index("obs_full")] == lcm.STATUS_OBS_FULL and status[BATCH.index("many_kp")] == lcm.STATUS_OVER_LIMIT
    assert [v for i, v in enumerate(status) if BATCH[i] not in ("obs_full", "many_kp")] == [0] * 5


def test_batch_limits_per_problem(gpu):
    """A problem with more keyframes than slots, and one whose map exceeds the pitch, are refused with
    bit 0; their neighbours are unaffected."""
    import torch

    cs = batch_cases()
    s = cs[0].settings
    problems = [cs[0].problem, cs[6].problem, cs[2].problem]
    packed = lcm.pack_problems(s, problems, kf_slots=3, obs_pitch=12, fill=0xA5)
    lcm.cheap_loop_closure_batch_device(s, packed)
    torch.cuda.synchronize()
    out = lcm.unpack_problems(packed)
    assert out["d_status"].tolist() == [0, lcm.STATUS_OVER_LIMIT, 0] and out["d_counts"][1].tolist() == [0, 0, 0]
    assert (out["d_closure"][1].view(np.uint8) == 0xA5).all()
    for i, j in ((0, 0), (2, 2)):
        h = lcm.cheap_loop_closure_and_connect(s, cs[j].problem, backend="host")
        assert out["d_counts"][i].tolist() == h.counts.tolist()
        assert out["d_state"][i, :len(h.state)].tobytes() == h.state.tobytes()
    packed = lcm.pack_problems(s, problems, map_pitch=120, obs_pitch=12, fill=0xA5)
    lcm.cheap_loop_closure_batch_device(s, packed)
    torch.cuda.synchronize()
    out = lcm.unpack_problems(packed)
    assert out["d_status"].tolist() == [lcm.STATUS_OVER_LIMIT, lcm.STATUS_OVER_LIMIT, 0]
    assert out["d_counts"].tolist()[:2] == [[0, 0, 0], [0, 0, 0]] and out["d_counts"][2, 0] == 100


def test_refresh_kernel_equals_twin(gpu):
    """0 / 1 / 2 / 33 / 70 observations (70: a second round of 64 lanes), ties in the summed distance
    (the first wins) and a zero-length view vector."""
    s, pos, obs, n = refresh_inputs()
    h = lcm.refresh_map_points(s, pos, obs, n, backend="host", prefill=0xA5)
    g = lcm.refresh_map_points(s, pos, obs, n, backend="hip", prefill=0xA5)
    assert g.tobytes() == h.tobytes()
    assert h["rep"][5] == 0 and h["rep"][0] == -1


def test_refresh_batch_device_status(gpu):
    import torch

    s, pos, obs, n = refresh_inputs()
    h = lcm.refresh_map_points(s, pos, obs, n, backend="host")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    over = n.copy()
    over[2] = 71  # over the pitch: bit 0, that state untouched
    state, status = dev(np.full(len(n) * 40, 0xA5, np.uint8)), dev(np.zeros(1, np.uint32))
    lcm.refresh_map_points_batch_device(s, len(n), dev(pos), dev(obs), 70, dev(over), state, status)
    torch.cuda.synchronize()
    got = state.cpu().numpy().view(_lib.MP_STATE_DTYPE)
    assert int(status.cpu().numpy().view(np.uint32)[0]) == 1
    keep = np.arange(len(n)) != 2
    assert got[keep].tobytes() == h[keep].tobytes() and (got[2:3].view(np.uint8) == 0xA5).all()
