"""The new-map-points kernel (mageslam_amd/csrc/newpoints.hip) against its plain C++ twin
(mage_new_map_points_host, itself checked against fp64 in test_new_points_reference.py): verdicts,
counts, indices and the order of the points identical and every float bit-identical, over the case
table of tests/new_points_cases.py; the batched device entry, alone and chained behind
mage_indexed_match_batch_device on one stream."""
import numpy as np
import pytest

from mageslam_amd import bow, mapping
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, NP_DTYPE
from tests import new_points_cases as nc

pytestmark = pytest.mark.gpu

CASES = list(nc.cases())


def host(name):
    p = nc.cases()[name]
    return mapping.new_map_points(p.settings, *p.args(), cap=p.cap, backend="host")


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_host_twin(gpu, name):
    p, h = nc.cases()[name], host(name)
    g = mapping.new_map_points(p.settings, *p.args(), cap=p.cap, backend="gpu")
    assert g.status == h.status
    assert len(g.points) == len(h.points)
    for k in range(len(p.matches)):
        assert np.array_equal(g.verdicts[k], h.verdicts[k]), (name, k)
    assert g.points.tobytes() == h.points.tobytes()


class Batch:
    """Device buffers of `problems` at fixed pitches (larger than the counts), all with one settings
    struct; run() launches mage_new_map_points_batch_device."""

    def __init__(self, problems, kc_slots, ki_pitch, kc_pitch, match_cap, cap):
        import torch

        n = len(problems)
        self.problems, self.kc_slots, self.ki_pitch, self.kc_pitch = problems, kc_slots, ki_pitch, kc_pitch
        self.match_cap, self.cap = match_cap, cap
        pairs = n * kc_slots
        ki_pose = np.zeros((n, 16), np.float32)
        kc_pose = np.zeros((pairs, 16), np.float32)
        kc_pose[:, 3], kc_pose[:, 7], kc_pose[:, 11], kc_pose[:, 14:] = 1, 1, 1, 1  # unused slots: identity, f = 1
        ki_kp = np.zeros((n, ki_pitch), KP_DTYPE)
        assoc = np.zeros((n, ki_pitch), np.uint8)
        kc_kp = np.zeros((pairs, kc_pitch), KP_DTYPE)
        m = np.zeros((pairs, match_cap), DM_DTYPE)
        m["query_idx"] = -7  # beyond the counts: never read
        n_ki, n_kc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        n_kckp, n_m = np.zeros(pairs, np.uint32), np.zeros(pairs, np.uint32)
        for i, p in enumerate(problems):
            ki_pose[i] = np.concatenate([p.ki_pos3, p.ki_r9, p.ki_intr4])
            n_ki[i], n_kc[i] = len(p.ki_kp), len(p.kc_kp)
            if len(p.ki_kp) <= ki_pitch:
                ki_kp[i, : len(p.ki_kp)] = p.ki_kp
                if p.ki_assoc is not None:
                    assoc[i, : len(p.ki_kp)] = p.ki_assoc
            for k in range(len(p.kc_kp)):
                pr = i * kc_slots + k
                kc_pose[pr] = np.concatenate([p.kc_pos3[k], p.kc_r9[k], p.kc_intr4[k]])
                kc_kp[pr, : len(p.kc_kp[k])] = p.kc_kp[k]
                m[pr, : len(p.matches[k])] = p.matches[k]
                n_kckp[pr], n_m[pr] = len(p.kc_kp[k]), len(p.matches[k])

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

        self.ki_pos3, self.ki_r9, self.ki_intr4 = dev(ki_pose[:, :3]), dev(ki_pose[:, 3:12]), dev(ki_pose[:, 12:])
        self.kc_pos3, self.kc_r9, self.kc_intr4 = dev(kc_pose[:, :3]), dev(kc_pose[:, 3:12]), dev(kc_pose[:, 12:])
        self.ki_kp, self.assoc, self.kc_kp, self.m = dev(ki_kp), dev(assoc), dev(kc_kp), dev(m)
        self.n_ki, self.n_kc, self.n_kckp, self.n_m = dev(n_ki), dev(n_kc), dev(n_kckp), dev(n_m)
        self.out = torch.zeros(n * cap * 48, dtype=torch.uint8, device="cuda")
        self.n_out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.verdict = torch.full((pairs * match_cap,), 0xFF, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(self, settings, stream=None, matches=None, n_matches=None):
        mapping.new_map_points_batch_device(
            settings, len(self.problems), self.kc_slots, self.ki_pos3, self.ki_r9, self.ki_intr4, self.ki_kp,
            self.ki_pitch, self.n_ki, self.assoc, self.n_kc, self.kc_pos3, self.kc_r9, self.kc_intr4, self.kc_kp,
            self.kc_pitch, self.n_kckp, self.m if matches is None else matches, self.match_cap,
            self.n_m if n_matches is None else n_matches, self.out, self.cap, self.n_out, self.verdict, self.status,
            stream)

    def results(self):
        """(status, per problem (points, per-slot verdicts))."""
        import torch

        torch.cuda.synchronize()
        out = self.out.cpu().numpy().view(NP_DTYPE).reshape(len(self.problems), self.cap)
        n_out = self.n_out.cpu().numpy()
        v = self.verdict.cpu().numpy().reshape(len(self.problems), self.kc_slots, self.match_cap)
        res = []
        for i, p in enumerate(self.problems):
            res.append((out[i, : n_out[i]], [v[i, k, : len(p.matches[k])] for k in range(len(p.matches))]))
        return int(self.status.item()), res, (self.out.cpu().numpy().tobytes(), self.verdict.cpu().numpy().tobytes(),
                                             n_out.tobytes())


@pytest.mark.parametrize("settings_of", ["parallax", "base"])
def test_batch_device_equals_per_problem(gpu, settings_of):
    """Five problems in one launch (the base scene, the parallax case, the grid-cap case, an empty
    problem and the 257-match case), pitches larger than the counts.  A launch has one settings
    struct: all five run under the parallax case's settings, then under the defaults, and each is
    compared with the C++ twin on the same problem under the same settings."""
    names = list(nc.BATCH_CASES)
    probs = [nc.cases()[n] for n in names]
    settings = nc.cases()[settings_of].settings
    b = Batch(probs, kc_slots=4, ki_pitch=400, kc_pitch=300, match_cap=320, cap=300)
    b.run(settings)
    status, res, _ = b.results()
    assert status == 0
    for i, (n, p) in enumerate(zip(names, probs)):
        h = mapping.new_map_points(settings, *p.args(), cap=300, backend="host")
        assert h.status == 0
        pts, verd = res[i]
        assert pts.tobytes() == h.points.tobytes(), n
        for k in range(len(verd)):
            assert np.array_equal(verd[k], h.verdicts[k]), (n, k)
    # beyond the counts nothing was written
    v = b.verdict.cpu().numpy().reshape(len(probs), 4, 320)
    for i, p in enumerate(probs):
        for k in range(4):
            nm = len(p.matches[k]) if k < len(p.matches) else 0
            assert (v[i, k, nm:] == 0xFF).all()


def test_batch_status_bits(gpu):
    """The 4097-keypoint problem sets bit 0 and reports no points, the over-cap problem sets bit 1
    and keeps its first `cap` points; the problem between them is untouched by either."""
    names = ["ki4097", "base", "over_cap"]
    probs = [nc.cases()[n] for n in names]
    for sel, want in (([0, 1], 1), ([1, 2], 2), ([0, 1, 2], 3), ([1], 0)):
        cap = 10 if 2 in sel else 300
        b = Batch([probs[i] for i in sel], kc_slots=3, ki_pitch=4100, kc_pitch=128, match_cap=128, cap=cap)
        b.run(probs[1].settings)
        status, res, _ = b.results()
        assert status == want, (sel, status)
        for (pts, verd), i in zip(res, sel):
            h = host(names[i])
            if names[i] == "ki4097":
                assert len(pts) == 0 and all((v == 0xFF).all() for v in verd)
                continue
            assert pts.tobytes() == h.points[:cap].tobytes()
            for k in range(len(verd)):
                assert np.array_equal(verd[k], h.verdicts[k])


def test_batch_twice_is_byte_identical(gpu):
    probs = [nc.cases()[n] for n in ("taken", "base", "grid_start", "counts")]
    raw = []
    for _ in range(2):
        b = Batch(probs, kc_slots=5, ki_pitch=512, kc_pitch=260, match_cap=260, cap=256)
        b.run(probs[1].settings)
        raw.append(b.results()[2])
    assert raw[0] == raw[1]


def test_end_to_end_from_descriptors(gpu):
    """Two-view descriptors with known correspondences through OnlineBowTree, find_leaves_device and
    mage_indexed_match_batch_device, then mage_new_map_points_batch_device on the same stream with
    no host copy in between; equal to host-buffer IndexedMatch plus the C++ twin."""
    import torch

    p = nc.cases()["open_grid"]
    rng = np.random.default_rng(31)
    n_ki, n_kc = len(p.ki_kp), len(p.kc_kp)
    ki_desc = rng.integers(0, 256, (n_ki, 32), dtype=np.uint8)
    kc_desc = []
    for k in range(n_kc):
        d = rng.integers(0, 256, (len(p.kc_kp[k]), 32), dtype=np.uint8)
        for m in p.matches[k]:
            d[m["query_idx"]] = ki_desc[m["train_idx"]]
            for bit in rng.choice(256, 3, replace=False):
                d[m["query_idx"], bit >> 3] ^= np.uint8(1 << (bit & 7))
        kc_desc.append(d)
    tree = bow.OnlineBowTree.CreateTree(np.concatenate([ki_desc] + kc_desc), levels=2, branching=4)
    maxd, mind = 30, 1
    # host side: IndexedMatch(Kc, Ki) per slot, then the twin
    hm = [bow.IndexedMatch(tree, kc_desc[k], ki_desc, maxHammingDist=maxd, minHammingDifference=mind)
          for k in range(n_kc)]
    assert sum(len(m) for m in hm) > 0.6 * p.n_matches
    h = mapping.new_map_points(p.settings, p.ki_pos3, p.ki_r9, p.ki_intr4, p.ki_kp, None, p.kc_pos3, p.kc_r9,
                               p.kc_intr4, p.kc_kp, hm, cap=300, backend="host")
    assert len(h.points) > 50

    # device side, one stream
    pitch, mcap = 384, 128
    b = Batch([p], kc_slots=n_kc, ki_pitch=pitch, kc_pitch=mcap, match_cap=mcap, cap=300)
    DA = torch.zeros((n_kc, mcap, 32), dtype=torch.uint8, device="cuda")
    DB = torch.zeros((n_kc, pitch, 32), dtype=torch.uint8, device="cuda")
    for k in range(n_kc):
        DA[k, : len(kc_desc[k])] = torch.from_numpy(kc_desc[k]).cuda()
        DB[k, :n_ki] = torch.from_numpy(ki_desc).cuda()
    LA = torch.zeros((n_kc, mcap), dtype=torch.int32, device="cuda")
    LB = torch.zeros((n_kc, pitch), dtype=torch.int32, device="cuda")
    na = torch.tensor([len(d) for d in kc_desc], dtype=torch.int32, device="cuda")
    nb = torch.full((n_kc,), n_ki, dtype=torch.int32, device="cuda")
    dm = torch.zeros(n_kc * mcap * 16, dtype=torch.uint8, device="cuda")
    ndm = torch.zeros(n_kc, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for k in range(n_kc):
            tree.find_leaves_device(DA[k], len(kc_desc[k]), LA[k], s.cuda_stream)
            tree.find_leaves_device(DB[k], n_ki, LB[k], s.cuda_stream)
        bow.indexed_match_batch_device(DA, LA, None, mcap, na, DB, LB, None, pitch, nb, n_kc, maxd, mind, dm, mcap,
                                       ndm, st, s.cuda_stream)
        b.run(p.settings, s.cuda_stream, matches=dm, n_matches=ndm)
    s.synchronize()
    assert int(st.item()) == 0
    got_n = ndm.cpu().numpy()
    assert got_n.tolist() == [len(m) for m in hm]
    gm = dm.cpu().numpy().view(DM_DTYPE).reshape(n_kc, mcap)
    for k in range(n_kc):
        assert gm[k, : got_n[k]].tobytes() == hm[k].tobytes()
    out = b.out.cpu().numpy().view(NP_DTYPE)[: int(b.n_out.cpu().numpy()[0])]
    assert int(b.status.item()) == 0
    assert out.tobytes() == h.points.tobytes()
    v = b.verdict.cpu().numpy().reshape(n_kc, mcap)
    for k in range(n_kc):
        assert np.array_equal(v[k, : got_n[k]], h.verdicts[k])
