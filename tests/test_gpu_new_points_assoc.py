"""The new-point association kernel (mageslam_amd/csrc/newpoints_assoc.hip) against its plain C++ twin
(mage_new_points_associate_host, itself checked against fp64 and the oracle's sequential loop in
test_new_points_assoc_reference.py): records, verdicts and masks identical byte for byte over the case
table of tests/new_points_assoc_cases.py; the batched device entry, alone and at the end of
find_leaves -> indexed_match_batch -> new_map_points_batch -> new_points_associate_batch on one
stream."""
import numpy as np
import pytest

from mageslam_amd import bow, mapping
from mageslam_amd._lib import KP_DTYPE, NA_DTYPE, NP_DTYPE
from tests import new_points_assoc_cases as ac
from tests import new_points_cases as nc

pytestmark = pytest.mark.gpu

CASES = list(ac.cases())


@pytest.fixture(scope="module")
def host():
    return {n: mapping.new_points_associate(*c.args(), backend="host") for n, c in ac.cases().items()}


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_host_twin(gpu, host, name):
    c = ac.cases()[name]
    hrec, hv, hmasks, hstatus = host[name]
    rec, v, masks, status = mapping.new_points_associate(*c.args(), backend="gpu")
    assert status == hstatus
    assert np.array_equal(v, hv)
    assert rec.tobytes() == hrec.tobytes()
    for k in range(len(c.kfs)):
        assert np.array_equal(masks[k], hmasks[k]), (name, k)
    if name in ("blob8", "blob9"):  # the kept list of 8 exactly full, and its first overflow
        assert (ac.start_candidates(c, hrec, hv, 0) == int(name[4:])).any()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


class Batch:
    """Device buffers of `cases` at fixed pitches (larger than the counts); run() launches
    mage_new_points_associate_batch_device.  Unused bytes hold 0xFF sentinels."""

    def __init__(self, cases, kf_slots, ki_pitch, kf_pitch, cap, n_points=None, n_kf=None):
        import torch

        n = len(cases)
        self.cases, self.kf_slots, self.ki_pitch, self.kf_pitch, self.cap = cases, kf_slots, ki_pitch, kf_pitch, cap
        pairs = n * kf_slots
        pts = np.zeros((n, cap), NP_DTYPE)
        pts["ki_index"] = 0xFFFFFFFF  # beyond the counts: never read
        ki_desc = np.zeros((n, ki_pitch, 32), np.uint8)
        pose = np.zeros((pairs, 16), np.float32)
        pose[:, 3], pose[:, 7], pose[:, 11], pose[:, 14:] = 1, 1, 1, 1  # unused pairs: identity, f = 1
        kp = np.zeros((pairs, kf_pitch), KP_DTYPE)
        desc = np.zeros((pairs, kf_pitch, 32), np.uint8)
        mask = np.full((pairs, kf_pitch), 0xFF, np.uint8)
        npts, nki, nkf = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        nkp, slot = np.zeros(pairs, np.uint32), np.full(pairs, -1, np.int32)
        for i, c in enumerate(cases):
            m = min(len(c.points), cap)
            pts[i, :m] = c.points[:m]
            npts[i] = len(c.points) if n_points is None else n_points[i]
            nki[i], nkf[i] = len(c.ki_desc), len(c.kfs)
            ki_desc[i, : len(c.ki_desc)] = c.ki_desc
            for k, kf in enumerate(c.kfs[:kf_slots]):
                pr = i * kf_slots + k
                pose[pr] = np.concatenate([kf.pos3, kf.r9, kf.intr4])
                nkp[pr], slot[pr] = len(kf.kp), kf.slot
                if len(kf.kp) <= kf_pitch:
                    kp[pr, : len(kf.kp)] = kf.kp
                    desc[pr, : len(kf.kp)] = kf.desc
                    mask[pr, : len(kf.kp)] = kf.mask
        if n_kf is not None:
            nkf[:] = n_kf
        self.mask0 = mask.copy()
        self.pts, self.npts, self.ki_desc, self.nki, self.nkf = dev(pts), dev(npts), dev(ki_desc), dev(nki), dev(nkf)
        self.pos3, self.r9, self.intr4 = dev(pose[:, :3]), dev(pose[:, 3:12]), dev(pose[:, 12:])
        self.kp, self.desc, self.mask, self.nkp, self.slot = dev(kp), dev(desc), dev(mask), dev(nkp), dev(slot)
        self.assoc = torch.full((n * cap * kf_slots * 16,), 0xFF, dtype=torch.uint8, device="cuda")
        self.verdict = torch.full((n * cap * kf_slots,), 0xFF, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(self, settings, assoc, stream=None, points=None, n_points=None):
        mapping.new_points_associate_batch_device(
            settings, assoc, len(self.cases), self.kf_slots, self.pts if points is None else points, self.cap,
            self.npts if n_points is None else n_points, self.ki_desc, self.ki_pitch, self.nki, self.nkf, self.pos3,
            self.r9, self.intr4, self.kp, self.desc, self.mask, self.kf_pitch, self.nkp, self.slot, self.assoc,
            self.verdict, self.status, stream)

    def results(self):
        import torch

        torch.cuda.synchronize()
        n = len(self.cases)
        rec = self.assoc.cpu().numpy().view(NA_DTYPE).reshape(n, self.cap, self.kf_slots)
        v = self.verdict.cpu().numpy().reshape(n, self.cap, self.kf_slots)
        m = self.mask.cpu().numpy().reshape(n, self.kf_slots, self.kf_pitch)
        return int(self.status.item()), rec, v, m


def untouched(rec):
    """The records still hold the 0xFF sentinel bytes."""
    return bool((np.ascontiguousarray(rec).view(np.uint8) == 0xFF).all())


def blank(rec):
    """The records are {0, 0, 0, -1}."""
    one = np.zeros(1, NA_DTYPE)
    one["keypoint"] = -1
    return np.ascontiguousarray(rec).tobytes() == one.tobytes() * rec.size


def check_batch(b, rec, v, m, settings, assoc, cap, skip=()):
    """Every problem of the batch (but those in `skip`) against the twin on the same problem under the
    same settings, and nothing written beyond the counts."""
    for i, c in enumerate(b.cases):
        if i in skip:
            continue
        npts = min(len(c.points), cap)
        nkf = len(c.kfs)
        if nkf and npts:
            a = list(c.args())
            a[0], a[1], a[2] = settings, assoc, c.points[:npts]
            hrec, hv, hmasks, _ = mapping.new_points_associate(*a, backend="host")
            assert rec[i, :npts, :nkf].tobytes() == hrec.tobytes(), c.name
            assert np.array_equal(v[i, :npts, :nkf], hv), c.name
            for k in range(nkf):
                assert np.array_equal(m[i, k, : len(c.kfs[k].kp)].astype(bool), hmasks[k]), (c.name, k)
        assert (v[i, npts:] == 0xFF).all() and (v[i, :, nkf:] == 0xFF).all(), c.name
        assert untouched(rec[i, npts:]) and untouched(rec[i, :, nkf:]), c.name
        for k in range(b.kf_slots):
            n = len(c.kfs[k].kp) if k < nkf else 0
            assert np.array_equal(m[i, k, n:], b.mask0[i * b.kf_slots + k, n:]), (c.name, k)
            if k >= nkf:
                assert np.array_equal(m[i, k], b.mask0[i * b.kf_slots + k]), (c.name, k)


def test_batch_device_equals_per_problem(gpu):
    """Five problems in one launch (the base scene, the contended one, an empty problem, the 257-point
    one capped at n_out == cap = 200 and one with d_n_kf = 0), pitches larger than the counts."""
    cs = [ac.cases()[n] for n in ac.BATCH_CASES]
    settings, assoc = cs[0].settings, cs[1].assoc
    raw = []
    for _ in range(2):
        b = Batch(cs, kf_slots=9, ki_pitch=300, kf_pitch=320, cap=200)
        b.run(settings, assoc)
        status, rec, v, m = b.results()
        assert status == 0
        raw.append((rec.tobytes(), v.tobytes(), m.tobytes()))
    check_batch(b, rec, v, m, settings, assoc, 200)
    assert raw[0] == raw[1]  # two identical launches, identical bytes
    assert (v[3, :200, 0] != 0xFF).all()  # n_out == cap: every record of the capped problem is written


def test_batch_status_bits(gpu):
    """Bit 0 per the header: a keyframe over 4096 keypoints, a keypoint count over kf_pitch, and
    d_n_kf over kf_slots; the flagged pairs keep their verdict bytes and masks and get {0, 0, 0, -1}
    records, the other problems and keyframes are unaffected."""
    base, big = ac.cases()["base"], ac.cases()["kp4097"]
    s, a = base.settings, base.assoc
    # a keypoint count over the pitch (kp4097's middle keyframe; 4097 is over both limits)
    b = Batch([base, big], kf_slots=8, ki_pitch=128, kf_pitch=256, cap=80)
    b.run(s, a)
    status, rec, v, m = b.results()
    assert status == 1
    assert (v[1, :40, 1] == 0xFF).all() and blank(rec[1, :40, 1]) and untouched(rec[1, 40:])
    assert np.array_equal(m[1, 1], b.mask0[8 + 1])
    hrec, hv, hmasks, hst = mapping.new_points_associate(*big.args(), backend="host")
    assert hst == 1 and rec[1, :40, :3].tobytes() == hrec.tobytes() and np.array_equal(v[1, :40, :3], hv)
    check_batch(b, rec, v, m, s, a, 80, skip=(1,))
    # more keyframes than slots: every pair of that problem is over the limit
    b = Batch([base, ac.cases()["contend"]], kf_slots=8, ki_pitch=128, kf_pitch=256, cap=80, n_kf=[9, 5])
    b.run(s, a)
    status, rec, v, m = b.results()
    assert status == 1
    assert (v[0] == 0xFF).all() and blank(rec[0, :72]) and untouched(rec[0, 72:])
    assert np.array_equal(m[0], b.mask0[:8])
    hrec, hv, _, _ = mapping.new_points_associate(s, a, *ac.cases()["contend"].args()[2:], backend="host")
    assert rec[1, :70, :5].tobytes() == hrec.tobytes() and np.array_equal(v[1, :70, :5], hv)


def test_end_to_end_from_descriptors(gpu):
    """Descriptors with known correspondences through find_leaves_device, indexed_match_batch_device,
    new_map_points_batch_device and new_points_associate_batch_device on one stream with no host copy
    in between; equal to host-buffer IndexedMatch + mage_new_map_points_host +
    mage_new_points_associate_host.  The scene is the `taken` case: every world point is seen by Ki and
    by two or three keyframes, with descriptors 3 bits from Ki's."""
    import torch

    from tests.test_gpu_new_points import Batch as PointsBatch

    p = nc.cases()["taken"]
    rng = np.random.default_rng(33)
    n_ki, n_kc = len(p.ki_kp), len(p.kc_kp)
    ki_desc = rng.integers(0, 256, (n_ki, 32), dtype=np.uint8)
    kc_desc = []
    for k in range(n_kc):
        d = rng.integers(0, 256, (len(p.kc_kp[k]), 32), dtype=np.uint8)
        for m in p.matches[k]:
            d[m["query_idx"]] = ac._flip(rng, ki_desc[m["train_idx"]], 3)
        kc_desc.append(d)
    tree = bow.OnlineBowTree.CreateTree(np.concatenate([ki_desc] + kc_desc), levels=2, branching=4)
    maxd, mind = 30, 1
    settings = mapping.NewMapPointsCreationSettings(**{**p.settings.__dict__, "max_grid_count": 30})
    assoc = mapping.NewPointsAssociationSettings(image_border=20.0)
    kc_mask = [rng.uniform(size=len(k)) < 0.9 for k in p.kc_kp]  # unassociated as IndexedMatch sees them
    # host side
    hm = [bow.IndexedMatch(tree, kc_desc[k], ki_desc, kc_mask[k], None, maxHammingDist=maxd, minHammingDifference=mind)
          for k in range(n_kc)]
    h = mapping.new_map_points(settings, p.ki_pos3, p.ki_r9, p.ki_intr4, p.ki_kp, None, p.kc_pos3, p.kc_r9, p.kc_intr4,
                               p.kc_kp, hm, cap=128, backend="host")
    assert h.status == 0 and len(h.points) > 30
    hrec, hv, hmasks, hst = mapping.new_points_associate(settings, assoc, h.points, ki_desc, p.kc_pos3, p.kc_r9,
                                                         p.kc_intr4, p.kc_kp, kc_desc, list(range(n_kc)), kc_mask,
                                                         backend="host")
    gained = int((hv == ac.ASSOCIATED).any(axis=1).sum())
    assert gained >= len(h.points) // 2, (gained, len(h.points))  # a sizeable share gains a third keyframe

    # device side, one stream
    pitch, mcap, cap = 160, 96, 128
    b = PointsBatch([p], kc_slots=n_kc, ki_pitch=pitch, kc_pitch=mcap, match_cap=mcap, cap=cap)
    DA = torch.zeros((n_kc, mcap, 32), dtype=torch.uint8, device="cuda")
    DB = torch.zeros((n_kc, pitch, 32), dtype=torch.uint8, device="cuda")
    MA = torch.zeros((n_kc, mcap), dtype=torch.uint8, device="cuda")
    for k in range(n_kc):
        DA[k, : len(kc_desc[k])] = torch.from_numpy(kc_desc[k]).cuda()
        DB[k, :n_ki] = torch.from_numpy(ki_desc).cuda()
        MA[k, : len(kc_desc[k])] = torch.from_numpy(kc_mask[k].astype(np.uint8)).cuda()
    LA = torch.zeros((n_kc, mcap), dtype=torch.int32, device="cuda")
    LB = torch.zeros((n_kc, pitch), dtype=torch.int32, device="cuda")
    na = torch.tensor([len(d) for d in kc_desc], dtype=torch.int32, device="cuda")
    nb = torch.full((n_kc,), n_ki, dtype=torch.int32, device="cuda")
    dm = torch.zeros(n_kc * mcap * 16, dtype=torch.uint8, device="cuda")
    ndm = torch.zeros(n_kc, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_assoc = torch.full((cap * n_kc * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_verdict = torch.full((cap * n_kc,), 0xFF, dtype=torch.uint8, device="cuda")
    d_slot = torch.arange(n_kc, dtype=torch.int32, device="cuda")
    d_ast = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for k in range(n_kc):
            tree.find_leaves_device(DA[k], len(kc_desc[k]), LA[k], s.cuda_stream)
            tree.find_leaves_device(DB[k], n_ki, LB[k], s.cuda_stream)
        bow.indexed_match_batch_device(DA, LA, MA, mcap, na, DB, LB, None, pitch, nb, n_kc, maxd, mind, dm, mcap, ndm,
                                       st, s.cuda_stream)
        b.run(settings, s.cuda_stream, matches=dm, n_matches=ndm)
        # the Kc arrays of the first half are the keyframe arrays of the second; MA is in/out
        mapping.new_points_associate_batch_device(
            settings, assoc, 1, n_kc, b.out, cap, b.n_out, DB[0], pitch, b.n_ki, b.n_kc, b.kc_pos3, b.kc_r9, b.kc_intr4,
            b.kc_kp, DA, MA, mcap, b.n_kckp, d_slot, d_assoc, d_verdict, d_ast, s.cuda_stream)
    s.synchronize()
    assert int(st.item()) == 0 and int(b.status.item()) == 0 and int(d_ast.item()) == hst == 0
    n_out = int(b.n_out.cpu().numpy()[0])
    assert n_out == len(h.points)
    assert b.out.cpu().numpy().view(NP_DTYPE)[:n_out].tobytes() == h.points.tobytes()
    rec = d_assoc.cpu().numpy().view(NA_DTYPE).reshape(cap, n_kc)
    v = d_verdict.cpu().numpy().reshape(cap, n_kc)
    assert rec[:n_out].tobytes() == hrec.tobytes() and np.array_equal(v[:n_out], hv)
    assert (v[n_out:] == 0xFF).all()
    m = MA.cpu().numpy()
    for k in range(n_kc):
        assert np.array_equal(m[k, : len(kc_desc[k])].astype(bool), hmasks[k])
