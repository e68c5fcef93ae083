"""GPU parity of describe_blurred_kernel's per-wave paths against the CPU oracle, byte for byte.

The kernel computes a lane's test offsets once per wave, adds each keypoint's window base and
column phase (x - R) & 15, collects the ballots of the wave's keypoints in one register pair and
stores them with one masked 8-byte store per lane.  The frames here put keypoints exactly where
those paths can go wrong: a background texture of 3 x 3 blocks whose amplitude (values 0 .. 9) is
under half the FAST threshold (20 here) yields no corner of its own but a blurred window that is
not constant, also on a pyramid level, and isolated bright dots (>= 8 px apart, fewer than
nfeatures, so raster order and no retain / ANMS) are the keypoints.
"""
import numpy as np
import pytest

from mageslam_amd import orb

pytestmark = pytest.mark.gpu

W, H = 203, 97  # width no multiple of 16 (nor of the 32-byte brick)
R = 7           # pattern radius of the default patch (15)
TEXTURE_SEED = 0  # chosen on the CPU: every oracle descriptor below has >= 16 set and >= 16 clear bits
NFEAT = 440
FAST_T = 20
COUNTS = (1, 7, 8, 9, 31, 32, 33, 40)  # store mask inside a wave (8 keypoints), at a wave edge, at a workgroup edge (32)
SETTINGS = {"nlevels": "nlevels", "patchSize": "patch_size", "useOrientation": "use_orientation",
            "gaussianKernelSize": "gaussian_kernel_size", "fastThreshold": "fast_threshold"}


def kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8)


def background():
    coarse = np.random.default_rng(TEXTURE_SEED).integers(0, FAST_T // 2, (H // 3 + 1, W // 3 + 1))
    return (100 + np.kron(coarse, np.ones((3, 3), np.int64))[:H, :W]).astype(np.uint8)


def grid_dots():
    """Dots 9 px apart from (7, 7), plus the last emitted column x = W - 8 and row y = H - 8:
    (x - 7) & 15 = 9 i & 15 takes all 16 phases, (y - 7) & 3 = j & 3 all 4; the edges x = 7,
    x = W - 8, y = 7, y = H - 8 are there, and windows [x - 7, x + 7] both inside one 32-pixel
    brick column and across two."""
    xs = list(range(R, W - R - 9, 9)) + [W - R - 1]
    ys = list(range(R, H - R - 9, 9)) + [H - R - 1]
    return [(x, y) for y in ys for x in xs]


def dot_frame(dots):
    img = background()
    for i, (x, y) in enumerate(dots):
        img[y, x] = 170 + (37 * i) % 80
    return img


def count_dots(c):
    """c dots of the grid, taken in a fixed shuffled order so that few of them already mix phases."""
    g = grid_dots()
    order = np.random.default_rng(3).permutation(len(g))
    return [g[i] for i in order[:c]]


_ref = {}


def detector(**kw):
    return orb.OrbDetector(nfeatures=NFEAT, fastThreshold=FAST_T, **kw)


def reference(oracle, key, img, **kw):
    """oracle.orb_detect of `img`, computed once per key and shared; asserts on the oracle's output
    alone that no descriptor is (nearly) constant, so a wrong window cannot hide."""
    if key not in _ref:
        kw = dict(kw, fastThreshold=FAST_T)
        st, okp, od = oracle.orb_detect(img, oracle.default_settings(NFEAT, **{SETTINGS[k]: v for k, v in kw.items()}))
        assert st == 0
        if len(od):
            ones = np.unpackbits(od, axis=1).sum(axis=1)
            assert ones.min() >= 16 and ones.max() <= 256 - 16, (key, int(ones.min()), int(ones.max()))
        _ref[key] = (okp, od)
    return _ref[key]


def test_phases_bricks_and_edges(gpu, oracle):
    dots = grid_dots()
    img = dot_frame(dots)
    okp, od = reference(oracle, "grid", img)
    # what the frame is for, on the oracle's keypoints: every dot is one, in raster order
    assert len(okp) == len(dots) < NFEAT
    xs, ys = okp["x"].astype(int), okp["y"].astype(int)
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(dots)
    assert set((xs - R) & 15) == set(range(16)) and set((ys - R) & 3) == set(range(4))
    assert {R, W - R - 1} <= set(xs) and {R, H - R - 1} <= set(ys)
    one_brick = (xs - R) // 32 == (xs + R) // 32
    assert one_brick.any() and (~one_brick).any()
    kp, d = detector().DetectAndCompute(img)
    assert np.array_equal(kp_bytes(kp), kp_bytes(okp))
    bad = np.flatnonzero((d != od).any(axis=1))
    assert bad.size == 0, [(int(xs[i]), int(ys[i])) for i in bad[:8]]


@pytest.mark.parametrize("count", COUNTS)
def test_counts(gpu, oracle, count):
    img = dot_frame(count_dots(count))
    okp, od = reference(oracle, ("count", count), img)
    assert len(okp) == count
    kp, d = detector().DetectAndCompute(img)
    assert np.array_equal(kp_bytes(kp), kp_bytes(okp))
    assert np.array_equal(d, od)


@pytest.mark.parametrize("batch", [1, 9, 17])
def test_batches_keep_bytes_past_the_count(gpu, oracle, batch):
    """The 1-D grid maps slot -> frame 8 * (slot / chunks) + xcd: batches off a multiple of 8, frames
    of different counts, one blank.  No byte past keypoint n[f] - 1 of a frame may be written."""
    import torch

    cap = 48
    counts = [((0,) + COUNTS)[(f + 1) % 9] if batch > 1 else 9 for f in range(batch)]
    assert batch == 1 or 0 in counts
    frames_np = np.stack([dot_frame(count_dots(c)) for c in counts])
    frames = torch.from_numpy(frames_np).cuda()
    kp = torch.zeros((batch, cap * 28), dtype=torch.uint8, device="cuda")
    desc = torch.full((batch, cap, 32), 0xA5, dtype=torch.uint8, device="cuda")
    n = torch.zeros(batch, dtype=torch.int32, device="cuda")
    det = detector()
    det.detect_and_compute_batch_device(frames, W, H, kp, desc, n, cap)
    det.device_status()
    kp_h, desc_h, n_h = kp.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()
    for f, c in enumerate(counts):
        okp, od = reference(oracle, ("count", c), frames_np[f])
        assert n_h[f] == len(okp) == c, f
        assert np.array_equal(kp_h[f, : 28 * c], kp_bytes(okp).reshape(-1)), f
        assert np.array_equal(desc_h[f, :c], od), f
        assert (desc_h[f, c:] == 0xA5).all(), (f, c)


@pytest.mark.parametrize("kw", [dict(patchSize=21),  # radius bound 13: no pairing of lane halves; random pattern
                                dict(patchSize=31),  # rBRIEF-31 without orientation: the wide windows
                                dict(useOrientation=True, nlevels=2),  # per-keypoint level and rotation
                                dict(patchSize=25, useOrientation=True)],  # random pattern rotated per keypoint
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_other_instantiations(gpu, oracle, kw):
    img = dot_frame(grid_dots())
    okp, od = reference(oracle, ("grid", tuple(sorted(kw.items()))), img, **kw)
    assert 0 < len(okp) < NFEAT
    kp, d = detector(**kw).DetectAndCompute(img)
    assert np.array_equal(kp_bytes(kp), kp_bytes(okp)), kw
    assert np.array_equal(d, od), kw
