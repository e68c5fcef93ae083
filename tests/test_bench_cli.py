"""bench.py's command line: a plain run is the headline ORB leg alone, --full switches the other legs
back on, and --dump-outputs writes the last timed step's outputs as float arrays."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

OUTPUT_NAMES = {"sample_frames", "keypoint_counts", "match_counts", "keypoints", "descriptors", "matches"}


def _parse(monkeypatch, *argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_leg_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    assert a.no_ba and a.no_pose and a.no_tracking and a.no_cpu_baseline and a.no_rbrief31 and a.no_all_cores
    assert a.pipelined_streams == 0 and a.batch_parity == 0
    assert a.profile == 1  # the roofline kernel's timing inside the timed region stays


def test_full_keeps_every_leg_and_its_switch(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_ba or a.no_pose or a.no_tracking or a.no_cpu_baseline or a.no_rbrief31
                           or a.no_all_cores)
    assert a.pipelined_streams == 2 and a.batch_parity == 4
    a = _parse(monkeypatch, "--full", "--no-ba", "--pipelined-streams", "0")
    assert a.no_ba and not a.no_pose and a.pipelined_streams == 0


def test_last_step_outputs_layout(monkeypatch, tmp_path):
    """The dump on host tensors with known records: float32 / float64 only, the same seeded frame
    sample every time, records past a frame's count zeroed (stale NaN bit patterns included)."""
    import torch

    import bench
    from mageslam_amd._lib import DM_DTYPE, KP_DTYPE

    B, N, b = 40, 6, 40  # the batch in ring slots [b + 1, b + B]
    a = _parse(monkeypatch, "--batch", str(B), "--features", str(N))
    rng = np.random.default_rng(1)
    kp = np.zeros((2 * B + 1, N), KP_DTYPE)
    for f in ("x", "y", "size", "angle", "response"):
        kp[f] = rng.random(kp.shape, np.float32)
    kp["octave"], kp["class_id"] = rng.integers(0, 4, kp.shape), -1
    cnt = rng.integers(0, N + 1, 2 * B + 1).astype(np.int32)
    kp["x"][np.arange(N)[None, :] >= cnt[:, None]] = np.nan
    desc = rng.integers(0, 256, (2 * B + 1, N, 32), dtype=np.uint8)
    mt = np.zeros((B, N), DM_DTYPE)
    mt["query_idx"], mt["train_idx"] = np.arange(N), rng.integers(0, N, (B, N))
    mt["distance"] = rng.integers(0, 30, (B, N))
    nm = rng.integers(0, N + 1, B).astype(np.int32)
    ring = dict(kp=torch.from_numpy(kp.view(np.uint8).reshape(2 * B + 1, N * 28)), desc=torch.from_numpy(desc),
                cnt=torch.from_numpy(cnt))
    out = dict(mt=torch.from_numpy(mt.view(np.uint8).reshape(B, N * 16)), nm=torch.from_numpy(nm))
    o = bench.last_step_outputs(a, ring, b, out)
    assert set(o) == OUTPUT_NAMES
    assert all(v.dtype in (np.float32, np.float64) for v in o.values())
    idx = o["sample_frames"].astype(int)
    assert len(idx) == bench.OUTPUT_SAMPLE_FRAMES and len(set(idx)) == len(idx) and idx.max() < B
    assert np.array_equal(idx, bench.last_step_outputs(a, ring, b, out)["sample_frames"])
    assert np.array_equal(o["keypoint_counts"], cnt[b + 1:b + B + 1]) and np.array_equal(o["match_counts"], nm)
    assert o["keypoints"].shape == (len(idx), N, 7) and o["descriptors"].shape == (len(idx), N, 32)
    assert o["matches"].shape == (len(idx), N, 4)
    for j, f in enumerate(idx):
        n, m = cnt[b + 1 + f], nm[f]
        assert np.array_equal(o["keypoints"][j, :n, 0], kp["x"][b + 1 + f, :n])
        assert np.array_equal(o["keypoints"][j, :n, 5], kp["octave"][b + 1 + f, :n])
        assert np.array_equal(o["descriptors"][j, :n], desc[b + 1 + f, :n])
        assert np.array_equal(o["matches"][j, :m, 1], mt["train_idx"][f, :m])
        assert not o["keypoints"][j, n:].any() and not o["descriptors"][j, n:].any() and not o["matches"][j, m:].any()
    bench.write_outputs(tmp_path / "dump", o)
    assert {p.stem for p in (tmp_path / "dump").glob("*.npy")} == OUTPUT_NAMES
    assert np.array_equal(np.load(tmp_path / "dump" / "keypoints.npy"), o["keypoints"])


@pytest.mark.gpu
def test_plain_bench_run_dumps_its_last_step(gpu, tmp_path):
    """One small plain run: --steps sets the timed steps, the result line carries ms_per_step and none
    of the --full legs, and the dump holds the last step's records of the sampled frames."""
    B, N, steps = 8, 500, 3
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(B), "--frames", "16", "--width", "640", "--height", "480", "--features", str(N),
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=120,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["full"] is False and d["n_gpus"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1000.0 * B / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert d["kernels"]["orb.fast_nms"]["launches"] == steps  # the timed region ran exactly --steps steps
    for leg in ("ba", "pose_ba", "tracking", "rbrief31", "pipelined", "cpu_baseline"):
        assert leg not in d
    assert d["parity"] is None
    o = {p.stem: np.load(p) for p in (tmp_path / "dump").glob("*.npy")}
    assert set(o) == OUTPUT_NAMES and sum(v.nbytes for v in o.values()) <= 64e6
    assert all(v.dtype in (np.float32, np.float64) for v in o.values())
    idx = o["sample_frames"].astype(int)
    assert o["keypoint_counts"].shape == (B,) and o["keypoints"].shape == (len(idx), N, 7)
    assert o["keypoint_counts"].mean() == pytest.approx(d["mean_keypoints"])
    assert o["match_counts"].mean() == pytest.approx(d["mean_matches"])
    assert o["keypoint_counts"].min() > 0 and o["match_counts"][1:].min() > 0
    for j, f in enumerate(idx):
        n, m = int(o["keypoint_counts"][f]), int(o["match_counts"][f])
        assert o["keypoints"][j, :n, 2].min() > 0 and not o["keypoints"][j, n:].any()  # size > 0 on real records
        assert o["descriptors"][j, :n].any(axis=1).all() and not o["descriptors"][j, n:].any()
        assert (o["matches"][j, :m, 0] < n).all() and not o["matches"][j, m:].any()
