"""Throughput of mage_new_map_points_batch_device next to mage_new_map_points_host on one thread:
`--problems` Ki (256) with `--slots` Kc each (5) and about `--matches` matches per Kc (600), default
settings.  Eight distinct scenes from the tests' generator are tiled over the batch.  The device time
is the median of `--reps` timed launches (device events, after warm-up, enough launches per sample
to fill a few milliseconds); the host time is one pass of the C++ twin over the same problems.  The
two sides are compared byte for byte before timing.  Prints one JSON line.

    python tools/bench_new_points.py
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mageslam_amd import mapping  # noqa: E402
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, NP_DTYPE  # noqa: E402
from tests import new_points_cases as nc  # noqa: E402


def scene(seed, slots, matches):
    total = sum(nc.BASE_KINDS.values())
    kinds = {k: max(1, round(v * matches / total)) for k, v in nc.BASE_KINDS.items()}
    sc = nc._Scene(seed, slots)
    for k in range(slots):
        sc.fill(k, kinds)
    sc.shuffle_ki()
    return sc.problem(f"bench{seed}", extra_ki=64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--matches", type=int, default=600)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the throughput is not measured")
    distinct = [scene(100 + i, a.slots, a.matches) for i in range(8)]
    probs = [distinct[i % 8] for i in range(a.problems)]
    settings = distinct[0].settings
    ki_pitch = max(len(p.ki_kp) for p in distinct)
    mcap = max(len(m) for p in distinct for m in p.matches)
    cap = max(p.n_matches for p in distinct)
    n, pairs = a.problems, a.problems * a.slots

    mapping.new_map_points(settings, *probs[0].args(), cap=cap, backend="host")  # warm-up
    t0 = time.perf_counter()
    host =[mapping.new_map_points(settings, *p.args(), cap=cap, backend="host") for p in probs]
    host_s = time.perf_counter() - t0

    ki_pose, kc_pose = np.zeros((n, 16), np.float32), np.zeros((pairs, 16), np.float32)
    ki_kp, kc_kp = np.zeros((n, ki_pitch), KP_DTYPE), np.zeros((pairs, mcap), KP_DTYPE)
    m = np.zeros((pairs, mcap), DM_DTYPE)
    n_ki, n_kc = np.zeros(n, np.uint32), np.full(n, a.slots, np.uint32)
    n_kckp, n_m = np.zeros(pairs, np.uint32), np.zeros(pairs, np.uint32)
    for i, p in enumerate(probs):
        ki_pose[i] = np.concatenate([p.ki_pos3, p.ki_r9, p.ki_intr4])
        ki_kp[i, : len(p.ki_kp)] = p.ki_kp
        n_ki[i] = len(p.ki_kp)
        for k in range(a.slots):
            pr = i * a.slots + k
            kc_pose[pr] = np.concatenate([p.kc_pos3[k], p.kc_r9[k], p.kc_intr4[k]])
            kc_kp[pr, : len(p.kc_kp[k])] = p.kc_kp[k]
            m[pr, : len(p.matches[k])] = p.matches[k]
            n_kckp[pr], n_m[pr] = len(p.kc_kp[k]), len(p.matches[k])

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()

    d = [dev(x) for x in (ki_pose[:, :3], ki_pose[:, 3:12], ki_pose[:, 12:], ki_kp, n_ki, n_kc, kc_pose[:, :3],
                          kc_pose[:, 3:12], kc_pose[:, 12:], kc_kp, n_kckp, m, n_m)]
    out = torch.zeros(n * cap * 48, dtype=torch.uint8, device="cuda")
    n_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    verdict = torch.zeros(pairs * mcap, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def launch():
        mapping.new_map_points_batch_device(settings, n, a.slots, d[0], d[1], d[2], d[3], ki_pitch, d[4], None, d[5],
                                            d[6], d[7], d[8], d[9], mcap, d[10], d[11], mcap, d[12], out, cap, n_out,
                                            verdict, status)

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got = out.cpu().numpy().view(NP_DTYPE).reshape(n, cap)
    cnt = n_out.cpu().numpy()
    for i in range(n):
        assert got[i, : cnt[i]].tobytes() == host[i].points.tobytes(), i
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.inner)
    ms.sort()
    total = int(n_m.sum())
    print(json.dumps({
        "problems": n, "kc_slots": a.slots, "matches": total, "points": int(cnt.sum()),
        "device_ms_per_launch_median": round(ms[len(ms) // 2], 4), "device_ms_min": round(ms[0], 4),
        "device_ms_max": round(ms[-1], 4), "device_matches_per_s": round(total / (ms[len(ms) // 2] * 1e-3)),
        "host_one_thread_ms": round(host_s * 1e3, 2), "host_matches_per_s": round(total / host_s),
        "host_includes": "ctypes call and array packing per problem",
        "samples": a.reps, "launches_per_sample": a.inner}))


if __name__ == "__main__":
    main()
