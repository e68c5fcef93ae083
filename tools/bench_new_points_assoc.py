"""Throughput of mage_new_points_associate_batch_device next to mage_new_points_associate_host on one
thread, on the shape of tools/bench_new_points.py: `--problems` Ki (256) with `--slots` Kc each (5) and
about `--matches` matches per Kc (600), plus `--extra` further keyframes with kf_slot = -1 (3), every
keyframe padded to `--keypoints` keypoints (2000).  Every keyframe sees the points the other keyframes
made (a keypoint at the projection, the predicted octave, Ki's descriptor three bits off), so the
association has real work.  The entry is timed alone and chained behind
mage_new_map_points_batch_device on one stream.  It updates the masks in place, so every timed launch
is preceded by a device copy that restores them; that copy is also timed alone and reported.  Device
times are the median of `--reps` samples of `--inner` launches (device events, after warm-up); the host
time is one pass of the C++ twin over the same problems.  The two sides are compared byte for byte
before timing.  Prints one JSON line.

    python tools/bench_new_points_assoc.py
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mageslam_amd import mapping  # noqa: E402
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, NA_DTYPE  # noqa: E402
from tests import new_points_assoc_cases as ac  # noqa: E402
from tests import new_points_cases as nc  # noqa: E402
from tools.bench_new_points import scene  # noqa: E402


def keyframes(p, pts, ki_desc, extra, n_kp, rng):
    """The problem's Kc slots and `extra` further keyframes as (pos3, r9, intr4, kp, desc, mask, slot):
    the slot's own keypoints first (the match indices stay valid), then a keypoint for every point
    another keyframe made, then distractors up to n_kp."""
    slots = len(p.kc_kp)
    poses = [(p.kc_pos3[k], p.kc_r9[k]) for k in range(slots)]
    for e in range(extra):
        C = np.array(ac.CENTRES[(slots + e) % len(ac.CENTRES)]) + rng.normal(0, 0.005, 3)
        R = nc._rot(*rng.normal(0, 0.03, 3))
        poses.append(((-(R @ C)).astype(np.float32), R.T.reshape(9).astype(np.float32)))
    scale = float(np.float32(p.settings.pyramid_scale))
    cx, cy, fx, fy = (float(v) for v in p.ki_intr4)
    out = []
    for k, (pos3, r9) in enumerate(poses):
        own = p.kc_kp[k] if k < slots else np.zeros(0, KP_DTYPE)
        desc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
        kp = np.zeros(n_kp, KP_DTYPE)
        kp["size"], kp["angle"], kp["response"], kp["class_id"] = 31.0, -1.0, 10.0, -1
        kp["x"], kp["y"] = rng.uniform(0, nc.W, n_kp), rng.uniform(0, nc.H, n_kp)
        kp["octave"] = rng.integers(0, 4, n_kp)
        kp[: len(own)] = own
        if k < slots:
            for m in p.matches[k]:
                desc[m["query_idx"]] = ac._flip(rng, ki_desc[m["train_idx"]], 3)
        R = np.asarray(r9, np.float64).reshape(3, 3).T
        t = np.asarray(pos3, np.float64)
        C = -(R.T @ t)
        i = len(own)
        for pt in pts:
            if int(pt["kc_slot"]) == k or i >= n_kp:
                continue
            X = np.asarray(pt["position"], np.float64)
            c = R @ X + t
            if c[2] <= 0.1:
                continue
            q = np.array([fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy]) + rng.normal(0, 0.7, 2)
            if not (0 <= q[0] < nc.W and 0 <= q[1] < nc.H):
                continue
            val = math.log2(np.linalg.norm(X - C) / float(pt["d_min"])) / math.log2(scale) - 0.5
            kp[i] = (q[0], q[1], 31.0, -1.0, 10.0, int(np.clip(math.floor(val + 0.5), 0, 7)), -1)
            desc[i] = ac._flip(rng, ki_desc[int(pt["ki_index"])], 3)
            i += 1
        mask = rng.uniform(size=n_kp) < 0.9
        if k < slots:
            mask[p.matches[k]["query_idx"]] = True
        out.append((pos3, r9, p.ki_intr4, kp, desc, mask, k if k < slots else -1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--extra", type=int, default=3)
    ap.add_argument("--matches", type=int, default=600)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the throughput is not measured")
    rng = np.random.default_rng(9)
    distinct = [scene(100 + i, a.slots, a.matches) for i in range(8)]
    settings = distinct[0].settings
    assoc = mapping.NewPointsAssociationSettings(image_border=20.0)
    cap = max(p.n_matches for p in distinct)
    nkf = a.slots + a.extra
    first, kis, kfs = [], [], []
    for p in distinct:
        h = mapping.new_map_points(settings, *p.args(), cap=cap, backend="host")
        ki_desc = rng.integers(0, 256, (len(p.ki_kp), 32), dtype=np.uint8)
        first.append(h)
        kis.append(ki_desc)
        kfs.append(keyframes(p, h.points, ki_desc, a.extra, a.keypoints, rng))

    def twin(i):
        k = kfs[i]
        return mapping.new_points_associate(settings, assoc, first[i].points, kis[i], [x[0] for x in k],
                                            [x[1] for x in k], [x[2] for x in k], [x[3] for x in k], [x[4] for x in k],
                                            [x[6] for x in k], [x[5] for x in k], backend="host")

    twin(0)  # warm-up
    t0 = time.perf_counter()
    host8 = [twin(i) for i in range(8)]
    host_s = (time.perf_counter() - t0) * a.problems / 8  # the batch tiles the eight scenes
    n, pairs, kpairs = a.problems, a.problems * a.slots, a.problems * nkf
    probs = [distinct[i % 8] for i in range(n)]
    ki_pitch = max(len(p.ki_kp) for p in distinct)
    mcap = max(len(m) for p in distinct for m in p.matches)

    ki_pose, kc_pose = np.zeros((n, 16), np.float32), np.zeros((pairs, 16), np.float32)
    ki_kp, kc_kp = np.zeros((n, ki_pitch), KP_DTYPE), np.zeros((pairs, mcap), KP_DTYPE)
    m = np.zeros((pairs, mcap), DM_DTYPE)
    n_ki, n_kc = np.zeros(n, np.uint32), np.full(n, a.slots, np.uint32)
    n_kckp, n_m = np.zeros(pairs, np.uint32), np.zeros(pairs, np.uint32)
    ki_desc = np.zeros((n, ki_pitch, 32), np.uint8)
    kf_pose = np.zeros((kpairs, 16), np.float32)
    kf_kp, kf_desc = np.zeros((kpairs, a.keypoints), KP_DTYPE), np.zeros((kpairs, a.keypoints, 32), np.uint8)
    kf_mask, kf_slot = np.zeros((kpairs, a.keypoints), np.uint8), np.zeros(kpairs, np.int32)
    n_kf, n_kfkp = np.full(n, nkf, np.uint32), np.full(kpairs, a.keypoints, np.uint32)
    for i, p in enumerate(probs):
        ki_pose[i] = np.concatenate([p.ki_pos3, p.ki_r9, p.ki_intr4])
        ki_kp[i, : len(p.ki_kp)] = p.ki_kp
        n_ki[i] = len(p.ki_kp)
        ki_desc[i, : len(p.ki_kp)] = kis[i % 8]
        for k in range(a.slots):
            pr = i * a.slots + k
            kc_pose[pr] = np.concatenate([p.kc_pos3[k], p.kc_r9[k], p.kc_intr4[k]])
            kc_kp[pr, : len(p.kc_kp[k])] = p.kc_kp[k]
            m[pr, : len(p.matches[k])] = p.matches[k]
            n_kckp[pr], n_m[pr] = len(p.kc_kp[k]), len(p.matches[k])
        for k, (pos3, r9, intr4, kp, desc, mask, slot) in enumerate(kfs[i % 8]):
            pr = i * nkf + k
            kf_pose[pr] = np.concatenate([pos3, r9, intr4])
            kf_kp[pr], kf_desc[pr], kf_mask[pr], kf_slot[pr] = kp, desc, mask, slot

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()

    d = [dev(x) for x in (ki_pose[:, :3], ki_pose[:, 3:12], ki_pose[:, 12:], ki_kp, n_ki, n_kc, kc_pose[:, :3],
                          kc_pose[:, 3:12], kc_pose[:, 12:], kc_kp, n_kckp, m, n_m)]
    f = [dev(x) for x in (ki_desc, n_kf, kf_pose[:, :3], kf_pose[:, 3:12], kf_pose[:, 12:], kf_kp, kf_desc, n_kfkp,
                          kf_slot)]
    mask0, mask = dev(kf_mask), dev(kf_mask)
    out = torch.zeros(n * cap * 48, dtype=torch.uint8, device="cuda")
    n_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    verdict = torch.zeros(pairs * mcap, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = torch.zeros(n * cap * nkf * 16, dtype=torch.uint8, device="cuda")
    averdict = torch.full((n * cap * nkf,), 0xFF, dtype=torch.uint8, device="cuda")
    astatus = torch.zeros(1, dtype=torch.int32, device="cuda")

    def create():
        mapping.new_map_points_batch_device(settings, n, a.slots, d[0], d[1], d[2], d[3], ki_pitch, d[4], None, d[5],
                                            d[6], d[7], d[8], d[9], mcap, d[10], d[11], mcap, d[12], out, cap, n_out,
                                            verdict, status)

    def reset():
        mask.copy_(mask0)

    def associate():
        mapping.new_points_associate_batch_device(settings, assoc, n, nkf, out, cap, n_out, f[0], ki_pitch, d[4], f[1],
                                                  f[2], f[3], f[4], f[5], f[6], mask, a.keypoints, f[7], f[8], rec,
                                                  averdict, astatus)

    create()
    reset()
    associate()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(astatus.item()) == 0
    cnt = n_out.cpu().numpy()
    got = rec.cpu().numpy().view(NA_DTYPE).reshape(n, cap, nkf)
    gv = averdict.cpu().numpy().reshape(n, cap, nkf)
    gm = mask.cpu().numpy().reshape(n, nkf, a.keypoints)
    for i in range(n):
        hrec, hv, hmasks, _ = host8[i % 8]
        assert cnt[i] == len(hrec)
        assert got[i, : cnt[i]].tobytes() == hrec.tobytes() and np.array_equal(gv[i, : cnt[i]], hv), i
        assert all(np.array_equal(gm[i, k].astype(bool), hmasks[k]) for k in range(nkf)), i

    def timed(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.inner)
        ms.sort()
        return ms

    t_reset = timed(reset)
    t_assoc = timed(lambda: (reset(), associate()))
    t_chain = timed(lambda: (create(), reset(), associate()))
    t_create = timed(create)
    med = lambda ms: round(ms[len(ms) // 2], 4)  # noqa: E731
    hv_all = np.concatenate([h[1].ravel() for h in host8])
    print(json.dumps({
        "problems": n, "kc_slots": a.slots, "extra_keyframes": a.extra, "keypoints_per_keyframe": a.keypoints,
        "points": int(cnt.sum()), "pairs_per_batch": int(cnt.sum()) * nkf,
        "associated_share_of_8_scenes": round(float((hv_all == 0).mean()), 4),
        "mask_reset_ms_median": med(t_reset),
        "reset_plus_associate_ms_median": med(t_assoc), "reset_plus_associate_ms_min": round(t_assoc[0], 4),
        "reset_plus_associate_ms_max": round(t_assoc[-1], 4),
        "associate_ms_median_less_reset": round(med(t_assoc) - med(t_reset), 4),
        "create_ms_median": med(t_create),
        "create_reset_associate_chained_ms_median": med(t_chain),
        "host_one_thread_ms": round(host_s * 1e3, 2),
        "host_includes": "ctypes call and array packing per problem; eight scenes timed, scaled to the batch",
        "samples": a.reps, "launches_per_sample": a.inner}))


if __name__ == "__main__":
    main()
