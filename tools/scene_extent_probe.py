"""Times the two scene-extent stages.  The volume of interest: PROBLEMS problems x KEYFRAMES keyframes
at the default settings as one chain of mage_volume_of_interest_batch_device, and its twin on one host
core, once.  The scene-depth stage: FRAMES frames of POINTS associated map points each (a fifth of them
outside the region of interest) as one launch of mage_bounding_plane_depths_batch_device, wall clock
around launch plus synchronise, warm, median of REPEATS; and its plain C++ twin on one host core,
frame by frame over the same frames.  Prints one JSON line.  The figures are one machine's
measurement.

    python tools/scene_extent_probe.py [--frames 256] [--points 2000] [--repeats 20] [--softness 0.0] [--problems 8] [--keyframes 500]
"""
import argparse
import ctypes as C
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mageslam_amd import _lib, scene  # noqa: E402
from mageslam_amd._lib import BD_RESULT_DTYPE, PP_DTYPE  # noqa: E402
from tests import scene_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--softness", type=float, default=0.0)
    ap.add_argument("--problems", type=int, default=8)
    ap.add_argument("--keyframes", type=int, default=500)
    a = ap.parse_args()
    import torch

    F, N = a.frames, a.points
    settings = dataclasses.replace(sc.DEFAULTS, near_depth_softness=a.softness, far_depth_softness=a.softness)
    cs = settings.to_c()
    frames = [sc.make_frame(900 + f, N - N // 5, N // 5) for f in range(F)]
    packed = scene.pack_frames(frames)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        scene.bounding_plane_depths_batch_device(cs, cap=N, stream=stream, **packed)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)

    # the twin on this thread: the arrays prepared once, the calls alone timed
    L = _lib.load()
    prepared = []
    for f in frames:
        arrs = scene._arrays(f)
        prepared.append((f, arrs, np.zeros(1, BD_RESULT_DTYPE), np.zeros(N, PP_DTYPE)))

    def run_host():
        for f, (pos3, r9, intr4, kp, mp, idx), res, sparse in prepared:
            _lib.check(L.mage_bounding_plane_depths_host(C.byref(cs), _lib.ptr(pos3), _lib.ptr(r9), _lib.ptr(intr4), f.width,
                                                         f.height, _lib.ptr(kp), len(kp), _lib.ptr(mp), _lib.ptr(idx), len(mp),
                                                         N, _lib.ptr(res), _lib.ptr(sparse)))

    run_host()
    host = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        run_host()
        host.append(time.perf_counter() - t)

    res = packed["result"].cpu().numpy().view(BD_RESULT_DTYPE)
    same = all(res[i].tobytes() == prepared[i][2].tobytes() for i in range(F))
    out = {
        "frames": F, "points": N, "softness": a.softness, "device": torch.cuda.get_device_name(0),
        "depth_ms_median": round(1e3 * statistics.median(times), 3),
        "depth_ms_min_max": [round(1e3 * min(times), 3), round(1e3 * max(times), 3)],
        "depth_per_frame_us": round(1e6 * statistics.median(times) / F, 2),
        "twin_one_core_ms_median": round(1e3 * statistics.median(host), 3),
        "twin_per_frame_us": round(1e6 * statistics.median(host) / F, 2),
        "records_equal_to_twin": bool(same), "n_valid_median": float(np.median(res["n_valid"]))}
    out["volume"] = volume(a, torch, stream)
    print(json.dumps(out))


def volume(a, torch, stream):
    """The volume of interest: PROBLEMS problems x KEYFRAMES keyframes on a ring at the default settings."""
    from mageslam_amd._lib import VOI_LEVEL_DTYPE, VOI_RESULT_DTYPE

    P, K = a.problems, a.keyframes
    settings = sc.VOI_DEFAULTS
    cs = settings.to_c()
    hist = [sc.voi_history("circle", K, 500 + p) for p in range(P)]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    kf, nf = up(np.stack([h[0] for h in hist])), up(np.stack([h[1] for h in hist]))
    cnt = up(np.full(P, K, np.uint32))
    res = torch.zeros(P * VOI_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    tr = torch.zeros(P * settings.iterations * VOI_LEVEL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(scene.volume_of_interest_scratch_bytes(P, K), dtype=torch.uint8, device="cuda")

    def run():
        scene.volume_of_interest_batch_device(cs, P, kf, K, cnt, res, scratch, near_far=nf, trace=tr, stream=stream)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    t = time.perf_counter()
    twins = [scene.calculate_volume_of_interest(cs, h[0], h[1], backend="host") for h in hist]
    host = time.perf_counter() - t
    r = res.cpu().numpy().view(VOI_RESULT_DTYPE)
    trace = tr.cpu().numpy().view(VOI_LEVEL_DTYPE).reshape(P, settings.iterations)
    return {"problems": P, "keyframes": K, "volume_ms_median": round(1e3 * statistics.median(times), 3),
            "volume_ms_min_max": [round(1e3 * min(times), 3), round(1e3 * max(times), 3)],
            "twin_one_core_ms": round(1e3 * host, 1), "voxels_per_problem": int(np.prod(trace[0]["dims"], 1).sum()),
            "records_equal_to_twin": bool(all(r[i].tobytes() == twins[i].result.tobytes() for i in range(P))),
            "statuses": [int(x) for x in r["status"]]}


if __name__ == "__main__":
    main()
