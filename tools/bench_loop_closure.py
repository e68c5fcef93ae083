"""Throughput of mage_cheap_loop_closure_batch_device next to mage_cheap_loop_closure_host on one
thread: `--problems` mapping tasks (256), each a map of `--points` points (199: all sampled, just under
MaxMapPoints) seen by a new keyframe and `--keyframes` covisible ones (8), every keyframe padded to
`--keypoints` keypoints (2000).  The scenes are those of tests/loop_closure_cases.py (a keypoint at the
projection of most points, the predicted octave, the point's descriptor two bits off), so the closure
and the connect stage have real work.  The step updates the map and the masks in place, so every timed
chain is preceded by device copies that restore them; those copies are also timed alone and reported.
Device times are the median of `--reps` samples of `--inner` chains (device events, after warm-up);
the three launches' own times come from the library's event timers in a pass of their own; the host
time is one pass of the C++ twin over the distinct scenes, scaled to the batch.  The two sides are
compared byte for byte before timing.  Prints one JSON line.

    python tools/bench_loop_closure.py
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mageslam_amd import _lib, loopclosure as lcm  # noqa: E402
from tests import loop_closure_cases as lc  # noqa: E402
from tests.new_points_cases import _rot  # noqa: E402


def scene(seed, n_points, n_kf, n_kp):
    sc = lc.Scene(seed, n_points, pitch=4 + n_kf)
    r = sc.rng

    def padded(kf):
        return dataclasses.replace(kf, kp=kf.kp[:n_kp], desc=kf.desc[:n_kp], kp_point=kf.kp_point[:n_kp])

    ki = padded(sc.ki(distract=n_kp))
    kfs = [padded(sc.keyframe(60 + k, np.array([0.2 * np.cos(0.8 * k), 0.2 * np.sin(0.8 * k), 0.02 * k]) + r.normal(0, 0.005, 3),
                              _rot(*r.normal(0, 0.02, 3)), distract=n_kp)) for k in range(n_kf)]
    return sc.case(f"bench{seed}", ki, kfs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--keyframes", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--points", type=int, default=199)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the throughput is not measured")
    distinct = [scene(200 + i, a.points, a.keyframes, a.keypoints) for i in range(8)]
    s = distinct[0].settings

    def twin(i):
        return lcm.cheap_loop_closure_and_connect(s, distinct[i].problem, backend="host")

    twin(0)  # warm-up
    t0 = time.perf_counter()
    host8 = [twin(i) for i in range(8)]
    host_s = (time.perf_counter() - t0) * a.problems / 8  # the batch tiles the eight scenes
    n = a.problems
    packed = lcm.pack_problems(s, [distinct[i % 8].problem for i in range(n)])
    keep = {k: packed[k].clone() for k in ("d_state", "d_obs", "d_kf_mask")}

    def reset():
        for k, v in keep.items():
            packed[k].copy_(v)

    def step():
        lcm.cheap_loop_closure_batch_device(s, packed)

    reset()
    step()
    torch.cuda.synchronize()
    out = lcm.unpack_problems(packed)
    for i in range(n):
        h = host8[i % 8]
        L = int(h.counts[0])
        assert out["d_counts"][i].tolist() == h.counts.tolist() and int(out["d_status"][i]) == 0, i
        assert out["d_state"][i].tobytes() == h.state.tobytes() and out["d_obs"][i].tobytes() == h.obs.tobytes(), i
        assert out["d_closure"][i, :L].tobytes() == h.closure[:L].tobytes(), i
        assert np.ascontiguousarray(out["d_connect"][i, :L]).tobytes() == np.ascontiguousarray(h.connect[:L]).tobytes(), i

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
    t_step = timed(lambda: (reset(), step()))
    L = _lib.load()
    L.mage_profile_reset()
    L.mage_profile_enable(1)
    for _ in range(a.reps):
        reset()
        step()
    torch.cuda.synchronize()
    L.mage_profile_enable(0)
    launches = {k: round(ms / cnt, 4) for k, (cnt, ms) in _lib.profile_report().items() if k.startswith("loopclose.") and cnt}
    med = lambda ms: round(ms[len(ms) // 2], 4)  # noqa: E731
    counts = np.array([h.counts for h in host8])
    print(json.dumps({
        "problems": n, "keyframes": a.keyframes, "keypoints_per_keyframe": a.keypoints,
        "sampled_per_problem": round(float(counts[:, 0].mean()), 1), "closed_per_problem": round(float(counts[:, 1].mean()), 1),
        "connected_per_problem": round(float(counts[:, 2].mean()), 1),
        "reset_ms_median": med(t_reset), "reset_plus_step_ms_median": med(t_step),
        "reset_plus_step_ms_min": round(t_step[0], 4), "reset_plus_step_ms_max": round(t_step[-1], 4),
        "step_ms_median_less_reset": round(med(t_step) - med(t_reset), 4), "launch_ms_mean": launches,
        "host_one_thread_ms": round(host_s * 1e3, 2),
        "host_includes": "ctypes call and array packing per problem; eight scenes timed, scaled to the batch",
        "samples": a.reps, "launches_per_sample": a.inner}))


if __name__ == "__main__":
    main()
