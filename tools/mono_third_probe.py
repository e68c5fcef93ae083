"""Times the third frame of the monocular map initialisation: the batched device chain
(mage_mono_init_third_frame_batch_device: match kernel, pack, pose-only bundle adjustment, finish)
for PROBLEMS problems x POINTS map points against a KEYPOINTS-keypoint third frame, warm, median of
REPEATS launches with wall clock around launch + synchronize; each of the chain's four kernels alone
(the pose bundle adjustment's included) from the library's event timers over the same number of
launches, taken in a loop of their own; and the plain C++ twin per problem on one
core, fed the GPU's outlier flags.  The verdicts and records are compared with the twin's before
anything is timed.  Prints one JSON line.  The figures are one machine's measurement.

    python tools/mono_third_probe.py [--problems 64] [--points 200] [--keypoints 2000] [--repeats 20]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mageslam_amd import _lib, mono  # noqa: E402
from mageslam_amd._lib import KP_DTYPE, M3_RESULT_DTYPE  # noqa: E402
from tests import mono_third_cases as tc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch

    P, N, K = a.problems, a.points, a.keypoints
    scenes = [tc._generic(f"probe{i}", N, 900 + i, n2_total=K) for i in range(P)]
    settings = scenes[0].settings
    n0, n1 = len(scenes[0].desc0), len(scenes[0].desc1)
    pos3, r9 = np.zeros((P, 6), np.float32), np.zeros((P, 18), np.float32)
    pts, idx = np.zeros((P, N, 3), np.float32), np.zeros((2, P, N), np.int32)
    d0, d1, d2 = np.zeros((P, n0, 32), np.uint8), np.zeros((P, n1, 32), np.uint8), np.zeros((P, K, 32), np.uint8)
    kp2 = np.zeros((P, K), KP_DTYPE)
    for i, c in enumerate(scenes):
        pos3[i], r9[i], pts[i], idx[0, i], idx[1, i] = c.pos3.reshape(6), c.r9.reshape(18), c.points, c.idx0, c.idx1
        d0[i], d1[i], d2[i], kp2[i] = c.desc0, c.desc1, c.desc2, c.kp2
    cnt = np.array([[N] * P, [n0] * P, [n1] * P, [K] * P], np.uint32)
    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    intr, d_pos3, d_r9, d_pts, d_idx = up(np.tile(tc.INTR, (P, 1))), up(pos3), up(r9), up(pts), up(idx)
    d_d0, d_d1, d_kp2, d_d2, d_cnt = up(d0), up(d1), up(kp2), up(d2), up(cnt)
    buf = lambda b: torch.zeros(b, dtype=torch.uint8, device=dev)  # noqa: E731
    sbytes, off = mono.third_scratch_layout(P, N)
    o = dict(result=buf(M3_RESULT_DTYPE.itemsize * P), keypoint=buf(4 * P * N), verdict=buf(P * N), dist=buf(8 * P * N),
             proj=buf(8 * P * N), mask=buf(P * K), uv=buf(8 * P * N), pt=buf(4 * P * N), cam=buf(4 * P * N),
             info=buf(4 * P * N), scratch=buf(sbytes))
    cs = settings.to_c()
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        mono.third_frame_batch_device(cs, P, intr, d_pos3, d_r9, d_pts, N, d_cnt.data_ptr(), d_idx.data_ptr(),
                                      d_idx.data_ptr() + 4 * P * N, d_d0, n0, d_cnt.data_ptr() + 4 * P, d_d1, n1,
                                      d_cnt.data_ptr() + 8 * P, d_kp2, d_d2, K, d_cnt.data_ptr() + 12 * P, 1, o["result"],
                                      o["keypoint"], o["verdict"], o["dist"], o["proj"], o["mask"], o["uv"], o["pt"],
                                      o["cam"], o["info"], o["scratch"], stream)

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    # the comparison first: every problem's record and per-point outputs against the twin
    res = o["result"].cpu().numpy().view(M3_RESULT_DTYPE)
    key = o["keypoint"].cpu().numpy().view(np.int32).reshape(P, N)
    sc = o["scratch"].cpu().numpy()
    start = sc[off["obs_start"]: off["obs_start"] + 4 * (P + 1)].view(np.uint32)
    flags = sc[off["outlier"]: off["outlier"] + P * N]
    opt_pos3 = sc[off["opt_pos3"]: off["opt_pos3"] + 12 * P].view(np.float32).reshape(P, 3)
    opt_r9 = sc[off["opt_r9"]: off["opt_r9"] + 36 * P].view(np.float32).reshape(P, 9)
    mean_sq = sc[off["mean_sq"]: off["mean_sq"] + 4 * P].view(np.float32)
    host, same = [], True
    for i, c in enumerate(scenes):
        t = time.perf_counter()
        h = mono.locate_third_frame(*c.args(), backend="host", outlier=flags[start[i]: start[i + 1]], opt_pos3=opt_pos3[i],
                                    opt_r9=opt_r9[i], mean_sq=float(mean_sq[i]))
        host.append(time.perf_counter() - t)
        same = same and h.result.tobytes() == res[i].tobytes() and h.keypoint.tobytes() == key[i].tobytes()
    times = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        launch()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    L = _lib.load()
    L.mage_profile_filter(b"")
    L.mage_profile_reset()
    L.mage_profile_enable(1)
    for _ in range(a.repeats):
        launch()
    torch.cuda.synchronize()
    rep = _lib.profile_report()
    L.mage_profile_enable(0)
    per = {k: round(v[1] / max(v[0], 1), 4) for k, v in rep.items() if k.startswith("monoinit.third") or k == "ba.pose_batch"}
    per["sum"] = round(sum(per.values()), 4)
    print(json.dumps({
        "problems": P, "points": N, "keypoints": K, "device": torch.cuda.get_device_name(0),
        "chain_ms_median": round(1e3 * statistics.median(times), 3),
        "chain_per_problem_us": round(1e6 * statistics.median(times) / P, 1),
        "kernel_ms_mean": per,
        "host_twin_per_problem_ms_median": round(1e3 * statistics.median(host), 3),
        "verdicts_ok": int((res["verdict"] == mono.M3_OK).sum()), "matched_mean": float(res["n_matched"].mean()),
        "outliers_total": int(res["n_outliers"].sum()), "gpu_equals_twin": bool(same)}))


if __name__ == "__main__":
    main()
