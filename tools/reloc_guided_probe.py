"""Times the guided half of the relocalisation: FRAMES lost frames x CANDIDATES candidate keyframes
of ASSOC associations each (every candidate a good one, a tenth of the frame's keypoints displaced),
as one launch chain of mage_reloc_guided_batch_device behind one run of the PnP stage, and the PnP
stage plus the guided stage together; wall clock around launch plus synchronise, warm, median of
REPEATS.  Prints one JSON line.  The figures are one machine's measurement.

    python tools/reloc_guided_probe.py [--frames 16] [--candidates 4] [--assoc 300] [--repeats 20]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mageslam_amd import reloc  # noqa: E402
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, RG_FRAME_DTYPE, RG_RESULT_DTYPE, RP_RESULT_DTYPE  # noqa: E402
from tests import reloc_guided_cases as gc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=4)
    ap.add_argument("--assoc", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch

    F, K, N = a.frames, a.candidates, a.assoc
    P = F * K
    scenes = [gc.natural(f"probe{f}", 700 + f, N, kinds=("good",) * K, n_pnp=100) for f in range(F)]
    kfp, kpp, mc = N + 7, N + 9, 100
    cap = kfp
    mp, kfkp, kfd = np.zeros((P, kfp, 4), np.float32), np.zeros((P, kfp), KP_DTYPE), np.zeros((P, kfp, 32), np.uint8)
    kp, desc, mm = np.zeros((P, kpp), KP_DTYPE), np.zeros((P, kpp, 32), np.uint8), np.zeros((P, mc), DM_DTYPE)
    cnt = np.zeros((3, P), np.uint32)  # n_kf, n_kp, n_matches
    for f, s in enumerate(scenes):
        for c, cand in enumerate(s.cands):
            i = f * K + c
            mp[i], kfkp[i], kfd[i], kp[i], desc[i] = cand.map_xyzi, cand.kp, cand.desc, s.kp, s.desc
            mm[i, : len(s.matches[c])] = s.matches[c]
            cnt[:, i] = len(cand.kp), len(s.kp), len(s.matches[c])
    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    buf = lambda b: torch.zeros(b, dtype=torch.uint8, device=dev)  # noqa: E731
    intr, d_mp, d_kfkp, d_kfd, d_kp, d_desc, d_mm, d_cnt = (up(x) for x in (np.tile(gc.INTR, (P, 1)), mp, kfkp, kfd, kp, desc, mm, cnt))
    cs = reloc.RelocalizationSettings().to_c()
    pres, idx, obs = buf(RP_RESULT_DTYPE.itemsize * P), buf(4 * P * mc), buf(4 * (P + 1))
    pnp = [buf(12 * P * mc), buf(8 * P * mc), buf(4 * P * mc), buf(12 * P), buf(36 * P)]
    pscr = buf(reloc.scratch_bytes(int(cs.ransac_iterations), P, mc, False))
    E = P * cap
    o = dict(result=buf(RG_RESULT_DTYPE.itemsize * P), frame=buf(RG_FRAME_DTYPE.itemsize * F), query_kp=buf(28 * E),
             query_pos=buf(8 * E), query_desc=buf(32 * E), query_ref=buf(4 * E), n_queries=buf(4 * P), radius=buf(16 * E),
             n_radius=buf(4 * P), assoc=buf(8 * E), ba_obs_start=buf(4 * (P + 1)), ba_points3=buf(12 * E), ba_uv=buf(8 * E),
             ba_info=buf(4 * E), ba_outlier=buf(E), scratch=buf(reloc.guided_scratch_bytes(P, cap, mc)))
    n = d_cnt.data_ptr()
    args = reloc.RelocGuidedArgsC.make(
        frames=F, candidates_per_frame=K, cap=cap, pnp_cap=mc, pose_max_hamming_distance=reloc.POSE_MATCHER[0],
        pose_min_hamming_difference=reloc.POSE_MATCHER[1], kf_pitch=kfp, kp_pitch=kpp, d_intr4=intr, d_map_xyzi=d_mp,
        d_kf_kp=d_kfkp, d_kf_desc=d_kfd, d_n_kf=n, d_kp=d_kp, d_desc=d_desc, d_n_kp=n + 4 * P, d_pnp_result=pres,
        d_obs_start=obs, d_points3=pnp[0], d_uv=pnp[1], d_info=pnp[2], d_pos3=pnp[3], d_r9=pnp[4], d_query_kp=o["query_kp"],
        d_query_pos=o["query_pos"], d_query_desc=o["query_desc"], d_query_ref=o["query_ref"], d_n_queries=o["n_queries"],
        d_radius_matches=o["radius"], d_n_radius=o["n_radius"], d_assoc=o["assoc"], d_ba_obs_start=o["ba_obs_start"],
        d_ba_points3=o["ba_points3"], d_ba_uv=o["ba_uv"], d_ba_info=o["ba_info"], d_ba_outlier=o["ba_outlier"],
        d_result=o["result"], d_frame_result=o["frame"], d_scratch=o["scratch"])
    stream = torch.cuda.current_stream().cuda_stream

    def run_pnp():
        reloc.pnp_ransac_batch_device(cs, P, intr, d_mp, kfp, d_kp, kpp, n + 4 * P, d_mm, mc, n + 8 * P, pres, idx, mc, obs,
                                      *pnp, None, pscr, stream)

    def run_guided():
        reloc.guided_search_batch_device(cs, stream=stream, args=args)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        return times

    run_pnp()
    guided = timed(run_guided)
    both = timed(lambda: (run_pnp(), run_guided()))
    res = o["result"].cpu().numpy().view(RG_RESULT_DTYPE)
    fr = o["frame"].cpu().numpy().view(RG_FRAME_DTYPE)
    print(json.dumps({
        "frames": F, "candidates": K, "associations": N, "device": torch.cuda.get_device_name(0),
        "guided_ms_median": round(1e3 * statistics.median(guided), 3),
        "guided_ms_min_max": [round(1e3 * min(guided), 3), round(1e3 * max(guided), 3)],
        "pnp_plus_guided_ms_median": round(1e3 * statistics.median(both), 3),
        "guided_per_problem_us": round(1e6 * statistics.median(guided) / P, 1),
        "verdicts_ok": int((res["verdict"] == reloc.RG_OK).sum()), "frames_relocalised": int((fr["index"] >= 0).sum()),
        "radius_matches_median": float(np.median(res["n_radius_matches"])), "outliers_median": float(np.median(res["n_outliers"]))}))


if __name__ == "__main__":
    main()
