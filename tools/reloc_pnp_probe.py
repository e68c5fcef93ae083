"""Times the relocalisation PnP stage: the batched device chain (mage_reloc_pnp_batch_device) for
PROBLEMS problems x MATCHES matches with half of them outliers, at 2 and at 256 RANSAC iterations,
wall clock around launch plus synchronise, warm, median of REPEATS; and the plain C++ twin per
problem on one core on the same inputs.  Prints one JSON line per iteration count.  The figures are
one machine's measurement.

    python tools/reloc_pnp_probe.py [--problems 64] [--matches 300] [--repeats 20]
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
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, RP_RESULT_DTYPE  # noqa: E402
from tests import reloc_pnp_cases as rc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch

    P, N = a.problems, a.matches
    scenes = [rc.make_case(f"probe{i}", 900 + i, N, outliers=0.5, extra_kf=0, extra_kp=0) for i in range(P)]
    mp, kp, mm = np.zeros((P, N, 4), np.float32), np.zeros((P, N), KP_DTYPE), np.zeros((P, N), DM_DTYPE)
    for i, c in enumerate(scenes):
        mp[i], kp[i], mm[i] = c.map_xyzi, c.kp, c.matches
    n = np.full((2, P), N, np.uint32)
    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    intr, d_mp, d_kp, d_mm, d_n = up(np.tile(rc.INTR, (P, 1))), up(mp), up(kp), up(mm), up(n)
    buf = lambda b: torch.zeros(b, dtype=torch.uint8, device=dev)  # noqa: E731
    result, idx, obs = buf(RP_RESULT_DTYPE.itemsize * P), buf(4 * P * N), buf(4 * (P + 1))
    ba = [buf(12 * P * N), buf(8 * P * N), buf(4 * P * N), buf(12 * P), buf(36 * P)]
    stream = torch.cuda.current_stream().cuda_stream
    for iters in (2, 256):
        cs = reloc.RelocalizationSettings(ransac_iterations=iters).to_c()
        scratch = buf(reloc.scratch_bytes(iters, P, N, False))

        def launch():
            reloc.pnp_ransac_batch_device(cs, P, intr, d_mp, N, d_kp, N, d_n.data_ptr(), d_mm, N, d_n.data_ptr() + 4 * P,
                                          result, idx, N, obs, *ba, None, scratch, stream)

        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            launch()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        res = result.cpu().numpy().view(RP_RESULT_DTYPE)
        host = []
        same = True
        for i, c in enumerate(scenes):
            t = time.perf_counter()
            h = reloc.pnp_ransac(cs, rc.INTR, c.map_xyzi, c.kp, c.matches, backend="host")
            host.append(time.perf_counter() - t)
            same = same and h.result.tobytes() == res[i].tobytes()
        print(json.dumps({
            "problems": P, "matches": N, "iterations": iters, "device": torch.cuda.get_device_name(0),
            "gpu_batch_ms_median": round(1e3 * statistics.median(times), 3),
            "gpu_batch_ms_min_max": [round(1e3 * min(times), 3), round(1e3 * max(times), 3)],
            "gpu_per_problem_us": round(1e6 * statistics.median(times) / P, 1),
            "host_twin_per_problem_ms_median": round(1e3 * statistics.median(host), 3),
            "host_twin_batch_ms": round(1e3 * sum(host), 3),
            "verdicts_ok": int((res["verdict"] == reloc.OK).sum()),
            "iterations_run_median": float(np.median(res["iterations_run"])), "gpu_equals_twin": bool(same)}))


if __name__ == "__main__":
    main()
