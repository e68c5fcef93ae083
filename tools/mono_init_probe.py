"""Times the monocular map initialisation's two-view stage: the batched device chain
(mage_mono_init_two_view_batch_device, matches given) for PAIRS frame pairs x MATCHES matches, warm,
median of REPEATS launches, and the plain C++ twin per pair on the same inputs.  Prints one JSON
line.  The figures are one machine's measurement.

    python tools/mono_init_probe.py [--pairs 64] [--matches 500] [--repeats 20]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mageslam_amd import mono  # noqa: E402
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE, MI_RESULT_DTYPE, SP_DTYPE  # noqa: E402
from tests import mono_init_cases as mc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--matches", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch

    P, N = a.pairs, a.matches
    settings = mono.MonoMapInitializationSettings()
    scenes = [mc._case(f"probe{i}", 500 + i, N, mc.SIDEWAYS_R, mc.SIDEWAYS_T, mono.OK, noise=0.3, outliers=N // 10)
              for i in range(P)]
    kp0, kp1 = np.zeros((P, N), KP_DTYPE), np.zeros((P, N), KP_DTYPE)
    mm = np.zeros((P, N), DM_DTYPE)
    for i, c in enumerate(scenes):
        kp0[i], kp1[i], mm[i] = c.kp0, c.kp1, c.matches
    n = np.full((3, P), N, np.uint32)
    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    intr, d_kp0, d_kp1, d_mm, d_n = up(np.tile(mc.INTR, (P, 1))), up(kp0), up(kp1), up(mm), up(n)
    buf = lambda b: torch.zeros(b, dtype=torch.uint8, device=dev)  # noqa: E731
    iters = settings.ransac_iterations_for_models
    result, out = buf(MI_RESULT_DTYPE.itemsize * P), buf(SP_DTYPE.itemsize * P * N)
    ba = [buf(12 * P * N), buf(16 * P * N), buf(8 * P * N), buf(8 * P * N), buf(8 * P * N)]
    scratch = buf(mono.scratch_bytes(iters, P, N, N, False, False))
    cs = settings.to_c()
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        mono.two_view_batch_device(cs, P, intr, d_kp0, None, N, d_n.data_ptr(), d_kp1, None, N, d_n.data_ptr() + 4 * P,
                                   d_mm, N, d_n.data_ptr() + 8 * P, result, out, N, *ba, None, scratch, stream)

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        launch()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    res = result.cpu().numpy().view(MI_RESULT_DTYPE)
    host = []
    same = True
    for i, c in enumerate(scenes):
        t = time.perf_counter()
        h = mono.initialize_with_frames(cs, mc.INTR, c.kp0, c.kp1, matches=c.matches, backend="host")
        host.append(time.perf_counter() - t)
        same = same and h.result.tobytes() == res[i].tobytes()
    print(json.dumps({
        "pairs": P, "matches": N, "iterations": iters, "device": torch.cuda.get_device_name(0),
        "gpu_batch_ms_median": round(1e3 * statistics.median(times), 3),
        "gpu_per_pair_us": round(1e6 * statistics.median(times) / P, 1),
        "host_twin_per_pair_ms_median": round(1e3 * statistics.median(host), 3),
        "verdicts_ok": int((res["verdict"] == mono.OK).sum()), "gpu_equals_twin": bool(same)}))


if __name__ == "__main__":
    main()
