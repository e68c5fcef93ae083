"""Per-phase timing of fast_nms_kernel from s_memtime stamps (development tool, not the product).

  python tools/fast_stamps.py build   # abl/fst/libmage_hot.so with -DMAGE_FAST_STAMPS=1 (CPU)
  python tools/fast_stamps.py run     # C2 batches (gate forced to 89) on the GPU

Each wave of the tiles of frames 0..14 stamps s_memtime at the phase boundaries of fast_tile's
gated path; the table is the mean over waves of each phase's cycles (the wave's own elapsed time,
which includes the cycles its SIMD spent on other waves), separately for interior tiles (load_tile's
interior path) and border tiles.
"""
import ctypes as C
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "abl" / "fst"
# the stamps the gated path writes (slots 9 and 10 belonged to a barrier the kernel no longer has)
STAMPS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12]
NAMES = ["load + barrier", "gate", "listing", "dense barrier", "exact scoring", "(to blur)", "blur",
         "scores barrier + nms + emission", "final barrier", "output"]


def build():
    sys.path.insert(0, str(ROOT))
    from mageslam_amd import build as B
    B.build()
    objs = [p for p in B.OBJ.glob("*.o") if not p.name.startswith("orb")]
    OUT.mkdir(parents=True, exist_ok=True)
    subprocess.run([B.hipcc(), "-x", "hip", f"--offload-arch={B.ARCH}", "-munsafe-fp-atomics", *B.COMMON,
                    "-DMAGE_FAST_STAMPS=1", "-c", str(B.CSRC / "orb.hip"), "-o", str(OUT / "orb.o")], check=True)
    subprocess.run([B.hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", str(OUT / "libmage_hot.so"),
                    str(OUT / "orb.o"), *map(str, objs)], check=True)
    print("built", OUT)


def run():
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from mageslam_amd import _lib, orb, synth
    L = C.CDLL(str(OUT / "libmage_hot.so"))
    _lib._declare(L)
    _lib._lib = L
    W, H, B, N = 1280, 720, 256, 2000
    frames = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    kp = torch.zeros((B, N * 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((B, N, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    orb.synth_frames_device(frames, B, W, H, 0, synth.FRAME_SEED)
    det = orb.OrbDetector(nfeatures=N)
    st = np.zeros((4096, 2, 16), np.uint64)
    # tile of each stamp slot (slot = frame * tiles + T.y * tiles_x + T.x): a tile whose 136 x 38
    # window lies wholly inside the frame is staged by load_tile's interior path, the rest are
    # border tiles; the right tile column is listed on its own (its blur strips are partly off-frame)
    tx_n, ty_n = (W + 119) // 120, (H + 29) // 30
    slot = np.arange(4096)
    tx, ty = slot % tx_n, (slot % (tx_n * ty_n)) // tx_n
    interior = (120 * tx - 8 >= 0) & (120 * tx + 128 <= W) & (30 * ty - 4 >= 0) & (30 * ty + 34 <= H)
    kind = np.where(interior, 0, np.where(tx == tx_n - 1, 2, 1))
    kind = np.repeat(kind, 2)  # two waves per tile
    acc, kinds = [], []
    for it in range(6):
        det.set_fast_gate(89)
        det.detect_and_compute_batch_device(frames, W, H, kp, desc, cnt, N)
        torch.cuda.synchronize()
        L.mage_debug_fast_stamps(st.ctypes.data_as(C.c_void_p))
        if it >= 2:
            s = st[:, :, STAMPS].reshape(-1, len(STAMPS)).astype(np.int64)
            ok = (s[:, 0] > 0) & np.all(np.diff(s, axis=1) >= 0, axis=1)
            acc.append(np.diff(s[ok], axis=1))
            kinds.append(kind[ok])
    d = np.concatenate(acc)
    k = np.concatenate(kinds)
    groups = [("all tiles", k >= 0), ("interior", k == 0), ("border", k != 0),
              ("border, not right column", k == 1), ("right column", k == 2)]
    print("mean cycles per wave and phase; gate forced to 89; %dx%d, %d frames" % (W, H, B))
    print("| phase | " + " | ".join(g for g, _ in groups) + " |")
    print("|---|" + "---|" * len(groups))
    print("| waves | " + " | ".join(str(int(m.sum())) for _, m in groups) + " |")
    for i, n in enumerate(NAMES):
        print(f"| {n} | " + " | ".join(f"{d[m, i].mean():.0f}" for _, m in groups) + " |")
    print("| lifetime | " + " | ".join(f"{d[m].sum(1).mean():.0f}" for _, m in groups) + " |")


if __name__ == "__main__":
    {"build": build, "run": run}[sys.argv[1]]()
