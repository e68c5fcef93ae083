"""Per-phase timing of select_kernel from s_memtime stamps (development tool, not the product).

  python tools/select_stamps.py build [name[@REV]]   # abl/<name>/libmage_hot.so with -DMAGE_SELECT_STAMPS=1
                                                     # (CPU; name defaults to sel, @REV: orb.hip as committed at REV)
  python tools/select_stamps.py run [name]           # C2 batches on the GPU

Phases (stamps 0..10): tile scan | histogram | cut | retained items | bbox + cell zero | cell
count + scan | cell scatter | ANMS search | sort | output.  `run` prints, per phase, the mean over
the frames and the phase's cycles in each batch's slowest frame (averaged over the timed batches),
with that frame's total: one workgroup per frame, so the launch lasts as long as its slowest frame.
"""
import ctypes as C
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["tiles", "hist", "cut", "items", "bbox", "cellcount", "scatter", "search", "sort", "output"]


def build(spec="sel"):
    sys.path.insert(0, str(ROOT))
    from mageslam_amd import build as B
    B.build()
    name, _, rev = spec.partition("@")
    out = ROOT / "abl" / name
    objs = [p for p in B.OBJ.glob("*.o") if not p.name.startswith("orb")]
    out.mkdir(parents=True, exist_ok=True)
    src, inc, tree = B.CSRC / "orb.hip", [], None
    if rev:  # the sources and headers as committed at REV, in a scratch tree
        import tempfile
        tree = Path(tempfile.mkdtemp(prefix="sel_rev_"))
        arch = subprocess.run(["git", "archive", rev, "mageslam_amd/csrc", "include"], cwd=ROOT, check=True,
                              capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", str(tree)], input=arch, check=True)
        src, inc = tree / "mageslam_amd" / "csrc" / "orb.hip", [f"-I{tree / 'include'}"]
    subprocess.run([B.hipcc(), "-x", "hip", f"--offload-arch={B.ARCH}", "-munsafe-fp-atomics", *inc, *B.COMMON,
                    "-DMAGE_SELECT_STAMPS=1", "-c", str(src), "-o", str(out / "orb.o")], check=True)
    if tree:
        import shutil
        shutil.rmtree(tree)
    subprocess.run([B.hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", str(out / "libmage_hot.so"),
                    str(out / "orb.o"), *map(str, objs)], check=True)
    print("built", out)


def run(name="sel"):
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from mageslam_amd import _lib, orb, synth
    L = C.CDLL(str(ROOT / "abl" / name / "libmage_hot.so"))
    _lib._declare(L)
    _lib._lib = L
    W, H, B, N = 1280, 720, 256, 2000
    frames = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    kp = torch.zeros((B, N * 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((B, N, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    orb.synth_frames_device(frames, B, W, H, 0, synth.FRAME_SEED)
    det = orb.OrbDetector(nfeatures=N)
    st = np.zeros((1024, 16), np.uint64)
    acc, sub, slow, slow_sub = [], [], [], []
    for it in range(6):
        det.detect_and_compute_batch_device(frames, W, H, kp, desc, cnt, N)
        torch.cuda.synchronize()
        L.mage_debug_select_stamps(st.ctypes.data_as(C.c_void_p))
        if it >= 2:
            s = st[:B, :11].astype(np.int64)
            d = np.diff(s, axis=1)
            acc.append(d)
            x = st[:B].astype(np.int64)
            sb = np.stack([x[:, 11] - x[:, 8], x[:, 12] - x[:, 11], x[:, 13] - x[:, 12], x[:, 9] - x[:, 13]], 1)
            sub.append(sb)
            worst = int(d.sum(1).argmax())
            slow.append(d[worst])
            slow_sub.append(sb[worst])
            print("start spread (cycles):", int(s[:, 0].max() - s[:, 0].min()), " end-start mean:",
                  int((s[:, 10] - s[:, 0]).mean()), " slowest frame:", worst, int(d[worst].sum()),
                  " fastest:", int(d.sum(1).min()), flush=True)
    d = np.concatenate(acc).mean(0)
    w = np.stack(slow).mean(0)
    tot, wtot = d.sum(), w.sum()
    print(f"{'phase':>10}  {'mean over frames':>22}  {'slowest frame':>22}")
    for n, v, u in zip(NAMES, d, w):
        print(f"{n:>10}: {v:9.0f} cycles {100 * v / tot:5.1f} %  {u:9.0f} cycles {100 * u / wtot:5.1f} %")
    for n, v, u in zip(["mhist", "mscan", "compact", "bitonic"], np.concatenate(sub).mean(0), np.stack(slow_sub).mean(0)):
        print(f"{n:>10}: {v:9.0f} cycles          {u:9.0f} cycles          (inside sort)")
    print(f"{'total':>10}: {tot:9.0f} cycles          {wtot:9.0f} cycles")


if __name__ == "__main__":
    {"build": build, "run": run}[sys.argv[1]](*sys.argv[2:3])
