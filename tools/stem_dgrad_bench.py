"""Times the stem input-gradient kernel (csrc/conv_stem_dgrad.hip) beside its two siblings on the same tensors -- the stem
forward and the stem weight gradient -- with events on the launch stream.  Per-launch kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stem_dgrad_bench.py
Usage: python tools/stem_dgrad_bench.py [--batch 256] [--hw 224x224] [--dtype bf16] [--reps 20]"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--hw", default="224x224")
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
lib = L.lib()
dev = "cuda"
dt = L.BF16 if a.dtype == "bf16" else L.F32
tdt = torch.bfloat16 if dt == L.BF16 else torch.float32
N, Cin, R = a.batch, 3, 7
H, W = (int(v) for v in a.hw.split("x"))
OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
x = torch.randn(N, Cin, H, W, device=dev).clamp_(-1, 1)
w = torch.randn(64, Cin, R, 7, device=dev) * 0.05
pk = torch.empty(lib.ecgmm_stem_packed_elems(Cin, R), device=dev, dtype=tdt)
L.check(lib.ecgmm_stem_pack(dt, ptr(w), ptr(pk), Cin, R, stream()))
y = torch.empty(N, OH, OW, 64, device=dev, dtype=tdt)
stats = torch.empty(lib.ecgmm_stem_wg_stats_rows(N, Cin, H, W, R) + lib.ecgmm_stem_stats_rows(N, Cin, H, W, R) + 64, 2, 64, device=dev)
dy = torch.randn(N, OH, OW, 64, device=dev).to(tdt)
dw = torch.empty(64, Cin, R, 7, device=dev)
dx = torch.empty(N, Cin, H, W, device=dev)
nb = lib.ecgmm_stem_bwd_weight_workspace(N, Cin, H, W, R)
ws = torch.empty(nb, device=dev, dtype=torch.uint8)


def fwd():
    f = lib.ecgmm_stem_fwd_wgrows if dt == L.BF16 else lib.ecgmm_stem_fwd
    L.check(f(dt, ptr(x), ptr(pk), None, ptr(y), ptr(stats), N, Cin, H, W, R, stream()))
def wgrad():
    L.check(lib.ecgmm_stem_bwd_weight(dt, ptr(x), ptr(dy), ptr(dw), 0, ptr(ws), nb, N, Cin, H, W, R, stream()))
def dgrad():
    L.check(lib.ecgmm_stem_bwd_data(dt, ptr(dy), ptr(w), ptr(dx), N, Cin, H, W, R, stream()))


es = 2 if dt == L.BF16 else 4
mb = (N * OH * OW * 64 * es + N * Cin * H * W * 4) / 1e6
for name, fn in (("stem_fwd", fwd), ("stem_bwd_weight(+reduce)", wgrad), ("stem_bwd_data", dgrad)):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.reps * 1e3
    print(f"B={N} {H}x{W} {a.dtype} {name}: {us:.1f} us ({mb:.0f} MB of tensors -> {mb / us:.2f} TB/s)")
