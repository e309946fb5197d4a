"""The CRNN recurrent stack of train_physionet2.py:75-76 -- LSTM(512 -> 200, 3 layers, bidirectional, batch_first), T = 70 --
on ecgmm.hip.nn.LSTM: forward alone (no_grad) and forward + backward, at B = 8 (the reference's batch size) and B = 256.

Method (as tools/infer_bench.py): one process; warm-up calls of every variant first; then ROUNDS rounds, each timing every
variant for REPS consecutive calls between two events on the current stream; reported: the median over rounds of the
per-call time and the min-max spread of the rounds.  Cache state: warm (same inputs and weights every call).

Next to each time: the call's algorithmic FLOPs (projection GEMMs 2 B T In_l 4H + recurrence 2 B T 4H H per layer and
direction; the backward counts the dgrad / wgrad GEMMs and the dh chain: 2x the forward, + nothing for the cell update)
over the exact-f32 MFMA peak of DESIGN section 4.1 (157.3 TFLOP/s), and the recurrence's L2 traffic: every 16-row slice
reads W_hh (4H x H fp32) once per step, T |W_hh| per slice, layer and direction (the backward reads it once more).

    python tools/lstm_bench.py [--rounds 7] [--reps 10] [--out profiles/lstm_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ecgmm.hip import functional as HF  # noqa: E402
from ecgmm.hip import nn as HN  # noqa: E402

dev = torch.device("cuda:0")
IN, H, LAYERS, T, D = 512, 200, 3, 70, 2
PEAK_F32 = 157.3e12


def fwd_flops(B):
    per = 0.0
    for layer in range(LAYERS):
        In = IN if layer == 0 else D * H
        per += D * (2.0 * B * T * In * 4 * H + 2.0 * B * T * 4 * H * H)
    return per


def l2_bytes(B, passes):
    slices = (B + 15) // 16
    return passes * LAYERS * D * slices * T * (4 * H * H * 4)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    torch.manual_seed(0)
    net = HN.LSTM(IN, H, LAYERS, batch_first=True, bidirectional=True).to(dev)
    variants = {}
    for B in (8, 256):
        x = torch.randn(B, T, IN, device=dev)
        xg = x.clone().requires_grad_()
        gy = torch.randn(B, T, D * H, device=dev)

        def fwd(x=x):
            with torch.no_grad():
                net(x)

        def fwd_bwd(xg=xg, gy=gy):
            HF.release_grads(net)
            y, _ = net(xg)
            y.backward(gy)

        variants[f"b{B}_fwd"] = (fwd, fwd_flops(B), l2_bytes(B, 1))
        variants[f"b{B}_fwd_bwd"] = (fwd_bwd, 3.0 * fwd_flops(B), l2_bytes(B, 2))
    for fn, _, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, _, _) in variants.items():
            rounds[k].append(timed(fn, args.reps))
    res = {"shape": {"In": IN, "H": H, "layers": LAYERS, "bidirectional": True, "T": T}, "rounds": args.rounds,
           "reps": args.reps, "peak_f32_mfma_tflops": PEAK_F32 / 1e12, "variants": {}}
    for k, (fn, flops, l2) in variants.items():
        ms = statistics.median(rounds[k])
        res["variants"][k] = {"ms_median": ms, "ms_min": min(rounds[k]), "ms_max": max(rounds[k]), "gflop": flops / 1e9,
                              "fraction_of_f32_mfma_peak": flops / (ms * 1e-3) / PEAK_F32,
                              "recurrence_l2_gbytes": l2 / 1e9, "recurrence_l2_tbytes_per_s": l2 / (ms * 1e-3) / 1e12}
        v = res["variants"][k]
        print(f"{k:14s} {ms:9.3f} ms (rounds {v['ms_min']:.3f} .. {v['ms_max']:.3f})  {v['gflop']:8.1f} GFLOP = "
              f"{100 * v['fraction_of_f32_mfma_peak']:.2f} % of the f32 MFMA peak;  W_hh from L2 {v['recurrence_l2_gbytes']:.2f} GB")
    out = args.out or os.path.join(ROOT, "profiles", "lstm_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"lstm_bench": out}))


if __name__ == "__main__":
    main()
