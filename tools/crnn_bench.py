"""Times the CRNN conv front end (forward, forward + backward) and the whole CRNN step (FocalLoss + FusedAdam) in both compute
dtypes at B = 256, F = 33, T = 573, next to the same modules through torch / MIOpen on the same card.  Prints one JSON line.
Warm-up first, then `--reps` repetitions timed with device events; the median is reported.
`--spectrogram` times only the log-spectrogram launch at `--records` x `--length` samples, next to the reference's
per-record scipy.signal.stft loop on the host, with the launch's algorithmic bytes and FLOP."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def spectrogram(a):
    import time

    import numpy as np
    import scipy.signal

    from ecgmm.spectrogram import compute_log_spectrogram, stft_frames
    dev = torch.device("cuda:0")
    S, Ln, T = a.records, a.length, stft_frames(a.length)
    x = torch.randn(S, Ln, device=dev)
    out = {"shape": [S, Ln], "frames": T, "device": torch.cuda.get_device_name(0),
           "bytes": 4 * S * (Ln + 33 * T), "flop": 2 * 64 * 66 * S * T}      # x read once, out written once; direct DFT
    out["log_spectrogram"] = timed(lambda: compute_log_spectrogram(x), a.warmup, a.reps)
    ms = out["log_spectrogram"]["median_ms"]
    out["GB_per_s"], out["GFLOP_per_s"] = out["bytes"] / ms / 1e6, out["flop"] / ms / 1e6
    xh = x.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    for row in xh:      # train_physionet2.py:30-34, 135-142: one record at a time
        np.log1p(np.abs(scipy.signal.stft(row, fs=300, window="tukey", nperseg=64, noverlap=32)[2]))
    out["scipy_host_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--F", type=int, default=33)
    ap.add_argument("--T", type=int, default=573)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spectrogram", action="store_true")
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--length", type=int, default=18286)
    a = ap.parse_args()
    if a.spectrogram:
        return spectrogram(a)
    from ecgmm.crnn import CRNN
    from ecgmm.hip import functional as HF
    from ecgmm.optim import FusedAdam
    import crnn_ref as R
    dev = torch.device("cuda:0")
    x = torch.randn(a.batch, 1, a.F, a.T, device=dev)
    lab = torch.randint(0, 2, (a.batch,), device=dev)
    out = {"shape": [a.batch, a.F, a.T], "device": torch.cuda.get_device_name(0)}
    for cd in ("bf16", "fp32"):
        net = CRNN(compute_dtype=cd).to(dev).train()
        opt = FusedAdam(net.parameters(), lr=1e-3)
        params, buffers = net._front_tables()
        g = torch.randn(a.batch, a.T // 8, 128 * (a.F // 8), device=dev)

        def front_fwd():
            with torch.no_grad():
                HF.crnn_front(x, params, buffers, True, 0.1, 1e-5, net._dtype)

        def front_fwd_bwd():
            HF.release_grads(net)
            HF.crnn_front(x, params, buffers, True, 0.1, 1e-5, net._dtype).backward(g)

        def step():
            opt.zero_grad()
            HF.focal_loss(net(x), lab).backward()
            opt.step()
        out[cd] = {"front_fwd": timed(front_fwd, a.warmup, a.reps), "front_fwd_bwd": timed(front_fwd_bwd, a.warmup, a.reps),
                   "step": timed(step, a.warmup, a.reps)}
    ref = R.CRNN().to(dev).train()
    opt_r = torch.optim.Adam(ref.parameters(), lr=1e-3)
    gr = torch.randn(a.batch, a.T // 8, 128 * (a.F // 8), device=dev)
    for name, ac in (("torch_fp32", False), ("torch_bf16_autocast", True)):
        def t_front_fwd():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                ref.front(x)

        def t_front_fwd_bwd():
            opt_r.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                s = ref.front(x)
            s.float().backward(gr)

        def t_step():
            opt_r.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                lg = ref(x)
            R.focal_loss(lg.float(), lab).backward()
            opt_r.step()
        out[name] = {"front_fwd": timed(t_front_fwd, a.warmup, a.reps),
                     "front_fwd_bwd": timed(t_front_fwd_bwd, a.warmup, a.reps), "step": timed(t_step, a.warmup, a.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
