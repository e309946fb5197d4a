"""Times the CRNN conv front end (forward, forward + backward) and the whole CRNN step (FocalLoss + FusedAdam) in both compute
dtypes at B = 256, F = 33, T = 573, next to the same modules through torch / MIOpen on the same card.  Prints one JSON line.
Warm-up first, then `--reps` repetitions timed with device events; the median is reported.
`--spectrogram` times only the log-spectrogram launch at `--records` x `--length` samples, next to the reference's
per-record scipy.signal.stft loop on the host, with the launch's algorithmic bytes and FLOP.
`--saliency` times what the spectrogram's input gradient costs, per compute dtype at the same shape: the front
end's plan backward without and with `dspec` (ecgmm_crnn_front_backward / _dx behind one training-mode forward, the two
alternated rep by rep), ecgmm_conv5_in1_bwd_data alone on a dy of that shape, and a device copy of the same dy bytes (read
once, written once) -- the floor of a kernel that must read dy once, measured in the same run and not taken from a data sheet.
Under ECGMM_LIB naming a build without the input gradient only the plan backward is timed (an A/B of the unchanged path)."""
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


def saliency(a):
    import ctypes as C

    from ecgmm.crnn import CRNN
    from ecgmm.hip import functional as HF
    from ecgmm.hip import lib as L
    ptr, stream = HF.ptr, HF.stream
    dev = torch.device("cuda:0")
    lib = L.lib()
    B, Fq, T = a.batch, a.F, a.T
    x = torch.randn(B, 1, Fq, T, device=dev)
    has_dx = hasattr(C.CDLL(L.LIB_PATH), "ecgmm_crnn_front_backward_dx")
    out = {"shape": [B, Fq, T], "device": torch.cuda.get_device_name(0), "reps": a.reps, "lib": os.path.basename(L.LIB_PATH)}
    for cd in ("bf16", "fp32"):
        net = CRNN(compute_dtype=cd).to(dev).train()
        params, buffers = net._front_tables()
        desc = L.CRNNFrontDesc(B, Fq, T, net._dtype, 1, 0.1, 1e-5)
        ws = HF.new_bytes(lib.ecgmm_crnn_front_fwd_workspace(C.byref(desc)), dev)
        bws = HF.new_bytes(lib.ecgmm_crnn_front_bwd_workspace(C.byref(desc)), dev)
        seq = torch.empty(B, T // 8, 128 * (Fq // 8), device=dev)
        L.check(lib.ecgmm_crnn_front_forward(C.byref(desc), ptr(x), HF._ptr_table(params), HF._ptr_table(buffers), ptr(seq),
                                             ptr(ws), ws.numel(), stream()), "crnn_front forward")
        g = torch.randn_like(seq)
        sinks = [torch.empty_like(p) for p in params]
        dspec = torch.empty_like(x)
        ptab, gtab = HF._ptr_table(params), HF._ptr_table(sinks)
        esz = 2 if cd == "bf16" else 4
        dy = torch.randn(B * Fq * T * 32, device=dev).to(torch.bfloat16 if cd == "bf16" else torch.float32)
        dy2, dx = torch.empty_like(dy), torch.empty(B, Fq, T, device=dev)
        w = params[0].detach()

        def bwd():
            L.check(lib.ecgmm_crnn_front_backward(C.byref(desc), ptr(x), ptr(g), ptab, gtab, ptr(ws), ptr(bws), bws.numel(),
                                                  stream()), "crnn_front backward")

        def bwd_dx():
            L.check(lib.ecgmm_crnn_front_backward_dx(C.byref(desc), ptr(x), ptr(g), ptab, gtab, ptr(ws), ptr(bws), bws.numel(),
                                                     ptr(dspec), stream()), "crnn_front backward_dx")

        def kernel():
            L.check(lib.ecgmm_conv5_in1_bwd_data(net._dtype, ptr(dy), ptr(w), ptr(dx), B, Fq, T, stream()), "conv5_in1_bwd_data")

        def copy():
            dy2.copy_(dy)
        fns = {"front_bwd": bwd, "front_bwd_dx": bwd_dx, "conv5_in1_bwd_data": kernel, "copy_dy": copy}
        if not has_dx:      # an ECGMM_LIB build from before the input gradient: the plan backward alone, for an A/B of it
            fns = {"front_bwd": bwd}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.reps):            # alternated rep by rep: drift hits every variant alike
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        r = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}
        out[cd] = r
        if not has_dx:
            continue
        r["dy_bytes"] = dy.numel() * esz
        r["dy_GB_per_s_kernel"] = r["dy_bytes"] / r["conv5_in1_bwd_data"]["median_ms"] / 1e6
        r["dy_GB_per_s_copy_read"] = r["dy_bytes"] / r["copy_dy"]["median_ms"] / 1e6
        r["kernel_over_copy"] = r["conv5_in1_bwd_data"]["median_ms"] / r["copy_dy"]["median_ms"]
        r["fma_TFLOP_per_s"] = 2 * 800 * B * Fq * T / r["conv5_in1_bwd_data"]["median_ms"] / 1e9
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--F", type=int, default=33)
    ap.add_argument("--T", type=int, default=573)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spectrogram", action="store_true")
    ap.add_argument("--saliency", action="store_true")
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--length", type=int, default=18286)
    a = ap.parse_args()
    if a.spectrogram:
        return spectrogram(a)
    if a.saliency:
        return saliency(a)
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
