"""Times the CRNN conv front end (forward, forward + backward) and the whole CRNN step (FocalLoss + FusedAdam) in both compute
dtypes at B = 256, F = 33, T = 573, next to the same modules through torch / MIOpen on the same card.  Prints one JSON line.
Warm-up first, then `--reps` repetitions timed with device events; the median is reported."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--F", type=int, default=33)
    ap.add_argument("--T", type=int, default=573)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
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
