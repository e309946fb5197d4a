"""PhysioNet-2017 path timings: one process, device events on the stream, warm-up then 7 rounds x 10
calls, medians of the per-call round means --
  (a) filter_zscore on [8528, 3000] (the challenge's training-set size),
  (b) gather_augment at B = 8 / 256 / 512 (augmentation on and off),
  (c) a ResNet1D_SE training step at [B, 1, 3000] fed by the device loader,
  (d) ecgmm.preprocess.preprocess_signal (baseline removal + default low-pass) on [256, 5000], under the same protocol,
and the reference pipeline restated with scipy / numpy per sample (filtfilt + z-score; augment_signal) on the host's
CPUs (a pool of --cpus processes, as DataLoader workers would run it) as the baseline for (a) and (b).
Writes profiles/physionet_bench.json and prints it.  --front-only: (a) and (d) alone, the two filtfilt launches, printed and
not written (an A/B of two builds of the library: ECGMM_LIB selects the build).  --resample: the Fourier resampler alone
(DESIGN section 29), 5000 -> 3000 at S = 256 and the lengths form on the synthetic records' lengths (2000 .. 18000, ratio
0.6), 3 rounds x 3 calls, next to scipy.signal.resample on the same rows in one host process; written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ROUNDS, CALLS = 7, 10
FLOOR_TBPS = (4.07, 4.45)   # what the BatchNorm passes reach on this hardware


def _cpu_pre(x):
    from scipy.signal import butter, filtfilt
    b, a = butter(4, [16 / 150, 149 / 150], btype="band")
    y = filtfilt(b, a, x)
    return ((y - np.mean(y)) / (np.std(y) + 1e-8)).astype(np.float32)


def _cpu_aug(x):
    x = x.copy()
    if np.random.rand() < 0.5:
        x += np.random.normal(0, 0.01, x.shape)
    if np.random.rand() < 0.5:
        x *= np.random.uniform(0.8, 1.2)
    if np.random.rand() < 0.5:
        x = np.roll(x, np.random.randint(-10, 10))
    return x.copy()


def _cpu_chunk(args):
    kind, n, seed = args
    rng = np.random.RandomState(seed)
    np.random.seed(seed)
    x = rng.randn(n, 3000).astype(np.float32)
    t0 = time.perf_counter()
    for i in range(n):
        (_cpu_pre if kind == "pre" else _cpu_aug)(x[i].astype(np.float64) if kind == "pre" else x[i])
    return time.perf_counter() - t0


def cpu_baseline(kind, n_per_proc, procs):
    """-> seconds per sample with `procs` worker processes busy at once (wall time of the slowest / samples)"""
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(_cpu_chunk, [(kind, 8, s) for s in range(procs)])          # warm the workers (imports, filter design)
        t0 = time.perf_counter()
        pool.map(_cpu_chunk, [(kind, n_per_proc, 100 + s) for s in range(procs)])
        wall = time.perf_counter() - t0
    return wall / (n_per_proc * procs)


def timed(fn, torch, rounds=ROUNDS, calls=CALLS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / calls)
    return {"ms_median": round(statistics.median(per_call), 5), "ms_min": round(min(per_call), 5),
            "ms_max": round(max(per_call), 5)}


def with_floor(r, nbytes):
    r["algorithmic_bytes"] = nbytes
    r["achieved_GBps"] = round(nbytes / r["ms_median"] / 1e6, 1)
    r["floor_us"] = [round(nbytes / (t * 1e12) * 1e6, 3) for t in reversed(FLOOR_TBPS)]
    r["x_floor"] = round(r["ms_median"] * 1e3 / r["floor_us"][1], 2)
    return r


def resample_bench(torch, dev):
    """the resampler's one-time cost: device milliseconds per call, twiddle products per second, and scipy on the host"""
    from scipy.signal import resample
    from ecgmm import preprocess as PP
    res = {"rounds": 3, "calls_per_round": 3, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(2)
    S, N, num = 256, 5000, 3000
    x = torch.randn(S, N, generator=g)
    xd = x.to(dev)
    r = timed(lambda: PP.resample(xd, num), torch, 3, 3, 1)
    K = min(N, num) // 2 + 1
    products = S * (N * K + K * num)
    r["twiddle_products"] = products
    r["Gproducts_per_s"] = round(products / r["ms_median"] / 1e6, 1)
    t0 = time.perf_counter()
    resample(x.numpy().astype(np.float64), num, axis=1)
    r["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["resample_256x5000_to_3000"] = r

    rng = np.random.RandomState(42)
    lengths = rng.randint(2000, 18001, size=S)
    Lmax = int(lengths.max())
    rows = torch.randn(S, Lmax, generator=g)
    rd, ld = rows.to(dev), torch.as_tensor(lengths, dtype=torch.int32, device=dev)
    r = timed(lambda: PP.resample(rd, ratio=0.6, lengths=ld), torch, 3, 3, 1)
    nums = [int(n * 0.6) for n in lengths]
    products = int(sum((n * (m // 2 + 1) + (m // 2 + 1) * m) for n, m in zip(lengths.tolist(), nums)))
    r["twiddle_products"] = products
    r["Gproducts_per_s"] = round(products / r["ms_median"] / 1e6, 1)
    r["records_per_s"] = round(S / r["ms_median"] * 1e3, 1)
    t0 = time.perf_counter()
    for i, n in enumerate(lengths):
        resample(rows[i, :n].numpy().astype(np.float64), nums[i])
    r["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["resample_lengths_256x2000_18000_ratio0.6"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "physionet_bench.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--front-only", action="store_true")
    ap.add_argument("--resample", action="store_true")
    args = ap.parse_args()
    import torch
    from ecgmm import train_physionet as TP
    from ecgmm.hip import functional as HF
    from ecgmm.optim import FusedAdam
    from ecgmm.signal_model import FocalLoss, ResNet1D_SE
    assert torch.cuda.is_available(), "physionet_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda:0")
    if args.resample:
        res = resample_bench(torch, dev)
        out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "physionet_resample_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    res = {"rounds": ROUNDS, "calls_per_round": CALLS, "device": torch.cuda.get_device_name(0)}

    S, Ln = 8528, 3000
    g = torch.Generator().manual_seed(1)
    raw = torch.randn(S, Ln, generator=g).to(dev)
    r = with_floor(timed(lambda: TP.preprocess_signal(raw), torch), S * Ln * 8)
    r["records_per_s"] = round(S / r["ms_median"] * 1e3, 1)
    res["filter_zscore_8528x3000"] = r

    from ecgmm import preprocess as PP
    sig = torch.randn(256, 5000, generator=g).to(dev)
    r = with_floor(timed(lambda: PP.preprocess_signal(sig), torch), 256 * 5000 * 8)
    r["signals_per_s"] = round(256 / r["ms_median"] * 1e3, 1)
    res["preprocess_signal_256x5000"] = r
    if args.front_only:
        print(json.dumps(res))
        return

    src = TP.preprocess_signal(raw)
    HF.manual_seed(1)
    for B in (8, 256, 512):
        idx = torch.randperm(S, generator=g)[:B].to(dev)
        for aug in (False, True):
            r = with_floor(timed(lambda: TP.gather_augment(src, idx, augment=aug, check_index=False), torch), 2 * B * Ln * 4)
            res[f"gather_augment_B{B}_{'aug' if aug else 'plain'}"] = r

    for B in (8, 256, 512):
        labels = torch.randint(0, 2, (S,), generator=g)
        ds = TP.SignalOnlyDataset(np.arange(S), labels.numpy(), list(raw.cpu().numpy()), augment=True, split="train", device=dev)
        loader = TP.DeviceSignalLoader(ds, B, shuffle=True, generator=g, drop_last=True)
        model = ResNet1D_SE(num_classes=2, compute_dtype="bf16").to(dev).train()
        crit, opt = FocalLoss(1.0, 2.0), FusedAdam(model.parameters(), lr=1e-3)
        it = iter(loader)

        def step():
            nonlocal it
            try:
                signals, lab = next(it)
            except StopIteration:
                it = iter(loader)
                signals, lab = next(it)
            opt.zero_grad()
            loss = crit(model(signals.unsqueeze(1)), lab)
            loss.backward()
            opt.step()

        r = timed(step, torch)
        r["samples_per_s"] = round(B / r["ms_median"] * 1e3, 1)
        res[f"train_step_B{B}_bf16_loader_fed"] = r
        del ds, loader, model, opt

    if not args.skip_cpu:
        pre = cpu_baseline("pre", 64, args.cpus)
        aug = cpu_baseline("aug", 2000, args.cpus)
        res["cpu_reference"] = {"processes": args.cpus, "filtfilt_zscore_us_per_record": round(pre * 1e6, 2),
                                "augment_us_per_record": round(aug * 1e6, 3)}
        fz = res["filter_zscore_8528x3000"]
        fz["x_cpu_reference"] = round(pre * S * 1e3 / fz["ms_median"], 1)
        for B in (8, 256, 512):
            ga = res[f"gather_augment_B{B}_aug"]
            ga["x_cpu_reference"] = round(aug * B * 1e3 / ga["ms_median"], 1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
