"""PTB-XL path timings: one process, device events on the stream, warm-up then 7 rounds x 10 calls,
medians of the per-call round means --
  (a) ecgmm_signal_preprocess_i16 on [2048][5000][12] int16 frames, lead II and all twelve leads: the C entry point with
      every operand on the device beforehand, next to its algorithmic bytes (the frames a launch has to touch + the fp32
      rows it writes), and the Python wrapper (which uploads gains and baselines and designs the filter per call),
  (b) the route composed from the entry points that existed before it: host decode of the lead to fp32, upload,
      ecgmm_signal_preprocess, slice -- its C entry point and its wrapper under the same protocol, and both routes end to
      end by wall clock (host array in, device rows out, three repeats),
  (c) weighted_sample at n = count = 13000,
  (d) one ResNet1D_SE training step at [16, 1, 2476] fed by the weighted loader,
and the reference's per-record numpy / scipy pipeline (train_signal_only_ptb.py:44-52) on --cpus processes as the baseline.
Writes profiles/ptbxl_bench.json and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.physionet_bench import timed  # noqa: E402

R, T, NSIG, LENGTH = 2048, 5000, 12, 2476


def _cpu_item(p_lead):
    from scipy.signal import butter, filtfilt
    x = p_lead[::2]
    x = x - np.convolve(x, np.ones(200) / 200, mode="same")
    b, a = butter(5, 40 / 125, btype="low")
    x = filtfilt(b, a, x)
    return x[:LENGTH].astype(np.float32)


def _cpu_chunk(args):
    n, seed = args
    d = np.random.RandomState(seed).randint(-2000, 2000, size=(n, T, NSIG)).astype(np.int16)
    t0 = time.perf_counter()
    for i in range(n):
        _cpu_item((d[i, :, 1] - 3) / 1000.0)       # the decode of one lead, then the reference's __getitem__
    return time.perf_counter() - t0


def cpu_baseline(n_per_proc, procs):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(_cpu_chunk, [(4, s) for s in range(procs)])
        t0 = time.perf_counter()
        pool.map(_cpu_chunk, [(n_per_proc, 100 + s) for s in range(procs)])
        wall = time.perf_counter() - t0
    return wall / (n_per_proc * procs)


def wall(fn, torch, repeats=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptbxl_bench.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from ecgmm import preprocess as PP
    from ecgmm import train_signal_only_ptb as TS
    from ecgmm.hip import functional as HF
    from ecgmm.hip import lib as L
    from ecgmm.hip.functional import ptr, stream
    from ecgmm.optim import FusedAdam
    from ecgmm.signal_model import FocalLoss, ResNet1D_SE
    assert torch.cuda.is_available(), "ptbxl_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda:0")
    res = {"rounds": 7, "calls_per_round": 10, "device": torch.cuda.get_device_name(0), "shape": [R, T, NSIG]}
    rng = np.random.RandomState(1)
    frames = rng.randint(-2000, 2000, size=(R, T, NSIG)).astype(np.int16)
    gain = rng.uniform(500.0, 1500.0, size=(R, NSIG))
    base = rng.randint(-50, 50, size=(R, NSIG))
    raw = torch.from_numpy(frames).to(dev)

    for name, leads in (("lead_II", [1]), ("twelve_leads", list(range(12)))):
        nc = len(leads)
        # the C entry point alone: gains, baselines and the output on the device, the filter designed, before the clock starts
        g_d = torch.from_numpy(np.ascontiguousarray(gain[:, leads])).to(dev)
        b_d = torch.from_numpy(np.ascontiguousarray(base[:, leads]).astype(np.int32)).to(dev)
        fb, fa = PP.butter_lowpass(5, 40 / 125)
        dbl = lambda v: (C.c_double * len(v))(*[float(t) for t in v])
        cb, ca, czi, chan = dbl(fb), dbl(fa), dbl(PP.lfilter_zi(fb, fa)), (C.c_int * nc)(*leads)
        out = torch.empty(R, nc, LENGTH, dtype=torch.float32, device=dev)
        fn = L.lib().ecgmm_signal_preprocess_i16

        def launch():
            L.check(fn(ptr(raw), R, T, NSIG, chan, nc, ptr(g_d), ptr(b_d), 2, ptr(out), LENGTH, 200, cb, ca, czi, 5, stream()))

        r = timed(launch, torch)
        rw = timed(lambda: PP.preprocess_i16(raw, leads, gain[:, leads], base[:, leads], step=2, out_len=LENGTH), torch)
        rw["note"] = "the Python wrapper: converts and uploads gains and baselines and designs the filter on every call"
        res[f"preprocess_i16_wrapper_{name}"] = rw
        # the frames the launch reads (2 bytes each; the cache lines behind them are more) + the fp32 rows
        r["algorithmic_bytes"] = R * nc * (T // 2) * 2 + R * nc * LENGTH * 4
        r["raw_payload_bytes"] = R * T * NSIG * 2
        r["achieved_GBps"] = round(r["algorithmic_bytes"] / r["ms_median"] / 1e6, 1)
        r["rows_per_s"] = round(R * nc / r["ms_median"] * 1e3, 1)
        res[f"preprocess_i16_{name}"] = r

        def decode():
            return ((frames[:, ::2, leads].astype(np.float32) - base[:, None, leads].astype(np.float32))
                    / gain[:, None, leads].astype(np.float32)).transpose(0, 2, 1).copy()

        x32 = torch.from_numpy(decode()).to(dev).reshape(R * nc, T // 2)
        y32 = torch.empty_like(x32)
        nb = L.lib().ecgmm_signal_preprocess_workspace(R * nc, T // 2, 5)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        fp = L.lib().ecgmm_signal_preprocess

        def launch32():
            L.check(fp(ptr(x32), ptr(y32), R * nc, T // 2, None, None, 200, cb, ca, czi, 5, ptr(ws), nb, stream()))

        r2 = timed(launch32, torch)
        r2["note"] = "the C entry point ecgmm_signal_preprocess alone on the decoded fp32 rows [R * nc, 2500], operands on the device"
        res[f"composed_launch_{name}"] = r2
        r3 = timed(lambda: PP.preprocess_signal(x32, cutoff=40, fs=250)[..., :LENGTH].contiguous(), torch)
        r3["note"] = "the Python wrapper of ecgmm_signal_preprocess on the decoded fp32 rows + slice"
        res[f"composed_wrapper_{name}"] = r3
        del y32, ws
        res[f"end_to_end_i16_{name}"] = wall(
            lambda: PP.preprocess_i16(torch.from_numpy(frames).to(dev), leads, gain[:, leads], base[:, leads], step=2,
                                      out_len=LENGTH), torch)
        res[f"end_to_end_composed_{name}"] = wall(
            lambda: PP.preprocess_signal(torch.from_numpy(decode()).to(dev), cutoff=40, fs=250)[..., :LENGTH].contiguous(), torch)
        del x32
    del raw

    n = 13000
    labels = (np.arange(n) % 10 == 0).astype(np.int64)
    sampler = TS.DeviceWeightedSampler(TS.class_weights(labels), n, device=dev)
    HF.manual_seed(1)
    r = timed(lambda: sampler.sample(), torch)
    r["draws_per_s"] = round(n / r["ms_median"] * 1e3, 1)
    res["weighted_sample_13000"] = r

    recs = [dict(frames=frames[i], gain=gain[i], baseline=base[i]) for i in range(1024)]
    ds = TS.PTBXLSignalDataset(recs, labels[:1024], device=dev)
    loader = TS.PTBXLLoader(ds, 16, sampler=TS.DeviceWeightedSampler(TS.class_weights(labels[:1024]), 1024, device=dev))
    model = ResNet1D_SE(compute_dtype="bf16").to(dev).train()
    crit, opt = FocalLoss(), FusedAdam(model.parameters(), lr=1e-3)
    it = iter(loader)

    def step():
        nonlocal it
        try:
            signals, lab = next(it)
        except StopIteration:
            it = iter(loader)
            signals, lab = next(it)
        opt.zero_grad()
        loss = crit(model(signals), lab)
        loss.backward()
        opt.step()

    r = timed(step, torch)
    r["samples_per_s"] = round(16 / r["ms_median"] * 1e3, 1)
    res["train_step_B16_bf16_loader_fed"] = r

    if not args.skip_cpu:
        per = cpu_baseline(32, args.cpus)
        res["cpu_reference"] = {"processes": args.cpus, "getitem_us_per_record": round(per * 1e6, 2)}
        res["preprocess_i16_lead_II"]["x_cpu_reference"] = round(per * R * 1e3 / res["preprocess_i16_lead_II"]["ms_median"], 1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
