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

--lengths adds the variable-length leg at the CRNN's shape on the challenge's longest record (T = 71 LSTM steps, B = 256):
a fixed seeded mix of 9 - 61 s records at 300 Hz (70 % of them 30 s, the rest uniform, one of 61 s), each cut to
clamp(stft_frames(samples) // 8, 1, T) steps.  Timed in the same rounds, alternating: the fixed entry; lengths all T;
the mix in drawn order; the mix sorted by descending length (what DeviceSpectrogramLoader hands over).  Next to the times
the two things they could follow: sum over the 16-row slices of the slice's longest row / (slices x T) -- the CU time of
the recurrence -- and max over the slices / T -- its duration when every slice has a CU of its own, as all 2 x 16 do at
B = 256.  The GEMMs around the recurrence run over all B T rows either way.

--dtype {fp32,bf16,both}: the recurrence's compute dtype (HN.LSTM(compute_dtype=...)).  `both` times the two
dtypes in one process on the same parameters and inputs, every round timing every variant of both in turn (so the dtypes
alternate inside each round); each bf16 variant then carries its ratio to the fp32 variant of the same rounds next to that
fp32 variant's own min-max spread, and a gain is claimed only where the gap exceeds the spread.  The fp32 legs are the
kernels of before there was a dtype, bit for bit.  Anything but the default fp32 writes profiles/lstm_bf16_bench.json.
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
ap.add_argument("--lengths", action="store_true", help="add the variable-length leg (T = 71, B = 256)")
ap.add_argument("--dtype", choices=("fp32", "bf16", "both"), default="fp32", help="compute dtype of the recurrence")
args = ap.parse_args()
DTYPES = ("fp32", "bf16") if args.dtype == "both" else (args.dtype,)
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


def record_steps(B, Tv, seed=2017):
    """LSTM steps of a seeded mix of 9 - 61 s records at 300 Hz, in drawn order"""
    import numpy as np

    from ecgmm.spectrogram import stft_frames
    rng = np.random.RandomState(seed)
    secs = np.where(rng.rand(B) < 0.7, 30.0, rng.uniform(9.0, 61.0, B))
    secs[rng.randint(B)] = 61.0
    return [min(max(stft_frames(int(round(sec * 300))) // 8, 1), Tv) for sec in secs]


def slice_figures(steps, Tv):
    tmax = [max(steps[i:i + 16]) for i in range(0, len(steps), 16)]
    return {"mean_steps": sum(steps) / len(steps), "sum_slice_tmax_over_slices_T": sum(tmax) / (len(tmax) * Tv),
            "max_slice_tmax_over_T": max(tmax) / Tv}


def main():
    torch.manual_seed(0)
    nets = {dt: HN.LSTM(IN, H, LAYERS, batch_first=True, bidirectional=True, compute_dtype=dt).to(dev) for dt in DTYPES}
    for dt in DTYPES[1:]:
        nets[dt].load_state_dict(nets[DTYPES[0]].state_dict())
    sfx = {dt: "" if args.dtype == "fp32" else "_" + dt for dt in DTYPES}
    variants = {}
    lengths_info, steps_of = {}, {}     # steps_of: the T of a variant that does not run at the module's T
    if args.lengths:
        B, Tv = 256, 71
        x = torch.randn(B, Tv, IN, device=dev)
        xg = x.clone().requires_grad_()
        gy = torch.randn(B, Tv, D * H, device=dev)
        mix = record_steps(B, Tv)
        legs = {"fixed": None, "all_T": [Tv] * B, "unsorted": mix, "sorted": sorted(mix, reverse=True)}
        for name, steps, dt in [(n, st, dt) for n, st in legs.items() for dt in DTYPES]:
            net = nets[dt]
            ln = None if steps is None else torch.tensor(steps, dtype=torch.int32, device=dev)
            if steps is not None:
                lengths_info[name] = slice_figures(steps, Tv)

            def fwd(x=x, ln=ln, net=net):
                with torch.no_grad():
                    net(x, lengths=ln)

            def fwd_bwd(xg=xg, gy=gy, ln=ln, net=net):
                HF.release_grads(net)
                y, _ = net(xg, lengths=ln)
                y.backward(gy)

            scale = Tv / T     # the FLOP / byte columns count all B T rows, as the fixed call does
            steps_of[f"t71_b256_{name}_fwd{sfx[dt]}"] = steps_of[f"t71_b256_{name}_fwd_bwd{sfx[dt]}"] = Tv
            variants[f"t71_b256_{name}_fwd{sfx[dt]}"] = (fwd, fwd_flops(B) * scale, l2_bytes(B, 1) * scale)
            variants[f"t71_b256_{name}_fwd_bwd{sfx[dt]}"] = (fwd_bwd, 3.0 * fwd_flops(B) * scale, l2_bytes(B, 2) * scale)
    for B in (8, 256):
        x = torch.randn(B, T, IN, device=dev)
        xg = x.clone().requires_grad_()
        gy = torch.randn(B, T, D * H, device=dev)

        for dt in DTYPES:
            def fwd(x=x, net=nets[dt]):
                with torch.no_grad():
                    net(x)

            def fwd_bwd(xg=xg, gy=gy, net=nets[dt]):
                HF.release_grads(net)
                y, _ = net(xg)
                y.backward(gy)

            variants[f"b{B}_fwd{sfx[dt]}"] = (fwd, fwd_flops(B), l2_bytes(B, 1))
            variants[f"b{B}_fwd_bwd{sfx[dt]}"] = (fwd_bwd, 3.0 * fwd_flops(B), l2_bytes(B, 2))
    for fn, _, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, _, _) in variants.items():
            rounds[k].append(timed(fn, args.reps))
    res = {"shape": {"In": IN, "H": H, "layers": LAYERS, "bidirectional": True, "T": T,
                     "note": "T of the b8_* / b256_* variants; every variant records its own T"}, "rounds": args.rounds,
           "reps": args.reps, "peak_f32_mfma_tflops": PEAK_F32 / 1e12, "dtype": args.dtype, "variants": {}}
    if args.lengths:
        res["lengths_leg"] = {"B": 256, "T": 71, "mix": "seed 2017: 70 % 30 s, 30 % uniform 9 - 61 s, one 61 s; 300 Hz",
                              "slices": lengths_info}
    for k, (fn, flops, l2) in variants.items():
        ms = statistics.median(rounds[k])
        res["variants"][k] = {"T": steps_of.get(k, T), "ms_median": ms, "ms_min": min(rounds[k]), "ms_max": max(rounds[k]), "gflop": flops / 1e9,
                              "fraction_of_f32_mfma_peak": flops / (ms * 1e-3) / PEAK_F32,
                              "recurrence_l2_gbytes": l2 / 1e9, "recurrence_l2_tbytes_per_s": l2 / (ms * 1e-3) / 1e12}
        v = res["variants"][k]
        print(f"{k:24s} {ms:9.3f} ms (rounds {v['ms_min']:.3f} .. {v['ms_max']:.3f})  {v['gflop']:8.1f} GFLOP = "
              f"{100 * v['fraction_of_f32_mfma_peak']:.2f} % of the f32 MFMA peak;  W_hh from L2 {v['recurrence_l2_gbytes']:.2f} GB")
    if args.dtype == "both":   # each bf16 variant against the fp32 variant of the same rounds, whose own spread is the yardstick
        for k in [k for k in res["variants"] if k.endswith("_bf16")]:
            v, base = res["variants"][k], res["variants"][k[:-5] + "_fp32"]
            spread = (base["ms_max"] - base["ms_min"]) / base["ms_median"]
            v["ratio_to_fp32"], v["fp32_rounds_spread"] = v["ms_median"] / base["ms_median"], spread
            v["gap_exceeds_fp32_spread"] = bool(v["ms_max"] < base["ms_min"] or v["ms_min"] > base["ms_max"])
            print(f"{k}: {v['ratio_to_fp32']:.3f} x the fp32 leg (whose rounds spread {100 * spread:.1f} %); "
                  f"ranges {'disjoint' if v['gap_exceeds_fp32_spread'] else 'overlap'}")
    if args.lengths and args.dtype == "fp32":   # each leg against the fixed entry of the same rounds; its own spread next to it
        for kind in ("fwd", "fwd_bwd"):
            base = res["variants"][f"t71_b256_fixed_{kind}"]
            spread = (base["ms_max"] - base["ms_min"]) / base["ms_median"]
            for name in ("all_T", "unsorted", "sorted"):
                v = res["variants"][f"t71_b256_{name}_{kind}"]
                v["ratio_to_fixed"] = v["ms_median"] / base["ms_median"]
                print(f"t71_b256_{name}_{kind}: {v['ratio_to_fixed']:.3f} x the fixed entry (whose rounds spread {100 * spread:.1f} %)")
            base["rounds_spread"] = spread
    out = args.out or os.path.join(ROOT, "profiles", "lstm_bench.json" if args.dtype == "fp32" else "lstm_bf16_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"lstm_bench": out}))


if __name__ == "__main__":
    main()
