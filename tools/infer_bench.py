"""Eval-mode forward: the training plans' eval mode against the inference plans (ecgmm.inference.Predictor), same process.

  (a) model.eval() under torch.no_grad()          -- what every validation / test pass ran before
  (b) Predictor(model)                            -- BatchNorm-folded inference plans, weights prepared once
  (c) Predictor(model) with refresh() every call  -- what preparing once buys
  (b-side) as (b) with the ResNet18 downsample convolutions on the library's side stream (ecgmm_infer_down_side(1))

Two workloads, bf16: the multimodal model at batch 256 (224 x 224 image, L = 5000, 24 clinical columns) and the
image-only classifier at batch 128.  Method: warm-up calls of every variant first; then ROUNDS rounds, each timing every
variant for REPS consecutive calls between two events on the current stream (variants interleaved in one process, so
clocks, allocator state and the other tenants of the machine are shared); reported: the median over rounds of the
per-call time, and for (a) the min-max spread of its rounds -- the run-to-run spread any difference has to exceed.
Cache state: warm (the same inputs every call; weights and the workspace stay resident in the Infinity Cache where they
fit), as in a validation loop.

    python tools/infer_bench.py [--rounds 7] [--reps 10] [--out FILE.json]
    python tools/infer_bench.py --only a|b --calls 20      # one variant alone, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/infer_bench.py --only b --calls 20
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", choices=["a", "b"], default=None)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--workload", choices=["multimodal", "image_only", "both"], default="both")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ecgmm.config import Config  # noqa: E402
from ecgmm.hip import lib as L  # noqa: E402
from ecgmm.inference import Predictor  # noqa: E402
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel  # noqa: E402
from ecgmm.train_image_only import ImageOnlyClassifier  # noqa: E402
from oracle import fill  # noqa: E402

dev = torch.device("cuda:0")


def workloads():
    if args.workload in ("multimodal", "both"):
        net = ECGMultimodalModel(type("Cfg", (Config,), {"compute_dtype": "bf16", "clinical_input_dim": 24})).to(dev).eval()
        img, sig, clin, _ = (t.to(dev) for t in fill.synthetic_batch(256, clin_dim=24, salt=3))
        yield "multimodal_b256", net, (img, sig, clin), 256
    if args.workload in ("image_only", "both"):
        net = ImageOnlyClassifier(compute_dtype="bf16").to(dev).eval()
        img = fill.synthetic_batch(128, salt=4)[0].to(dev)
        yield "image_only_b128", net, (img,), 128


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


result = {}
for name, net, inputs, batch in workloads():
    predict = Predictor(net)
    lib = L.lib()

    def a():
        with torch.no_grad():
            return net(*inputs)

    def b():
        lib.ecgmm_infer_down_side(0)
        return predict(*inputs)

    def b_side():
        lib.ecgmm_infer_down_side(1)
        out = predict(*inputs)
        lib.ecgmm_infer_down_side(0)
        return out

    def c():
        lib.ecgmm_infer_down_side(0)
        return predict.refresh()(*inputs)

    if args.only:
        fn = a if args.only == "a" else b
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"workload": name, "variant": args.only, "calls": args.calls}))
        continue
    variants = {"a_eval": a, "b_predictor": b, "c_refresh_each_call": c, "b_down_side": b_side}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(timed(fn, args.reps))
    rec = {}
    for k, v in rounds.items():
        med = statistics.median(v)
        rec[k] = {"ms": round(med, 4), "samples_per_s": round(batch / med * 1e3, 1), "round_min_ms": round(min(v), 4),
                  "round_max_ms": round(max(v), 4)}
    rec["a_spread_ms"] = round(max(rounds["a_eval"]) - min(rounds["a_eval"]), 4)
    rec["b_over_a"] = round(rec["b_predictor"]["ms"] / rec["a_eval"]["ms"], 4)
    rec["batch"] = batch
    result[name] = rec
    print(name, json.dumps(rec))
    del predict, net
    torch.cuda.empty_cache()

if result:
    line = json.dumps({"tool": "infer_bench", "dtype": "bf16", "rounds": args.rounds, "reps": args.reps, **result})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
