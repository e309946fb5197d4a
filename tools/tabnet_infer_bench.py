"""Eval-mode forward of the TabNet clinical encoder: the module's own forward under torch.no_grad() (every op a launch
through a torch.autograd.Function) against the inference plan (ecgmm.inference.Predictor(ClinicalTabNetEncoder): one launch of
ecgmm_tabnet_infer on a folded blob), same process; and the multimodal TabNet Predictor with clinical_plan on and off.

  encoder       (a) module.eval() under torch.no_grad()       -- what Predictor ran for the clinical branch before the plan
                (b) the plan
                (c) the plan with refresh() before every call  (fold + forward: what forward_masks pays per call)
                at B in {8, 256, 4096} and D in {2, 16}, n_d = n_a = 32, 3 steps, 2 shared + 2 independent layers
  multimodal    Predictor(model, clinical_plan=True) against clinical_plan=False at batch 256 (224 x 224 pictures, 5000 samples)

Method (as tools/transformer_infer_bench.py): warm-up calls of every variant first; then ROUNDS rounds, each timing every
variant for REPS consecutive calls (variants interleaved in one process).  Two clocks per round:
  ms        between two events on the current stream, per call: what the stream was busy or waiting for
  host_ms   the host's wall time to ENQUEUE the calls (perf_counter around the loop, before the synchronize), per call
reported as the median over rounds with the min / max of the rounds -- a difference has to exceed the round-to-round spread of
the slower variant.  Cache state: warm (the same input every call), as in a validation loop.
`launches`: library calls that launch kernels in one forward, counted by wrapping every entry of the ctypes table for one call.

    python tools/tabnet_infer_bench.py [--rounds 7] [--reps 20] [--no-multimodal] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=256, help="batch of the multimodal run")
ap.add_argument("--no-multimodal", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ecgmm.config import Config  # noqa: E402
from ecgmm.hip import lib as L  # noqa: E402
from ecgmm.inference import Predictor  # noqa: E402
from ecgmm.multimodal import ECGMultimodalModel  # noqa: E402
from ecgmm.tabnet import ClinicalTabNetEncoder  # noqa: E402

assert torch.cuda.is_available(), "tabnet_infer_bench needs the GPU: a time taken elsewhere says nothing"
dev = torch.device("cuda:0")
NOT_LAUNCHES = ("_workspace", "_bytes", "_scratch", "_rows", "_last_error", "_version", "_len", "_lanes", "_frames", "_tile",
                "_switch_")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3 / reps
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host


def measure(variants, reps):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(timed(fn, reps))
    out = {}
    for k, v in rounds.items():
        d, h = [p[0] for p in v], [p[1] for p in v]
        out[k] = {"ms": round(statistics.median(d), 4), "round_min_ms": round(min(d), 4), "round_max_ms": round(max(d), 4),
                  "host_ms": round(statistics.median(h), 4), "host_round_min_ms": round(min(h), 4),
                  "host_round_max_ms": round(max(h), 4)}
    return out


def count_launches(fn):
    """library calls of one fn() that launch kernels: every entry of the ctypes table is wrapped for the one call"""
    lib, seen, saved = L.lib(), {}, {}
    for name in L.SIGNATURES:
        if any(s in name for s in NOT_LAUNCHES):
            continue
        real = getattr(lib, name)
        saved[name] = real
        setattr(lib, name, (lambda real, name: lambda *a: (seen.__setitem__(name, seen.get(name, 0) + 1), real(*a))[1])(real, name))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for name, real in saved.items():
            setattr(lib, name, real)
    return seen


def verdict(rec, a, b):
    """b is 'slower' only beyond a's own round-to-round spread"""
    rec["b_over_a"] = round(rec[b]["ms"] / rec[a]["ms"], 4)
    rec["b_over_a_host"] = round(rec[b]["host_ms"] / rec[a]["host_ms"], 4)
    rec["b_slower_beyond_a_spread"] = bool(rec[b]["ms"] > rec[a]["round_max_ms"])


result = {}
for D in (2, 16):
    torch.manual_seed(0)
    enc = ClinicalTabNetEncoder(D, 32).to(dev).eval()
    with torch.no_grad():      # running statistics as after training: not the identity
        for m in enc.modules():
            if getattr(m, "running_mean", None) is not None:
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.8, 1.2)
    predict = Predictor(enc)
    for B in (8, 256, 4096):
        x = torch.randn(B, D, device=dev)

        def a():
            with torch.no_grad():
                return enc(x)[0]

        b = lambda: predict(x)
        c = lambda: predict.refresh()(x)
        rec = measure({"a_eval": a, "b_plan": b, "c_plan_refresh": c}, args.reps)
        verdict(rec, "a_eval", "b_plan")
        rec["launches"] = {"a_eval": sum(count_launches(a).values()), "b_plan": sum(count_launches(b).values()),
                           "c_plan_refresh": sum(count_launches(c).values())}
        rec["max_abs_diff_b_vs_a"] = float((a() - b()).abs().max())
        rec["max_abs_a"] = float(a().abs().max())     # the scale of z: default-initialised TabNet weights give large outputs
        result["D%d_B%d" % (D, B)] = rec
        print("D%d_B%d" % (D, B), json.dumps(rec), flush=True)
    del predict, enc

if not args.no_multimodal:
    torch.manual_seed(0)
    cfg = type("Cfg", (Config,), {"compute_dtype": "bf16"})
    net = ECGMultimodalModel(cfg).to(dev).eval()
    Bm = args.batch
    xs = (torch.randn(Bm, 3, 224, 224, device=dev), torch.randn(Bm, 5000, device=dev), torch.randn(Bm, 2, device=dev))
    on, off = Predictor(net, clinical_plan=True), Predictor(net, clinical_plan=False)
    rec = measure({"a_clinical_module": lambda: off(*xs), "b_clinical_plan": lambda: on(*xs)}, max(2, args.reps // 4))
    verdict(rec, "a_clinical_module", "b_clinical_plan")
    rec["batch"], rec["compute_dtype"] = Bm, "bf16"
    rec["launches"] = {"a_clinical_module": sum(count_launches(lambda: off(*xs)).values()),
                       "b_clinical_plan": sum(count_launches(lambda: on(*xs)).values())}
    rec["max_abs_diff_logits"] = float((on(*xs)[3] - off(*xs)[3]).abs().max())
    result["multimodal"] = rec
    print("multimodal", json.dumps(rec), flush=True)

line = json.dumps({"tool": "tabnet_infer_bench", "rounds": args.rounds, "reps": args.reps, **result})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
