"""SHAP path timings at D = 768, H = 128, C = 2, a background of N = 100 rows, nsamples = 200, for
B = 16 (the reference's loader batch) and B = 256: ecgmm_shap_gradient and ecgmm_shap_deep through hip/functional.py, timed
with device events on the stream after a warm-up, the median of --rounds calls each; the whole
``GradientExplainer.shap_values`` (host draws included) by wall clock; the same draws through the Python loop
``shap_fusion_modal_balance.expected_gradients`` as it stands; and the float64 restatement of tests/shap_ref.py on the CPU.
A record, not a gate.  Writes profiles/shap_bench.json and prints it as one line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

D, H, C, N, K = 768, 128, 2, 100, 200
BATCHES = (16, 256)


def timed(fn, torch, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def wall(fn, torch, rounds):
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_bench.json"))
    args = ap.parse_args()
    import torch
    from ecgmm import shap_explainers as SE
    from ecgmm import shap_fusion_modal_balance as X
    from ecgmm.config import Config
    from ecgmm.hip import functional as HF
    from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel
    from tests import shap_ref as R
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = type("C", (Config,), {"device": "cuda:0", "compute_dtype": "fp32"})
    model = ECGMultimodalModel(cfg).to(dev).eval()
    head = X.FusionClassifierWrapper(model.fusion_classifier)
    w1, b1, w2, _ = SE.mlp_weights(head)
    assert tuple(w1.shape) == (H, D) and w2.shape[0] == C
    res = {"shape": {"D": D, "H": H, "C": C, "N": N, "nsamples": K}, "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "batches": {}}
    for B in BATCHES:
        x, bg = (torch.from_numpy(a).to(dev) for a in R.make_inputs(B, N, D, H, C, seed=B)[:2])
        ridx, t = SE.draws_like_expected_gradients(0, K, B, N)
        rd, td = torch.from_numpy(ridx).to(dev), torch.from_numpy(t).to(dev)
        ex = SE.GradientExplainer(head, bg)
        r = {"shap_gradient_ms": timed(lambda: HF.shap_gradient(x, bg, rd, td, w1, b1, w2), torch, args.rounds),
             "shap_gradient_with_var_ms": timed(lambda: HF.shap_gradient(x, bg, rd, td, w1, b1, w2, want_var=True), torch,
                                                args.rounds),
             "shap_deep_ms": timed(lambda: HF.shap_deep(x, bg, w1, b1, w2), torch, args.rounds),
             "gradient_explainer_wall_ms": wall(lambda: ex.shap_values(x, nsamples=K, rseed=1), torch, 3),
             "gradient_explainer_given_draws_wall_ms": wall(lambda: ex.shap_values(x, draws=(ridx, t)), torch, 3)}
        t0 = time.perf_counter()
        SE.draws_like_shap(1, B, K, N)
        r["draws_like_shap_host_ms"] = (time.perf_counter() - t0) * 1e3
        # the Python loop on the same draws (seed 0 of its own generator), as it stands
        r["expected_gradients_python_loop_ms"] = wall(lambda: X.expected_gradients(head, bg, x, nsamples=K, seed=0), torch, 3)
        got = ex.shap_values(x, draws=(ridx, t))
        old = X.expected_gradients(head, bg, x, nsamples=K, seed=0).cpu().numpy()
        r["max_abs_difference_to_python_loop"] = float(np.abs(got - old).max())
        r["max_abs_value"] = float(np.abs(old).max())
        xn, bgn = x.cpu().numpy(), bg.cpu().numpy()
        wn = [a.cpu().numpy() for a in (w1, b1, w2)]
        t0 = time.perf_counter()
        R.expected_gradients(xn, bgn, ridx, t, *wn)
        r["cpu_float64_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        res["batches"][str(B)] = r
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
