"""LIME path timings: per explained sample, the three stages of ``explain_batch`` at D = 768, N = 1000,
B = 64 -- ecgmm_lime_perturb, the default predict_fn (fusion_classifier + softmax on the HIP ops) over the B * N perturbed
rows, ecgmm_lime_ridge (alpha = 1, all columns, one label) -- timed with device events on the stream after a warm-up, the
median of --rounds calls each; and the whole ``explain_batch`` by wall clock.  Beside it the float64 restatement of
tests/lime_ref.py (numpy bins + scipy.stats.truncnorm.ppf for the perturbation, the numpy ridge for the fit) on --cpus
processes of one BLAS / OpenMP thread, one sample each.  A record, not a gate.  Writes profiles/lime_bench.json and prints it as one line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

D, N, B = 768, 1000, 64


def background():
    rng = np.random.default_rng(1)
    return (rng.normal(size=(100, D)) * rng.uniform(0.2, 2.0, size=D)).astype(np.float32)


def _cpu_sample(seed):
    from ecgmm.lime_tabular import QuartileDiscretizer
    from tests import lime_ref as R
    bg = background()
    host = QuartileDiscretizer(bg).host_table()
    row = bg[seed % len(bg)]
    t0 = time.perf_counter()
    nn, ff = np.meshgrid(np.arange(N), np.arange(D), indexing="ij")
    ub, uv = R.perturb_uniforms(R.SEED, 0, seed, nn, ff)
    bins = R.draw_bins(ub, host["cdf"], host["nbins"])
    mean, std, lo, hi = (host["stats"][i][ff, bins].ravel() for i in range(4))
    inv, _ = R.truncnorm_value(uv.ravel(), mean, std, lo, hi)
    xb = np.array([np.searchsorted(host["qts"][f, :host["nbins"][f] - 1], row[f]) for f in range(D)])
    Z = (bins == xb).astype(np.float64)
    Z[0] = 1
    t1 = time.perf_counter()
    y = 1 / (1 + np.exp(-inv.reshape(N, D)[:, :8].sum(1)))
    R.explain(Z, (Z == 0).sum(1), y, 0.75 * np.sqrt(D), D)
    return t1 - t0, time.perf_counter() - t1


def _cpu_warm(_):
    from ecgmm.lime_tabular import QuartileDiscretizer  # noqa: F401
    from scipy.stats import truncnorm
    from tests import lime_ref  # noqa: F401
    return float(truncnorm.ppf(0.5, -1.0, 1.0))


def cpu_baseline(procs):
    import multiprocessing as mp
    # one BLAS / OpenMP thread per worker: `procs` workers share `procs` CPUs (the spawned children read the environment)
    pins = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS")
    saved = {k: os.environ.get(k) for k in pins}
    os.environ.update({k: "1" for k in pins})
    try:
        return _cpu_baseline(mp.get_context("spawn"), procs)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cpu_baseline(ctx, procs):
    with ctx.Pool(procs) as pool:
        pool.map(_cpu_warm, range(procs))          # process start-up and imports stay outside the timed region
        t0 = time.perf_counter()
        parts = pool.map(_cpu_sample, range(procs))
        wall = time.perf_counter() - t0
    return {"processes": procs, "threads_per_process": 1, "per_sample_s": wall / procs, "perturb_s_in_process": statistics.median(p[0] for p in parts),
            "ridge_s_in_process": statistics.median(p[1] for p in parts)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lime_bench.json"))
    args = ap.parse_args()
    import torch
    from ecgmm.config import Config
    from ecgmm.hip import functional as HF
    from ecgmm.lime_fusion_modal_balance import FusionClassifierWrapper, make_predict_fn
    from ecgmm.lime_tabular import LimeTabularExplainer
    from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = type("C", (Config,), {"device": "cuda:0", "compute_dtype": "fp32"})
    model = ECGMultimodalModel(cfg).to(dev).eval()
    predict_fn = make_predict_fn(FusionClassifierWrapper(model.fusion_classifier))
    bg = background()
    ex = LimeTabularExplainer(bg, random_state=1)
    rows = torch.from_numpy(bg[:B].copy()).to(dev)
    table = ex.discretizer.table(dev)
    Z, inverse, d2 = HF.lime_perturb(rows, table, N, seed_offset=(1, 0))
    probs = predict_fn(inverse.view(B * N, D))
    y = probs.view(B, N, 2)[:, :, 1:2].permute(0, 2, 1).contiguous()
    res = {"shape": {"D": D, "N": N, "B": B}, "device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    per = {"perturb": timed(lambda: HF.lime_perturb(rows, table, N, seed_offset=(1, 0)), torch, args.rounds),
           "predict": timed(lambda: predict_fn(inverse.view(B * N, D)), torch, args.rounds),
           "ridge": timed(lambda: HF.lime_ridge(Z, d2, y, ex.kernel_width, 1.0), torch, args.rounds)}
    res["per_sample_ms"] = {k: v / B for k, v in per.items()}
    res["per_sample_ms"]["sum"] = sum(per.values()) / B
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex.explain_batch(rows, predict_fn, num_features=D, num_samples=N)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    res["explain_batch_wall_ms_per_sample"] = min(walls[1:]) * 1e3 / B
    res["cpu_float64_restatement"] = cpu_baseline(args.cpus)
    res["cpu_over_gpu"] = res["cpu_float64_restatement"]["per_sample_s"] * 1e3 / res["explain_batch_wall_ms_per_sample"]
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
