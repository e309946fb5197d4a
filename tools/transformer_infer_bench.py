"""Eval-mode forward of ECGTransformer1D: the model's own forward under torch.no_grad() (the training composition of
ecgmm.hip.nn.TransformerEncoderLayer, nine launches per layer) against the inference plan
(ecgmm.inference.Predictor(ECGTransformer1D), four per layer), same process, and the two fused layer tails alone against the
ops they replace.

Shapes (DESIGN section 24's three), 2 layers, fp32:
    across      S = 8,    N = 3000, E = 128, heads 4, ff 256   the reference's attention across the batch (B = 8, L = 3000)
    time-3000   S = 3000, N = 8,    same widths               time_attention=True
    time-750    S = 750,  N = 32,   E = 64,  heads 4, ff 128   time_attention=True

  whole forward   (a) model.eval() under torch.no_grad()   -- what the validation / test passes ran
                  (b) Predictor(model)
  out_proj tail   ecgmm_linear_res_ln  against  ecgmm_linear_fwd + ecgmm_ew add + ecgmm_layernorm_fwd
  feed-forward    ecgmm_ffn_res_ln     against  ecgmm_linear_fwd(ReLU) + ecgmm_linear_fwd + ecgmm_ew add + ecgmm_layernorm_fwd

Method (as tools/crnn_infer_bench.py): warm-up calls of every variant first; then ROUNDS rounds, each timing every variant
for REPS consecutive calls between two events on the current stream (variants interleaved in one process); reported: the
median over rounds of the per-call time and the min / max of the rounds -- a difference has to exceed the round-to-round
spread of the slower variant.  Cache state: warm (the same input every call), as in a validation loop.
`launches`: library calls that launch kernels in one forward, counted by wrapping every entry of the ctypes table for one
call (no profiler); size queries and error lookups are not counted.

    python tools/transformer_infer_bench.py [--rounds 7] [--reps 10] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ecgmm.hip import lib as L  # noqa: E402
from ecgmm.hip.functional import ptr, stream  # noqa: E402
from ecgmm.inference import Predictor  # noqa: E402
from ecgmm.train_physionet import ECGTransformer1D  # noqa: E402

assert torch.cuda.is_available(), "transformer_infer_bench needs the GPU: a time taken elsewhere says nothing"
dev = torch.device("cuda:0")
SHAPES = {"across": dict(B=8, Ln=3000, E=128, heads=4, ff=256, time=False),
          "time-3000": dict(B=8, Ln=3000, E=128, heads=4, ff=256, time=True),
          "time-750": dict(B=32, Ln=750, E=64, heads=4, ff=128, time=True)}
NOT_LAUNCHES = ("_workspace", "_bytes", "_scratch", "_rows", "_last_error", "_version", "_len", "_lanes", "_frames", "_tile",
                "_switch_")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(variants):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(timed(fn, args.reps))
    return {k: {"ms": round(statistics.median(v), 4), "round_min_ms": round(min(v), 4), "round_max_ms": round(max(v), 4)}
            for k, v in rounds.items()}


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


result = {}
for tag, sh in SHAPES.items():
    B, Ln, E, heads, ff = sh["B"], sh["Ln"], sh["E"], sh["heads"], sh["ff"]
    R = B * Ln
    torch.manual_seed(0)
    net = ECGTransformer1D(seq_len=Ln, d_model=E, nhead=heads, num_layers=args.layers, dim_feedforward=ff,
                           time_attention=sh["time"]).to(dev).eval()
    with torch.no_grad():
        net.pos_embedding.normal_(0, 0.5)
    x = torch.randn(B, 1, Ln, device=dev)
    predict = Predictor(net)

    def a():
        with torch.no_grad():
            return net(x)

    b = lambda: predict(x)
    rec = measure({"a_eval": a, "b_predictor": b})
    rec["b_over_a"] = round(rec["b_predictor"]["ms"] / rec["a_eval"]["ms"], 4)
    la, lb = count_launches(a), count_launches(b)
    rec["launches"] = {"a_eval": sum(la.values()), "b_predictor_library_calls": sum(lb.values()),
                       "b_predictor_kernel_launches": 1 + 4 * args.layers + 3,
                       "a_eval_per_layer": (sum(la.values()) - 4) // args.layers, "b_predictor_per_layer": 4}
    rec["max_abs_diff_b_vs_a"] = float((a() - b()).abs().max())
    rec["workspace_bytes"] = predict.encoder.workspace_bytes(B, Ln)

    # ---- the two tails alone, on a layer's own weights
    lib, k = L.lib(), net.transformer_encoder.layers[0]
    g = lambda *s: torch.randn(*s, device=dev)
    att, cur = g(R, E), g(R, E)
    t1, t2, t3, hid = [torch.empty(R, E, device=dev) for _ in range(3)] + [torch.empty(R, ff, device=dev)]
    stat = torch.empty(R, 2, device=dev)
    fused1, fused2 = torch.empty(R, E, device=dev), torch.empty(R, E, device=dev)
    ow, ob = k.self_attn.out_proj.weight, k.self_attn.out_proj.bias
    seg, dims = (C.c_void_p * 3)(t2.data_ptr(), None, None), (C.c_int * 3)(E, 0, 0)

    def ln(gamma, beta, out):
        L.check(lib.ecgmm_layernorm_fwd(seg, dims, 1, None, ptr(gamma), ptr(beta), ptr(out), ptr(stat), None, R, k.norm1.eps, stream()))

    def tail1_chain():
        L.check(lib.ecgmm_linear_fwd(ptr(att), ptr(ow), ptr(ob), ptr(t1), R, E, E, L.ACT_NONE, stream()))
        L.check(lib.ecgmm_ew(7, ptr(cur), ptr(t1), ptr(t2), R * E, 0.0, stream()))
        ln(k.norm1.weight, k.norm1.bias, t3)

    def tail1_fused():
        L.check(lib.ecgmm_linear_res_ln(ptr(att), ptr(ow), ptr(ob), ptr(cur), ptr(k.norm1.weight), ptr(k.norm1.bias), ptr(fused1),
                                        R, E, E, k.norm1.eps, stream()))

    ops = measure({"linear_res_ln_chain": tail1_chain, "linear_res_ln_fused": tail1_fused})
    ops["linear_res_ln_max_abs_diff"] = float((t3 - fused1).abs().max())
    ops["linear_res_ln_fused_over_chain"] = round(ops["linear_res_ln_fused"]["ms"] / ops["linear_res_ln_chain"]["ms"], 4)
    rec.update(ops)

    def tail2_chain():
        L.check(lib.ecgmm_linear_fwd(ptr(cur), ptr(k.linear1.weight), ptr(k.linear1.bias), ptr(hid), R, E, ff, L.ACT_RELU, stream()))
        L.check(lib.ecgmm_linear_fwd(ptr(hid), ptr(k.linear2.weight), ptr(k.linear2.bias), ptr(t1), R, ff, E, L.ACT_NONE, stream()))
        L.check(lib.ecgmm_ew(7, ptr(cur), ptr(t1), ptr(t2), R * E, 0.0, stream()))
        ln(k.norm2.weight, k.norm2.bias, t3)

    def tail2_fused():
        L.check(lib.ecgmm_ffn_res_ln(ptr(cur), ptr(k.linear1.weight), ptr(k.linear1.bias), ptr(k.linear2.weight),
                                     ptr(k.linear2.bias), ptr(k.norm2.weight), ptr(k.norm2.bias), ptr(fused2), R, E, ff,
                                     k.norm2.eps, stream()))

    ops = measure({"ffn_res_ln_chain": tail2_chain, "ffn_res_ln_fused": tail2_fused})
    ops["ffn_res_ln_max_abs_diff"] = float((t3 - fused2).abs().max())
    ops["ffn_res_ln_fused_over_chain"] = round(ops["ffn_res_ln_fused"]["ms"] / ops["ffn_res_ln_chain"]["ms"], 4)
    rec.update(ops)
    result[tag] = {**{kk: vv for kk, vv in sh.items()}, **rec}
    print(tag, json.dumps(result[tag]))
    del predict, net
    torch.cuda.empty_cache()

line = json.dumps({"tool": "transformer_infer_bench", "layers": args.layers, "dtype": "fp32", "rounds": args.rounds,
                   "reps": args.reps, **result})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
