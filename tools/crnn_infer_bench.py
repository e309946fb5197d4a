"""Eval-mode forward of the spectrogram CRNN: the training plan's eval mode against the inference plan
(ecgmm.inference.Predictor(CRNN)), same process, and the pieces of the front end per op.

Workload: B = 256, F = 33, T = 280 (a 9000-sample record), bf16 and fp32.

  whole forward   (a) model.eval() under torch.no_grad()       -- what train_physionet2's validation / test passes ran
                  (b) Predictor(model)                          -- folded front end, weights prepared once
                  (c) Predictor(model) with refresh() per call  -- what preparing once buys
  block 1         ecgmm_conv5_in1_relu_pool2  against  ecgmm_conv5_in1_fwd(stats = NULL) + ecgmm_relu_maxpool2
  front end       ecgmm_crnn_front_infer      against  ecgmm_crnn_front_forward(training = 0)

Method (as tools/infer_bench.py): warm-up calls of every variant first; then ROUNDS rounds, each timing every variant for
REPS consecutive calls between two events on the current stream (variants interleaved in one process, so clocks, allocator
state and the other tenants of the machine are shared); reported: the median over rounds of the per-call time and the
min / max of the rounds -- a difference has to exceed the round-to-round spread of the slower variant.  Cache state: warm
(the same input every call), as in a validation loop.  `front_share_of_a`: the front end's eval-path time over (a).

    python tools/crnn_infer_bench.py [--rounds 7] [--reps 10] [--out FILE.json]
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
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ecgmm.crnn import CRNN  # noqa: E402
from ecgmm.hip import lib as L  # noqa: E402
from ecgmm.hip.encoders import _table  # noqa: E402
from ecgmm.hip.functional import ptr, stream  # noqa: E402
from ecgmm.inference import Predictor  # noqa: E402

dev = torch.device("cuda:0")
B, FQ, T = args.batch, 33, 280


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


result = {}
for name in ("bf16", "fp32"):
    torch.manual_seed(0)
    net = CRNN(compute_dtype=name).to(dev).eval()
    with torch.no_grad():   # running statistics away from (0, 1), as after training
        for blk in (net.conv1, net.conv2, net.conv3):
            blk.block[1].running_mean.normal_(0, 0.2)
            blk.block[1].running_var.uniform_(0.5, 1.5)
    x = torch.randn(B, 1, FQ, T, device=dev)
    predict = Predictor(net)
    lib, dt, es = L.lib(), net._dtype, 2 if name == "bf16" else 4

    def a():
        with torch.no_grad():
            return net(x)

    # the lstm_dtype leg: the same weights with the BiLSTM's recurrence in bf16, in the same rounds
    net_l = CRNN(compute_dtype=name, lstm_dtype="bf16").to(dev).eval()
    net_l.load_state_dict(net.state_dict())
    predict_l = Predictor(net_l)

    def a_l():
        with torch.no_grad():
            return net_l(x)

    rec = measure({"a_eval": a, "b_predictor": lambda: predict(x), "c_refresh_each_call": lambda: predict.refresh()(x),
                   "a_eval_lstm_bf16": a_l, "b_predictor_lstm_bf16": lambda: predict_l(x)})
    rec["b_over_a"] = round(rec["b_predictor"]["ms"] / rec["a_eval"]["ms"], 4)
    rec["b_lstm_bf16_over_b"] = round(rec["b_predictor_lstm_bf16"]["ms"] / rec["b_predictor"]["ms"], 4)
    rec["lstm_bf16_logit_max_abs_diff"] = float((predict_l(x) - predict(x)).abs().max())
    del predict_l, net_l

    # ---- per op, same call: block 1 fused against its two-launch chain
    params, buffers = net._front_tables()
    w1, b1 = params[0], params[1]
    y = torch.empty(B * FQ * T * 32 * es, dtype=torch.uint8, device=dev)
    p_chain = torch.empty(B * (FQ // 2) * (T // 2) * 32 * es, dtype=torch.uint8, device=dev)
    p_fused = torch.empty_like(p_chain)

    def chain1():
        L.check(lib.ecgmm_conv5_in1_fwd(dt, ptr(x), ptr(w1), ptr(b1), ptr(y), None, B, FQ, T, stream()))
        L.check(lib.ecgmm_relu_maxpool2(dt, ptr(y), ptr(p_chain), B, FQ, T, 32, 0, stream()))

    def fused1():
        L.check(lib.ecgmm_conv5_in1_relu_pool2(dt, ptr(x), ptr(w1), ptr(b1), ptr(p_fused), B, FQ, T, stream()))

    ops = measure({"block1_chain": chain1, "block1_fused": fused1})
    assert torch.equal(p_chain, p_fused), "the fused block-1 kernel and its chain disagree"
    rec.update(ops)
    rec["block1_fused_over_chain"] = round(ops["block1_fused"]["ms"] / ops["block1_chain"]["ms"], 4)

    # ---- the front-end plans
    d = L.CRNNFrontDesc(B, FQ, T, dt, 0, 0.1, 1e-5)
    ws_eval = torch.empty(lib.ecgmm_crnn_front_fwd_workspace(C.byref(d)), dtype=torch.uint8, device=dev)
    ws_inf = torch.empty(lib.ecgmm_crnn_front_infer_workspace(C.byref(d)), dtype=torch.uint8, device=dev)
    blob = torch.empty(lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
    seq_eval = torch.empty(B, T // 8, 128 * (FQ // 8), device=dev)
    seq_inf = torch.empty_like(seq_eval)
    tp, tb = _table(params), _table(buffers)
    L.check(lib.ecgmm_crnn_front_infer_prepare(C.byref(d), tp, tb, ptr(blob), blob.numel(), stream()))

    def front_eval():
        L.check(lib.ecgmm_crnn_front_forward(C.byref(d), ptr(x), tp, tb, ptr(seq_eval), ptr(ws_eval), ws_eval.numel(), stream()))

    def front_infer():
        L.check(lib.ecgmm_crnn_front_infer(C.byref(d), ptr(x), ptr(blob), blob.numel(), ptr(seq_inf), ptr(ws_inf), ws_inf.numel(),
                                           stream()))

    plans = measure({"front_eval_plan": front_eval, "front_infer_plan": front_infer})
    rec.update(plans)
    rec["front_infer_over_eval"] = round(plans["front_infer_plan"]["ms"] / plans["front_eval_plan"]["ms"], 4)
    rec["front_share_of_a"] = round(plans["front_eval_plan"]["ms"] / rec["a_eval"]["ms"], 4)
    rec["front_max_abs_diff"] = float((seq_eval - seq_inf).abs().max())
    rec["workspace_bytes"] = {"eval": ws_eval.numel(), "infer": ws_inf.numel()}
    result[name] = rec
    print(name, json.dumps(rec))
    del predict, net, y, ws_eval
    torch.cuda.empty_cache()

line = json.dumps({"tool": "crnn_infer_bench", "B": B, "F": FQ, "T": T, "rounds": args.rounds, "reps": args.reps, **result})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
