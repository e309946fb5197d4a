"""The Transformer encoder layer of train_physionet.py:219 on ecgmm.hip.nn: the attention kernels alone (forward, and
forward + backward, csrc/attention.hip) and one whole post-norm encoder layer forward + backward, at three shapes:

    ref_as_written   S = 8,    N = 3000, E = 128, 4 heads, batch_first = False   the reference as written: it attends across
                                                                                 its batch of 8, the 3000 positions are N
    bf_3000          S = 3000, N = 8,    E = 128, 4 heads, batch_first = True    the same tensor read the intended way
    bf_750           S = 750,  N = 32,   E = 64,  4 heads, batch_first = True    the commented-out signal encoder's regime

Beside ours: torch's own nn.TransformerEncoderLayer (fp32, dropout 0, train mode) on the same inputs and weights, forward +
backward, and torch's scaled_dot_product_attention forward + backward on the same q, k, v.  The torch figures are the
yardstick; they are reported, not asserted.

Method (as tools/lstm_bench.py): one process; warm-up calls of every variant first; then ROUNDS rounds, each timing every
variant for REPS consecutive calls between two events on the current stream; reported: the median over rounds of the
per-call time and the min-max spread of the rounds.  Cache state: warm (same inputs and weights every call).  Attention
FLOPs: forward 4 S^2 d per (n, head); backward 10 S^2 d (the two passes recompute the scores: 2 x (QK^T, dO V^T) + dV, dK,
dQ), over the exact-f32 MFMA peak of DESIGN section 4.1 (157.3 TFLOP/s).

    python tools/transformer_bench.py [--rounds 7] [--reps 10] [--out profiles/transformer_bench.json]

--lengths: the same three measurements of OURS at bf_3000 and bf_750 with one length per attention-batch element, drawn
uniformly from [S / 4, S] under a fixed seed, as drawn ("unsorted") and in descending order ("sorted"), beside the all-full run
without lengths of the same process ("full").  Reported with them: sum(len^2) / (N S^2), the share of the score tiles that
hold a live (query, key) pair, which the attention time should follow; the layer also keeps its projections, LayerNorms and
feed-forward over all rows.  Default output profiles/transformer_bench_lengths.json.

--maps: at bf_3000 and bf_750, the head-averaged attention map (ecgmm_mha_weights, 4 N S^2 bytes written) and one rollout step
(ecgmm_mha_rollout_step) from the qkv and the lse of a forward, beside the attention forward of the same process.  Both redo
the forward's QK^T half and its exponentials (2 S^2 d FLOPs per (n, head)).  Default output profiles/transformer_bench_maps.json.
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
ap.add_argument("--lengths", action="store_true", help="time the kernels with per-element lengths (see the module docstring)")
ap.add_argument("--maps", action="store_true", help="time the attention maps and the rollout step (see the module docstring)")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from ecgmm.hip import functional as HF  # noqa: E402
from ecgmm.hip import nn as HN  # noqa: E402

dev = torch.device("cuda:0")
PEAK_F32 = 157.3e12
SHAPES = {"ref_as_written": (8, 3000, 128, 4, 256, False), "bf_3000": (3000, 8, 128, 4, 256, True),
          "bf_750": (750, 32, 64, 4, 128, True)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def lengths_variants():
    """{name: (fn, flops or None)} and {shape: description of its lengths} for --lengths"""
    variants, drawn = {}, {}
    gen = torch.Generator().manual_seed(20170)
    for name in ("bf_3000", "bf_750"):
        S, N, E, heads, ff, bf = SHAPES[name]
        d = E // heads
        ours = HN.TransformerEncoderLayer(E, heads, ff, dropout=0.0, batch_first=bf).to(dev).train()
        x = torch.randn(N, S, E, device=dev)
        gy = torch.randn(N, S, E, device=dev)
        qkv = torch.randn(S * N, 3 * E, device=dev)
        ga = torch.randn(S * N, E, device=dev)
        unsorted = torch.randint(S // 4, S + 1, (N,), generator=gen, dtype=torch.int32)
        share = float((unsorted.double() ** 2).sum() / (N * float(S) ** 2))
        drawn[name] = {"lengths": unsorted.tolist(), "work_share_sum_len2_over_N_S2": share}
        full_flops = 4.0 * S * S * d * N * heads
        for tag, ln in (("full", None), ("unsorted", unsorted.to(dev)),
                        ("sorted", torch.sort(unsorted, descending=True).values.to(dev))):
            flops = full_flops * (1.0 if ln is None else share)

            def attn_fwd(qkv=qkv, S=S, N=N, heads=heads, ln=ln):
                with torch.no_grad():
                    HF.multi_head_attention(qkv, S, N, heads, True, lengths=ln)

            def attn_fwd_bwd(qkv=qkv, ga=ga, S=S, N=N, heads=heads, ln=ln):
                t = qkv.detach().requires_grad_()
                HF.multi_head_attention(t, S, N, heads, True, lengths=ln).backward(ga)

            def layer(ours=ours, x=x, gy=gy, ln=ln):
                HF.release_grads(ours)
                t = x.detach().requires_grad_()
                (ours(t) if ln is None else ours(t, lengths=ln)).backward(gy)

            variants[f"{name}/{tag}/attention_fwd"] = (attn_fwd, flops)
            variants[f"{name}/{tag}/attention_fwd_bwd"] = (attn_fwd_bwd, 3.5 * flops)
            variants[f"{name}/{tag}/layer_fwd_bwd"] = (layer, None)
    return variants, drawn


def maps_variants():
    """{name: (fn, flops)} for --maps"""
    variants = {}
    for name in ("bf_3000", "bf_750"):
        S, N, E, heads, _ff, bf = SHAPES[name]
        qkv = torch.randn(S * N, 3 * E, device=dev)
        v = torch.full((N, S), 1.0 / S, device=dev)
        with torch.no_grad():
            _, lse = HF.multi_head_attention(qkv, S, N, heads, bf, return_lse=True)
        flops = 4.0 * S * S * (E // heads) * N * heads

        def attn_fwd(qkv=qkv, S=S, N=N, heads=heads, bf=bf):
            with torch.no_grad():
                HF.multi_head_attention(qkv, S, N, heads, bf)

        def weights(qkv=qkv, lse=lse, S=S, N=N, heads=heads, bf=bf):
            HF.attention_weights(qkv, lse, S, N, heads, bf)

        def step(qkv=qkv, lse=lse, v=v, S=S, N=N, heads=heads, bf=bf):
            HF.attention_rollout_step(qkv, lse, v, S, N, heads, bf)

        variants[name + "/attention_fwd"] = (attn_fwd, flops)
        variants[name + "/weights_averaged"] = (weights, flops / 2)
        variants[name + "/rollout_step"] = (step, flops / 2)
    return variants


def main():
    torch.manual_seed(0)
    variants, drawn = lengths_variants() if args.lengths else ({}, None)
    if args.maps:
        variants = maps_variants()
    for name, (S, N, E, heads, ff, bf) in ({} if args.lengths or args.maps else SHAPES).items():
        d = E // heads
        ours = HN.TransformerEncoderLayer(E, heads, ff, dropout=0.0, batch_first=bf).to(dev).train()
        ref = nn.TransformerEncoderLayer(E, heads, ff, dropout=0.0, batch_first=bf).to(dev).train()
        ref.load_state_dict(ours.state_dict(), strict=True)
        shape = (N, S, E) if bf else (S, N, E)
        x = torch.randn(shape, device=dev)
        gy = torch.randn(shape, device=dev)
        qkv = torch.randn(S * N, 3 * E, device=dev)
        ga = torch.randn(S * N, E, device=dev)
        q, k, v = (torch.randn(N, heads, S, d, device=dev, requires_grad=True) for _ in range(3))
        go = torch.randn(N, heads, S, d, device=dev)
        flops = 4.0 * S * S * d * N * heads

        def attn_fwd(qkv=qkv, S=S, N=N, heads=heads, bf=bf):
            with torch.no_grad():
                HF.multi_head_attention(qkv, S, N, heads, bf)

        def attn_fwd_bwd(qkv=qkv, ga=ga, S=S, N=N, heads=heads, bf=bf):
            t = qkv.detach().requires_grad_()
            HF.multi_head_attention(t, S, N, heads, bf).backward(ga)

        def layer(ours=ours, x=x, gy=gy):
            HF.release_grads(ours)
            ours(x.detach().requires_grad_()).backward(gy)

        def torch_layer(ref=ref, x=x, gy=gy):
            ref.zero_grad(set_to_none=True)
            ref(x.detach().requires_grad_()).backward(gy)

        def torch_sdpa(q=q, k=k, v=v, go=go):
            q.grad = k.grad = v.grad = None
            nn.functional.scaled_dot_product_attention(q, k, v).backward(go)

        variants[name + "/attention_fwd"] = (attn_fwd, flops)
        variants[name + "/attention_fwd_bwd"] = (attn_fwd_bwd, 3.5 * flops)
        variants[name + "/layer_fwd_bwd"] = (layer, None)
        variants[name + "/torch_layer_fwd_bwd"] = (torch_layer, None)
        variants[name + "/torch_sdpa_fwd_bwd"] = (torch_sdpa, None)
    for fn, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, _) in variants.items():
            rounds[k].append(timed(fn, args.reps))
    res = {"shapes": {k: dict(zip(("S", "N", "E", "heads", "dim_feedforward", "batch_first"), v)) for k, v in SHAPES.items()},
           "rounds": args.rounds, "reps": args.reps, "peak_f32_mfma_tflops": PEAK_F32 / 1e12, "variants": {}}
    if drawn is not None:
        res["lengths"] = drawn
        for name, dsc in drawn.items():
            print(f"{name}: sum(len^2) / (N S^2) = {dsc['work_share_sum_len2_over_N_S2']:.4f}", flush=True)
    for k, (fn, flops) in variants.items():
        ms = statistics.median(rounds[k])
        v = res["variants"][k] = {"ms_median": ms, "ms_min": min(rounds[k]), "ms_max": max(rounds[k])}
        line = f"{k:38s} {ms:9.3f} ms (rounds {v['ms_min']:.3f} .. {v['ms_max']:.3f})"
        if flops:
            v["gflop"] = flops / 1e9
            v["fraction_of_f32_mfma_peak"] = flops / (ms * 1e-3) / PEAK_F32
            line += f"  {v['gflop']:8.2f} GFLOP = {100 * v['fraction_of_f32_mfma_peak']:.2f} % of the f32 MFMA peak"
        print(line, flush=True)
    if args.maps:   # each over the attention forward of the same shape
        for k, v in res["variants"].items():
            name, what = k.split("/")
            if what != "attention_fwd":
                v["time_over_attention_fwd"] = v["ms_median"] / res["variants"][name + "/attention_fwd"]["ms_median"]
                print(f"{k:38s} {v['time_over_attention_fwd']:.3f} of the attention forward's time", flush=True)
    if drawn is not None:   # each lengths run over the full run of the same shape
        for k, v in res["variants"].items():
            name, tag, what = k.split("/")
            if tag != "full":
                v["time_over_full"] = v["ms_median"] / res["variants"][f"{name}/full/{what}"]["ms_median"]
                print(f"{k:38s} {v['time_over_full']:.3f} of the full run's time", flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "transformer_bench_maps.json" if args.maps else
                                   "transformer_bench_lengths.json" if args.lengths else "transformer_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"transformer_bench": out}))


if __name__ == "__main__":
    main()
