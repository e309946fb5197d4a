"""References for the bf16 recurrence of the native LSTM (csrc/lstm.hip: lstm_seq_fwd_bf16_kernel / lstm_seq_bwd_bf16_kernel).

Contract (include/ecgmm.h): only the recurrent operands are rounded, to nearest even --
    pre_t = P_t + b_hh + bf(h_{t-1}) bf(W_hh)^T          dh_{t-1} = dy_{t-1} + bf(dgates_t) bf(W_hh)
-- products exact, sums fp32; everything stored (y, h_n, c_n, dgates, the gradients) is unrounded fp32.

Rounding is discontinuous: an fp32-sized difference in h can flip a rounding and move that operand by 2^-8 relative, so a
free-running float64 chain with its own roundings cannot be held to an fp32 bar.  The reference here is OPERAND-FORCED, in the
spirit of tests/plan_replay.py: the float64 chain takes as the recurrent operand of step t the rounding of the KERNEL's own
stored fp32 value (y[t -+ 1], or h0 at a row's first step; dgates[t] in the backward's dh carry), and everything else is its
own float64 carry.  Deviations are then fp32-accumulation-sized and continuous, and f64check's per-slice chain rule applies:
every slice m_t <= CHAIN_MARGIN * max(u, max_t m_t(own32)), own32 being the same forced reference evaluated in float32.

chain(...) is the one implementation: forced (forward operands from `y`, backward operands from `dgates`) in any dtype, or
free-running (emulate: a CPU fp32 step-by-step model of the kernel, the kernel's stand-in in the CPU tests and the
quantisation yardstick of tests/test_lstm_bf16_gpu.py), with the slips a kernel could make switched on by name.
One layer, one or both directions, fixed or variable lengths (masked hold, as tests/lstm_varlen_ref.py describes it)."""
import copy

import torch

from . import f64check as fc

SLIPS = ("w_unrounded", "y_rounded", "c_rounded", "truncate", "kpad", "gate_swap", "dgates_rounded", "dead_carry")


def bf(t):
    """round-to-nearest-even to bf16, returned as fp32: integer arithmetic on the fp32 bit patterns (NaN stays NaN)"""
    t = t.detach().to(torch.float32).contiguous()
    x = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (x + 0x7FFF + ((x >> 16) & 1)) & 0xFFFF0000
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32).view(torch.float32)
    return torch.where(torch.isnan(t), t, r)


def trunc(t):
    """the slip: the low 16 bits dropped"""
    t = t.detach().to(torch.float32).contiguous()
    return (t.view(torch.int32) & -65536).view(torch.float32)


def ident(t):
    """rounding switched off: the value in its own dtype"""
    return t.detach()


def _tb(t, batch_first):
    return t.movedim(1, 0) if batch_first else t


def params_of(mod, k):
    sfx = "_l0" + ("_reverse" if k else "")
    return [getattr(mod, n + sfx).detach() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def chain(ins, lengths=None, use=("y", "h", "c"), dtype=torch.float64, y=None, dgates=None, rnd=bf, slip=None,
          backward=True):
    """The one-layer LSTM of `ins` = (torch module, x, h0, c0, gy, gh, gc), step by step in `dtype`, operands rounded by `rnd`.
    y given: the forward's recurrent operand is rnd(y[t -+ 1]) (forced); None: the chain's own h.  dgates (one tensor per
    direction, rows as x, 4H wide) given: the dh carry is rnd(dgates[t]) rnd(W_hh) (forced); None: the chain's own.
    Returns the tensors as f64check.lstm_run names them, plus "dgates0" / "dgates1"."""
    assert slip is None or slip in SLIPS, slip
    mod, x, h0, c0, gy, gh, gc = ins
    assert mod.num_layers == 1
    H, D, bfst = mod.hidden_size, (2 if mod.bidirectional else 1), mod.batch_first
    xs = _tb(x.detach(), bfst).to(dtype)
    T, B, In = xs.shape
    yk = None if y is None else _tb(y.detach().cpu().float(), bfst)
    Ln = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.as_tensor(lengths).long().cpu().clamp(0, T)
    rnd_op = trunc if slip == "truncate" else rnd
    rnd_w = ident if slip == "w_unrounded" else rnd
    out = {"y": torch.zeros(T, B, D * H, dtype=dtype), "hn": torch.zeros(D, B, H, dtype=dtype),
           "cn": torch.zeros(D, B, H, dtype=dtype), "dx": torch.zeros(T, B, In, dtype=dtype)}
    if h0 is not None:
        out["dh0"], out["dc0"] = torch.zeros(D, B, H, dtype=dtype), torch.zeros(D, B, H, dtype=dtype)
    gys = _tb(gy, bfst).to(dtype)
    for k in range(D):
        sfx = "_l0" + ("_reverse" if k else "")
        w_ih, w_hh, b_ih, b_hh = params_of(mod, k)
        Wb = rnd_w(w_hh).to(dtype)
        P = xs @ w_ih.to(dtype).t() + b_ih.to(dtype)
        h0k = torch.zeros(B, H) if h0 is None else h0[k].detach().float()
        h = h0k.to(dtype)
        c = torch.zeros(B, H, dtype=dtype) if c0 is None else c0[k].detach().to(dtype)
        gates, cs, cprev, hprev = (torch.zeros(T, B, n, dtype=dtype) for n in (4 * H, H, H, H))
        order = list(range(T)) if k == 0 else list(range(T - 1, -1, -1))
        for t in order:
            lm = (t < Ln)[:, None]
            tp = t - 1 if k == 0 else t + 1
            first = ((Ln * 0 + t) == 0 if k == 0 else t == Ln - 1)[:, None]
            if yk is None:
                op = h
            else:
                prev = yk[tp][:, k * H:(k + 1) * H] if 0 <= tp < T else torch.zeros(B, H)
                op = torch.where(first, h0k, prev)
            pre = P[t] + b_hh.to(dtype) + rnd_op(op).to(dtype) @ Wb.t()
            if slip == "kpad":   # a padding column of h times a padding column of W_hh, both 2^-6 instead of 0
                pre = pre + 2.0 ** -12
            i, f, g, o = (torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]),
                          torch.sigmoid(pre[:, 3 * H:]))
            cnew = f * c + i * g
            if slip == "c_rounded":
                cnew = bf(cnew).to(dtype)
            hnew = o * torch.tanh(cnew)
            hprev[t], cprev[t] = h, c
            gates[t] = torch.where(lm, torch.cat([i, f, g, o], 1), torch.zeros((), dtype=dtype))
            c, h = torch.where(lm, cnew, c), torch.where(lm, hnew, h)
            cs[t] = c
            ystore = bf(hnew).to(dtype) if slip == "y_rounded" else hnew
            out["y"][t, :, k * H:(k + 1) * H] = torch.where(lm, ystore, torch.zeros((), dtype=dtype))
        out["hn"][k], out["cn"][k] = h, c
        if not backward:
            continue
        dgk = None if dgates is None else _tb(dgates[k].detach().cpu().float().reshape(x.shape[0], x.shape[1], 4 * H), bfst)
        Wt = Wb
        if slip == "gate_swap":   # the transposed operand with the f and g blocks exchanged
            Wt = torch.cat([Wb[:H], Wb[2 * H:3 * H], Wb[H:2 * H], Wb[3 * H:]], 0)
        dhc = gh[k].to(dtype) if "h" in use else torch.zeros(B, H, dtype=dtype)
        dc = gc[k].to(dtype) if "c" in use else torch.zeros(B, H, dtype=dtype)
        dg_all = torch.zeros(T, B, 4 * H, dtype=dtype)
        for t in reversed(order):
            lm = (t < Ln)[:, None]
            dh = (gys[t][:, k * H:(k + 1) * H] if "y" in use else 0) + dhc
            i, f, g, o = gates[t][:, :H], gates[t][:, H:2 * H], gates[t][:, 2 * H:3 * H], gates[t][:, 3 * H:]
            tc = torch.tanh(cs[t])
            dcx = dh * o * (1 - tc * tc) + dc
            dgt = torch.cat([dcx * g * i * (1 - i), dcx * cprev[t] * f * (1 - f), dcx * i * (1 - g * g),
                             dh * tc * o * (1 - o)], 1)
            dgt = torch.where(lm, dgt, torch.zeros((), dtype=dtype))
            dc = torch.where(lm, dcx * f, dc)
            src = dgt if dgk is None else dgk[t]
            carry = rnd_op(src).to(dtype) @ Wt
            dhc = carry if slip == "dead_carry" else torch.where(lm, carry, dhc)
            dg_all[t] = bf(dgt).to(dtype) if slip == "dgates_rounded" else dgt
        if h0 is not None:
            out["dh0"][k], out["dc0"][k] = dhc, dc
        flat = dg_all.reshape(T * B, 4 * H)
        out["dweight_ih" + sfx] = flat.t() @ xs.reshape(T * B, In)
        out["dweight_hh" + sfx] = flat.t() @ hprev.reshape(T * B, H)
        out["dbias_ih" + sfx] = flat.sum(0)
        out["dbias_hh" + sfx] = flat.sum(0)
        out["dx"] += dg_all @ w_ih.to(dtype)
        out["dgates%d" % k] = dg_all.movedim(0, 1) if bfst else dg_all
    if not backward:
        del out["dx"]
        out.pop("dh0", None), out.pop("dc0", None)
    for key in ("y", "dx"):
        if key in out and bfst:
            out[key] = out[key].movedim(0, 1)
    return {k_: v.contiguous() for k_, v in out.items()}


def forced_forward(ins, y_kernel, lengths=None, dtype=torch.float64):
    return chain(ins, lengths, dtype=dtype, y=y_kernel, backward=False)


def forced_backward(ins, y_kernel, dgates_kernel, lengths=None, use=("y", "h", "c"), dtype=torch.float64):
    """forward and backward, both forced (the backward reads the forced forward's own float64 saved tensors)"""
    return chain(ins, lengths, use, dtype, y=y_kernel, dgates=dgates_kernel)


def emulate(ins, lengths=None, use=("y", "h", "c"), slip=None, backward=True, rnd=bf):
    """CPU fp32 step-by-step model of the kernels (free-running); rnd=ident: the unquantised LSTM"""
    return {k: v.float() for k, v in chain(ins, lengths, use, torch.float32, rnd=rnd, slip=slip, backward=backward).items()}


def slice_dim(key, batch_first):
    if key.startswith("dgates"):
        return 1 if batch_first else 0
    return fc.lstm_slice_dim(key, batch_first)


def check_forced(out, ins, lengths=None, use=("y", "h", "c"), name="lstm bf16", backward=True, quiet=True):
    """every tensor of `out` (a kernel's, or emulate's) against the operand-forced float64 chain, per slice, at f64check's
    chain bar with the forced float32 chain as the yardstick.  out["dgates0" / "dgates1"] are needed with backward=True.
    Raises AssertionError naming the tensor; returns the worst Report."""
    mod = ins[0]
    D = 2 if mod.bidirectional else 1
    dg = [out["dgates%d" % k] for k in range(D)] if backward else None
    r64 = chain(ins, lengths, use, torch.float64, y=out["y"], dgates=dg, backward=backward)
    r32 = chain(ins, lengths, use, torch.float32, y=out["y"], dgates=dg, backward=backward)
    worst = None
    for k in r64:
        got = out[k].detach().cpu().reshape(r64[k].shape)
        r = fc.seq_chain_check(got, r64[k], r32[k].double(), slice_dim(k, mod.batch_first), name + " " + k, quiet)
        if worst is None or r.ratio >= worst.ratio:
            worst = r
    print("[lstm bf16] %-34s worst %.3g = %.1f u (%s, slice %s), ratio to its bar %.3g" %
          (name, worst.kernel, worst.kernel / fc.U, worst.name.split()[-1], worst.where, worst.ratio))
    return worst


def rounded_ins(ins):
    """ins with W_hh and h0 replaced by their bf16 roundings: what one step of the kernel multiplies exactly (bf16 x bf16 is
    exact in fp32), so f64check.lstm_step_check's derived bound applies unchanged"""
    mod = copy.deepcopy(ins[0])
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if "weight_hh" in n:
                p.copy_(bf(p))
    return (mod, ins[1], None if ins[2] is None else bf(ins[2])) + tuple(ins[3:])


def representable_ins(ins):
    """ins whose W_hh and h0 are bf16-representable (the rounding is then the identity)"""
    return rounded_ins(ins)


def quant_figures(out, ref64, batch_first, keys):
    """worst per-slice deviation m_t of each tensor from the unquantised float64 LSTM: {key: figure}"""
    return {k: float(fc.seq_slice_figures(out[k].detach().cpu().reshape(ref64[k].shape), ref64[k],
                                          fc.lstm_slice_dim(k, batch_first))[0].max()) for k in keys}
