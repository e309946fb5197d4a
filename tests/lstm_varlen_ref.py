"""References and the C-ABI runner of the variable-length LSTM (ecgmm_lstm_forward_varlen / ecgmm_lstm_backward_varlen), shared
by tests/test_lstm_varlen_cpu.py and tests/test_lstm_varlen_gpu.py.

  packed_run       torch.nn.LSTM on pack_padded_sequence(x, lengths, enforce_sorted=False) on the CPU, re-padded to T: THE
                   reference (float64 the answer, float32 the yardstick), in the dictionary shape of f64check.lstm_run
  masked_hold_run  the same function restated step by step as the kernels compute it: at step t row b is live iff
                   t < lengths[b]; a dead row holds h and c and outputs 0.  Autograd gives its gradients.
  run              the C entry points as tests/lstm_abi.py runs the fixed ones: every output a NaN-filled view between
                   sentinel zones, workspace and scratch NaN-filled, of exactly the reported size and followed by sentinels;
                   every run checks every sentinel and that no NaN / inf is left in any output.

Inputs are f64check.lstm_inputs' tuples (module, x, h0, c0, gy, gh, gc), never modified."""
import copy
import ctypes as C

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from . import f64check as F64  # noqa: F401  (the callers' checks; the dictionary shape is lstm_run's)

# (B, T, In, H, layers, bidirectional, batch_first, h0 / c0 given) and the lengths; every set has max(lengths) == T, so no
# time slice of the float64 reference is all padding
L17_ODD = (6, 1, 4, 3, 2, 5, 6, 1, 2, 3, 4, 5, 6, 3, 2, 1, 3)    # slice 0: 1, T and middling; slice 1 (one row): 3 steps, odd
L17_EVEN = (6, 1, 4, 3, 2, 5, 6, 1, 2, 3, 4, 5, 6, 3, 2, 1, 4)   # slice 1: 4 steps, even
L9 = (24, 1, 13, 7, 24, 2, 19, 8, 11)
L33 = (4, 1, 2, 3) * 8 + (2,)                                    # slices 0 and 1 full, slice 2 one row of 2 steps
VARLEN_CASES, VARLEN_IDS = [], []
for bf in (True, False):
    for given in (True, False):
        for tag, lens in (("odd", L17_ODD), ("even", L17_EVEN)):
            VARLEN_CASES.append(((17, 6, 5, 20, 2, True, bf, given), lens))
            VARLEN_IDS.append("b17_%s_%s_%s" % ("bf" if bf else "tb", "hx" if given else "nohx", tag))
VARLEN_CASES += [((9, 24, 20, 132, 1, False, True, False), L9), ((33, 4, 16, 1, 1, True, True, True), L33)]
VARLEN_IDS += ["h132", "h1"]
ALL = ("y", "h", "c")


def _loss(y, hn, cn, gy, gh, gc, dtype, use):
    loss = 0
    if "y" in use:
        loss = loss + (y * gy.to(dtype)).sum()
    if "h" in use:
        loss = loss + (hn * gh.to(dtype)).sum()
    if "c" in use:
        loss = loss + (cn * gc.to(dtype)).sum()
    return loss


def _collect(y, hn, cn, x, hx, named):
    out = {"y": y, "hn": hn, "cn": cn, "dx": x.grad}
    if hx is not None:
        out["dh0"], out["dc0"] = hx[0].grad, hx[1].grad
    for n, p in named:
        out["d" + n] = p.grad
    return {k: v.detach() for k, v in out.items()}


def packed_run(ins, lengths, dtype, use=ALL):
    """torch's packed LSTM on the CPU in `dtype`: y re-padded to T (zeros behind each row's length), h_n, c_n and every
    gradient of sum y gy + sum h_n gh + sum c_n gc (the terms named in `use`)."""
    mod, x, h0, c0, gy, gh, gc = ins
    m = copy.deepcopy(mod).to(dtype)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    x = leaf(x)
    hx = None if h0 is None else (leaf(h0), leaf(c0))
    T = x.shape[1] if m.batch_first else x.shape[0]
    packed = pack_padded_sequence(x, torch.as_tensor(lengths, dtype=torch.int64), batch_first=m.batch_first,
                                  enforce_sorted=False)
    yp, (hn, cn) = m(packed, hx)
    y, _ = pad_packed_sequence(yp, batch_first=m.batch_first, total_length=T)
    _loss(y, hn, cn, gy, gh, gc, dtype, use).backward()
    return _collect(y, hn, cn, x, hx, m.named_parameters())


def masked_hold_run(ins, lengths, dtype, use=ALL):
    """The recurrence step by step with a per-row live mask (what csrc/lstm.hip computes), same outputs as packed_run."""
    mod, x, h0, c0, gy, gh, gc = ins
    m = copy.deepcopy(mod).to(dtype)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    x = leaf(x)
    hx = None if h0 is None else (leaf(h0), leaf(c0))
    bf, H, D = m.batch_first, m.hidden_size, 2 if m.bidirectional else 1
    seq = x if bf else x.transpose(0, 1)          # [B, T, In]
    B, T = seq.shape[0], seq.shape[1]
    lens = torch.as_tensor(lengths, dtype=torch.int64).clamp(0, T)
    hns, cns = [], []
    for layer in range(m.num_layers):
        outs = []
        for d in range(D):
            sfx = "_l%d%s" % (layer, "_reverse" if d else "")
            w_ih, w_hh = getattr(m, "weight_ih" + sfx), getattr(m, "weight_hh" + sfx)
            b_ih, b_hh = getattr(m, "bias_ih" + sfx), getattr(m, "bias_hh" + sfx)
            h = hx[0][layer * D + d] if hx is not None else seq.new_zeros(B, H)
            c = hx[1][layer * D + d] if hx is not None else seq.new_zeros(B, H)
            ys = [None] * T
            for t in (range(T - 1, -1, -1) if d else range(T)):
                live = (t < lens).to(dtype)[:, None]
                gates = seq[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
                i, f, g, o = gates.split(H, dim=1)
                c1 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h1 = torch.sigmoid(o) * torch.tanh(c1)
                # a hold, not a blend: the dead branch's values never enter (its x is finite, so 0 * it is 0)
                c = torch.where(live.bool(), c1, c)
                h = torch.where(live.bool(), h1, h)
                ys[t] = torch.where(live.bool(), h1, torch.zeros_like(h1))
            outs.append(torch.stack(ys, 1))
            hns.append(h)
            cns.append(c)
        seq = torch.cat(outs, 2)
    y = seq if bf else seq.transpose(0, 1)
    hn, cn = torch.stack(hns), torch.stack(cns)
    _loss(y, hn, cn, gy, gh, gc, dtype, use).backward()
    return _collect(y, hn, cn, x, hx, m.named_parameters())


def pad_mask(lengths, T, batch_first):
    """bool [B, T] (or [T, B]): True at padded positions"""
    m = torch.arange(T)[None, :] >= torch.as_tensor(lengths, dtype=torch.int64).clamp(0, T)[:, None]
    return m if batch_first else m.t()


def refill_padding(t, lengths, batch_first, seed, magnitude=1e3):
    """a copy of the padded [B, T, F] / [T, B, F] tensor whose padded positions hold finite values of size `magnitude`"""
    T = t.shape[1] if batch_first else t.shape[0]
    m = pad_mask(lengths, T, batch_first)
    g = torch.Generator().manual_seed(seed)
    noise = (torch.rand(t.shape, generator=g) + 0.5) * magnitude * (torch.randint(0, 2, t.shape, generator=g) * 2 - 1)
    out = t.clone()
    out[m] = noise.to(t.dtype)[m]
    return out


def row_inputs(ins, b, l, batch_first):
    """the inputs of row b alone, cut to its first l steps (B = 1, T = l), for the fixed entry points"""
    mod, x, h0, c0, gy, gh, gc = ins
    cut = (lambda t: t[b:b + 1, :l].contiguous()) if batch_first else (lambda t: t[:l, b:b + 1].contiguous())
    st = lambda t: None if t is None else t[:, b:b + 1].contiguous()
    return mod, cut(x), st(h0), st(c0), cut(gy), st(gh), st(gc)


def run(case, ins, lengths, use=ALL, save=1, backward=True, entry="varlen"):
    """ecgmm_lstm_forward_varlen / _backward_varlen (entry = "varlen"; lengths = None passes a null pointer) or the fixed
    ecgmm_lstm_forward / _backward (entry = "fixed"; lengths ignored) on `ins` of `case`.  lengths: any integers, handed
    to the device as int32 unvalidated (the entry points clamp).  Returns {name: device tensor} named as packed_run names
    them."""
    from ecgmm.hip import lib as L
    from ecgmm.hip.functional import ptr, stream

    from . import lstm_abi as A

    B, T, In, H, layers, bi, bf, given = case
    mod, x, h0, c0, gy, gh, gc = ins
    lib = L.lib()
    names = [n for n, _ in mod.named_parameters()]
    params = [p.detach().to(A.DEV).contiguous() for p in mod.parameters()]
    dv = lambda t: None if t is None else t.to(A.DEV).contiguous()
    x, h0, c0, gy, gh, gc = (dv(t) for t in (x, h0, c0, gy, gh, gc))
    lens = None
    if lengths is not None and entry == "varlen":   # between sentinels as well: it is only read
        lens = torch.full((B + 2 * A.GUARD,), -7, device=A.DEV, dtype=torch.int32)
        lens[A.GUARD:A.GUARD + B] = torch.as_tensor(lengths, dtype=torch.int32).to(A.DEV)
        lens = lens[A.GUARD:A.GUARD + B]
    d = L.LSTMDesc(B, T, In, H, layers, int(bi), int(bf), int(save))
    nf = lib.ecgmm_lstm_fwd_workspace(C.byref(d))
    assert nf > 0 and nf % 4 == 0, lib.ecgmm_last_error()
    shapes = {"y": gy.shape, "hn": gh.shape, "cn": gc.shape}
    if backward:
        shapes["dx"] = x.shape
        if given:
            shapes["dh0"], shapes["dc0"] = h0.shape, c0.shape
        for n, p in zip(names, params):
            shapes["d" + n] = p.shape
    ar = A.Arena(shapes)
    v = ar.views
    ws = A.guarded_bytes(nf)
    tp = A.table(params)
    if entry == "varlen":
        L.check(lib.ecgmm_lstm_forward_varlen(C.byref(d), ptr(x), ptr(lens), tp, ptr(h0), ptr(c0), ptr(v["y"]), ptr(v["hn"]),
                                              ptr(v["cn"]), ptr(ws), nf, stream()), "lstm_forward_varlen")
    else:
        L.check(lib.ecgmm_lstm_forward(C.byref(d), ptr(x), tp, ptr(h0), ptr(c0), ptr(v["y"]), ptr(v["hn"]), ptr(v["cn"]),
                                       ptr(ws), nf, stream()), "lstm_forward")
    sc = None
    if backward:
        nb = lib.ecgmm_lstm_bwd_workspace(C.byref(d))
        assert nb > 0 and nb % 4 == 0, lib.ecgmm_last_error()
        sc = A.guarded_bytes(nb)
        grads = A.table([v.get("d" + n) for n in names])
        cot = (ptr(gy if "y" in use else None), ptr(gh if "h" in use else None), ptr(gc if "c" in use else None))
        if entry == "varlen":
            L.check(lib.ecgmm_lstm_backward_varlen(C.byref(d), ptr(x), ptr(lens), tp, ptr(h0), ptr(c0), *cot, ptr(ws),
                                                   ptr(v["dx"]), grads, ptr(v.get("dh0")), ptr(v.get("dc0")), ptr(sc), nb,
                                                   stream()), "lstm_backward_varlen")
        else:
            L.check(lib.ecgmm_lstm_backward(C.byref(d), ptr(x), tp, ptr(h0), ptr(c0), *cot, ptr(ws), ptr(v["dx"]), grads,
                                            ptr(v.get("dh0")), ptr(v.get("dc0")), ptr(sc), nb, stream()), "lstm_backward")
    torch.cuda.synchronize()
    assert not ar.touched(), "written outside an output, next to: %s" % ar.touched()
    assert not A.tail_touched(ws), "written past the end of the forward workspace"
    assert sc is None or not A.tail_touched(sc), "written past the end of the backward scratch"
    for k, t in v.items():
        assert bool(torch.isfinite(t).all()), "%s: NaN / inf left in an output" % k
    return dict(v)
