"""The variable-length LSTM (csrc/lstm.hip, VL instantiations; ecgmm_lstm_forward_varlen / _backward_varlen) and the masked
mean (ecgmm_seq_mean_varlen_fwd / _bwd) on the GPU.

Reference: torch's packed LSTM on the CPU, re-padded (tests/lstm_varlen_ref.packed_run) -- float64 the answer, float32 the
yardstick -- under the per-slice chain bar of tests/f64check.py (F64.lstm_chain_check), unchanged: every case has
max(lengths) == T, so no time slice of the reference is all padding and LSTM_MIN_RMS holds as it stands.  Everything else
here is exact: zeros at padded positions, identity with the fixed entry points, independence from what the padding holds,
and each row bit-identical to the fixed call on that row alone at T = its length (which derives no tolerance and catches a
wrong c_{t-1}, a wrong h_n parity and a wrong carry at once).  Every run goes through the C ABI with NaN-filled outputs,
workspace and scratch between sentinels (tests/lstm_varlen_ref.run), so an unwritten hprev or dgates tail shows as a NaN in
a parameter gradient.

Cases (tests/lstm_varlen_ref.VARLEN_CASES): (17, 6, 5, 20, 2 layers, bidirectional) with both layouts, with and without
h0 / c0, slice 0 holding lengths 1, T and middling ones and slice 1 (one row) 3 steps (odd: the h_n parity, the zero tail)
or 4 (even); (9, 24, 20, 132) where wave 0 takes a second tile; (33, 4, 16, H = 1).

Measured on the MI355X (the module runs in about 4 s, no test above 0.6 s): worst ratio to the per-slice chain bar 0.70 (dc0
at H = 1: 9.5 u against torch fp32's own 11.2 u), 0.13 - 0.21 on the other cases; masked mean, forward / backward ratio to the
bound: (3, 7, 400) 0.34 / 0.42, (17, 5, 5) 0.31 / 0.37, (2, 9, 1030) 0.23 / 0.44; every exact check holds, the fixed-call
identity at every shape included (H = 1: lstm_seq_fwd_kernel<false, true> against <false, false> at the same B and T).  One defect found
while building it: with the dead rows branched around, the compiler fused other products in the backward cell of the VL kernel
than in the fixed one, and "lengths all T" differed from the fixed call in the last bit of dx (csrc/lstm.hip pins them now)."""
import functools

import pytest
import torch

from ecgmm.hip import functional as HF
from ecgmm.hip import nn as HN

from . import f64check as F64
from . import lstm_varlen_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = pytest.mark.parametrize("case,lengths", V.VARLEN_CASES, ids=V.VARLEN_IDS)


def cpu(out):
    return {k: v.detach().cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def refs(case, lengths):
    ins = F64.lstm_inputs(case)
    return V.packed_run(ins, lengths, torch.float64), V.packed_run(ins, lengths, torch.float32)


@functools.lru_cache(maxsize=None)
def ours(case, lengths):
    return cpu(V.run(case, F64.lstm_inputs(case), lengths))


def same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


@CASES
def test_against_packed_lstm_in_float64(case, lengths):
    """every tensor under the per-slice chain bar against torch's packed LSTM; y and dx exactly 0 at padded positions"""
    out = ours(case, lengths)
    r64, r32 = refs(case, lengths)
    assert sorted(out) == sorted(r64)
    F64.lstm_chain_check(out, r64, r32, case[6], "varlen %s" % (case,))
    pad = V.pad_mask(lengths, case[1], case[6])
    assert bool(pad.any())
    for k in ("y", "dx"):
        assert not out[k][pad].any(), "%s is not exactly 0 at a padded position" % k
        assert not r64[k][pad].any()


@CASES
def test_padding_contents_change_no_bit(case, lengths):
    """x's padding refilled with finite values of size 1e3, and dy's likewise: every output and gradient keeps its bits"""
    bf = case[6]
    ins = F64.lstm_inputs(case)
    noisy = (ins[0], V.refill_padding(ins[1], lengths, bf, 11), ins[2], ins[3], V.refill_padding(ins[4], lengths, bf, 12)) + ins[5:]
    pad = V.pad_mask(lengths, case[1], bf)
    assert float(noisy[1][pad].abs().min()) >= 500 and float(noisy[4][pad].abs().min()) >= 500
    same_bits(ours(case, lengths), cpu(V.run(case, noisy, lengths)), "refilled padding")


@CASES
def test_each_row_is_the_fixed_call_on_that_row_alone(case, lengths):
    """row b of length l: y[:l], h_n, c_n, dx[:l], dh0, dc0 bit-identical to ecgmm_lstm_forward / _backward at B = 1, T = l"""
    B, T, In, H, layers, bi, bf, given = case
    ins = F64.lstm_inputs(case)
    out = ours(case, lengths)
    for b, l in enumerate(lengths):
        alone = cpu(V.run((1, l, In, H, layers, bi, bf, given), V.row_inputs(ins, b, l, bf), None, entry="fixed"))
        for k in ("y", "dx"):
            got = out[k][b:b + 1, :l] if bf else out[k][:l, b:b + 1]
            assert torch.equal(got, alone[k]), "row %d (length %d): %s" % (b, l, k)
        for k in ("hn", "cn") + (("dh0", "dc0") if given else ()):
            assert torch.equal(out[k][:, b:b + 1], alone[k]), "row %d (length %d): %s" % (b, l, k)


# every distinct shape once (this test does not use the cases' lengths): the four layout / hx variants of the 17-row shape, H = 132
# and H = 1 -- the one shape on the 4-byte W_hh loads, lstm_seq_fwd_kernel<false, true> against <false, false>
SHAPES = [(17, 6, 5, 20, 2, True, True, True), (17, 6, 5, 20, 2, True, True, False), (17, 6, 5, 20, 2, True, False, True),
          (17, 6, 5, 20, 2, True, False, False), (9, 24, 20, 132, 1, False, True, False), (33, 4, 16, 1, 1, True, True, True)]
SHAPE_IDS = ["b17_bf_hx", "b17_bf_nohx", "b17_tb_hx", "b17_tb_nohx", "h132", "h1"]
assert sorted(set(c for c, _ in V.VARLEN_CASES)) == sorted(SHAPES)


@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_full_lengths_and_null_lengths_are_the_fixed_call(case):
    ins = F64.lstm_inputs(case)
    fixed = cpu(V.run(case, ins, None, entry="fixed"))
    same_bits(fixed, cpu(V.run(case, ins, None)), "lengths = null")
    same_bits(fixed, cpu(V.run(case, ins, (case[1],) * case[0])), "lengths all T")
    same_bits(fixed, cpu(V.run(case, ins, (case[1] + 5,) * case[0])), "lengths all T + 5")


CLAMP = [0, 3, 4, 7]     # batch_first and time-major, each with h0 / c0 given (odd lengths) and without (even)


@pytest.mark.parametrize("case,lengths", [V.VARLEN_CASES[i] for i in CLAMP], ids=[V.VARLEN_IDS[i] for i in CLAMP])
def test_lengths_are_clamped_on_the_device(case, lengths):
    """T + 5 is T; 0 (and below) is a row without a live step: y = 0, hn = h0, cn = c0, dx = 0, dh0 = dhn, dc0 = dcn, and
    the rest of the batch is what it is without that row"""
    B, T, In, H, layers, bi, bf, given = case
    ins = F64.lstm_inputs(case)
    mod, x, h0, c0, gy, gh, gc = ins
    zero = (2, 16)                                   # one in the full slice, and the whole second slice
    wild = tuple(-3 if b == 2 else 0 if b == 16 else T + 5 if l == T else l for b, l in enumerate(lengths))
    tame = tuple(0 if b in zero else l for b, l in enumerate(lengths))
    out = cpu(V.run(case, ins, wild))
    same_bits(out, cpu(V.run(case, ins, tame)), "clamped lengths")
    row = (lambda t, b: t[b]) if bf else (lambda t, b: t[:, b])
    for b in zero:
        assert not row(out["y"], b).any() and not row(out["dx"], b).any()
        if given:
            assert torch.equal(out["hn"][:, b], h0[:, b]) and torch.equal(out["cn"][:, b], c0[:, b])
            assert torch.equal(out["dh0"][:, b], gh[:, b]) and torch.equal(out["dc0"][:, b], gc[:, b])
        else:
            assert not out["hn"][:, b].any() and not out["cn"][:, b].any()
    keep = [b for b in range(B) if b not in zero]
    rows = (lambda t: t[keep].contiguous()) if bf else (lambda t: t[:, keep].contiguous())
    st = lambda t: None if t is None else t[:, keep].contiguous()
    sub = (mod, rows(x), st(h0), st(c0), rows(gy), st(gh), st(gc))
    sub_len = tuple(lengths[b] for b in keep)
    r64, r32 = V.packed_run(sub, sub_len, torch.float64), V.packed_run(sub, sub_len, torch.float32)
    cut = {k: (rows(v) if k in ("y", "dx") else st(v) if k in ("hn", "cn", "dh0", "dc0") else v) for k, v in out.items()}
    F64.lstm_chain_check(cut, r64, r32, bf, "varlen, rows of length 0 left out")


@pytest.mark.parametrize("bf", [True, False])
def test_module_path_is_the_abi(bf):
    """HN.LSTM(x, hx, lengths=...) under autograd: the bits of the C entry points; lists, CPU and device tensors alike"""
    case, lengths = (17, 6, 5, 20, 2, True, bf, True), V.L17_ODD
    mod, x, h0, c0, gy, gh, gc = F64.lstm_inputs(case)
    ref = ours(case, lengths)
    net = HN.LSTM(5, 20, 2, batch_first=bf, bidirectional=True)
    net.load_state_dict(mod.state_dict(), strict=True)
    net = net.to(DEV)
    for form in (list(lengths), torch.tensor(lengths), torch.tensor(lengths, device=DEV)):
        net.zero_grad()
        leaf = lambda t: t.to(DEV).requires_grad_()
        xd, hd, cd = leaf(x), leaf(h0), leaf(c0)
        y, (hn, cn) = net(xd, (hd, cd), lengths=form)
        ((y * gy.to(DEV)).sum() + (hn * gh.to(DEV)).sum() + (cn * gc.to(DEV)).sum()).backward()
        got = {"y": y, "hn": hn, "cn": cn, "dx": xd.grad, "dh0": hd.grad, "dc0": cd.grad}
        got.update({"d" + n: p.grad for n, p in net.named_parameters()})
        same_bits(ref, cpu(got), "module path")
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0"):
        net(x.to(DEV), lengths=[6, 0] + [1] * 15)
    with torch.no_grad():                              # the forward that keeps nothing for a backward
        y, (hn, cn) = net(x.to(DEV), (h0.to(DEV), c0.to(DEV)), lengths=list(lengths))
    same_bits({k: ref[k] for k in ("y", "hn", "cn")}, cpu({"y": y, "hn": hn, "cn": cn}), "no_grad forward")


# ----------------------------------------------------------------------------------------------------------------------
# the masked mean
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lengths", [((3, 7, 400), (7, 1, 4)), ((17, 5, 5), (5, 1, 2, 3, 4) * 3 + (5, 1)),
                                           ((2, 9, 1030), (1, 9))], ids=["3x7x400", "17x5x5", "2x9x1030"])
def test_masked_mean_against_float64(shape, lengths):
    """the bounds tests/test_lstm_f64_gpu.py applies to seq_mean with the row's own length l as the term count:
    forward |out - ref| <= g_k(l + 1) * mean_{t < l} |x|;  backward |dx - ref| <= g_k(2) * |dy| / l, exactly 0 behind l.
    The padding of x holds 1e3-sized values."""
    B, T, Cn = shape
    g = torch.Generator().manual_seed(B * 1000 + T)
    x, dy = torch.randn(shape, generator=g) + 0.3, torch.randn(B, Cn, generator=g)
    x = V.refill_padding(x, lengths, True, 21)
    xd = x.to(DEV).requires_grad_()
    out = HF.seq_mean(xd, lengths=list(lengths))
    assert tuple(out.shape) == (B, Cn) and out.is_contiguous()
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    dx, out = xd.grad.cpu(), out.detach().cpu()
    assert tuple(dx.shape) == shape and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(out).all())
    worst_f = worst_b = 0.0
    for b, l in enumerate(lengths):
        x64 = x[b, :l].double()
        rf = F64._ratio((out[b].double() - x64.mean(0)).abs(), F64.g_k(l + 1) * x64.abs().mean(0))
        ref_dx = (dy[b].double() / l)[None, :].expand(l, Cn)
        rb = F64._ratio((dx[b, :l].double() - ref_dx).abs(), F64.g_k(2) * ref_dx.abs())
        worst_f, worst_b = max(worst_f, float(rf.max())), max(worst_b, float(rb.max()))
        assert not dx[b, l:].any(), "dx of row %d is not exactly 0 behind its length" % b
    print("[seq_mean varlen] %s: worst ratio to the bound: forward %.3g, backward %.3g" % (shape, worst_f, worst_b))
    assert worst_f <= 1.0 and worst_b <= 1.0


def test_masked_mean_of_an_empty_row_is_zero():
    """a device tensor of lengths is taken as given and clamped: 0 gives a mean of 0 and a gradient of 0, not NaN"""
    x = torch.randn(3, 4, 6, generator=torch.Generator().manual_seed(1))
    xd = x.to(DEV).requires_grad_()
    out = HF.seq_mean(xd, lengths=torch.tensor([0, 9, -2], device=DEV))
    out.sum().backward()
    out, dx = out.detach().cpu(), xd.grad.cpu()
    assert not out[0].any() and not out[2].any() and not dx[0].any() and not dx[2].any()
    assert torch.allclose(out[1], x[1].mean(0), atol=1e-6) and torch.equal(dx[1], torch.full((4, 6), 0.25))
