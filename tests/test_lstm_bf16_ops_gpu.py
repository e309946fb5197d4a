"""The bf16 recurrence of the native LSTM through the C ABI (ecgmm_lstm_*_dt, tests/lstm_bf16_abi.py: arena, sentinels, NaN
prefills), against the operand-forced float64 reference of tests/lstm_bf16_ref.py.

One step (T = 1): f64check's derived bound with bf(h0), bf(W_hh) as the operands (bf16 x bf16 is exact in fp32, so the bound
is unchanged), at LSTM_STEP_H plus 192, 208, 209, 224 -- the K-padding (multiples of 32) and residency boundaries (H <= 128
all of W_hh in registers, <= 208 registers + LDS, above that partly streamed; two tiles per wave from 129, three from 257).
Chains: every slice of every tensor (y, hn, cn, dx, dh0, dc0, dgates of each direction, every parameter gradient) at the
per-slice chain bar, the forced float32 chain as the yardstick, with and without lengths.  torch.nn.LSTM has no reverse-only
form, so the reverse direction is checked as direction 1 of the bidirectional cases.
Multi-layer: the call against single-layer calls chained through the ABI, bit for bit (the same launches in the same order).
Each test prints its figures (run with -s)."""
import ctypes as C

import pytest
import torch

from ecgmm.hip import lib as L

from . import f64check as F64
from . import lstm_abi
from . import lstm_bf16_abi as abi
from . import lstm_bf16_ref as R

pytestmark = pytest.mark.gpu
ALL = ("y", "h", "c")
STEP_H = tuple(F64.LSTM_STEP_H) + (192, 208, 209, 224)
CHAIN_SHAPES = [(16, 70, 24, 200), (9, 24, 20, 132), (17, 3, 24, 384), (17, 3, 24, 256), (33, 4, 16, 1), (17, 5, 512, 200)]


def cpu(out):
    return {k: v.detach().cpu() for k, v in out.items() if not k.startswith("_")}


def lengths_of(B, T):
    """full rows, one short row and (B > 2) a row of length 1; row 0 keeps T so that no time slice is all padding"""
    ln = [T] * B
    if B > 1:
        ln[1] = max(1, T // 2)
    if B > 2:
        ln[2] = 1
    return ln


def same(a, b, what=""):
    for k in a:
        if k.startswith("_"):
            continue
        assert torch.equal(a[k], b[k]), "%s: %s differs (max %.3g)" % (what, k, float((a[k] - b[k]).abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# one step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", STEP_H)
def test_single_step_bound(H):
    worst = 0.0
    for B in F64.LSTM_STEP_B:
        for bi in (False, True):
            case = F64.lstm_step_case(B, 24, H, bi)
            ins = F64.lstm_inputs(case)
            rep = R.representable_ins(ins)   # bf16-representable h0 / W_hh: the kernel's products are the fp32 kernel's
            out = cpu(abi.run(case, rep, backward=False))
            r1 = F64.lstm_step_check(out, rep, "bf16 exact operands H=%d B=%d D=%d" % (H, B, 1 + bi))
            out = cpu(abi.run(case, ins, backward=False))
            r2 = F64.lstm_step_check(out, R.rounded_ins(ins), "bf16 general operands H=%d B=%d D=%d" % (H, B, 1 + bi))
            worst = max(worst, r1.ratio, r2.ratio)
    print("[lstm bf16 step] H = %d: worst ratio to the derived bound %.3g" % (H, worst))


# ----------------------------------------------------------------------------------------------------------------------
# forced chains
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("varlen", (False, True), ids=("fixed", "lengths"))
@pytest.mark.parametrize("bi", (False, True), ids=("fwd", "bidir"))
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "b%d_t%d_in%d_h%d" % s)
def test_forced_chain(shape, bi, varlen):
    B, T, In, H = shape
    case = (B, T, In, H, 1, bi, True, True)
    ins = F64.lstm_inputs(case)
    ln = lengths_of(B, T) if varlen else None
    out = cpu(abi.run(case, ins, lengths=ln))
    R.check_forced(out, ins, ln, ALL, "%s D=%d %s" % (shape, 1 + bi, "lengths" if varlen else "fixed"))


# ----------------------------------------------------------------------------------------------------------------------
# exact properties in bf16 mode
# ----------------------------------------------------------------------------------------------------------------------
PROP = (17, 6, 24, 200, 1, True, True, True)


def test_save_flag_changes_no_bit():
    ins = F64.lstm_inputs(PROP)
    a = cpu(abi.run(PROP, ins, save=1, backward=False))
    b = cpu(abi.run(PROP, ins, save=0, backward=False))
    same(a, b, "save=0 / save=1")


def test_lengths_all_T_equal_the_fixed_call_and_two_calls_agree():
    ins = F64.lstm_inputs(PROP)
    a = cpu(abi.run(PROP, ins))
    same(a, cpu(abi.run(PROP, ins)), "second call")
    same(a, cpu(abi.run(PROP, ins, lengths=[PROP[1]] * PROP[0])), "lengths all T")


def test_padding_is_zero_and_its_contents_change_no_bit():
    B, T = PROP[0], PROP[1]
    ins = F64.lstm_inputs(PROP)
    ln = lengths_of(B, T)
    a = cpu(abi.run(PROP, ins, lengths=ln))
    x2 = ins[1].clone()
    for b, l in enumerate(ln):
        x2[b, l:] = 1e3
    same(a, cpu(abi.run(PROP, ins, lengths=ln, x_override=x2)), "padding contents")
    for b, l in enumerate(ln):
        for k in ("y", "dx", "dgates0", "dgates1"):
            assert not bool(a[k][b, l:].any()), "%s: row %d is not exactly zero from its length %d on" % (k, b, l)


def test_row_alone_equals_the_row_in_the_batch():
    B, T, In, H = PROP[:4]
    ins = F64.lstm_inputs(PROP)
    mod, x, h0, c0, gy, gh, gc = ins
    ln = lengths_of(B, T)
    a = cpu(abi.run(PROP, ins, lengths=ln))
    b, l = 1, ln[1]
    one = (1, l, In, H, 1, True, True, True)
    ins1 = (mod, x[b:b + 1, :l], h0[:, b:b + 1], c0[:, b:b + 1], gy[b:b + 1, :l], gh[:, b:b + 1], gc[:, b:b + 1])
    o = cpu(abi.run(one, ins1))
    for k in ("y", "dx"):
        assert torch.equal(o[k][0], a[k][b, :l]), k
    for k in ("hn", "cn", "dh0", "dc0"):
        assert torch.equal(o[k][:, 0], a[k][:, b]), k


@pytest.mark.parametrize("null", [("hn", "cn"), ("dx",), ("dh0", "dc0"), ("grads",), (("grad", 0),), (("grad", 1), ("grad", 3))],
                         ids=("states", "dx", "dstates", "grads", "w_ih", "w_hh_b_hh"))
def test_null_pointers_leave_the_rest_bit_identical(null):
    ins = F64.lstm_inputs(PROP)
    a = cpu(abi.run(PROP, ins))
    b = cpu(abi.run(PROP, ins, null=null))
    for k in b:
        assert torch.equal(a[k], b[k]), k
    if "grads" not in null and ("grad", 3) not in null and ("grad", 2) not in null:
        assert torch.equal(b["dbias_ih_l0"], b["dbias_hh_l0"])
    c = cpu(abi.run(PROP, ins, use=()))   # every cotangent null: all gradients are zero
    assert not bool(c["dx"].any())


@pytest.mark.parametrize("H", (8, 200))
def test_misaligned_w_hh(H):
    case = (5, 4, 12, H, 1, True, True, True)
    ins = F64.lstm_inputs(case)
    same(cpu(abi.run(case, ins)), cpu(abi.run(case, ins, misalign_whh=True)), "misaligned W_hh")


# ----------------------------------------------------------------------------------------------------------------------
# multi-layer: the call against single-layer calls chained through the ABI
# ----------------------------------------------------------------------------------------------------------------------
def layer_module(mod, l, In):
    D = 2 if mod.bidirectional else 1
    m = torch.nn.LSTM(In, mod.hidden_size, 1, batch_first=mod.batch_first, bidirectional=mod.bidirectional)
    with torch.no_grad():
        for k in range(D):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                sfx = "_reverse" if k else ""
                getattr(m, n + "_l0" + sfx).copy_(getattr(mod, "%s_l%d%s" % (n, l, sfx)))
    return m


@pytest.mark.parametrize("case", [(4, 7, 20, 200, 3, True, True, True), (3, 5, 16, 8, 8, False, False, True)],
                         ids=("3_layers_bidir_h200", "8_layers"))
def test_multi_layer_equals_chained_single_layer_calls(case):
    B, T, In, H, layers, bi, bf, given = case
    D = 2 if bi else 1
    ins = F64.lstm_inputs(case)
    mod, x, h0, c0, gy, gh, gc = ins
    whole = cpu(abi.run(case, ins))
    sl = lambda t, l: t[l * D:(l + 1) * D]
    xs, mods = [x], []
    for l in range(layers):   # forward chain
        Inl = In if l == 0 else D * H
        mods.append(layer_module(mod, l, Inl))
        one = (B, T, Inl, H, 1, bi, bf, True)
        zero = torch.zeros(xs[l].shape[0], xs[l].shape[1], D * H)
        o = cpu(abi.run(one, (mods[l], xs[l], sl(h0, l), sl(c0, l), zero, sl(gh, l), sl(gc, l)), backward=False))
        xs.append(o["y"])
        assert torch.equal(o["hn"], sl(whole["hn"], l)) and torch.equal(o["cn"], sl(whole["cn"], l)), "layer %d states" % l
    assert torch.equal(xs[-1], whole["y"])
    dy = gy
    for l in range(layers - 1, -1, -1):   # backward chain
        Inl = In if l == 0 else D * H
        one = (B, T, Inl, H, 1, bi, bf, True)
        o = cpu(abi.run(one, (mods[l], xs[l], sl(h0, l), sl(c0, l), dy, sl(gh, l), sl(gc, l))))
        assert torch.equal(o["dh0"], sl(whole["dh0"], l)) and torch.equal(o["dc0"], sl(whole["dc0"], l)), "layer %d dh0" % l
        for n, _ in mods[l].named_parameters():
            assert torch.equal(o["d" + n], whole["d" + n.replace("_l0", "_l%d" % l)]), "layer %d %s" % (l, n)
        dy = o["dx"]
    assert torch.equal(dy, whole["dx"])


# ----------------------------------------------------------------------------------------------------------------------
# ECGMM_F32 through the _dt entry points is the old entry points, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,use", F64.LSTM_CHAIN_CASES, ids=F64.LSTM_CHAIN_IDS)
def test_f32_through_dt_is_the_old_entry_point(case, use):
    ins = F64.lstm_inputs(case)
    old = cpu(lstm_abi.run(case, ins, use))
    new = cpu(abi.run(case, ins, dtype=L.F32, use=use))
    for k in old:
        assert torch.equal(old[k], new[k]), k
    d = L.LSTMDesc(*case[:4], case[4], int(case[5]), int(case[6]), 1)
    lib = L.lib()
    assert lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), L.F32) == lib.ecgmm_lstm_fwd_workspace(C.byref(d))
    assert lib.ecgmm_lstm_bwd_workspace_dt(C.byref(d), L.F32) == lib.ecgmm_lstm_bwd_workspace(C.byref(d))
