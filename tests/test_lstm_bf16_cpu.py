"""The bf16 recurrence of the native LSTM without a GPU: the reference helper (tests/lstm_bf16_ref.py) checked against torch
and against itself -- its bf() is torch's bfloat16 rounding; with rounding off the chain is torch.nn.LSTM in float64; its
checks accept the CPU model of the kernel (emulate) on every case of the GPU test and reject, naming the tensor, each slip a
kernel could make -- and the parts of the feature that need no device: the _dt workspace queries, the view query, the
keyword of HN.LSTM / HF.lstm / CRNN."""
import ctypes as C

import pytest
import torch

from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip import nn as HN

from . import f64check as F64
from . import lstm_bf16_ref as R

ALL = ("y", "h", "c")
CHAIN_SHAPES = [(16, 70, 24, 200), (9, 24, 20, 132), (17, 3, 24, 384), (17, 3, 24, 256), (33, 4, 16, 1), (17, 5, 512, 200)]


def lengths_of(B, T):
    ln = [T] * B
    if B > 1:
        ln[1] = max(1, T // 2)
    if B > 2:
        ln[2] = 1
    return ln


def bits(v):
    return torch.tensor(v, dtype=torch.int64).to(torch.int32).view(torch.float32) if False else \
        torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in v], dtype=torch.int32).view(torch.float32)


def test_bf_is_torchs_bfloat16_rounding():
    pats = []
    for hi in (0x3F80, 0x3F81, 0x0001, 0x0000, 0x7F7F, 0x7F00, 0x0080, 0x007F, 0x4049):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):   # below, at and above the tie, for even and odd hi
            pats += [(hi << 16) | lo, (1 << 31) | (hi << 16) | lo]
    x = torch.cat([bits(pats), torch.randn(4096), torch.randn(512) * 1e-39, torch.tensor([float("inf"), -float("inf"), 0.0, -0.0])])
    want = x.bfloat16().float()
    got = R.bf(x)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isinf(R.bf(bits([0x7F7FFFFF])))[0])          # overflow rounds to inf, as the hardware conversion
    assert bool(torch.isnan(R.bf(torch.tensor([float("nan")])))[0])
    assert not torch.equal(R.trunc(x), got)                          # the slip differs from the rounding on this data


@pytest.mark.parametrize("case", [(9, 24, 20, 132, 1, True, True, True), (5, 6, 12, 37, 1, False, False, False)],
                         ids=("bidir_batch_first", "fwd_time_first"))
def test_unrounded_chain_is_torch_lstm_in_float64(case):
    ins = F64.lstm_inputs(case)
    ref = F64.lstm_run(ins, torch.float64)
    got = R.chain(ins, dtype=torch.float64, rnd=R.ident)
    for k in ref:
        assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), k


def test_unrounded_varlen_chain_is_torchs_packed_lstm():
    case = (6, 9, 10, 20, 1, True, True, True)
    mod, x, h0, c0, gy, gh, gc = F64.lstm_inputs(case)
    ln = [9, 4, 1, 9, 7, 2]
    m = torch.nn.LSTM(10, 20, 1, batch_first=True, bidirectional=True).double()
    m.load_state_dict(mod.state_dict())
    xd = x.double().requires_grad_()
    packed = torch.nn.utils.rnn.pack_padded_sequence(xd, ln, batch_first=True, enforce_sorted=False)
    y, (hn, cn) = m(packed, (h0.double(), c0.double()))
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=9)
    ((y * gy.double()).sum() + (hn * gh.double()).sum() + (cn * gc.double()).sum()).backward()
    got = R.chain((mod, x, h0, c0, gy, gh, gc), ln, dtype=torch.float64, rnd=R.ident)
    for k, ref in (("y", y), ("hn", hn), ("cn", cn), ("dx", xd.grad), ("dweight_hh_l0_reverse", m.weight_hh_l0_reverse.grad),
                   ("dbias_ih_l0", m.bias_ih_l0.grad)):
        assert float((got[k] - ref.detach()).abs().max()) <= 1e-12, k


@pytest.mark.parametrize("varlen", (False, True), ids=("fixed", "lengths"))
@pytest.mark.parametrize("bi", (False, True), ids=("fwd", "bidir"))
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "b%d_t%d_in%d_h%d" % s)
def test_checks_accept_the_emulation(shape, bi, varlen):
    """also asserts LSTM_MIN_RMS on every slice of the reference (inside seq_chain_check)"""
    B, T, In, H = shape
    case = (B, T, In, H, 1, bi, True, True)
    ins = F64.lstm_inputs(case)
    ln = lengths_of(B, T) if varlen else None
    r = R.check_forced(R.emulate(ins, ln), ins, ln, ALL, str(shape))
    assert r.min_rms >= F64.LSTM_MIN_RMS


def test_one_step_bound_accepts_the_emulation():
    for H in (16, 200, 209):
        case = F64.lstm_step_case(17, 24, H, True)
        ins = F64.lstm_inputs(case)
        out = R.emulate(ins, backward=False)
        F64.lstm_step_check(out, R.rounded_ins(ins), "emulate H=%d" % H)


SLIP_TENSOR = {"w_unrounded": "y", "y_rounded": "y", "c_rounded": ("y", "cn"), "truncate": "y", "kpad": "y", "gate_swap": "dx",
               "dgates_rounded": ("dx", "dgates"), "dead_carry": ("dx", "dh0")}


@pytest.mark.parametrize("slip", R.SLIPS)
def test_checks_reject_the_slip_and_name_the_tensor(slip):
    case = (9, 24, 20, 132, 1, True, True, True)
    ins = F64.lstm_inputs(case)
    ln = lengths_of(9, 24)
    with pytest.raises(AssertionError) as e:
        R.check_forced(R.emulate(ins, ln, slip=slip), ins, ln, ALL, "slip")
    named = SLIP_TENSOR[slip]
    named = (named,) if isinstance(named, str) else named
    assert any(("slip " + n) in str(e.value) for n in named), str(e.value)


# ----------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ----------------------------------------------------------------------------------------------------------------------
def desc(case, save=1):
    B, T, In, H, layers, bi, bf, _ = case
    return L.LSTMDesc(B, T, In, H, layers, int(bi), int(bf), save)


@pytest.mark.parametrize("case,use", F64.LSTM_CHAIN_CASES, ids=F64.LSTM_CHAIN_IDS)
def test_f32_workspace_queries_equal_the_old_ones(case, use):
    lib = L.lib()
    for save in (0, 1):
        d = desc(case, save)
        f, b = lib.ecgmm_lstm_fwd_workspace(C.byref(d)), lib.ecgmm_lstm_bwd_workspace(C.byref(d))
        assert f > 0 and b > 0
        assert lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), L.F32) == f
        assert lib.ecgmm_lstm_bwd_workspace_dt(C.byref(d), L.F32) == b
        assert lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), L.BF16) > f     # + the packed bf(W_hh)
        assert lib.ecgmm_lstm_bwd_workspace_dt(C.byref(d), L.BF16) > b


def test_bad_dtype_and_h_above_the_cap_return_zero_with_a_message():
    lib = L.lib()
    d = desc((8, 70, 512, 200, 3, True, True, True))
    assert lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), 7) == 0
    assert b"dtype" in lib.ecgmm_last_error()
    assert lib.ecgmm_lstm_bwd_workspace_dt(C.byref(d), -1) == 0
    assert b"dtype" in lib.ecgmm_last_error()
    d = desc((8, 70, 512, 385, 3, True, True, True))
    for dt in (L.F32, L.BF16):
        assert lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), dt) == 0
        assert b"cap of 384" in lib.ecgmm_last_error()
    off, nb = C.c_size_t(), C.c_size_t()
    assert lib.ecgmm_lstm_ws_view(C.byref(d), L.BF16, b"gates", 0, 0, C.byref(off), C.byref(nb)) != 0
    d = desc((8, 70, 512, 200, 3, True, True, True))
    assert lib.ecgmm_lstm_ws_view(C.byref(d), L.BF16, b"nonsense", 0, 0, C.byref(off), C.byref(nb)) != 0
    assert b"unknown view" in lib.ecgmm_last_error()
    assert lib.ecgmm_lstm_ws_view(C.byref(d), L.BF16, b"gates", 3, 0, C.byref(off), C.byref(nb)) != 0


@pytest.mark.parametrize("dt", (L.F32, L.BF16), ids=("f32", "bf16"))
def test_views_lie_inside_the_workspaces_without_overlap(dt):
    lib = L.lib()
    case = (8, 70, 512, 200, 3, True, True, True)
    d = desc(case)
    nf, nb_ = lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), dt), lib.ecgmm_lstm_bwd_workspace_dt(C.byref(d), dt)
    spans, BT, H = [], 8 * 70, 200
    for l in range(3):
        for k in range(2):
            for which, n in (("gates", 4 * H), ("c", H), ("hprev", H)):
                off, nb = C.c_size_t(), C.c_size_t()
                L.check(lib.ecgmm_lstm_ws_view(C.byref(d), dt, which.encode(), l, k, C.byref(off), C.byref(nb)), which)
                assert nb.value == BT * n * 4
                spans.append((off.value, off.value + nb.value))
        if l < 2:
            off, nb = C.c_size_t(), C.c_size_t()
            L.check(lib.ecgmm_lstm_ws_view(C.byref(d), dt, b"out", l, 0, C.byref(off), C.byref(nb)), "out")
            assert nb.value == BT * 2 * H * 4
            spans.append((off.value, off.value + nb.value))
    spans.sort()
    assert spans[0][0] >= 0 and spans[-1][1] <= nf
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    dg = []
    for k in range(2):
        off, nb = C.c_size_t(), C.c_size_t()
        L.check(lib.ecgmm_lstm_ws_view(C.byref(d), dt, b"dgates", 0, k, C.byref(off), C.byref(nb)), "dgates")
        dg.append((off.value, off.value + nb.value))
    assert dg[0][1] <= dg[1][0] and dg[1][1] <= nb_


# ----------------------------------------------------------------------------------------------------------------------
# the keyword
# ----------------------------------------------------------------------------------------------------------------------
def test_compute_dtype_keyword():
    from ecgmm.crnn import CRNN
    ref = HN.LSTM(12, 10, 2, bidirectional=True)
    m = HN.LSTM(12, 10, 2, bidirectional=True, compute_dtype="bf16")
    assert m.compute_dtype == "bf16" and ref.compute_dtype == "fp32"
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys()) == list(torch.nn.LSTM(12, 10, 2, bidirectional=True).state_dict().keys())
    assert all(p.dtype == torch.float32 for p in m.parameters())
    ref.load_state_dict(m.state_dict(), strict=True)       # a checkpoint does not carry the dtype
    assert ref.compute_dtype == "fp32"
    with pytest.raises(ValueError, match="fp16"):
        HN.LSTM(12, 10, compute_dtype="fp16")
    with pytest.raises(ValueError, match="compute_dtype"):
        HF.lstm(torch.zeros(2, 3, 12), None, list(m.parameters()), 10, compute_dtype="int8")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HN.LSTM(8, 16, batch_first=True, compute_dtype="bf16")(torch.zeros(2, 3, 8))
    assert CRNN(compute_dtype="bf16").bilstm.compute_dtype == "fp32"          # None means fp32 whatever compute_dtype is
    c = CRNN(compute_dtype="fp32", lstm_dtype="bf16")
    assert c.bilstm.compute_dtype == "bf16" and c.lstm_dtype == "bf16"
    assert list(c.state_dict().keys()) == list(CRNN().state_dict().keys())
    with pytest.raises(ValueError):
        CRNN(lstm_dtype="fp8")
