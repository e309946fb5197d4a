"""nn.LSTM on the HIP recurrence kernels against torch.nn.LSTM on the CPU in float64 (the call train_physionet2.py:75-76,94
makes), same weights, inputs and states.  Error per tensor: max|a - ref| / max|ref|; bar 2e-5, the project's fp32 op-level
bar.  Every test prints its worst figure next to torch-CPU-fp32's own deviation from float64 (run with -s).

Which file holds which check: this one holds the whole-tensor bar above and the behaviour of the module path (frozen
parameters, gradient sinks, state dicts, no_grad, the three-step tail); tests/test_lstm_f64_gpu.py holds the element-by-element
float64 checks of the recurrence (the per-time-step chain bar at every tiling of H, the derived single-step bound, null
pointers, sentinels, causality, seq_mean), whose bounds are derived in tests/f64check.py.  test_partial_cotangents and
test_parity_with_torch_float64 run the per-slice check on y and dx as well.  The ABI runner is tests/lstm_abi.py."""
import functools

import pytest
import torch

from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip import nn as HN
from ecgmm.optim import FusedAdam

from . import f64check as F64
from . import lstm_abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-5
# (B, T, In, H, layers, bidirectional, batch_first, h0/c0 given)
CASES = [
    (1, 1, 8, 4, 1, False, True, False),       # single row, single step, H below one MFMA tile
    (5, 7, 3, 37, 2, True, True, True),        # odd H, In below the MFMA path of linear, layer 2 reading 2H
    (17, 5, 512, 200, 1, True, True, False),   # CRNN layer-1 widths, H = 12*16 + 8, one full slice + one row
    (33, 12, 512, 200, 3, True, True, True),   # the CRNN stack, two slices + one row, 400-wide inner layers
    (16, 70, 24, 200, 1, False, False, True),  # CRNN's T, time-major memory, exactly one slice
    (3, 4, 400, 200, 1, True, False, False),   # time-major + reverse direction
]
IDS = ["b1t1h4", "b5h37x2bi", "b17h200bi", "b33crnn", "t70tmajor", "tmajor_rev"]
SMALL = CASES[1]


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(a).all(), "NaN / inf in a result"
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


inputs = F64.lstm_inputs     # (torch module, x, h0, c0, gy, gh, gc) of a case, cached


def torch_run(case, dtype, wscale=1.0, xscale=1.0, use=("y", "h", "c")):
    """torch.nn.LSTM on the CPU in `dtype`: outputs and every gradient of sum y gy + sum h_n gh + sum c_n gc."""
    return F64.lstm_run(inputs(case, wscale, xscale), dtype, use)


@functools.lru_cache(maxsize=None)
def reference(case, wscale=1.0, xscale=1.0, use=("y", "h", "c")):
    """(float64 reference, torch-fp32's own worst deviation from it); computed once per case and never modified"""
    r64, r32 = F64.lstm_refs(case, tuple(use), wscale, xscale)
    own = max(rel(r32[k], r64[k]) for k in r64)
    return r64, own


def abi_run(case, wscale=1.0, xscale=1.0):
    """the C entry points with every output, the workspace and the scratch NaN-filled first (tests/lstm_abi.py)"""
    return lstm_abi.run(case, inputs(case, wscale, xscale))


def slice_check(out, case, tag, use=("y", "h", "c")):
    """the per-slice float64 check (tests/f64check.py, the LSTM section) of y and dx"""
    r64, r32 = F64.lstm_refs(case, tuple(use))
    F64.lstm_chain_check({k: out[k].detach().cpu() for k in ("y", "dx")}, r64, r32, case[6], tag, keys=("y", "dx"))


def check(out, case, tag, wscale=1.0, xscale=1.0, use=("y", "h", "c"), keys=None):
    ref, own = reference(case, wscale, xscale, use)
    errs = {k: rel(out[k], ref[k]) for k in (keys or ref)}
    worst = max(errs, key=errs.get)
    print(f"\n[lstm {tag}] worst {errs[worst]:.2e} ({worst}); torch-fp32's own worst {own:.2e}; bar {BAR:.0e}")
    assert errs[worst] < BAR, errs
    return errs


def module_for(case, wscale=1.0, xscale=1.0):
    B, T, In, H, layers, bi, bf, given = case
    mod = inputs(case, wscale, xscale)[0]
    m = HN.LSTM(In, H, layers, batch_first=bf, bidirectional=bi)
    m.load_state_dict(mod.state_dict(), strict=True)
    return m.to(DEV)


def module_run(case, use=("y", "h", "c"), x_grad=True, freeze=False, m=None):
    mod, x, h0, c0, gy, gh, gc = inputs(case)
    m = m or module_for(case)
    if freeze:
        for p in m.parameters():
            p.requires_grad_(False)
    x = x.to(DEV).requires_grad_(x_grad)
    hx = None if h0 is None else (h0.to(DEV).requires_grad_(), c0.to(DEV).requires_grad_())
    y, (hn, cn) = m(x, hx)
    loss = 0
    if "y" in use:
        loss = loss + (y * gy.to(DEV)).sum()
    if "h" in use:
        loss = loss + (hn * gh.to(DEV)).sum()
    if "c" in use:
        loss = loss + (cn * gc.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = {"y": y, "hn": hn, "cn": cn}
    if x_grad:
        out["dx"] = x.grad
    if hx is not None:
        out["dh0"], out["dc0"] = hx[0].grad, hx[1].grad
    for n, p in m.named_parameters():
        if p.grad is not None:
            out["d" + n] = p.grad
    return out, m


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_with_torch_float64(case):
    out = abi_run(case)
    check(out, case, "parity " + IDS[CASES.index(case)])
    slice_check(out, case, "parity " + IDS[CASES.index(case)])


def test_saturated_gates_stay_finite_and_exact():
    case = CASES[4]
    ref, _ = reference(case, 3.0, 4.0)
    assert all(torch.isfinite(v).all() for v in ref.values())
    check(abi_run(case, 3.0, 4.0), case, "saturation (weights x3, inputs x4)", 3.0, 4.0)


def test_frozen_parameters_only_dx():
    out, m = module_run(SMALL, freeze=True)
    assert all(p.grad is None for p in m.parameters())
    check(out, SMALL, "frozen parameters", keys=["y", "hn", "cn", "dx", "dh0", "dc0"])


def test_input_without_grad_gives_the_same_parameter_gradients():
    full, _ = module_run(SMALL)
    part, _ = module_run(SMALL, x_grad=False)
    assert "dx" not in part
    for k in full:
        if k.startswith("dweight") or k.startswith("dbias"):
            assert torch.equal(full[k], part[k]), k
    check(full, SMALL, "module path, full request")


@pytest.mark.parametrize("use", [("y",), ("h",)], ids=["loss_on_y", "loss_on_hn"])
def test_partial_cotangents(use):
    out, _ = module_run(SMALL, use=use)
    check(out, SMALL, "cotangent " + use[0] + " only", use=use)
    slice_check(out, SMALL, "cotangent " + use[0] + " only", use=use)


def test_no_grad_saves_nothing_and_matches():
    mod, x, h0, c0, *_ = inputs(SMALL)
    m = module_for(SMALL)
    with torch.no_grad():
        y, (hn, cn) = m(x.to(DEV), (h0.to(DEV), c0.to(DEV)))
    assert y.grad_fn is None
    check({"y": y, "hn": hn, "cn": cn}, SMALL, "no_grad forward", keys=["y", "hn", "cn"])


def test_two_identical_calls_are_bit_identical():
    a, b = abi_run(CASES[3]), abi_run(CASES[3])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_rows_do_not_depend_on_the_rest_of_the_batch():
    case = CASES[3]
    B, T, In, H, layers, bi, bf, given = case
    mod, x, h0, c0, *_ = inputs(case)
    m = module_for(case)
    with torch.no_grad():
        y33, (h33, c33) = m(x.to(DEV), (h0.to(DEV), c0.to(DEV)))
        y5, (h5, c5) = m(x[:5].contiguous().to(DEV), (h0[:, :5].contiguous().to(DEV), c0[:, :5].contiguous().to(DEV)))
    assert torch.equal(y33[:5], y5) and torch.equal(h33[:, :5], h5) and torch.equal(c33[:, :5], c5)


def test_second_backward_into_a_dirty_sink_raises():
    _, m = module_run(SMALL)
    with pytest.raises(RuntimeError, match="gradient sink written twice"):
        module_run(SMALL, m=m)
    HF.release_grads(m)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    out, _ = module_run(SMALL, m=m)
    check(out, SMALL, "after release_grads")


def test_autograd_grad_wrt_inputs_leaves_dot_grad_alone():
    mod, x, *_ = inputs(CASES[2])
    m = module_for(CASES[2])
    xd = x.to(DEV).requires_grad_()
    y, _ = m(xd)
    (dx,) = torch.autograd.grad(y.sum(), xd)
    assert all(p.grad is None for p in m.parameters()) and torch.isfinite(dx).all()


def test_state_dicts_move_both_ways():
    case = CASES[2]
    mod, x, *_ = inputs(case)
    m = module_for(case)            # torch -> ours (strict)
    with torch.no_grad():
        y, (hn, cn) = m.eval()(x.to(DEV))
        yt, _ = m.train()(x.to(DEV))
    assert torch.equal(y, yt)       # train and eval compute the same function
    check({"y": y, "hn": hn, "cn": cn}, case, "interop", keys=["y", "hn", "cn"])
    back = torch.nn.LSTM(case[2], case[3], case[4], batch_first=case[6], bidirectional=case[5])
    back.load_state_dict(m.state_dict(), strict=True)
    for (n, p), (_, q) in zip(back.named_parameters(), mod.named_parameters()):
        assert torch.equal(p, q), n


class _Tail(torch.nn.Module):
    """train_physionet2.py:75-95 behind the conv front end, without Dropout(0.3): BiLSTM -> mean over T -> classifier"""

    def __init__(self, hip):
        super().__init__()
        nn_ = HN if hip else torch.nn
        self.hip = hip
        self.bilstm = nn_.LSTM(512, 200, 3, batch_first=True, bidirectional=True)
        self.fc1, self.fc2 = nn_.Linear(400, 64), nn_.Linear(64, 2)

    def forward(self, x):
        y, _ = self.bilstm(x)
        if self.hip:
            return self.fc2(self.fc1(HF.seq_mean(y), act=L.ACT_RELU))
        return self.fc2(torch.relu(self.fc1(y.mean(dim=1))))


def test_crnn_tail_three_optimizer_steps():
    torch.manual_seed(7)
    ref = _Tail(False)
    ours = _Tail(True)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ours = ours.to(DEV)
    ref = ref.double()
    xs = torch.randn(3, 8, 9, 512)
    ys = torch.randint(0, 2, (3, 8))
    o_ref, o_hip = torch.optim.Adam(ref.parameters(), lr=1e-4), FusedAdam(ours.parameters(), lr=1e-4)
    for i in range(3):
        ce = torch.nn.functional.cross_entropy(ref(xs[i].double()), ys[i], reduction="none")
        lr_ = ((1 - torch.exp(-ce)) ** 2 * ce).mean()      # FocalLoss(alpha=1, gamma=2), train_physionet2.py:104-117
        o_ref.zero_grad()
        lr_.backward()
        o_ref.step()
        lh = HF.focal_loss(ours(xs[i].to(DEV)), ys[i].to(DEV))
        o_hip.zero_grad()
        lh.backward()
        o_hip.step()
        print(f"\n[lstm tail] step {i}: loss {lh.item():.6f} vs float64 {lr_.item():.6f}")
        assert abs(lh.item() - lr_.item()) < 2e-3
    errs = {n: rel(p, dict(ref.bilstm.named_parameters())[n]) for n, p in ours.bilstm.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"[lstm tail] worst LSTM weight after 3 steps: {errs[worst]:.2e} ({worst}); bar 1e-3")
    assert errs[worst] < 1e-3, errs
