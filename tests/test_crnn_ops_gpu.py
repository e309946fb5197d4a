"""Per-op checks of the CRNN front end's kernels (csrc/crnn_front.hip; train_physionet2.py:55-65, 87-93) against torch on the
CPU in float64, built inside the test from the same operands.

5x5 convolutions, per op and per dtype: forward (+ BatchNorm partial rows) and input gradient through the implicit-GEMM
kernel at R = S = 5, pad 2, which no other test runs; the weight gradient through ecgmm_conv5_bwd_weight; the Cin = 1
convolution through ecgmm_conv5_in1_fwd / ecgmm_conv5_in1_bwd_weight.  bf16 goes through tests/f64check.py with its
constants unchanged (operands rounded to bf16); fp32 is held to the project's op bar max|a - ref| / max|ref| <= 2e-5
(tests/test_lstm_gpu.py's BAR).  Every output and workspace is NaN-filled first.

[BatchNorm -> ReLU -> MaxPool2d(2)] forward and backward against nn.BatchNorm2d -> ReLU -> MaxPool2d(2) in float64, train
and eval mode.  ReLU masks and pool winners are discontinuous, so the inputs are drawn (first seed of 50 that qualifies, on
the CPU, from the reference alone) such that no pre-activation lies within DELTA * max|z| of zero and no window's two largest
values are closer than that; DELTA = 1e-5 is 20x what separates the kernel's fp32 z from the reference's (the rounding of
the coefficients and one fma, ~4 ulp of max|z|).  Ties are covered by small-integer inputs, where values and routing must
equal torch's exactly.  Run with -s to see every figure."""
import copy
import ctypes as C
import functools

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from . import crnn_ref as R
from .util import DEV, TDT, bf16_round, conv_desc, dev, from_nhwc, pack_weight, rel_err, to_nhwc

pytestmark = pytest.mark.gpu
BAR = 2e-5
DELTA = 1e-5
# (N, H, W, Cin, Cout)
CONV_CASES = [(1, 4, 4, 32, 64),       # image smaller than filter plus pad
              (2, 7, 9, 32, 64),
              (3, 16, 37, 64, 128),    # ragged width
              (4, 16, 143, 32, 64)]    # enough pixels for several split-K slices
IN1_CASES = [(2, 9, 11), (1, 33, 70), (3, 5, 8)]
POOL_CASES = [(2, 9, 11, 32),          # both extents odd
              (3, 6, 13, 64),
              (2, 5, 8, 128),
              (1, 2, 2, 32)]
DTYPES = [L.BF16, L.F32]
DT_IDS = ["bf16", "fp32"]


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def relmax(a, ref, name):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(a).all(), name + ": NaN / inf in a result"
    r = ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()
    print("%-28s max|a - ref| / max|ref| = %.3g" % (name, r))
    return r


def colsum_ok(got, want, mag, name):
    """fp32 column sums (BatchNorm rows, bias gradients).  The op bar holds each summand to BAR of the largest one; a sum of
    them is then off by at most BAR * sum of magnitudes, which is the bound used here, and not by BAR * |sum|: `sum y` of a
    zero-mean conv output cancels to a small fraction of its magnitudes (about 1/8 at the (4, 16, 143) case), and no fp32
    summation can be held relative to that.  The measured ratio is printed; it is below 1e-6 in every case run here."""
    err = (got.double().cpu() - want.double()).abs()
    r = (err / mag.double().clamp_min(1e-300)).max().item()
    print("%-28s max |err| / sum of magnitudes = %.3g" % (name, r))
    assert torch.isfinite(got).all(), name
    return r <= BAR


def fp32_stats_ok(st, ref):
    y = ref.y
    return (colsum_ok(st[:, 0].double().sum(0), y.sum((0, 2, 3)), y.abs().sum((0, 2, 3)), "stats sum y")
            and colsum_ok(st[:, 1].double().sum(0), (y * y).sum((0, 2, 3)), (y * y).sum((0, 2, 3)), "stats sum y^2"))


@functools.lru_cache(maxsize=None)
def conv_inputs(case, dt):
    N, H, W, Cin, Cout = case
    torch.manual_seed(100 + N * 31 + W)
    rnd = bf16_round if dt == L.BF16 else (lambda t: t)
    x = rnd(torch.randn(N, Cin, H, W))
    w = rnd(torch.randn(Cout, Cin, 5, 5) / (25 * Cin) ** 0.5)
    b = torch.randn(Cout) * 0.1
    dy = rnd(torch.randn(N, Cout, H, W))
    ref = F64.conv_ref64(x, w, dy, padding=(2, 2), bias=b)
    return x, w, b, dy, ref


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv5_fwd_dgrad_wgrad(case, dt):
    """bf16: f64check's constants as they are."""
    N, H, W, Cin, Cout = case
    x, w, b, dy, ref = conv_inputs(case, dt)
    lib = L.lib()
    d = conv_desc(N, H, W, Cin, Cout, 5, 5, 1, 2, 2)
    xg, dyg = to_nhwc(x, dt), to_nhwc(dy, dt)
    wf, wd = pack_weight(w, dt)
    M = N * H * W
    rows = lib.ecgmm_conv_stats_rows(M)
    y = nan(M * Cout, dtype=TDT[dt])
    stats = nan(rows + 64, 2, Cout)
    n = C.c_int(0)
    L.check(lib.ecgmm_conv_fwd_wgrows(dt, C.byref(d), ptr(xg), ptr(wf), ptr(dev(b)), ptr(y), ptr(stats), C.byref(n), 0,
                                      stream()), "conv_fwd_wgrows")
    dx = nan(M * Cin, dtype=TDT[dt])
    L.check(lib.ecgmm_conv_bwd_data(dt, C.byref(d), ptr(dyg), ptr(wd), None, ptr(dx), stream()), "conv_bwd_data")
    nws = lib.ecgmm_conv5_bwd_weight_workspace(dt, C.byref(d))
    assert nws >= Cout * Cin * 25 * 4
    if case == CONV_CASES[3]:
        assert nws > Cout * Cin * 25 * 4, "this case is meant to run several split-K slices"
    ws = nan(nws // 4)
    dw = nan(Cout, Cin, 5, 5)
    L.check(lib.ecgmm_conv5_bwd_weight(dt, C.byref(d), ptr(xg), ptr(dyg), ptr(dw), 0, ptr(ws), nws, stream()),
            "conv5_bwd_weight")
    torch.cuda.synchronize()
    assert 1 <= n.value <= rows
    yc, dxc = from_nhwc(y, dt, (N, Cout, H, W)), from_nhwc(dx, dt, (N, Cin, H, W))
    st = stats[:n.value].cpu()
    if dt == L.BF16:
        F64.check_bf16(yc, ref.y, ref.ay, name="y")
        F64.check_stats(st, ref, name="stats")
        F64.check_bf16(dxc, ref.dx, ref.adx, name="dx")
        F64.check_dw(dw.cpu(), ref.dw, ref.adw, name="dw")
    else:
        assert relmax(yc, ref.y, "y") <= BAR
        assert fp32_stats_ok(st, ref)
        assert relmax(dxc, ref.dx, "dx") <= BAR
        assert relmax(dw, ref.dw, "dw") <= BAR


def test_conv5_bwd_weight_accumulate_and_rerun():
    """accumulate = 1 adds into dw; a second run gives the same bits (fixed-order reduce)"""
    case, dt = CONV_CASES[1], L.F32
    N, H, W, Cin, Cout = case
    x, w, b, dy, ref = conv_inputs(case, dt)
    lib = L.lib()
    d = conv_desc(N, H, W, Cin, Cout, 5, 5, 1, 2, 2)
    xg, dyg = to_nhwc(x, dt), to_nhwc(dy, dt)
    nws = lib.ecgmm_conv5_bwd_weight_workspace(dt, C.byref(d))
    ws = nan(nws // 4)
    torch.manual_seed(5)
    base = torch.randn(Cout, Cin, 5, 5)
    dw = dev(base.clone())
    L.check(lib.ecgmm_conv5_bwd_weight(dt, C.byref(d), ptr(xg), ptr(dyg), ptr(dw), 1, ptr(ws), nws, stream()))
    again = [nan(Cout, Cin, 5, 5) for _ in range(2)]
    for t in again:
        L.check(lib.ecgmm_conv5_bwd_weight(dt, C.byref(d), ptr(xg), ptr(dyg), ptr(t), 0, ptr(ws), nws, stream()))
    torch.cuda.synchronize()
    assert relmax(dw.cpu().double() - base.double(), ref.dw, "dw (accumulate)") <= BAR
    assert torch.equal(again[0], again[1])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", IN1_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv5_in1_fwd_and_bwd_weight(case, dt):
    """bf16: f64check's constants as they are."""
    N, H, W = case
    torch.manual_seed(200 + N * 31 + W)
    rnd = bf16_round if dt == L.BF16 else (lambda t: t)
    x = torch.randn(N, 1, H, W)
    w = torch.randn(32, 1, 5, 5) * 0.2
    b = torch.randn(32) * 0.1
    dy = rnd(torch.randn(N, 32, H, W))
    ref = F64.conv_ref64(rnd(x), rnd(w), dy, padding=(2, 2), bias=b)   # the kernel rounds x and w itself
    db_ref, adb = dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
    lib = L.lib()
    M = N * H * W
    rows = lib.ecgmm_conv5_in1_stats_rows(N, H, W)
    assert rows >= 1
    y = nan(M * 32, dtype=TDT[dt])
    stats = nan(rows + 64, 2, 32)
    xg, wg = dev(x), dev(w)
    L.check(lib.ecgmm_conv5_in1_fwd(dt, ptr(xg), ptr(wg), ptr(dev(b)), ptr(y), ptr(stats), N, H, W, stream()), "conv5_in1_fwd")
    nws = lib.ecgmm_conv5_in1_bwd_weight_workspace(N, H, W)
    assert nws > 0
    ws = nan(nws // 4)
    dw, db = nan(32, 1, 5, 5), nan(32)
    dyg = to_nhwc(dy, dt)
    L.check(lib.ecgmm_conv5_in1_bwd_weight(dt, ptr(xg), ptr(dyg), ptr(dw), ptr(db), 0, ptr(ws), nws, N, H, W, stream()),
            "conv5_in1_bwd_weight")
    dw2, db2 = dw.clone(), db.clone()
    L.check(lib.ecgmm_conv5_in1_bwd_weight(dt, ptr(xg), ptr(dyg), ptr(dw2), ptr(db2), 1, ptr(ws), nws, N, H, W, stream()),
            "conv5_in1_bwd_weight accumulate")
    torch.cuda.synchronize()
    yc, st = from_nhwc(y, dt, (N, 32, H, W)), stats[:rows].cpu()
    assert torch.equal(dw2, 2 * dw) and torch.equal(db2, 2 * db)
    if dt == L.BF16:
        F64.check_bf16(yc, ref.y, ref.ay, name="y")
        F64.check_stats(st, ref, name="stats")
        F64.check_dw(dw.cpu(), ref.dw, ref.adw, name="dw")
        F64.check_dw(db.cpu(), db_ref, adb, name="dbias")
    else:
        assert relmax(yc, ref.y, "y") <= BAR
        assert fp32_stats_ok(st, ref)
        assert relmax(dw, ref.dw, "dw") <= BAR
        assert colsum_ok(db, db_ref, adb, "dbias")


# ---------------------------------------------------------------------------------------------------
# [BatchNorm -> ReLU -> MaxPool2d(2)]
# ---------------------------------------------------------------------------------------------------
def pool_reference(y, gamma, beta, rm, rv, dp, training, eps=1e-5, momentum=0.1):
    """float64 nn modules; returns outputs, gradients, buffers and the pre-activation z"""
    Cn = y.shape[1]
    bn = torch.nn.BatchNorm2d(Cn, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train(training)
    yy = y.double().clone().requires_grad_()
    z = bn(yy)
    out = torch.nn.MaxPool2d(2)(torch.relu(z))
    out.backward(dp.double())
    return {"out": out.detach(), "dy": yy.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "z": z.detach(),
            "rm": bn.running_mean.clone(), "rv": bn.running_var.clone(), "nbt": int(bn.num_batches_tracked)}


def margins_ok(z, delta):
    d = delta * z.abs().max()
    if (z.abs() < d).any():
        return False
    N, Cn, H, W = z.shape
    r = torch.relu(z)[:, :, :H // 2 * 2, :W // 2 * 2]
    win = r.reshape(N, Cn, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, Cn, H // 2, W // 2, 4)
    top = win.sort(-1, descending=True).values
    gap = top[..., 0] - top[..., 1]   # (equal values are a tie, which both sides give to the first element: no hazard)
    return not ((gap > 0) & (gap < d)).any()


@functools.lru_cache(maxsize=None)
def pool_inputs(case, training, dt):
    N, H, W, Cn = case
    rnd = bf16_round if dt == L.BF16 else (lambda t: t)
    for seed in range(50):
        torch.manual_seed(1000 * seed + N * 7 + W)
        y = rnd(torch.randn(N, Cn, H, W) * 1.5 + 0.3)
        gamma, beta = torch.rand(Cn) + 0.5, torch.randn(Cn) * 0.3
        rm, rv = torch.randn(Cn) * 0.2, torch.rand(Cn) + 0.5
        dp = rnd(torch.randn(N, Cn, H // 2, W // 2))
        ref = pool_reference(y, gamma, beta, rm, rv, dp, training)
        if margins_ok(ref["z"], DELTA):
            return y, gamma, beta, rm, rv, dp, ref
    raise AssertionError("no seed among the first 50 keeps every pre-activation and pool window clear of its margin")


def pool_run(y, gamma, beta, rm, rv, dp, training, dt, seq=False, eps=1e-5, momentum=0.1):
    """col_stats + bn_finalize (or bn_eval_coef) -> ecgmm_bnrelu_maxpool2 -> ecgmm_pool2_bn_bwd, outputs NaN-filled first"""
    lib = L.lib()
    N, Cn, H, W = y.shape
    PH, PW, M = H // 2, W // 2, N * H * W
    yg = to_nhwc(y, dt)
    g, b, rmg, rvg = dev(gamma), dev(beta), dev(rm), dev(rv)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    coef = nan(4, Cn)
    if training:
        rows = lib.ecgmm_col_stats_rows(dt, M, Cn)
        part = nan(rows + 64, 2, Cn)
        L.check(lib.ecgmm_col_stats(dt, ptr(yg), M, Cn, ptr(part), stream()), "col_stats")
        L.check(lib.ecgmm_bn_finalize(ptr(part), rows, Cn, float(M), ptr(g), ptr(b), ptr(rmg), ptr(rvg), ptr(nbt), momentum,
                                      eps, ptr(coef), stream()), "bn_finalize")
    else:
        L.check(lib.ecgmm_bn_eval_coef(Cn, ptr(g), ptr(b), ptr(rmg), ptr(rvg), eps, ptr(coef), stream()), "bn_eval_coef")
    odt = torch.float32 if seq else TDT[dt]
    out = nan(N * PH * PW * Cn, dtype=odt)
    idx = torch.full((N * PH * PW * Cn,), 255, dtype=torch.uint8, device=DEV)
    L.check(lib.ecgmm_bnrelu_maxpool2(dt, ptr(yg), ptr(coef), ptr(out), ptr(idx), N, H, W, Cn, int(seq), stream()),
            "bnrelu_maxpool2")
    if seq:
        dpg = dev(dp.permute(0, 3, 1, 2).reshape(N, PW, Cn * PH).float())
    else:
        dpg = to_nhwc(dp, dt)
    nws = lib.ecgmm_pool2_bn_bwd_workspace(N, H, W, Cn)
    assert nws > 0
    ws = nan(nws // 4)
    dy = nan(M * Cn, dtype=TDT[dt])
    dgamma, dbeta, dbias = nan(Cn), nan(Cn), nan(Cn)
    L.check(lib.ecgmm_pool2_bn_bwd(dt, ptr(dpg), ptr(idx), ptr(yg), ptr(coef), int(training), ptr(dgamma), ptr(dbeta), ptr(dy),
                                   ptr(dbias), N, H, W, Cn, int(seq), ptr(ws), nws, stream()), "pool2_bn_bwd")
    torch.cuda.synchronize()
    if seq:
        o = out.view(N, PW, Cn, PH).permute(0, 2, 3, 1).cpu()
    else:
        o = from_nhwc(out, dt, (N, Cn, PH, PW))
    return {"out": o, "dy": from_nhwc(dy, dt, (N, Cn, H, W)), "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu(),
            "dbias": dbias.cpu(), "idx": idx.view(N, PH, PW, Cn).permute(0, 3, 1, 2).cpu(), "rm": rmg.cpu(), "rv": rvg.cpu(),
            "nbt": int(nbt.item())}


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool2_fp32_vs_float64(case, training):
    y, gamma, beta, rm, rv, dp, ref = pool_inputs(case, training, L.F32)
    got = pool_run(y, gamma, beta, rm, rv, dp, training, L.F32)
    for k in ("out", "dy", "dgamma", "dbeta"):
        assert relmax(got[k], ref[k], k) <= BAR, k
    # the bias gradient of the convolution in front is the column sum of dy (exactly 0 in training mode): held to the
    # op bar relative to the column's sum of magnitudes
    err = (got["dbias"].double() - ref["dy"].sum((0, 2, 3))).abs().max().item()
    mag = ref["dy"].abs().sum((0, 2, 3)).max().item()
    print("dbias: |err| %.3g, sum|dy| %.3g" % (err, mag))
    assert err <= BAR * mag
    if training:
        assert relmax(got["rm"], ref["rm"], "running_mean") <= BAR and relmax(got["rv"], ref["rv"], "running_var") <= BAR
        assert got["nbt"] == ref["nbt"] == 1
    else:
        assert torch.equal(got["rm"], rm) and torch.equal(got["rv"], rv) and got["nbt"] == 0
    # rows / columns the floor dropped: no pooled gradient reaches them (eval mode: dy is exactly zero there)
    N, H, W, Cn = case
    if not training:
        assert (got["dy"][:, :, H // 2 * 2:, :] == 0).all() and (got["dy"][:, :, :, W // 2 * 2:] == 0).all()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_pool2_lstm_layout(training):
    """the third block's pool writes seq[b][t][c * F' + f] fp32 and its backward reads dseq the same way"""
    case = POOL_CASES[2]
    y, gamma, beta, rm, rv, dp, ref = pool_inputs(case, training, L.F32)
    plain = pool_run(y, gamma, beta, rm, rv, dp, training, L.F32)
    got = pool_run(y, gamma, beta, rm, rv, dp, training, L.F32, seq=True)
    for k in ("out", "dy", "dgamma", "dbeta", "dbias", "idx"):
        assert torch.equal(got[k], plain[k]), k
    assert relmax(got["out"], ref["out"], "seq out") <= BAR


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool2_bf16_vs_float64(case, training):
    """bf16 storage: y and dp are given in bf16 (exactly, to both sides), so the kernel's fp32 z and with it every mask and
    winner are the reference's (same margins as fp32); what differs is the rounding of the stored out / dy: half a bf16 ulp
    (2^-9 relative) plus the fp32 bar, and for the fp32 sums the fp32 bar alone."""
    y, gamma, beta, rm, rv, dp, ref = pool_inputs(case, training, L.BF16)
    got = pool_run(y, gamma, beta, rm, rv, dp, training, L.BF16)
    for k in ("out", "dy"):
        a, r = got[k].double(), ref[k]
        err = (a - r).abs()
        bound = F64.half_ulp_bf16(r.abs() + BAR * r.abs().max()) + BAR * r.abs().max()
        print("%-8s worst |err| / bound %.3g" % (k, (err / bound).max().item()))
        assert torch.isfinite(a).all() and (err <= bound).all(), k
    for k in ("dgamma", "dbeta"):
        assert relmax(got[k], ref[k], k) <= BAR, k


def test_pool2_ties_match_torch_exactly():
    """small integers, identity BatchNorm (gamma = 1, beta = 0, running_mean = 0, running_var + eps = 1): windows full of
    ties; pooled values, winners and the routed gradient must equal torch's bit for bit"""
    N, Cn, H, W = 2, 32, 7, 10
    torch.manual_seed(3)
    y = torch.randint(-1, 3, (N, Cn, H, W)).float()
    dp = torch.randint(1, 9, (N, Cn, H // 2, W // 2)).float()
    one, zero = torch.ones(Cn), torch.zeros(Cn)
    rv, eps = torch.full((Cn,), 0.75), 0.25
    for dt in DTYPES:
        got = pool_run(y, one, zero, zero, rv, dp, False, dt, eps=eps)
        yy = y.clone().requires_grad_()
        out, idx = torch.nn.functional.max_pool2d(torch.relu(yy), 2, return_indices=True)
        out.backward(dp)
        assert torch.equal(got["out"], out.detach())
        assert torch.equal(got["dy"], yy.grad)
        h0 = torch.arange(H // 2).view(1, 1, -1, 1) * 2
        w0 = torch.arange(W // 2).view(1, 1, 1, -1) * 2
        want = ((idx // W) - h0) * 2 + ((idx % W) - w0)
        assert torch.equal(got["idx"].long(), want)
        assert torch.equal(got["dbeta"], yy.grad.sum((0, 2, 3)))


# ---------------------------------------------------------------------------------------------------
# One block and the whole front end through the launch plan (ecgmm_crnn_front_*, HF.crnn_front)
# ---------------------------------------------------------------------------------------------------
# The issue's shapes (3, 33, 45), (2, 17, 24), (5, 8, 8) hold 1e4 .. 2e5 pre-activations; with a margin of 1e-4 * max|z| about
# 3e-4 of them fall inside it, so no seed can clear them (searched: none of the first 50).  As the margin must not shrink,
# the cases do: one sample with both extents odd, one with a ragged time axis, one with two samples at the smallest extents.
FRONT_CASES = [(1, 9, 9), (1, 8, 11), (2, 8, 8)]
FRONT_DELTA = 1e-4


@functools.lru_cache(maxsize=None)
def front_inputs(case, training):
    B, Fq, T = case
    for seed in range(50):
        m = R.front_only(seed).double()
        m.train(training)
        torch.manual_seed(7000 + seed)
        x = torch.randn(B, 1, Fq, T)
        with torch.no_grad():
            bad = R.margin_violations(copy.deepcopy(m), x.double(), FRONT_DELTA)
        if not bad:
            torch.manual_seed(9000 + seed)
            return m, x, torch.randn(B, T // 8, 128 * (Fq // 8))
    raise AssertionError("no seed among the first 50 clears the margins for %r" % (case,))


def front_reference(m, x, g, training):
    m = copy.deepcopy(m)
    m.train(training)
    assert not R.margin_violations(copy.deepcopy(m), x.double(), FRONT_DELTA)   # on the reference alone, nothing excluded
    seq = m.front(x.double())
    (seq * g.double()).sum().backward()
    return seq.detach(), {k: p.grad for k, p in m.named_parameters()}, {k: v for k, v in m.named_buffers()}


def front_run(m, x, g, training, dtype):
    from ecgmm.hip import functional as HF
    mine = copy.deepcopy(m).float().to(DEV)
    params, buffers = [], []
    for name in ("conv1", "conv2", "conv3"):
        conv, bn = getattr(mine, name).block[0], getattr(mine, name).block[1]
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
        buffers += [bn.running_mean, bn.running_var, bn.num_batches_tracked]
    seq = HF.crnn_front(dev(x), params, buffers, training, 0.1, 1e-5, dtype)
    (seq * dev(g)).sum().backward()
    torch.cuda.synchronize()
    return seq.detach().cpu(), {k: p.grad.cpu() for k, p in mine.named_parameters()}, {k: v.cpu() for k, v in mine.named_buffers()}


def compare_front(got, ref, training):
    """test_models_gpu.py's fp32 bars: output within 1e-3 * max(1, |ref|max), each gradient rel_err < 5e-3.  A conv bias in front
    of a training-mode BatchNorm has a true gradient of exactly zero (rounding noise on both sides): held absolutely, as
    test_models_gpu.py does for the signal encoder's."""
    seq, grads, bufs = got
    rseq, rgrads, rbufs = ref
    err = (seq.double() - rseq).abs().max().item()
    print("seq max|err| %.3g (|ref|max %.3g)" % (err, rseq.abs().max().item()))
    assert torch.isfinite(seq).all() and err <= 1e-3 * max(1.0, rseq.abs().max().item())
    for k, r in rgrads.items():
        if training and k.endswith("block.0.bias"):
            print("%-28s |grad|max %.3g (true value 0)" % (k, grads[k].abs().max().item()))
            assert grads[k].abs().max().item() < 1e-3, k
            continue
        e = rel_err(grads[k], r)
        print("%-28s rel_err %.3g" % (k, e))
        assert e < 5e-3, (k, e)
    for k, r in rbufs.items():
        assert torch.allclose(bufs[k].double(), r.double(), rtol=5e-3, atol=1e-4), k


@pytest.mark.parametrize("case", FRONT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_front_end_fp32_train(case):
    m, x, g = front_inputs(case, True)
    compare_front(front_run(m, x, g, True, L.F32), front_reference(m, x, g, True), True)


def test_front_end_fp32_eval_forward_backward():
    m, x, g = front_inputs(FRONT_CASES[0], False)
    compare_front(front_run(m, x, g, False, L.F32), front_reference(m, x, g, False), False)


@pytest.mark.parametrize("case", FRONT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_one_block_fp32(case):
    """the first block alone out of the plan's forward workspace is not exposed; one block = the per-op chain a host composes
    (INTEGRATION.md): conv5_in1_fwd -> bn_finalize over its rows -> bnrelu_maxpool2 -> pool2_bn_bwd (dbias) -> conv5_in1_bwd_weight"""
    m, x, _ = front_inputs(case, True)
    blk = copy.deepcopy(m.conv1).double().train()
    B, Fq, T = case
    torch.manual_seed(11)
    dp = torch.randn(B, 32, Fq // 2, T // 2)
    out = blk(x.double())
    (out * dp.double()).sum().backward()
    lib = L.lib()
    conv, bn = blk.block[0], blk.block[1]
    M = B * Fq * T
    xg, w, b = dev(x), dev(conv.weight.detach().float()), dev(conv.bias.detach().float())
    rows = lib.ecgmm_conv5_in1_stats_rows(B, Fq, T)
    y, stats, coef = nan(M * 32), nan(rows + 64, 2, 32), nan(4, 32)
    L.check(lib.ecgmm_conv5_in1_fwd(L.F32, ptr(xg), ptr(w), ptr(b), ptr(y), ptr(stats), B, Fq, T, stream()))
    gm, bt = dev(torch.ones(32)), dev(torch.zeros(32))
    rm, rv, nbt = dev(torch.zeros(32)), dev(torch.ones(32)), torch.zeros((), dtype=torch.long, device=DEV)
    L.check(lib.ecgmm_bn_finalize(ptr(stats), rows, 32, float(M), ptr(gm), ptr(bt), ptr(rm), ptr(rv), ptr(nbt), 0.1, 1e-5,
                                  ptr(coef), stream()))
    PH, PW = Fq // 2, T // 2
    o, idx = nan(B * PH * PW * 32), torch.zeros(B * PH * PW * 32, dtype=torch.uint8, device=DEV)
    L.check(lib.ecgmm_bnrelu_maxpool2(L.F32, ptr(y), ptr(coef), ptr(o), ptr(idx), B, Fq, T, 32, 0, stream()))
    nws = lib.ecgmm_pool2_bn_bwd_workspace(B, Fq, T, 32)
    ws, dy, dgm, dbt, dbias = nan(nws // 4), nan(M * 32), nan(32), nan(32), nan(32)
    L.check(lib.ecgmm_pool2_bn_bwd(L.F32, ptr(to_nhwc(dp, L.F32)), ptr(idx), ptr(y), ptr(coef), 1, ptr(dgm), ptr(dbt), ptr(dy),
                                   ptr(dbias), B, Fq, T, 32, 0, ptr(ws), nws, stream()))
    nw2 = lib.ecgmm_conv5_in1_bwd_weight_workspace(B, Fq, T)
    ws2, dw = nan(nw2 // 4), nan(32, 1, 5, 5)
    L.check(lib.ecgmm_conv5_in1_bwd_weight(L.F32, ptr(xg), ptr(dy), ptr(dw), None, 0, ptr(ws2), nw2, B, Fq, T, stream()))
    torch.cuda.synchronize()
    oc = from_nhwc(o, L.F32, (B, 32, PH, PW))
    assert (oc.double() - out.detach()).abs().max().item() <= 1e-3 * max(1.0, out.abs().max().item())
    for name, a, r in (("weight", dw.cpu(), conv.weight.grad), ("bn.weight", dgm.cpu(), bn.weight.grad),
                       ("bn.bias", dbt.cpu(), bn.bias.grad)):
        e = rel_err(a, r)
        print("%-10s rel_err %.3g" % (name, e))
        assert e < 5e-3, name
    assert dbias.abs().max().item() < 1e-3
    assert torch.allclose(rm.cpu().double(), bn.running_mean, rtol=5e-3, atol=1e-4)
    assert torch.allclose(rv.cpu().double(), bn.running_var, rtol=5e-3, atol=1e-4) and int(nbt) == 1


@pytest.mark.parametrize("case", [(3, 33, 45)], ids=lambda c: "x".join(map(str, c)))
def test_front_end_bf16_vs_autocast(case):
    """the project's bf16 yardstick (test_models_gpu.py): deviation from the fp32 reference at most 1.3x that of torch's CPU
    bf16 autocast of the same modules, plus 0.02"""
    B, Fq, T = case
    m = R.front_only(3)
    torch.manual_seed(77)
    x, g = torch.randn(B, 1, Fq, T), torch.randn(B, T // 8, 128 * (Fq // 8))

    def run_ref(autocast):
        r = copy.deepcopy(m).train()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f = r.front(x)
        (f.float() * g).sum().backward()
        return f.detach().float(), {k: p.grad.clone() for k, p in r.named_parameters()}
    f32, g32 = run_ref(False)
    f16, g16 = run_ref(True)
    seq, grads, _ = front_run(m, x, g, True, L.BF16)
    assert torch.isfinite(seq).all()
    mine, theirs = rel_err(seq, f32), rel_err(f16, f32)
    print("seq: ours %.3g, autocast %.3g" % (mine, theirs))
    assert mine < 1.3 * theirs + 0.02
    bad = []
    for k in g32:
        if k.endswith("block.0.bias"):   # true gradient 0 in front of a training-mode BatchNorm
            continue
        a, b = rel_err(grads[k], g32[k]), rel_err(g16[k], g32[k])
        print("%-28s ours %.3g, autocast %.3g" % (k, a, b))
        if not a < 1.3 * b + 0.02:
            bad.append((k, a, b))
    assert not bad, bad
