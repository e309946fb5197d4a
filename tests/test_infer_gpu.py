"""The inference plans on the GPU: the fold kernel against float64, the fused forward conv epilogue (bias + addend + ReLU)
at the step's layer shapes, the encoders through ``ecgmm.inference.Predictor`` against the goldens and the CPU oracle,
behaviour (batch independence, determinism, no side effects, stale weights, workspace) and the callers.

Tolerances are those of the tests of the eval path being shadowed (tests/test_models_gpu.py, tests/test_ops_gpu.py,
tests/f64check.py); the new constants FOLD_F32_REL / FOLD_F32_BIAS_REL are calibrated below by the rule of tests/f64check.py.

Not here but in tests/test_infer_chain_gpu.py: ecgmm_relu_maxpool and ecgmm_gate_res_relu element by element, every op of
both plans against float64 at ragged shapes (odd extents, 999-sample records, N = 3, the smallest input), and the plans'
features bit for bit against the same network built from the per-op entry points (tests/infer_chain.py).  Cases of that
kind belong there."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ecgmm.config import Config
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.image_encoder import ResNet18
from ecgmm.inference import Predictor
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel, ResNet1D_SE
from ecgmm.optim import FusedAdam
from oracle import fill, ref_models as O

from . import f64check as F64
from .infer_ref import check_relu_bf16, fold_ref64
from .test_conv_layers_f64_gpu import Geo, _gen, _nchw, _nhwc
from .util import DEV, TDT, dev, from_nhwc, rel_err, to_nhwc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# fp32 fold against the float64 formula: the kernel differs by the fp32 rounding of (rv + eps), one sqrt, one divide and one
# multiply (w'), one subtract and one multiply-add (b').  Measured on the MI355X over the cases below (the test prints them):
# worst |w' - ref| / |ref| = 1.59e-7 (3x3), worst |b' - ref| / (|beta| + |conv_bias - rm| |scale|) = 1.33e-7 (conv1d_bias),
# worst scale error 1.03e-7.  Each constant is at most 4x the measured value (the calibration rule of tests/f64check.py).
FOLD_F32_REL = 6.0e-7
FOLD_F32_BIAS_REL = 5.0e-7


# ------------------------------------------------------------------------------------------------ fold kernel
def _bn_case(cout, seed, with_bias):
    g = torch.Generator().manual_seed(seed)
    gamma = 1.0 + 0.3 * torch.randn(cout, generator=g)
    gamma[::3] = -gamma[::3]                    # negative
    gamma[1], gamma[4], gamma[7] = 0.0, 1e-6, -3e-7   # zero and tiny
    beta = 0.2 * torch.randn(cout, generator=g)
    rm = 0.5 * torch.randn(cout, generator=g)
    rv = torch.rand(cout, generator=g) * 2 + 0.05
    rv[2], rv[5] = 3.0e4, 1e-7                  # large; far below eps
    cb = 0.1 * torch.randn(cout, generator=g) if with_bias else None
    return gamma, beta, rm, rv, cb


def _fold_gpu(dt, layout, w, cb, gamma, beta, rm, rv, eps):
    cout, cin = w.shape[0], w.shape[1]
    if layout == 1:
        R = w.shape[2]
        n_out = L.lib().ecgmm_stem_packed_elems(cin, R)
        rs = R
    else:
        n_out, rs = w.numel(), int(np.prod(w.shape[2:]))
    wout = torch.full((n_out,), float("nan"), device=DEV, dtype=TDT[dt])
    bout = torch.full((cout,), float("nan"), device=DEV)
    sout = torch.full((cout,), float("nan"), device=DEV)
    # (device copies held in names: a temporary freed before the launch would hand its block to the next copy)
    dw, dcb, dg, db, dm, dv = (None if t is None else dev(t) for t in (w, cb, gamma, beta, rm, rv))
    L.check(L.lib().ecgmm_fold_conv_bn(dt, layout, ptr(dw), ptr(dcb), ptr(dg), ptr(db), ptr(dm), ptr(dv), eps, ptr(wout),
                                       ptr(bout), ptr(sout), cout, cin, rs, stream()), "fold")
    torch.cuda.synchronize()
    wout = wout.cpu()
    if layout == 1:   # [64][KP], k = (c * R + r) * 8 + s
        ng = cin * rs
        full = wout.view(64, -1, 8)
        assert (full[:, ng:, :].float() == 0).all() and (full[:, :, 7].float() == 0).all(), "stem pack padding not zero"
        unpacked = full[:, :ng, :7].reshape(64, cin, rs, 7)
    else:             # [Cout][RS][Cin]
        unpacked = wout.view(cout, rs, cin).permute(0, 2, 1).reshape(w.shape)
    return unpacked, bout.cpu(), sout.cpu()


FOLD_CASES = {"3x3": ((128, 64, 3, 3), 0, False), "1x1": ((128, 64, 1, 1), 0, False), "stem7x7": ((64, 3, 7, 7), 1, False),
              "conv1d_bias": ((128, 64, 1, 3), 0, True), "stem1d_bias": ((64, 12, 1, 7), 1, True),
              "odd_tiles": ((72, 40, 1, 3), 0, True)}


@pytest.mark.parametrize("case", sorted(FOLD_CASES))
@pytest.mark.parametrize("dt", [L.F32, L.BF16])
def test_fold_kernel_against_float64(case, dt):
    shape, layout, with_bias = FOLD_CASES[case]
    w = fill.hash_tensor(shape, 31 + len(case), 0.2)
    gamma, beta, rm, rv, cb = _bn_case(shape[0], 7, with_bias)
    eps = float(np.float32(1e-5))          # the ABI takes a float: this IS the eps the kernel sees
    got_w, got_b, got_s = _fold_gpu(dt, layout, w, cb, gamma, beta, rm, rv, eps)
    ref_w, ref_b, ref_s = fold_ref64(w, cb, gamma, beta, rm, rv, eps)
    assert torch.isfinite(got_w.float()).all() and torch.isfinite(got_b).all()
    # the bias is fp32 in both dtypes; relative to the magnitudes that enter it (the subtraction may cancel)
    cbv = torch.zeros_like(beta) if cb is None else cb
    mag = beta.double().abs() + (cbv.double() - rm.double()).abs() * ref_s.abs()
    berr = float(((got_b.double() - ref_b).abs() / mag.clamp_min(1e-300)).max())
    serr = float(((got_s.double() - ref_s).abs() / ref_s.abs().clamp_min(1e-300))[ref_s != 0].max())
    print(f"fold {case} dtype {dt}: bias rel err {berr:.3g}, scale rel err {serr:.3g}")
    assert berr <= FOLD_F32_BIAS_REL
    assert (got_s[gamma == 0] == 0).all() and (got_w.float()[gamma == 0] == 0).all(), "zero gamma must fold to exact zeros"
    if dt == L.F32:
        nz = ref_w != 0
        werr = float(((got_w.double() - ref_w).abs()[nz] / ref_w.abs()[nz]).max())
        print(f"fold {case} fp32: weight rel err {werr:.3g}")
        assert werr <= FOLD_F32_REL
    else:
        # exactly bf16_round of the fp32 product the kernel forms (its own scale, returned through scale_out); one bf16
        # ulp is allowed only where that fp32 product sits on a rounding tie
        prod = w.float() * got_s.view(-1, *([1] * (w.dim() - 1)))
        want = prod.to(BF)
        bits = prod.view(torch.int32) & 0xFFFF
        tie = bits == 0x8000
        diff = (got_w.view(torch.int16).int() - want.view(torch.int16).int()).abs()
        print(f"fold {case} bf16: {int((diff != 0).sum())} of {diff.numel()} differ, {int(tie.sum())} ties")
        assert (diff[~tie] == 0).all(), "bf16 folded weight is not the rounded fp32 product"
        assert (diff[tie] <= 1).all()
        assert serr <= FOLD_F32_REL


# ------------------------------------------------------------------------------------------------ fused forward conv
def _fused(dt, g, x, wf, bias, addend, act):
    y = torch.full((g.M * g.Cout,), float("nan"), device=DEV, dtype=TDT[dt])
    L.check(L.lib().ecgmm_conv_fwd_fused(dt, C.byref(g.d), ptr(x), ptr(wf), ptr(bias), ptr(addend), ptr(y), act, stream()),
            "conv_fwd_fused")
    torch.cuda.synchronize()
    return y


def _pack_fwd(dt, w):
    f = torch.empty(w.numel(), device=DEV, dtype=TDT[dt])
    L.check(L.lib().ecgmm_pack_conv_weight(dt, ptr(w.contiguous()), ptr(f), None, w.shape[0], w.shape[1],
                                           w.shape[2] * w.shape[3], stream()))
    return f


# the step's layer shapes (batch 256, 224 x 224 / L = 5000) that reach each instantiation the inference plans use
FUSED_SHAPES = {
    "l1_64_56_halo_tile": Geo(256, 56, 56, 64, 64, 3, 3, 1, 1, 1),        # bias / act keep it off the stream form
    "l2_128_28_pingpong": Geo(256, 28, 28, 128, 128, 3, 3, 1, 1, 1),
    "l3_256_14_pingpong": Geo(256, 14, 14, 256, 256, 3, 3, 1, 1, 1),
    "l4_512_7_pingpong": Geo(256, 7, 7, 512, 512, 3, 3, 1, 1, 1),
    "l2_entry_3x3s2_igemm": Geo(256, 56, 56, 64, 128, 3, 3, 2, 1, 1),
    "l3_entry_3x3s2_igemm": Geo(256, 28, 28, 128, 256, 3, 3, 2, 1, 1),
    "l4_entry_3x3s2_igemm": Geo(256, 14, 14, 256, 512, 3, 3, 2, 1, 1),
    "l2_down_1x1s2_igemm": Geo(256, 56, 56, 64, 128, 1, 1, 2, 0, 0),
    "sig_b1_1x3_128": Geo(256, 1, 625, 128, 128, 1, 3, 1, 0, 1),
    "sig_b0_1x3_64": Geo(256, 1, 1250, 64, 64, 1, 3, 1, 0, 1),
}


@pytest.mark.parametrize("name", sorted(FUSED_SHAPES))
@pytest.mark.parametrize("form", ["bias_addend_relu", "bias_relu", "bias_only"])
def test_fused_forward_conv_bf16_against_float64(name, form):
    g = FUSED_SHAPES[name]
    x = _gen((g.N, g.Cin, g.H, g.W), 11, "act")
    w = _gen((g.Cout, g.Cin, g.R, g.S), 12, "w", fan_in=g.Cin * g.R * g.S)
    bias = _gen((1, g.Cout), 13, "grad").view(-1).contiguous()        # fp32 operand, signed
    addend = _gen((g.N, g.Cout, g.OH, g.OW), 14, "grad") if form == "bias_addend_relu" else None
    act = 0 if form == "bias_only" else 1
    y = _fused(L.BF16, g, _nhwc(x), _pack_fwd(L.BF16, w), bias, None if addend is None else _nhwc(addend), act)
    ref = F64.conv_ref64(x, w, None, stride=g.stride, padding=(g.ph, g.pw), bias=bias)
    ry, ay = ref.y, ref.ay
    if addend is not None:
        ry, ay = ry + addend.double(), ay + addend.double().abs()
    out = _nchw(y, g.N, g.OH, g.OW, g.Cout)
    if act:
        check_relu_bf16(out, ry, ay, name=f"{name} {form}")
    else:
        F64.check_bf16(out, ry, ay, name=f"{name} {form}")


@pytest.mark.parametrize("geo", [(8, 56, 56, 64, 64, 3, 3, 1, 1, 1), (8, 28, 28, 128, 128, 3, 3, 1, 1, 1),
                                 (8, 56, 56, 64, 128, 3, 3, 2, 1, 1), (8, 56, 56, 64, 128, 1, 1, 2, 0, 0),
                                 (8, 1, 625, 128, 128, 1, 3, 1, 0, 1)])
def test_fused_forward_conv_fp32_against_torch(geo):
    """fp32 compute dtype against F.conv2d (+ bias + addend, ReLU) on the CPU: the bar tests/test_ops_gpu.py holds
    ecgmm_conv_fwd to"""
    N, H, W, Cin, Cout, R, S, st, ph, pw = geo
    g = Geo(*geo)
    x = fill.hash_tensor((N, Cin, H, W), 41, 1.0)
    w = fill.hash_tensor((Cout, Cin, R, S), 42, (2.0 / (Cin * R * S)) ** 0.5)
    bias = fill.hash_tensor((Cout,), 43, 0.5)
    addend = fill.hash_tensor((N, Cout, g.OH, g.OW), 44, 1.0)
    want = torch.relu(F.conv2d(x, w, bias, stride=st, padding=(ph, pw)) + addend)
    y = _fused(L.F32, g, to_nhwc(x, L.F32), _pack_fwd(L.F32, dev(w)), dev(bias), to_nhwc(addend, L.F32), 1)
    got = from_nhwc(y, L.F32, tuple(want.shape))
    e = rel_err(got, want)
    print(f"fused fp32 {geo}: rel err {e:.3g}")
    assert e < 2e-5


# ------------------------------------------------------------------------------------------------ encoders vs goldens
def test_predictor_resnet18_golden_g6(golden_dir):
    g6 = np.load(f"{golden_dir}/g6_resnet18.npz")
    ref = fill.hash_fill_module(O.ResNet18(num_classes=256), "r18.")
    net = ResNet18(num_classes=256, compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    predict = Predictor(net.to(DEV).eval())
    f = predict(dev(fill.hash_tensor((2, 3, 224, 224), 606)))
    f2 = predict(dev(fill.hash_tensor((1, 3, 250, 2500), 606)))      # one blob, two image sizes
    assert (f.cpu() - torch.from_numpy(g6["feat_224"])).abs().max() < 1e-3
    assert (f2.cpu() - torch.from_numpy(g6["feat_250x2500"])).abs().max() < 1e-3


def test_predictor_resnet1d_golden_g1(golden_dir):
    g1 = np.load(f"{golden_dir}/g1_ptbxl_eval.npz")
    sd = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/best_ptbxl_tensors.npz").items()}
    net = ResNet1D_SE(1, 2, compute_dtype="fp32")
    net.load_state_dict(sd, strict=True)
    predict = Predictor(net.to(DEV).eval())
    for Ln in (2476, 5000):
        out = predict(dev(fill.hash_tensor((4, 1, Ln), 77 + Ln, 1.5)))
        assert (out.cpu() - torch.from_numpy(g1[f"logits_{Ln}"])).abs().max() < 1e-3


def _disable_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _build_pair(cd):
    cfg = type("Cfg", (Config,), {})
    cfg.compute_dtype, cfg.clinical_input_dim = cd, 16
    ref = O.disable_dropout(fill.hash_fill_module(O.ECGMultimodalModel(2, 16), "mm."))
    net = ECGMultimodalModel(cfg)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, _disable_dropout(net).to(DEV)


NAMES = ("img_logits", "sig_logits", "clin_logits", "fusion_logits", "var_loss", "soft_w")


@pytest.mark.parametrize("cd,tol", [("fp32", 1e-3), ("bf16", 0.06)])
def test_predictor_multimodal_golden_g5(golden_dir, cd, tol):
    g5 = np.load(f"{golden_dir}/g5_multimodal.npz")
    _, net = _build_pair(cd)
    net.eval()
    img, sig, clin, _ = fill.synthetic_batch(8, salt=5)
    out = Predictor(net)(dev(img), dev(sig), dev(clin))
    assert len(out) == 6
    for n, o in zip(NAMES, out):
        e = float((o.cpu() - torch.from_numpy(g5["eval." + n])).abs().max())
        print(f"g5 {cd} {n}: {e:.3g}")
        assert e < tol, n


@pytest.mark.parametrize("tag", ["pmb", "tab"])
def test_predictor_multimodal_reference_golden_g9(golden_dir, tag):
    from ecgmm.multimodal import ECGMultimodalModel as TabVariant
    from oracle import tabnet_ref as T
    g9 = np.load(f"{golden_dir}/g9_reference_composition.npz")
    cfg = type("Cfg", (Config,), {"compute_dtype": "fp32"})
    if tag == "pmb":
        ref, net, clin_in = O.ECGMultimodalModel(2, 24), ECGMultimodalModel(cfg), 24
    else:
        ref, net, clin_in = T.multimodal_tabnet_model(2), TabVariant(cfg), 2
    net.load_state_dict(fill.hash_fill_module(ref, "mm.").state_dict(), strict=True)
    net = _disable_dropout(net).to(DEV).eval()
    img, sig, clin, _ = fill.synthetic_batch(8, clin_dim=clin_in, salt=9)
    out = Predictor(net)(dev(img), dev(sig), dev(clin))
    for n, o in zip(NAMES, out):
        assert (o.cpu() - torch.from_numpy(g9[f"{tag}.eval.{n}"])).abs().max() < 1e-3, n


def _perturb_bn(ref):
    """a third of the BatchNorm gammas negated, running statistics moved (oracle/fill.py only makes gamma ~ 1 +- 0.1)"""
    k = 0
    for m in ref.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.weight[k % 3::3] *= -1.0
                m.weight[(k + 1) % 5] = 0.0
                m.running_mean.add_(0.05 * fill.hash_tensor(tuple(m.running_mean.shape), 900 + k))
                m.running_var.mul_(1.0 + 0.5 * fill.hash_tensor(tuple(m.running_var.shape), 950 + k).abs())
            k += 1
    return ref


@pytest.mark.parametrize("which", ["resnet18", "resnet1d"])
def test_predictor_negative_gamma_against_cpu_oracle(which):
    if which == "resnet18":
        ref = _perturb_bn(fill.hash_fill_module(O.ResNet18(num_classes=64), "r18.")).eval()
        net, x = ResNet18(num_classes=64, compute_dtype="fp32"), fill.hash_tensor((3, 3, 96, 160), 611)
    else:
        ref = _perturb_bn(fill.hash_fill_module(O.ResNet1D_SE(1, 32), "r1d.")).eval()
        net, x = ResNet1D_SE(1, 32, compute_dtype="fp32"), fill.hash_tensor((3, 1, 2476), 612, 1.5)
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV).eval()
    with torch.no_grad():
        want = ref(x)
        own = net(dev(x))
    got = Predictor(net)(dev(x))
    scale = max(1.0, float(want.abs().max()))
    e, e_own = float((got.cpu() - want).abs().max()), float((own.cpu() - want).abs().max())
    print(f"negated gamma {which}: predictor {e:.3g}, eval path {e_own:.3g}, |ref| max {scale:.3g}")
    assert e < 1e-3 * scale


# ------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("which", ["resnet18", "resnet1d"])
def test_predictor_bf16_no_worse_than_the_eval_path(which):
    """feature error against the fp32 CPU oracle: err_infer < 1.3 * err_eval + 0.02 (the form and constants
    tests/test_models_gpu.py uses against torch autocast)"""
    if which == "resnet18":
        ref = fill.hash_fill_module(O.ResNet18(num_classes=256), "r18.").eval()
        net, x = ResNet18(num_classes=256, compute_dtype="bf16"), fill.hash_tensor((8, 3, 128, 96), 607)
    else:
        ref = fill.hash_fill_module(O.ResNet1D_SE(1, 256), "r1d.").eval()
        net, x = ResNet1D_SE(1, 256, compute_dtype="bf16"), fill.hash_tensor((8, 1, 5000), 608, 1.5)
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV).eval()
    with torch.no_grad():
        want = ref(x)
        own = net(dev(x))
    got = Predictor(net)(dev(x))
    err_infer, err_eval = rel_err(got.cpu(), want), rel_err(own.cpu(), want)
    print(f"bf16 {which}: err_infer {err_infer:.4g}, err_eval {err_eval:.4g}")
    assert err_infer < 1.3 * err_eval + 0.02


# ------------------------------------------------------------------------------------------------ behaviour
def _r18(cd="fp32", nc=32):
    ref = fill.hash_fill_module(O.ResNet18(num_classes=nc), "r18.")
    net = ResNet18(num_classes=nc, compute_dtype=cd)
    net.load_state_dict(ref.state_dict(), strict=True)
    return net.to(DEV)


def test_batch_independence_determinism_and_no_side_effects():
    net = _r18().train()                       # even in training mode: the plan reads no mode flag
    for p in net.parameters():
        p.grad = torch.full_like(p, 0.25)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    grads = [p.grad.clone() for p in net.parameters()]
    predict = Predictor(net)
    x = dev(fill.hash_tensor((8, 3, 64, 96), 21))
    f8, f8b, f1 = predict(x), predict(x), predict(x[:1])
    torch.cuda.synchronize()
    assert torch.equal(f8, f8b), "two calls differ"
    assert (f1[0] - f8[0]).abs().max() < 1e-3                      # nothing batch-dependent in an eval plan
    assert net.training is True and not f8.requires_grad
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    for p, g in zip(net.parameters(), grads):
        assert torch.equal(p.grad, g)
    # the signal encoder likewise
    ref = fill.hash_fill_module(O.ResNet1D_SE(1, 16), "r1d.")
    s = ResNet1D_SE(1, 16, compute_dtype="fp32")
    s.load_state_dict(ref.state_dict(), strict=True)
    s = s.to(DEV).train()
    before = {k: v.clone() for k, v in s.state_dict().items()}
    ps = Predictor(s)
    xs = dev(fill.hash_tensor((8, 1, 1000), 22, 1.5))
    a, b, c = ps(xs), ps(xs), ps(xs[:1])
    assert torch.equal(a, b) and (c[0] - a[0]).abs().max() < 1e-3 and s.training is True
    with torch.no_grad():
        assert (a - s.eval()(xs)).abs().max() < 1e-3               # no dropout, running statistics
    for k, v in s.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_stale_until_refresh_and_one_blob_for_all_shapes():
    net = _r18().train()
    predict = Predictor(net)
    x = dev(fill.hash_tensor((4, 3, 64, 64), 23))
    x2 = dev(fill.hash_tensor((2, 3, 96, 160), 24))
    old, old2 = predict(x).clone(), predict(x2).clone()            # two batch sizes, two image sizes, one blob
    with torch.no_grad():
        assert (old - net.eval()(x)).abs().max() < 1e-3 and (old2 - net(x2)).abs().max() < 1e-3
    net.train()
    opt = FusedAdam(net.parameters(), lr=1e-3)
    net(x).square().mean().backward()
    opt.step()                                                       # weights AND running statistics moved
    torch.cuda.synchronize()
    assert torch.equal(predict(x), old), "a prepared predictor must keep answering from its snapshot"
    new = predict.refresh()(x)
    with torch.no_grad():
        want = net.eval()(x)
    assert (new - want).abs().max() < 1e-3 * max(1.0, float(want.abs().max()))
    assert (new - old).abs().max() > 1e-3


def test_refusals():
    net = _r18().eval()
    predict = Predictor(net)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        predict(torch.zeros(1, 1, 64, 64, device=DEV))
    net.compute_dtype = "bf16"
    with pytest.raises(RuntimeError, match="compute dtype"):
        predict(torch.zeros(1, 3, 64, 64, device=DEV))
    predict.refresh()(torch.zeros(1, 3, 64, 64, device=DEV))
    _, mm = _build_pair("fp32")
    pm = Predictor(mm.train())
    img, sig, clin, _ = fill.synthetic_batch(2, img_hw=(64, 64), sig_len=1000, salt=3)
    with pytest.raises(RuntimeError, match="model.eval"):
        pm(dev(img), dev(sig), dev(clin))
    assert mm.training is True


def test_workspace_ratio_at_batch_256():
    """Count the buffers, in units of U = one [256, 56, 56, 64] bf16 tensor (102.8 MB).
    Training layout (csrc/plan_resnet18.hip layout_fwd), activations alone: stem output 4 U, pooled 1 U, pool indices 0.5 U;
    layer 1: 2 blocks x (y1, a1, y2, out) = 8 U; layer 2 (U / 2 each): 5 + 4 tensors = 4.5 U; layer 3: 2.25 U; layer 4:
    1.125 U  ->  at least 21.375 U (ReLU bits, weights packs, coefficient and statistics rows come on top).
    Inference layout (csrc/plan_infer.hip layout_ws18): the stem output (4 U; three rotating block buffers alias it once
    the max-pool has read it) + the fourth rotating buffer (1 U) + the pooled features [256, 512] fp32 and alignment
    (< 0.01 U)  ->  at most 5.01 U.  Ratio < 5.01 / 21.375 = 0.2344."""
    lib = L.lib()
    d = L.ResNet18Desc(256, 224, 224, 256, L.BF16, 0, 0.1, 1e-5)
    U = 256 * 56 * 56 * 64 * 2
    train_ws, infer_ws = lib.ecgmm_resnet18_fwd_workspace(C.byref(d)), lib.ecgmm_resnet18_infer_workspace(C.byref(d))
    print(f"workspace at batch 256: training plan {train_ws / 1e9:.3f} GB, inference plan {infer_ws / 1e9:.3f} GB")
    assert train_ws >= 21.375 * U
    assert 5.0 * U <= infer_ws <= 5.01 * U
    assert infer_ws / train_ws < 5.01 / 21.375
    # the same count for the signal encoder, V = one [256, 1250, 64] bf16 tensor: training >= stem 2 V + pooled 1 V +
    # indices 0.5 V + 4 V + 2.5 V + 1.25 V = 11.25 V; inference = 3 V aliasing the stem output + 1 V
    s = L.ResNet1DDesc(256, 1, 5000, 256, L.BF16, 0, 0.1, 1e-5, 0.0, 0, 0)
    V = 256 * 1250 * 64 * 2
    t1, i1 = lib.ecgmm_resnet1d_fwd_workspace(C.byref(s)), lib.ecgmm_resnet1d_infer_workspace(C.byref(s))
    assert t1 >= 11.25 * V and 4.0 * V <= i1 <= 4.05 * V


def test_large_batch_runs_in_a_quarter_of_the_training_workspace():
    """batch 512 at 224 x 224 (fp32: training-plan workspace 9.3 GB) runs through the inference plan in a workspace under a
    quarter of that; its rows equal a small batch of the same images at the fp32 goldens' tolerance"""
    net = _r18("fp32", 16).eval()
    predict = Predictor(net)
    N = 512
    d = L.ResNet18Desc(N, 224, 224, 16, L.F32, 0, 0.1, 1e-5)
    lib = L.lib()
    assert lib.ecgmm_resnet18_infer_workspace(C.byref(d)) * 4 < lib.ecgmm_resnet18_fwd_workspace(C.byref(d))
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(N, 3, 224, 224, device=DEV, generator=g) * 2 - 1
    f = predict(x)
    f_head = predict(x[:4].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(f).all()
    assert (f[:4] - f_head).abs().max() < 1e-3 * max(1.0, float(f_head.abs().max()))


# ------------------------------------------------------------------------------------------------ callers
def _cfg(**kw):
    base = {"device": DEV, "compute_dtype": "fp32", "clinical_input_dim": 16, "batch_size": 8,
            "synthetic_train_size": 16, "synthetic_val_size": 8, "synthetic_test_size": 24, "img_height": 64,
            "img_width": 64, "signal_length": 1000}
    base.update(kw)
    return type("C", (Config,), base)


def test_train_evaluate_with_and_without_a_predictor():
    from ecgmm import train
    from ecgmm.dataset import get_dataloaders
    cfg = _cfg()
    _, net = _build_pair("fp32")
    net.eval()
    _, val_loader, test_loader = get_dataloaders(cfg)
    predict = Predictor(net)
    own = train.evaluate(net, test_loader, DEV)
    via = train.evaluate(net, test_loader, DEV, predictor=predict)
    print("evaluate:", own, via)
    for k in own:
        assert (np.isnan(own[k]) and np.isnan(via[k])) or abs(own[k] - via[k]) < 1e-3, k
    # the same predictions, batch by batch, and the same validation epoch
    with torch.no_grad():
        for *batch, _idx in test_loader:
            img, ecg, clin, _lab = (t.to(DEV) for t in batch)
            a, b = net(img, ecg, clin)[3], predict(img, ecg, clin)[3]
            assert (a - b).abs().max() < 1e-3 and torch.equal(a.argmax(1), b.argmax(1))
    e_own, e_via = train.run_epoch(net, val_loader, DEV), train.run_epoch(net, val_loader, DEV, predictor=predict)
    assert all(abs(x - y) < 1e-3 for x, y in zip(e_own, e_via)), (e_own, e_via)
    with pytest.raises(ValueError, match="no backward"):
        train.run_epoch(net, val_loader, DEV, optimizer=object(), predictor=predict)
    # predict_proba: rows sum to one, loader order
    prob, labels, index = predict.predict_proba(test_loader)
    assert prob.shape == (24, 2) and torch.allclose(prob.sum(1), torch.ones(24), atol=1e-6)
    want_lab = torch.cat([b[3].cpu() for b in test_loader])
    want_idx = torch.cat([torch.as_tensor(b[4]).cpu() for b in test_loader])
    assert torch.equal(labels, want_lab) and torch.equal(index, want_idx)
    with torch.no_grad():
        first = next(iter(test_loader))
        lg = net(*(t.to(DEV) for t in first[:3]))[3]
    assert torch.allclose(prob[:8], torch.softmax(lg.float().cpu(), 1), atol=1e-4)


def test_train_main_with_predictor(tmp_path):
    from ecgmm import train
    cfg = _cfg(compute_dtype="bf16", checkpoint_dir=str(tmp_path / "ck"), num_epochs=1, synthetic_test_size=8)
    hist, results, _ = train.main(cfg, num_epochs=1, quiet=True, use_predictor=True)
    assert len(hist) == 1 and np.isfinite(hist[0]["val_loss"]) and set(results) == {"best", "last"}
