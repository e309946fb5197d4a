"""Input gradients and eval-mode backward of both encoder plans (csrc/plan_resnet18.hip, plan_resnet1d.hip), and the stem
input-gradient kernel (csrc/conv_stem_dgrad.hip) at op level.  Every comparison is against the CPU oracle
(oracle/ref_models.py, plain torch autograd) or float64 torch on the CPU."""
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.image_encoder import ResNet18
from ecgmm.multimodal_paper_modal_balance import ResNet1D_SE
from oracle import fill, ref_models as O

from .f64check import KAPPA, conv_ref64
from .util import DEV, bf16_round, dev, rel_err, switches, to_nhwc

pytestmark = pytest.mark.gpu

# Conv1d biases in front of a BatchNorm (tests/test_models_gpu.py excludes them from its training-mode comparisons)
SIG_BIAS_SKIP = ("initial.0.bias", "conv1.bias", "conv2.bias", "downsample.0.bias")
R18_SHAPES = [(4, 3, 64, 64), (2, 3, 96, 160)]
R1D_SHAPES = [(4, 1, 1000), (2, 12, 1000)]


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _pair(kind, shape, cd):
    """(oracle, HIP module) with the same hash-filled state; dropout disabled"""
    if kind == "r18":
        ref = fill.hash_fill_module(O.ResNet18(num_classes=256), "r18.")
        net = ResNet18(num_classes=256, compute_dtype=cd)
    else:
        ref = O.disable_dropout(fill.hash_fill_module(O.ResNet1D_SE(shape[1], 2), "sig."))
        net = ResNet1D_SE(shape[1], 2, compute_dtype=cd)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, _no_dropout(net).to(DEV)


def _input(kind, shape):
    return fill.hash_tensor(shape, 607) if kind == "r18" else fill.hash_tensor(shape, 91, 1.5)


def _oracle_dx(ref, x, train, autocast=False):
    ref.train(train)
    ref.zero_grad()
    x = x.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        f = ref(x)
    f.float().square().mean().backward()
    return x.grad.detach()


def _hip_dx(net, x, train):
    net.train(train)
    xd = dev(x).requires_grad_(True)
    f = net(xd)
    f.square().mean().backward()   # (torch elementwise on the features: host-side test glue)
    torch.cuda.synchronize()
    return xd.grad


CASES = [("r18", s) for s in R18_SHAPES] + [("r1d", s) for s in R1D_SHAPES]
TOL = {"r18": 5e-3, "r1d": 2e-3}   # what tests/test_models_gpu.py applies to the same encoder's parameter gradients


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_input_gradient_exists_in_both_modes(train):
    """before this feature: image.grad stayed None in training mode, and the eval-mode backward raised"""
    for kind, shape in (("r18", R18_SHAPES[0]), ("r1d", R1D_SHAPES[0])):
        _ref, net = _pair(kind, shape, "fp32")
        dx = _hip_dx(net, _input(kind, shape), train)
        assert dx is not None and tuple(dx.shape) == shape and dx.dtype == torch.float32
        assert torch.isfinite(dx).all() and dx.abs().max().item() > 0


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind,shape", CASES)
def test_encoder_input_gradient_fp32_vs_oracle(kind, shape, train):
    ref, net = _pair(kind, shape, "fp32")
    x = _input(kind, shape)
    want = _oracle_dx(ref, x, train)
    got = _hip_dx(net, x, train).cpu()
    e = rel_err(got, want)
    print(f"{kind} {shape} train={train}: rel_err(dx) = {e:.3e}")
    assert e < TOL[kind]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind,shape", CASES)
def test_encoder_input_gradient_bf16_no_worse_than_torch_autocast(kind, shape, train):
    """the project's autocast-relative bar (test_models_gpu._dev_vs_autocast), on the input gradient"""
    ref, net = _pair(kind, shape, "bf16")
    x = _input(kind, shape)
    d32 = _oracle_dx(ref, x, train)
    d16 = _oracle_dx(ref, x, train, autocast=True)
    got = _hip_dx(net, x, train).cpu()
    mine, theirs = rel_err(got, d32), rel_err(d16, d32)
    print(f"{kind} {shape} train={train}: rel_err(dx) = {mine:.4f}, CPU autocast {theirs:.4f}")
    assert mine < 1.3 * theirs + 0.02


@pytest.mark.parametrize("kind,shape", CASES)
def test_eval_backward_parameter_gradients_and_untouched_statistics(kind, shape):
    ref, net = _pair(kind, shape, "fp32")
    x = _input(kind, shape)
    _oracle_dx(ref, x, train=False)
    net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    _hip_dx(net, x, train=False)
    bad = []
    for k, p in ref.named_parameters():
        g = dict(net.named_parameters())[k].grad
        assert g is not None, k
        e = rel_err(g.cpu(), p.grad)
        # (the training-mode tests skip SIG_BIAS_SKIP: there BatchNorm cancels a Conv1d bias and its true gradient is 0.  In
        #  eval mode it does not -- the gradient is a real number and held to the same bar as every other parameter)
        if kind == "r1d" and any(s in k for s in SIG_BIAS_SKIP):
            print(f"{k}: rel_err = {e:.3e}")
        if not e < TOL[kind]:
            bad.append((k, e))
    assert not bad, bad
    after = net.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,shape", [CASES[0], CASES[2]])
def test_eval_retain_graph_two_backwards_equal_separate_runs(kind, shape, cd):
    _ref, net = _pair(kind, shape, cd)
    net.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    x = dev(_input(kind, shape))

    def separate(c):
        xd = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(net(xd)[:, c].sum(), xd)
        return g

    want = [separate(0), separate(1)]
    xd = x.clone().requires_grad_(True)
    f = net(xd)
    g0, = torch.autograd.grad(f[:, 0].sum(), xd, retain_graph=True)
    g1, = torch.autograd.grad(f[:, 1].sum(), xd)
    torch.cuda.synchronize()
    assert torch.equal(g0, want[0]) and torch.equal(g1, want[1])
    assert not torch.equal(g0, g1)


def test_second_backward_through_training_forward_fails_clearly():
    _ref, net = _pair("r18", R18_SHAPES[0], "fp32")
    net.train()
    f = net(dev(_input("r18", R18_SHAPES[0])))
    f.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="workspace was released"):
        f.sum().backward()


def test_stem_recompute_refuses_input_gradient():
    lib = L.lib()
    _ref, net = _pair("r18", R18_SHAPES[0], "bf16")   # (the recomputing stem exists for bf16 only)
    with switches(lib, ECGMM_STEM_RECOMPUTE=1):
        xd = dev(_input("r18", R18_SHAPES[0])).requires_grad_(True)
        f = net.train()(xd)
        with pytest.raises(RuntimeError, match="ecgmm_stem_recompute"):
            f.sum().backward()


# ---------------------------------------------------------------------------------------------------------------------
# op level: ecgmm_stem_bwd_data against float64 autograd of F.conv2d
# ---------------------------------------------------------------------------------------------------------------------
def _half_ulp_f32(v):
    """half a unit in the last place of the fp32 binade of |v| (0 for 0)"""
    _m, e = torch.frexp(v.double().abs())
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 25))


STEM_2D = [(2, 3, 224, 224), (1, 3, 250, 2500), (3, 3, 65, 97)]
STEM_1D = [(4, 1, 1, 5000), (2, 12, 1, 1000), (3, 1, 1, 999)]


@pytest.mark.parametrize("dt", [L.F32, L.BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", STEM_2D + STEM_1D)
def test_stem_bwd_data_vs_float64(shape, dt):
    N, cin, H, W = shape
    R = 7 if H > 1 else 1
    pad = (3, 3) if R == 7 else (0, 3)
    OH, OW = (H + 2 * pad[0] - R) // 2 + 1, (W + 6 - 7) // 2 + 1
    w = fill.hash_tensor((64, cin, R, 7), 31, (6.0 / (cin * R * 7)) ** 0.5)
    dy = fill.hash_tensor((N, 64, OH, OW), 32)
    if dt == L.BF16:          # operands rounded first: float64 of them is then the exact answer
        w, dy = bf16_round(w), bf16_round(dy)
    ref = conv_ref64(torch.zeros(N, cin, H, W), w, dy, stride=2, padding=pad)
    dx = torch.full((N, cin, H, W), float("nan"), device=DEV, dtype=torch.float32)   # an unwritten element fails
    dy_dev, w_dev = to_nhwc(dy, dt), dev(w)   # (named: a temporary would be freed, and its memory reused, before the launch)
    L.check(L.lib().ecgmm_stem_bwd_data(dt, ptr(dy_dev), ptr(w_dev), ptr(dx), N, cin, H, W, R, stream()), "stem_bwd_data")
    torch.cuda.synchronize()
    got = dx.cpu().double()
    assert torch.isfinite(got).all()
    if dt == L.F32:
        e = rel_err(got, ref.dx)
        print(f"stem_bwd_data fp32 {shape}: rel_err = {e:.3e}")
        assert e < 2e-5
    else:
        err = (got - ref.dx).abs()
        bound = KAPPA * ref.adx + _half_ulp_f32(ref.dx)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
        print(f"stem_bwd_data bf16 {shape}: worst |err| / bound = {float(ratio.max()):.3f}")
        assert bool((err <= bound).all()), float(ratio.max())
    # an input row / column the stride-2 convolution never reads has gradient exactly 0
    zero = ref.adx == 0
    assert bool((got[zero] == 0).all())
