"""ecgmm/explain.py on the GPU: whole-model input gradients against torch.autograd.grad on the CPU oracle, and Grad-CAM
against the textbook computation on the oracle (hooks on the last stage: gradient of the logit w.r.t. the activation,
spatial mean, weighted sum, ReLU, max-normalise, bilinear upsample with align_corners=False)."""
import pytest
import torch
import torch.nn.functional as F

from ecgmm import explain
from ecgmm.config import Config
from ecgmm.hip import encoders as E
from ecgmm.hip import functional as HF
from ecgmm.image_encoder import ResNet18
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel, ResNet1D_SE
from oracle import fill, ref_models as O

from .util import DEV, dev, rel_err

pytestmark = pytest.mark.gpu


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _model_pair(tag):
    """the two variants test_multimodal_vs_reference_object_golden_g9 builds, fp32 compute"""
    cfg = type("Cfg", (Config,), {"compute_dtype": "fp32"})
    if tag == "pmb":
        ref, net, clin_in = O.ECGMultimodalModel(2, 24), ECGMultimodalModel(cfg), 24
    else:
        from ecgmm.multimodal import ECGMultimodalModel as TabVariant
        from oracle import tabnet_ref as T
        ref, net, clin_in = T.multimodal_tabnet_model(2), TabVariant(cfg), 2
    net.load_state_dict(fill.hash_fill_module(ref, "mm.").state_dict(), strict=True)
    return O.disable_dropout(ref), _no_dropout(net).to(DEV), clin_in


@pytest.mark.parametrize("tag", ["pmb", "tab"])
def test_input_gradients_whole_model_vs_oracle(tag):
    ref, net, clin_in = _model_pair(tag)
    img, sig, clin, _lab = fill.synthetic_batch(4, img_hw=(96, 160), sig_len=1000, clin_dim=clin_in, salt=9)
    ref.eval()
    xs = [t.clone().requires_grad_(True) for t in (img, sig, clin)]
    logits = ref(*xs)[3]
    target = logits.detach().argmax(dim=1)
    want = torch.autograd.grad(logits.gather(1, target[:, None]).sum(), xs)
    net.train()                     # input_gradients evaluates in eval() and puts the mode back
    got = explain.input_gradients(net, dev(img), dev(sig), dev(clin), target=target)
    torch.cuda.synchronize()
    assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())
    for name, g, w, tol in zip(("image", "signal", "clinical"), got, want, (5e-3, 2e-3, 2e-3)):
        assert g.shape == w.shape and w.abs().max() > 0
        e = rel_err(g.cpu(), w)
        print(f"{tag} d_{name}: rel_err = {e:.3e}")
        assert e < tol, name
    # default target = the predicted class; a branch output leaves the other modalities' gradients at zero
    again = explain.input_gradients(net, dev(img), dev(sig), dev(clin))
    pred = net.eval()(dev(img), dev(sig), dev(clin))[3].argmax(dim=1).cpu()
    if torch.equal(pred, target):
        assert all(torch.equal(a, b) for a, b in zip(again, got))
    only_img = explain.input_gradients(net, dev(img), dev(sig), dev(clin), target=1, output="image")
    assert only_img[0].abs().max() > 0 and only_img[1].abs().max() == 0 and only_img[2].abs().max() == 0


def test_training_step_parameter_gradients_unchanged_by_input_gradient():
    """the input gradient is one more output of the same backward, not another path"""
    grads = []
    for want_dx in (False, True):
        _ref, net, clin_in = _model_pair("pmb")
        net.train()
        img, sig, clin, lab = fill.synthetic_batch(4, img_hw=(64, 64), sig_len=1000, clin_dim=clin_in, salt=9)
        image = dev(img).requires_grad_(want_dx)
        out = net(image, dev(sig), dev(clin))
        HF.cross_entropy_plus(out[3], dev(lab), out[4], 0.1).backward()
        torch.cuda.synchronize()
        assert (image.grad is not None) == want_dx
        if want_dx:
            assert image.grad.shape == image.shape and image.grad.abs().max() > 0
        grads.append({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def _cam_of(a, g, size):
    """the textbook map from an activation and the gradient of the logit w.r.t. it (fp32, whatever dtype they come in) ->
    (map at `size`, per-sample maximum of the coarse map before the normalisation)"""
    a, g = a.detach().float(), g.detach().float()
    if a.dim() == 3:                       # [N, C, L'] -> [N, C, 1, L']
        a, g = a[:, :, None, :], g[:, :, None, :]
    alpha = g.mean(dim=(2, 3), keepdim=True)
    cam = F.relu((alpha * a).sum(dim=1)).detach()
    mx = cam.flatten(1).max(dim=1).values[:, None, None]
    cam = torch.where(mx > 0, cam / mx.clamp_min(1e-30), torch.zeros_like(cam))
    up = F.interpolate(cam[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]
    return up, mx.reshape(-1)


def _textbook_cam(ref, layer, x, size, target=None, autocast=False, with_max=False):
    acts = {}
    h = layer.register_forward_hook(lambda _m, _i, o: acts.__setitem__("a", o))
    try:
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            logits = ref.eval()(x)
    finally:
        h.remove()
    a = acts["a"]
    if target is None:
        target = logits.detach().argmax(dim=1)
    g, = torch.autograd.grad(logits.float().gather(1, target[:, None]).sum(), a)
    up, mx = _cam_of(a, g, size)
    return (up, target, mx) if with_max else (up, target)


@pytest.mark.parametrize("shape", [(2, 3, 224, 224), (1, 3, 250, 2500)])
def test_grad_cam_resnet18_vs_textbook(shape):
    ref = fill.hash_fill_module(O.ResNet18(num_classes=2), "r18.")
    net = ResNet18(num_classes=2, compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV)
    x = fill.hash_tensor(shape, 606)
    want, target = _textbook_cam(ref, ref.layer4, x, shape[2:])
    assert want.flatten(1).max(dim=1).values.max() > 0      # not a comparison of zeros with zeros
    cam = explain.encoder_grad_cam(net, dev(x), target=target).cpu()
    assert cam.shape == (shape[0],) + shape[2:] and cam.dtype == torch.float32
    assert cam.min() >= 0 and cam.max() <= 1
    d = (cam - want).abs().max().item()
    print(f"grad-cam resnet18 {shape}: max |diff| = {d:.3e}")
    assert d < 1e-3
    for n in range(shape[0]):
        if want[n].max() == 0:
            assert cam[n].max() == 0


def test_grad_cam_resnet1d_vs_textbook():
    shape = (2, 1, 5000)
    ref = O.disable_dropout(fill.hash_fill_module(O.ResNet1D_SE(1, 2), "sig."))
    net = ResNet1D_SE(1, 2, compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV)
    x = fill.hash_tensor(shape, 91, 1.5)
    want, target = _textbook_cam(ref, ref.layer3, x, (1, shape[2]))
    want = want[:, 0]
    assert want.max(dim=1).values.max() > 0
    cam = explain.encoder_grad_cam(net, dev(x), target=target).cpu()
    assert cam.shape == (2, 5000) and cam.min() >= 0 and cam.max() <= 1
    d = (cam - want).abs().max().item()
    print(f"grad-cam resnet1d {shape}: max |diff| = {d:.3e}")
    assert d < 1e-3
    for n in range(2):
        if want[n].max() == 0:
            assert cam[n].max() == 0


def test_grad_cam_whole_model_and_pictures(tmp_path):
    """the model-level entry: maps of the right shape in [0, 1] for both encoders, equal to the encoder-level route fed with
    the head's gradient; main() writes the PNG pairs"""
    _ref, net, clin_in = _model_pair("pmb")
    img, sig, clin, _lab = fill.synthetic_batch(2, img_hw=(96, 160), sig_len=1000, clin_dim=clin_in, salt=9)
    cam_img, cam_sig = explain.grad_cam(net.train(), dev(img), dev(sig), dev(clin))
    torch.cuda.synchronize()
    assert net.training and cam_img.shape == (2, 96, 160) and cam_sig.shape == (2, 1000)
    for c in (cam_img, cam_sig):
        assert torch.isfinite(c).all() and c.min() >= 0 and c.max() <= 1
    cfg = type("Tiny", (Config,), {"compute_dtype": "fp32", "synthetic": True, "synthetic_train_size": 8,
                                   "synthetic_val_size": 4, "synthetic_test_size": 4, "batch_size": 4, "device": "cuda"})
    files = explain.main(cfg, out_dir=str(tmp_path), samples=2, quiet=True)
    from PIL import Image
    assert [f.rsplit("/", 1)[1] for f in files] == ["gradcam_0.png", "gradcam_0_overlay.png", "gradcam_1.png",
                                                    "gradcam_1_overlay.png"]
    for f in files:
        assert Image.open(f).mode == "RGB" and Image.open(f).size == (224, 224)   # the synthetic dataset's pictures


# ----------------------------------------------------------------------------------------------------------------------
# the product entry point, explain.grad_cam: against the textbook on the CPU oracle, against the encoder-level route it claims
# to equal, in bf16, and what it leaves behind
# ----------------------------------------------------------------------------------------------------------------------
CAM_BATCH = dict(img_hw=(96, 160), sig_len=1000, salt=9)


def _textbook_model_cams(ref, img, sig, clin, output):
    """hooks on the oracle's image_encoder.layer4 and signal_encoder.layer3, the gradient of the chosen output's logit of its
    own predicted class through the head -> (cam_image [N,H,W], cam_signal [N,L], target [N], coarse maxima of the two)"""
    acts = {}
    hooks = [layer.register_forward_hook(lambda _m, _i, o, k=k: acts.__setitem__(k, o))
             for k, layer in (("img", ref.image_encoder.layer4), ("sig", ref.signal_encoder.layer3))]
    try:
        logits = ref.eval()(img, sig, clin)[explain.OUTPUTS[output]]
    finally:
        for h in hooks:
            h.remove()
    target = logits.detach().argmax(dim=1)
    grads = torch.autograd.grad(logits.gather(1, target[:, None]).sum(), [acts["img"], acts["sig"]], allow_unused=True)
    cams = []
    for a, g, size in ((acts["img"], grads[0], img.shape[2:]), (acts["sig"], grads[1], (1, sig.shape[1]))):
        cams.append(_cam_of(a, torch.zeros_like(a) if g is None else g, size))
    return cams[0][0], cams[1][0][:, 0], target, cams[0][1], cams[1][1]


@pytest.mark.parametrize("output", ["fusion", "image", "signal"])
@pytest.mark.parametrize("tag", ["pmb", "tab"])
def test_grad_cam_whole_model_vs_textbook(tag, output):
    """which branch's gradient, which sample's weights, which way round the coarse grid: the map of the product entry point
    against the textbook one, the same class explained on both sides"""
    ref, net, clin_in = _model_pair(tag)
    img, sig, clin, _lab = fill.synthetic_batch(2, clin_dim=clin_in, **CAM_BATCH)
    want_img, want_sig, target, mx_img, mx_sig = _textbook_model_cams(ref, img, sig, clin, output)
    cam_img, cam_sig = explain.grad_cam(net.train(), dev(img), dev(sig), dev(clin), target=target, output=output)
    torch.cuda.synchronize()
    assert net.training and cam_img.shape == want_img.shape and cam_sig.shape == want_sig.shape
    for name, cam, want, mx, used in (("image", cam_img.cpu(), want_img, mx_img, output != "signal"),
                                      ("signal", cam_sig.cpu(), want_sig, mx_sig, output != "image")):
        if not used:                                     # the other branch's logit does not depend on this encoder
            assert float(want.abs().max()) == 0 and float(cam.abs().max()) == 0, name
            continue
        assert float(mx.max()) > 0, name                 # not a comparison of zeros with zeros
        d = (cam - want).abs().max().item()
        print(f"grad_cam {tag} output={output} {name}: max |diff| = {d:.3e}, coarse maxima {mx.tolist()}")
        assert cam.min() >= 0 and cam.max() <= 1 and d < 1e-3, name
        for n in range(cam.shape[0]):
            if mx[n] == 0:
                assert cam[n].max() == 0


@pytest.mark.parametrize("output", ["fusion", "signal"])
def test_grad_cam_is_the_encoder_level_route_fed_with_the_heads_gradient(output):
    """the docstring's claim, bit for bit.  The other route: the encoders' outputs are cut out of the graph and made leaves, so
    no encoder backward node exists; torch.autograd.grad of the logit w.r.t. those leaves is the head's gradient, and
    plan_grad_cam gets it"""
    _ref, net, clin_in = _model_pair("pmb")
    img, sig, clin, _lab = fill.synthetic_batch(2, clin_dim=clin_in, **CAM_BATCH)
    target = torch.tensor([1, 0])
    got = explain.grad_cam(net, dev(img), dev(sig), dev(clin), target=target, output=output)
    encoders = (net.image_encoder, net.signal_encoder)
    leaves = {}

    def cut(k):
        def hook(_m, _i, out):
            leaves[k] = out.detach().requires_grad_(True)
            return leaves[k]
        return hook

    hooks = [e.register_forward_hook(cut(k)) for k, e in enumerate(encoders)]
    try:
        with explain._Frozen(net), explain._recorded(encoders):
            logits = net(dev(img), dev(sig), dev(clin))[explain.OUTPUTS[output]]
            dfeat = torch.autograd.grad(logits.gather(1, target.to(DEV)[:, None]).sum(), [leaves[0], leaves[1]], allow_unused=True)
            want = [E.plan_grad_cam(e._spec, torch.zeros_like(leaves[k]) if dfeat[k] is None else dfeat[k])
                    for k, e in enumerate(encoders)]
    finally:
        for h in hooks:
            h.remove()
    torch.cuda.synchronize()
    # (the fused head hands back zeros, not None, for an encoder its chosen output does not depend on)
    assert (dfeat[0] is None or float(dfeat[0].abs().max()) == 0) == (output == "signal") and float(dfeat[1].abs().max()) > 0
    assert (float(got[0].abs().max()) == 0) == (output == "signal")
    for name, g, w in zip(("image", "signal"), got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), name
    assert float(got[1].max()) > 0


def _bf16_cam_case(kind):
    if kind == "r18":
        ref = fill.hash_fill_module(O.ResNet18(num_classes=2), "r18.")
        return ref, ref.layer4, ResNet18(num_classes=2, compute_dtype="bf16"), fill.hash_tensor((2, 3, 96, 160), 606), (96, 160)
    ref = O.disable_dropout(fill.hash_fill_module(O.ResNet1D_SE(1, 2), "sig."))
    return ref, ref.layer3, ResNet1D_SE(1, 2, compute_dtype="bf16"), fill.hash_tensor((2, 1, 1000), 91, 1.5), (1, 1000)


@pytest.mark.parametrize("kind", ["r18", "r1d"])
def test_encoder_grad_cam_bf16_no_worse_than_torch_autocast(kind):
    """bf16 is the benchmarked compute dtype: the map against the fp32 oracle's, no further from it than the CPU oracle under
    torch.autocast(bfloat16) is (the bar of tests/test_models_gpu.py, _dev_vs_autocast), the class fixed on all three sides"""
    ref, layer, net, x, size = _bf16_cam_case(kind)
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV)
    want, target, mx = _textbook_cam(ref, layer, x, size, with_max=True)
    assert bool((mx > 0).all()), mx                      # every sample has a map to compare
    auto, _t = _textbook_cam(ref, layer, x, size, target=target, autocast=True)
    cam = explain.encoder_grad_cam(net, dev(x), target=target).cpu()
    if kind == "r1d":
        want, auto = want[:, 0], auto[:, 0]
    assert cam.shape == want.shape and cam.dtype == torch.float32 and cam.min() >= 0 and cam.max() <= 1
    mine, theirs = rel_err(cam, want), rel_err(auto, want)
    print(f"grad-cam {kind} bf16: rel_err {mine:.3e} (this library), {theirs:.3e} (torch CPU autocast)")
    assert mine < 1.3 * theirs + 0.02


def _state(net):
    return net.training, [p.requires_grad for p in net.parameters()], [p.grad is None for p in net.parameters()]


def test_grad_cam_leaves_no_state_behind():
    _ref, net, clin_in = _model_pair("pmb")
    img, sig, clin, _lab = fill.synthetic_batch(2, clin_dim=clin_in, **CAM_BATCH)
    specs = (net.image_encoder._spec, net.signal_encoder._spec)
    list(net.parameters())[3].requires_grad_(False)      # a parameter the caller froze stays frozen
    for mode in (True, False):
        net.train(mode)
        before = _state(net)
        explain.grad_cam(net, dev(img), dev(sig), dev(clin))
        assert _state(net) == before and all(g for g in before[2])
        assert all(s.keep_last is False and s.last is None for s in specs)
    enc = ResNet18(num_classes=2, compute_dtype="fp32").to(DEV).train()
    before = _state(enc)
    explain.encoder_grad_cam(enc, dev(img))
    assert _state(enc) == before and enc._spec.keep_last is False and enc._spec.last is None
    # a refused call (a CPU tensor) puts everything back as well
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain.grad_cam(net, dev(img), sig, dev(clin))
    assert all(s.keep_last is False and s.last is None for s in specs) and not net.image_encoder._forward_hooks


def test_grad_cam_between_a_training_forward_and_its_backward_changes_no_gradient():
    """the map's eval forward and head backward run between a training step's forward and backward: they share the backward
    scratch buffer and the encoders' specs with it, and must leave the step's parameter gradients as they were, bit for bit"""
    grads = []
    for with_cam in (False, True):
        _ref, net, clin_in = _model_pair("pmb")
        net.train()
        img, sig, clin, lab = fill.synthetic_batch(4, img_hw=(64, 64), sig_len=1000, clin_dim=clin_in, salt=9)
        out = net(dev(img), dev(sig), dev(clin))
        if with_cam:
            other = fill.synthetic_batch(2, clin_dim=clin_in, **CAM_BATCH)
            cams = explain.grad_cam(net, *(dev(t) for t in other[:3]))
            assert net.training and float(cams[0].max()) > 0
        HF.cross_entropy_plus(out[3], dev(lab), out[4], 0.1).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
        buffers = {k: b.clone() for k, b in net.named_buffers()}
        grads[-1].update({"buffer " + k: b.float() for k, b in buffers.items()})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 100
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
