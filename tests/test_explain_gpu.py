"""ecgmm/explain.py on the GPU: whole-model input gradients against torch.autograd.grad on the CPU oracle, and Grad-CAM
against the textbook computation on the oracle (hooks on the last stage: gradient of the logit w.r.t. the activation,
spatial mean, weighted sum, ReLU, max-normalise, bilinear upsample with align_corners=False)."""
import pytest
import torch
import torch.nn.functional as F

from ecgmm import explain
from ecgmm.config import Config
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


def _textbook_cam(ref, layer, x, size):
    acts = {}
    h = layer.register_forward_hook(lambda _m, _i, o: acts.__setitem__("a", o))
    try:
        logits = ref.eval()(x)
    finally:
        h.remove()
    a = acts["a"]
    target = logits.detach().argmax(dim=1)
    g, = torch.autograd.grad(logits.gather(1, target[:, None]).sum(), a)
    if a.dim() == 3:                       # [N, C, L'] -> [N, C, 1, L']
        a, g = a[:, :, None, :], g[:, :, None, :]
    alpha = g.mean(dim=(2, 3), keepdim=True)
    cam = F.relu((alpha * a).sum(dim=1)).detach()
    mx = cam.flatten(1).max(dim=1).values[:, None, None]
    cam = torch.where(mx > 0, cam / mx.clamp_min(1e-30), torch.zeros_like(cam))
    up = F.interpolate(cam[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]
    return up, target


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
