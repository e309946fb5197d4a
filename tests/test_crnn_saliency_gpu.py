"""Saliency of the spectrogram CRNN on the GPU (ecgmm/explain.py: spectrogram_gradients, spectrogram_grad_cam; the input
gradient of ecgmm/crnn.py's CRNN in both modes; train_physionet2.main(saliency_samples=k)) against the nn restatement of the
reference (tests/crnn_ref.py) on the CPU, same weights, built as tests/test_crnn_gpu.py builds its pair (B, F, T = 4, 33, 40,
dropout 0).

ReLU masks and pool winners are discontinuous, so the inputs are drawn -- first seed of 50 that qualifies, on the CPU, from the
reference alone, per mode -- such that R.margin_violations reports none.  Its default delta (1e-4 of max|z|) and 1e-5 qualify
no seed here: the three blocks hold 2.4e5 pre-activations, of which a share of about 0.8 * delta * max|z| lies inside the
margin, 80 and 8 of them (searched: none of the first 50 seeds either way).  DELTA = 1e-6 it is: an expected 0.8 violations
per draw, and still several times what separates the fp32 z of the first block (a 25-term dot product) from float64's.

Bars: tests/test_crnn_gpu.py's -- gradients rel_err <= 5e-3 in fp32; bf16 within 1.3x torch's CPU autocast + 0.02."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from ecgmm import explain as X
from ecgmm import train_physionet2 as T2
from ecgmm.config import Config
from ecgmm.crnn import CRNN, FocalLoss
from ecgmm.hip import functional as HF

from . import crnn_ref as R
from . import crnn_saliency_ref as S
from .util import DEV, dev, rel_err

pytestmark = pytest.mark.gpu
B, FQ, T = 4, 33, 40
DELTA = 1e-6
BAR = 5e-3
LAB = torch.tensor([0, 1, 1, 0])
LENGTHS = [40, 33, 17, 8]


@functools.lru_cache(maxsize=None)
def reference(training):
    """(the reference model fp32 on the CPU, dropout 0; x [B,1,F,T]) with every margin of ``training`` mode clear"""
    torch.manual_seed(0)
    ref = R.CRNN()
    ref.classifier[2].p = 0.0
    for seed in range(50):
        torch.manual_seed(100 + seed)
        x = torch.randn(B, 1, FQ, T)
        probe = copy.deepcopy(ref).double().train(training)
        with torch.no_grad():
            if not R.margin_violations(probe, x.double(), DELTA):
                return ref, x
    raise AssertionError("no seed among the first 50 clears the margins")


def ours(ref, dtype="fp32"):
    net = CRNN(compute_dtype=dtype)
    net.load_state_dict(ref.state_dict(), strict=True)
    net.classifier[2].p = 0.0
    return net.to(DEV)


def ref64_gradient(ref, x, target, lengths=None):
    """float64, eval mode: d (logit of target) / d x per record, and the logits"""
    m = copy.deepcopy(ref).double().eval()
    xr = x.double().requires_grad_()
    if lengths is None:
        logits = m(xr)
    else:       # as tests/test_crnn_varlen_gpu.py: packed LSTM over clamp(frames // 8, 1, T // 8) steps, mean over a record's own
        steps = torch.tensor(lengths).div(8, rounding_mode="floor").clamp(1, T // 8)
        yp, _ = m.bilstm(pack_padded_sequence(m.front(xr), steps, batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(yp, batch_first=True, total_length=T // 8)
        live = (torch.arange(T // 8)[None, :] < steps[:, None]).double()[:, :, None]
        logits = m.classifier((y * live).sum(1) / steps.double()[:, None])
    if target is None:
        target = logits.detach().argmax(1)
    elif not torch.is_tensor(target):
        target = torch.full((B,), int(target))
    (g,) = torch.autograd.grad(logits.gather(1, target.view(-1, 1)).sum(), xr)
    return g, logits.detach()


def snapshot(net):
    return ({k: v.clone() for k, v in net.named_buffers()}, [p.requires_grad for p in net.parameters()], net.training)


def assert_untouched(net, snap):
    bufs, flags, training = snap
    assert net.training == training
    assert [p.requires_grad for p in net.parameters()] == flags
    assert all(p.grad is None for p in net.parameters())
    for k, v in net.named_buffers():
        assert torch.equal(v, bufs[k]), k


@pytest.mark.parametrize("target", [None, 1, torch.tensor([0, 1, 1, 0])], ids=["predicted", "class1", "per-record"])
def test_spectrogram_gradients_fp32_eval(target):
    ref, x = reference(False)
    net = ours(ref).train()            # the call switches to eval mode and back
    net.classifier[0].bias.requires_grad_(False)
    snap = snapshot(net)
    g = X.spectrogram_gradients(net, dev(x), target=target)
    torch.cuda.synchronize()
    assert_untouched(net, snap)
    want, logits = ref64_gradient(ref, x, target)
    if target is None:                 # the predicted class is the reference's
        with torch.no_grad():
            mine = net.eval()(dev(x)).cpu()
        assert torch.equal(mine.argmax(1), logits.argmax(1)) and float((mine.double() - logits).abs().max()) < 1e-3
    assert tuple(g.shape) == (B, 1, FQ, T) and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
    e = rel_err(g.cpu(), want)
    print("d logit / d x: rel_err %.3g (|ref|max %.3g)" % (e, float(want.abs().max())))
    assert float(want.abs().max()) > 0 and e <= BAR


def _train_step(net, x, requires_grad):
    xg = dev(x).requires_grad_(requires_grad)
    loss = FocalLoss()(net(xg), dev(LAB))
    loss.backward()
    torch.cuda.synchronize()
    return xg, loss


def test_input_gradient_fp32_training_mode():
    ref, x = reference(True)
    net = ours(ref).train()
    xg, loss = _train_step(net, x, True)
    m = copy.deepcopy(ref).double().train()
    xr = x.double().requires_grad_()
    loss_r = R.focal_loss(m(xr), LAB)
    loss_r.backward()
    assert xg.grad is not None and abs(loss.item() - loss_r.item()) < 1e-3
    e = rel_err(xg.grad.cpu(), xr.grad)
    print("d loss / d x, training mode: rel_err %.3g (|ref|max %.3g)" % (e, float(xr.grad.abs().max())))
    assert bool(torch.isfinite(xg.grad).all()) and e <= BAR


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_parameter_gradients_are_bit_identical_with_and_without_input_gradient(dtype):
    ref, x = reference(True)
    grads = []
    for requires_grad in (False, True):
        net = ours(ref, dtype).train()
        xg, _ = _train_step(net, x, requires_grad)
        assert (xg.grad is not None) == requires_grad
        grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    assert all(bool(torch.isfinite(g).all()) for g in grads[0].values())
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_input_gradient_bf16_within_autocast_yardstick():
    """the form and constants of test_crnn_bf16_step_within_autocast_yardstick, applied to d loss / d x"""
    ref, x = reference(True)

    def cpu_grad(autocast):
        m = copy.deepcopy(ref).train()
        xr = x.clone().requires_grad_()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            lg = m(xr)
        R.focal_loss(lg.float(), LAB).backward()
        return xr.grad.float()
    f32, f16 = cpu_grad(False), cpu_grad(True)
    net = ours(ref, "bf16").train()
    xg, _ = _train_step(net, x, True)
    assert bool(torch.isfinite(xg.grad).all())
    mine, theirs = rel_err(xg.grad.cpu(), f32), rel_err(f16, f32)
    print("d loss / d x: ours %.3g, autocast %.3g" % (mine, theirs))
    assert mine < 1.3 * theirs + 0.02


def test_lengths_gradients_and_grad_cam(monkeypatch):
    """gradients against the float64 varlen reference; the map exactly 0 behind each record's frames and equal to the float64
    restatement fed the device's own seq / dseq within the op bound (tests/test_crnn_saliency_ops_gpu.py)"""
    ref, x = reference(False)
    net = ours(ref).eval()
    snap = snapshot(net)
    g = X.spectrogram_gradients(net, dev(x), LENGTHS)
    want, logits = ref64_gradient(ref, x, None, LENGTHS)
    with torch.no_grad():
        assert torch.equal(net(dev(x), LENGTHS).cpu().argmax(1), logits.argmax(1))
    e = rel_err(g.cpu(), want)
    print("d logit / d x with lengths: rel_err %.3g" % e)
    assert e <= BAR
    assert float(g[3, :, :, LENGTHS[3]:].abs().max()) > 0      # the convolutions see the padding: not zero just behind the end
    seen = {}
    inner = HF.crnn_grad_cam

    def spy(seq, dseq, steps, frames, *rest):
        seen.update(seq=seq.detach().cpu(), dseq=dseq.detach().cpu(), steps=steps.cpu(), frames=frames.cpu())
        return inner(seq, dseq, steps, frames, *rest)
    monkeypatch.setattr(HF, "crnn_grad_cam", spy)
    cam = X.spectrogram_grad_cam(net, dev(x), LENGTHS)
    torch.cuda.synchronize()
    assert_untouched(net, snap)
    cam = cam.cpu()
    assert tuple(cam.shape) == (B, FQ, T) and cam.dtype == torch.float32
    assert seen["steps"].tolist() == [5, 4, 2, 1] and seen["frames"].tolist() == LENGTHS
    for b, n in enumerate(LENGTHS):
        assert bool((cam[b, :, n:] == 0).all())
        assert bool((seen["dseq"][b, seen["steps"][b]:] == 0).all())      # the variable-length LSTM leaves exact zeros
    assert float(cam.min()) >= 0 and float(cam.max()) <= 1 and float(cam.amax((1, 2)).min()) > 0
    args = (seen["seq"], seen["dseq"], seen["steps"], seen["frames"], 128, FQ, T)
    err, bound = (cam.double() - S.gradcam_ref(*args)).abs(), S.gradcam_bound(*args)
    assert bool(torch.isfinite(bound).all())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("grad-cam with lengths: worst |err| %.3g, worst |err| / bound %.3g" % (float(err.max()), worst))
    assert bool((err <= bound).all())


def test_grad_cam_leaves_the_model_alone_and_matches_its_restatement(monkeypatch):
    ref, x = reference(False)
    net = ours(ref).train()
    net.conv2.block[1].weight.requires_grad_(False)
    snap = snapshot(net)
    seen = {}
    inner = HF.crnn_grad_cam

    def spy(seq, dseq, steps, frames, *rest):
        seen.update(seq=seq.detach().cpu(), dseq=dseq.detach().cpu(), steps=steps, frames=frames)
        return inner(seq, dseq, steps, frames, *rest)
    monkeypatch.setattr(HF, "crnn_grad_cam", spy)
    cam = X.spectrogram_grad_cam(net, dev(x), target=torch.tensor([1, 0, 1, 0])).cpu()
    assert_untouched(net, snap)
    assert seen["steps"] is None and seen["frames"] is None
    # dseq is the gradient of the chosen logits w.r.t. the front end's output: the reference's, in its layout
    m = copy.deepcopy(ref).double().eval()
    s = m.front(x.double()).detach().requires_grad_()
    y, _ = m.bilstm(s)
    (ds,) = torch.autograd.grad(m.classifier(y.mean(dim=1)).gather(1, torch.tensor([[1], [0], [1], [0]])).sum(), s)
    print("seq rel_err %.3g, dseq rel_err %.3g" % (rel_err(seen["seq"], s.detach()), rel_err(seen["dseq"], ds)))
    assert rel_err(seen["seq"], s.detach()) <= 1e-3 and rel_err(seen["dseq"], ds) <= BAR
    args = (seen["seq"], seen["dseq"], None, None, 128, FQ, T)
    err, bound = (cam.double() - S.gradcam_ref(*args)).abs(), S.gradcam_bound(*args)
    assert bool(torch.isfinite(bound).all()) and bool((err <= bound).all())
    assert float(cam.min()) >= 0 and float(cam.max()) <= 1


class _ShortSynthetic(Config):
    """the synthetic records of tests/test_spectrogram_gpu.py's entry-point test (its own copy)"""
    synthetic, synthetic_train_size, synthetic_val_size, synthetic_test_size = True, 24, 8, 8
    physionet2_max_len = 6000        # T = 189: the generated records run to 18000 samples
    device, compute_dtype = "cuda", "bf16"


def test_trainer_writes_the_saliency_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (_ShortSynthetic,), {"checkpoint_dir": str(tmp_path / "ck")})
    _, results, ckpt = T2.main(cfg, num_epochs=1, quiet=True, saliency_samples=2)
    assert np.isfinite(results["last"]["accuracy"])
    path = os.path.join(ckpt, "spectrogram_saliency.npz")
    assert os.path.exists(path)
    z = np.load(path)
    Tn = z["grad_cam"].shape[2]
    assert sorted(z.files) == ["frames", "grad_cam", "gradients", "labels", "probs"]
    assert z["grad_cam"].shape == (2, 33, Tn) and z["gradients"].shape == (2, 33, Tn) and Tn >= 8
    assert z["frames"].shape == (2,) and z["labels"].shape == (2,) and z["probs"].shape == (2, 2)
    assert all(np.isfinite(z[k]).all() for k in z.files)
    assert z["grad_cam"].min() >= 0 and z["grad_cam"].max() <= 1 and np.abs(z["gradients"]).max() > 0
    assert np.allclose(z["probs"].sum(1), 1, atol=1e-5) and (z["frames"] == Tn).all()
    # off by default: nothing is written
    cfg0 = type("Synth0", (_ShortSynthetic,), {"checkpoint_dir": str(tmp_path / "ck0")})
    _, _, ckpt0 = T2.main(cfg0, num_epochs=1, quiet=True)
    assert not os.path.exists(os.path.join(ckpt0, "spectrogram_saliency.npz"))
