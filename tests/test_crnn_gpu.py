"""The CRNN module (ecgmm/crnn.py; train_physionet2.py:55-117) against the nn restatement of the reference (tests/crnn_ref.py)
on the CPU in float64, same weights: logits, FocalLoss, every parameter gradient, three Adam steps, train / eval / train,
checkpoint round trip, one bf16 step.  Bars: tests/test_models_gpu.py's (logits and loss 1e-3, gradients rel_err < 5e-3,
three-step losses 2e-3, bf16 within 1.3x torch's CPU autocast + 0.02)."""
import copy

import numpy as np
import pytest
import torch

from ecgmm.crnn import CRNN, FocalLoss
from ecgmm.hip import functional as HF
from ecgmm.optim import FusedAdam

from . import crnn_ref as R
from .util import DEV, dev, rel_err

pytestmark = pytest.mark.gpu
B, FQ, T = 4, 33, 40


def pair(dtype="fp32", seed=0):
    torch.manual_seed(seed)
    ref = R.CRNN()
    ref.classifier[2].p = 0.0
    net = CRNN(compute_dtype=dtype)
    net.load_state_dict(ref.state_dict(), strict=True)
    net.classifier[2].p = 0.0
    torch.manual_seed(100 + seed)
    x = torch.randn(B, 1, FQ, T)
    lab = torch.tensor([0, 1, 1, 0])
    return ref, net.to(DEV), x, lab


def test_crnn_fp32_logits_loss_and_gradients():
    ref, net, x, lab = pair()
    ref = ref.double().train()
    lr = ref(x.double())
    loss_r = R.focal_loss(lr, lab)
    loss_r.backward()
    net.train()
    lg = net(dev(x))
    loss = FocalLoss()(lg, dev(lab))
    loss.backward()
    torch.cuda.synchronize()
    assert (lg.detach().cpu().double() - lr.detach()).abs().max().item() < 1e-3
    assert abs(loss.item() - loss_r.item()) < 1e-3
    bad = []
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        if k.endswith("block.0.bias"):   # conv bias in front of a training-mode BatchNorm: true gradient 0
            assert p.grad.abs().max().item() < 1e-3, k
            continue
        e = rel_err(p.grad.cpu(), q.grad)
        print("%-32s rel_err %.3g" % (k, e))
        if not e < 5e-3:
            bad.append((k, e))
    assert not bad, bad
    for (k, v), (_, r) in zip(net.named_buffers(), ref.named_buffers()):
        assert torch.allclose(v.cpu().double(), r.double(), rtol=5e-3, atol=1e-4), k


def test_crnn_three_adam_steps_track_torch():
    ref, net, x, lab = pair(seed=1)
    ref.train(); net.train()
    opt_r = torch.optim.Adam(ref.parameters(), lr=1e-3)
    opt = FusedAdam(net.parameters(), lr=1e-3)
    lr_, lm = [], []
    for _ in range(3):
        opt_r.zero_grad()
        l = R.focal_loss(ref(x), lab)
        l.backward(); opt_r.step(); lr_.append(l.item())
        opt.zero_grad()
        l = HF.focal_loss(net(dev(x)), dev(lab))
        l.backward(); opt.step(); lm.append(l.item())
    print(lm, lr_)
    assert np.allclose(lm, lr_, atol=2e-3), (lm, lr_)


def test_crnn_train_eval_train_and_checkpoint(tmp_path):
    ref, net, x, lab = pair(seed=2)
    outs_r, outs = [], []
    for mode in (True, False, True):
        ref.train(mode); net.train(mode)
        with torch.no_grad():
            outs_r.append(ref(x))
            outs.append(net(dev(x)).cpu())
    for a, r in zip(outs, outs_r):
        assert (a - r).abs().max().item() < 1e-3
    path = tmp_path / "crnn.pth"
    torch.save(ref.state_dict(), path)
    fresh = CRNN()
    fresh.load_state_dict(torch.load(path), strict=True)
    fresh = fresh.to(DEV).eval()
    ref.eval()
    with torch.no_grad():
        assert (fresh(dev(x)).cpu() - ref(x)).abs().max().item() < 1e-3
    back = R.CRNN()
    back.load_state_dict({k: v.cpu() for k, v in fresh.state_dict().items()}, strict=True)


def test_crnn_bf16_step_within_autocast_yardstick():
    ref, net, x, lab = pair("bf16", seed=3)
    ref.train(); net.train()
    with torch.no_grad():
        f32 = copy.deepcopy(ref)(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            f16 = copy.deepcopy(ref)(x).float()
    opt = FusedAdam(net.parameters(), lr=1e-3)
    lg = net(dev(x))
    loss = HF.focal_loss(lg, dev(lab))
    loss.backward(); opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(lg).all() and np.isfinite(loss.item())
    assert all(torch.isfinite(p).all() for p in net.parameters())
    mine, theirs = rel_err(lg.detach().cpu(), f32), rel_err(f16, f32)
    print("logits: ours %.3g, autocast %.3g" % (mine, theirs))
    assert mine < 1.3 * theirs + 0.02
