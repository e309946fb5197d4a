"""CRNN.forward(x, lengths) and train_physionet2.main(use_lengths=True) on the GPU.

Model check: logits and every parameter gradient against the same weights evaluated as HF.crnn_front (the front end is the
reference's arithmetic, padding included, with or without lengths), then torch's packed LSTM in float64 on the CPU over
clamp(frames // 8, 1, T // 8) steps per record, a mean over each record's own steps and the classifier; the gradient of the
sequence goes back through the front end's own backward.  Bars: tests/test_crnn_gpu.py's (logits and loss 1e-3, gradients
rel_err < 5e-3, a conv bias in front of a training-mode BatchNorm below 1e-3)."""
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from ecgmm import train_physionet2 as T2
from ecgmm.crnn import CRNN, FocalLoss
from ecgmm.hip import functional as HF

from . import crnn_ref as R
from .util import DEV, dev, rel_err

pytestmark = pytest.mark.gpu
B, FQ, T = 5, 33, 64
FRAMES = [64, 9, 40, 64, 17]       # // 8: 8 (= T // 8), 1, 5, 8, 2


def _pair(seed=0):
    torch.manual_seed(seed)
    ref = R.CRNN()
    ref.classifier[2].p = 0.0
    nets = []
    for _ in range(2):
        net = CRNN(compute_dtype="fp32")
        net.load_state_dict(ref.state_dict(), strict=True)
        net.classifier[2].p = 0.0
        nets.append(net.to(DEV).train())
    torch.manual_seed(100 + seed)
    x = torch.randn(B, 1, FQ, T)       # noise behind each record's frames too: the padding only has to be finite
    return ref.double().train(), nets[0], nets[1], x, torch.tensor([0, 1, 1, 0, 1])


def test_crnn_with_lengths_logits_and_gradients():
    ref, net, twin, x, lab = _pair()
    steps = torch.tensor(FRAMES).div(8, rounding_mode="floor").clamp(1, T // 8)
    assert steps.tolist() == [8, 1, 5, 8, 2]
    # ours
    lg = net(dev(x), FRAMES)
    loss = FocalLoss()(lg, dev(lab))
    loss.backward()
    # the reference: the twin's front end on the device, the rest in float64 on the CPU
    params, buffers = twin._front_tables()
    bn = twin.conv1.block[1]
    seq = HF.crnn_front(dev(x), params, buffers, True, bn.momentum, bn.eps, twin._dtype)
    assert tuple(seq.shape) == (B, T // 8, 512)
    s64 = seq.detach().cpu().double().requires_grad_()
    yp, _ = ref.bilstm(pack_padded_sequence(s64, steps, batch_first=True, enforce_sorted=False))
    y, _ = pad_packed_sequence(yp, batch_first=True, total_length=T // 8)
    live = (torch.arange(T // 8)[None, :] < steps[:, None]).double()[:, :, None]
    lr = ref.classifier((y * live).sum(1) / steps.double()[:, None])
    loss_r = R.focal_loss(lr, lab)
    loss_r.backward()
    seq.backward(s64.grad.float().to(DEV))
    torch.cuda.synchronize()
    assert (lg.detach().cpu().double() - lr.detach()).abs().max().item() < 1e-3
    assert abs(loss.item() - loss_r.item()) < 1e-3
    bad = []
    theirs = dict(ref.named_parameters())
    for (k, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        if k.endswith("block.0.bias"):   # conv bias in front of a training-mode BatchNorm: true gradient 0
            assert p.grad.abs().max().item() < 1e-3, k
            continue
        want = q.grad.cpu() if k.startswith("conv") else theirs[k].grad
        e = rel_err(p.grad.cpu(), want)
        print("%-32s rel_err %.3g" % (k, e))
        if not e < 5e-3:
            bad.append((k, e))
    assert not bad, bad
    # and it is not the fixed model: leaving the padding out moves the logits by more than the bar above
    with torch.no_grad():
        assert (net(dev(x)) - net(dev(x), FRAMES)).abs().max().item() > 1e-3


def test_crnn_frames_below_eight_are_one_step():
    _, net, _, x, _ = _pair(seed=1)
    net.eval()
    with torch.no_grad():
        a = net(dev(x), [64, 3, 40, 64, 17])
        b = net(dev(x), [64, 15, 40, 64, 17])
        c = net(dev(x), torch.tensor([64, 8, 40, 64, 17], device=DEV))
    assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())
    with pytest.raises(ValueError, match=r"lengths\[1\] = 65"):
        net(dev(x), [64, 65, 40, 64, 17])


def test_trainer_with_lengths_trains_on_a_data_tree(tmp_path, monkeypatch):
    from .test_spectrogram_gpu import _write_tree
    monkeypatch.chdir(tmp_path)
    cfg, _, _ = _write_tree(tmp_path)
    seen = []
    forward = CRNN.forward

    def spy(self, x, lengths=None):
        seen.append(None if lengths is None else lengths.detach().cpu())
        return forward(self, x, lengths)

    monkeypatch.setattr(CRNN, "forward", spy)
    history, results, ckpt = T2.main(cfg, num_epochs=1, batch_size=16, quiet=True, use_lengths=True)
    print(history, results)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["val_loss"])
    assert os.path.exists(os.path.join(ckpt, "last.pth")) and os.path.exists(os.path.join(ckpt, "best.pth"))
    for tag in ("best", "last"):
        assert all(np.isfinite(results[tag][k]) for k in ("accuracy", "f1", "auc")), results
    # every forward got the records' own frames, longest first within the batch
    assert seen and all(l is not None and bool((l[1:] <= l[:-1]).all()) for l in seen)
    assert any(int(l.min()) < int(l.max()) for l in seen)
