"""``ecgmm.inference.Predictor`` of the spectrogram CRNN (ecgmm/crnn.py) at the shapes of tests/test_crnn_gpu.py (B = 4, F = 33,
T = 40): against the nn restatement of the reference in float64 and against the model's own eval forward (bars of
tests/test_crnn_gpu.py: 1e-3 on fp32 logits, bf16 within 1.3x torch's CPU autocast + 0.02), lengths, row independence,
stale weights, side effects, shape errors, ``predict_proba`` and the trainer."""
import copy

import numpy as np
import pytest
import torch

from ecgmm import train_physionet2 as T2
from ecgmm.config import Config
from ecgmm.crnn import CRNN
from ecgmm.hip import functional as HF
from ecgmm.inference import Predictor
from ecgmm.optim import FusedAdam

from . import crnn_ref as R
from .util import DEV, dev, rel_err

pytestmark = pytest.mark.gpu
B, FQ, T = 4, 33, 40


def pair(dtype="fp32", seed=0):
    """reference and model with the same weights; BatchNorm statistics and affine parameters away from their initial
    (0, 1, 1, 0), a few gammas negative, so that the fold has something to fold"""
    torch.manual_seed(seed)
    ref = R.CRNN()
    with torch.no_grad():
        for blk in (ref.conv1, ref.conv2, ref.conv3):
            bn = blk.block[1]
            n = bn.num_features
            bn.running_mean.copy_(0.2 * torch.randn(n))
            bn.running_var.copy_(torch.rand(n) + 0.5)
            bn.weight.copy_(1.0 + 0.2 * torch.randn(n))
            bn.weight[::5] = -bn.weight[::5]
            bn.bias.copy_(0.1 * torch.randn(n))
            bn.num_batches_tracked.fill_(3)
    net = CRNN(compute_dtype=dtype)
    net.load_state_dict(ref.state_dict(), strict=True)
    torch.manual_seed(100 + seed)
    x = torch.randn(B, 1, FQ, T)
    return ref.eval(), net.to(DEV).eval(), x


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def test_predictor_fp32_against_float64_and_the_eval_forward():
    ref, net, x = pair()
    with torch.no_grad():
        want = copy.deepcopy(ref).double()(x.double())
        own = net(dev(x))
    got = Predictor(net)(dev(x))
    assert got.shape == (B, 2) and torch.isfinite(got).all()
    e_ref, e_own = maxerr(got, want), maxerr(got, own)
    print("predictor vs float64 %.3g, vs net.eval() %.3g, net.eval() vs float64 %.3g" % (e_ref, e_own, maxerr(own, want)))
    assert e_ref < 1e-3 and e_own < 1e-3
    assert not got.requires_grad


def test_predictor_lengths():
    ref, net, x = pair(seed=1)
    p = Predictor(net)
    lengths = [40, 17, 8, 33]
    xg = dev(x)
    with torch.no_grad():
        own = net(xg, lengths)
    got = p(xg, lengths)
    assert maxerr(got, own) < 1e-3
    assert torch.equal(p(xg, lengths=torch.tensor(lengths)), got)           # keyword, CPU tensor
    assert torch.equal(p(xg, torch.tensor(lengths, device=DEV)), got)       # device tensor, taken as given
    full = p(xg)
    # a row whose length is the whole spectrogram: the no-lengths answer (other kernels, another summation order: same bar)
    assert maxerr(got[0], full[0]) < 1e-3
    assert not torch.equal(got[1], full[1])
    with pytest.raises(ValueError, match="lengths"):
        p(xg, [40, 17, 8, 41])


def test_predictor_bf16_within_autocast_yardstick():
    """the yardstick of test_crnn_bf16_step_within_autocast_yardstick: autocast is the reference, 1.3x + 0.02 the margin"""
    ref, net, x = pair("bf16", seed=3)
    with torch.no_grad():
        f32 = copy.deepcopy(ref)(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            f16 = copy.deepcopy(ref)(x).float()
        own = net(dev(x))
    got = Predictor(net)(dev(x))
    assert torch.isfinite(got).all()
    mine, theirs, evals = rel_err(got.cpu(), f32), rel_err(f16, f32), rel_err(own.cpu(), f32)
    print("logits: predictor %.3g, eval path %.3g, autocast %.3g" % (mine, evals, theirs))
    assert mine < 1.3 * theirs + 0.02


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predictor_row_independence_and_determinism(dtype):
    _, net, x = pair(dtype, seed=4)
    p = Predictor(net)
    xg = dev(x)
    four, one = p(xg), p(xg[:1].contiguous())
    assert torch.equal(four[:1], one), "row 0 of the batch-4 call differs from the batch-1 call"
    assert torch.equal(p(xg), four)


def test_predictor_is_stale_until_refresh_and_has_no_side_effects():
    _, net, x = pair(seed=5)
    xg, lab = dev(x), dev(torch.tensor([0, 1, 1, 0]))
    p = Predictor(net)
    old = p(xg)
    # a training step: FusedAdam writes the parameters through raw pointers, the forward moves the running statistics
    net.train()
    net.classifier[2].p = 0.0
    opt = FusedAdam(net.parameters(), lr=1e-2)
    HF.focal_loss(net(xg), lab).backward()
    opt.step()
    torch.cuda.synchronize()
    # called on a model in train mode, with .grad populated: nothing but the answer may come of it
    state = {k: v.clone() for k, v in net.state_dict().items()}
    grads = {k: q.grad.clone() for k, q in net.named_parameters()}
    assert torch.equal(p(xg), old), "the predictor must keep answering from its snapshot until refresh()"
    assert torch.equal(p(xg, [40, 17, 8, 33]), p(xg, [40, 17, 8, 33]))
    assert net.training and all(m.training for m in net.modules())
    for k, v in net.state_dict().items():      # parameters and every buffer, num_batches_tracked included
        assert torch.equal(v, state[k]), k
    for k, q in net.named_parameters():
        assert torch.equal(q.grad, grads[k]), k
    assert int(net.conv1.block[1].num_batches_tracked) == 4
    net.eval()
    with torch.no_grad():
        new = net(xg)
    assert maxerr(new, old) > 1e-3, "the step was meant to move the logits"
    assert torch.equal(p(xg), old)
    assert p.refresh() is p
    assert maxerr(p(xg), new) < 1e-3
    assert not net.training


def test_predictor_refuses_a_changed_compute_dtype_and_bad_shapes():
    _, net, x = pair(seed=6)
    p = Predictor(net)
    xg = dev(x)
    for bad, exc in ((xg[:, 0], ValueError), (torch.cat([xg, xg], 1), ValueError), (dev(torch.randn(2, 1, 40, T)), ValueError),
                     (dev(torch.randn(2, 1, FQ, 7)), ValueError), (x, RuntimeError)):
        with pytest.raises(exc) as own:
            net(bad)
        with pytest.raises(exc) as mine:
            p(bad)
        assert str(mine.value).split(":")[-1] == str(own.value).split(":")[-1]    # CRNN._front's messages
    with pytest.raises(TypeError):
        p(xg, [40] * 4, [40] * 4)
    net.compute_dtype = "bf16"
    with pytest.raises(RuntimeError, match="refresh"):
        p(xg)
    net.compute_dtype = "fp32"
    p(xg)


def test_predict_proba_in_both_batch_forms():
    _, net, x = pair(seed=7)
    p = Predictor(net)
    spec = dev(torch.cat([x, x.flip(0), 0.5 * x])[:10])
    labels = torch.arange(10) % 2
    frames = torch.tensor([40, 33, 8, 17, 40, 25, 40, 9, 39, 16], dtype=torch.int32)
    plain = [(spec[i:i + 4], labels[i:i + 4]) for i in range(0, 10, 4)]
    withlen = [((spec[i:i + 4], dev(frames[i:i + 4])), labels[i:i + 4]) for i in range(0, 10, 4)]
    prob, lab, idx = p.predict_proba(plain)
    assert prob.shape == (10, 2) and torch.equal(lab, labels) and torch.equal(idx, torch.arange(10))
    assert torch.allclose(prob.sum(1), torch.ones(10), atol=1e-6)
    with torch.no_grad():
        want = torch.softmax(net(spec).cpu(), 1)
        want_len = torch.softmax(net(spec, frames).cpu(), 1)
    assert (prob - want).abs().max().item() < 1e-3
    prob2, lab2, _ = p.predict_proba(withlen)
    assert torch.equal(lab2, labels) and (prob2 - want_len).abs().max().item() < 1e-3
    assert torch.equal(p.logits(spec[:4]), p(spec[:4]))


class _ShortSynthetic(Config):    # the synthetic data of tests/test_spectrogram_gpu.py::test_entry_point_runs_without_data
    synthetic, synthetic_train_size, synthetic_val_size, synthetic_test_size = True, 24, 8, 8
    physionet2_max_len = 6000
    device, compute_dtype = "cuda", "fp32"


@pytest.mark.parametrize("use_lengths", [False, True], ids=["padded_argument", "lengths_config_switch"])
def test_trainer_with_predictor(tmp_path, monkeypatch, use_lengths):
    """padded batches with ``main(use_predictor=True)``; batches with lengths with ``config.physionet2_use_predictor``"""
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (_ShortSynthetic,), {"checkpoint_dir": str(tmp_path / "ck"), "physionet2_use_predictor": use_lengths})
    refreshed, real = [], Predictor.refresh

    def counting(self):
        refreshed.append(self)
        return real(self)
    monkeypatch.setattr(Predictor, "refresh", counting)
    history, results, ckpt = T2.main(cfg, num_epochs=1, quiet=True, use_predictor=not use_lengths, use_lengths=use_lengths)
    monkeypatch.setattr(Predictor, "refresh", real)
    assert len(refreshed) >= 2, "fit() and test_checkpoints() refresh the predictor: after the epoch, after each checkpoint load"
    print(history, results)
    assert len(history) == 1 and np.isfinite(history[0]["val_loss"]) and np.isfinite(history[0]["val_acc"])
    assert np.isfinite(results["last"]["accuracy"])
    # the same test split through both forwards, with the weights the run ended on
    import os
    model = CRNN(compute_dtype="fp32")
    model.load_state_dict(torch.load(os.path.join(ckpt, "last.pth"), map_location="cpu"))
    model = model.to(DEV)
    _, _, test_loader = T2.get_spectrogram_dataloaders(cfg, use_lengths=use_lengths)
    p = Predictor(model)
    y_own, prob_own, _ = T2.predict_split(model, test_loader)
    y_p, prob_p, _ = T2.predict_split(model, test_loader, predictor=p)
    assert np.array_equal(y_own, y_p) and len(y_p) == len(test_loader.dataset) > 0
    err = np.abs(prob_p[:, 1] - prob_own[:, 1]).max()
    print("class-1 probabilities: max |predictor - eval forward| = %.3g" % err)
    assert err < 1e-3
    res = T2.evaluate(model, test_loader, predictor=p)
    assert np.isfinite(res["accuracy"])
