"""The Transformer encoder on the GPU: ecgmm.hip.nn.TransformerEncoderLayer against torch's float64 layer, the golden of the
reference's own ECGTransformer1D (tests/golden/g11_transformer.npz, tools/make_transformer_golden.py), dropout in training
and train_physionet.main(model="transformer").  The yardstick of every chain is torch-fp32-CPU's own error against float64
on the same module (f64check.check_chain), never the code under test."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.hip import nn as HN
from ecgmm.signal_model import FocalLoss, ResNet1D_SE
from oracle import fill

from . import f64check as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, (nn.MultiheadAttention, HN.MultiheadAttention)):
            m.dropout = 0.0
    return model


def _torch_run(layer, x, dout):
    layer.zero_grad()
    x = x.clone().requires_grad_(True)
    out = layer(x)
    (out * dout).sum().backward()
    return out.detach(), x.grad.detach(), {k: p.grad.detach() for k, p in layer.named_parameters()}


@pytest.mark.parametrize("d_model,nhead,ff,bf", [(128, 4, 256, False), (64, 4, 128, True)])
def test_layer_against_torch_float64(d_model, nhead, ff, bf):
    tl = fill.hash_fill_module(nn.TransformerEncoderLayer(d_model, nhead, ff, dropout=0.0, batch_first=bf), "tr.").train()
    x = fill.hash_tensor((6, 40, d_model), 801, 1.0)
    dout = fill.hash_tensor((6, 40, d_model), 802, 1.0)
    o64, dx64, g64 = _torch_run(copy.deepcopy(tl).double(), x.double(), dout.double())
    o32, dx32, g32 = _torch_run(tl, x, dout)
    ours = HN.TransformerEncoderLayer(d_model, nhead, ff, dropout=0.0, batch_first=bf)
    ours.load_state_dict(tl.state_dict(), strict=True)
    ours = ours.to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    out = ours(xg)
    (out * dout.to(DEV)).sum().backward()
    name = "layer %d/%d/%d bf%d " % (d_model, nhead, ff, bf)
    FC.check_chain(out.detach().cpu(), o64, o32, name + "out")
    FC.check_chain(xg.grad.cpu(), dx64, dx32, name + "dx")
    for k, p in ours.named_parameters():
        FC.check_chain(p.grad.cpu(), g64[k], g32[k], name + k)
    with torch.no_grad():
        assert torch.equal(ours.eval()(xg), out), "eval mode differs from train mode at dropout 0"


def _golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "g11_transformer.npz"))
    sd = {str(k): torch.from_numpy(z["sd/" + str(k)]) for k in z["keys"]}
    # a float64 gradient is stored as the float32 pair (torch-fp32-CPU's own gradient, float64 - that): see the tool
    g = {k[4:]: (torch.from_numpy(z[k]).double() + torch.from_numpy(z["g64lo/" + k[4:]]).double(), torch.from_numpy(z[k]))
         for k in z.files if k.startswith("g32/")}
    return z, sd, g


def _golden_model(sd):
    from ecgmm.train_physionet import ECGTransformer1D
    m = _no_dropout(ECGTransformer1D(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train()


def test_golden_of_the_reference_class(golden_dir):
    z, sd, g = _golden(golden_dir)
    m = _golden_model(sd)
    assert set(g) == {k for k, _ in m.named_parameters()}
    x, labels = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV)
    logits = m(x)
    loss = FocalLoss(alpha=1.0, gamma=2.0)(logits, labels)
    loss.backward()
    FC.check_chain(logits.detach().cpu(), torch.from_numpy(z["logits64"]), torch.from_numpy(z["logits32"]), "g11 logits")
    FC.check_chain(loss.detach().cpu().reshape(1), torch.from_numpy(z["loss64"]).reshape(1),
                   torch.from_numpy(z["loss32"]).reshape(1), "g11 focal loss")
    for k, p in m.named_parameters():
        FC.check_chain(p.grad.cpu(), g[k][0], g[k][1], "g11 grad " + k)


def test_golden_attends_across_the_batch(golden_dir):
    """the reference feeds [B, L, E] to batch_first=False layers: adding 1 to sample 0 moves the logits of samples 1-4 by the
    stored amounts.  Each logit is held to the chain bar of the golden, so a difference of two is held to the sum of both."""
    z, sd, _ = _golden(golden_dir)
    m = _golden_model(sd)
    x = torch.from_numpy(z["x"]).to(DEV)
    xp = x.clone()
    xp[0] += 1.0
    with torch.no_grad():
        moved = (m(xp) - m(x)).cpu().double()
    l64, l64p = torch.from_numpy(z["logits64"]), torch.from_numpy(z["logits64_perturbed"])
    want = l64p - l64
    bar = FC.CHAIN_MARGIN * max(FC.chain_figure(torch.from_numpy(z["logits32"]), l64), FC.U)
    tol = bar * (l64.abs() + l64.pow(2).mean().sqrt() + l64p.abs() + l64p.pow(2).mean().sqrt())
    print("moved", moved[1:].abs().max().item(), "stored", want[1:].abs().max().item(), "tolerance", tol.max().item())
    assert float(want[1:].abs().max()) > 100 * float(tol.max()), "the golden's samples do not interact"
    assert bool(((moved - want).abs() <= tol).all()), \
        "batch_first slip: the logits of samples 1-4 do not follow sample 0 as the reference's do"


def test_dropout_in_training_is_seeded():
    from ecgmm.train_physionet import ECGTransformer1D
    torch.manual_seed(3)
    m = ECGTransformer1D(seq_len=40, d_model=64, nhead=4, num_layers=2, dim_feedforward=128).to(DEV).train()
    assert m.transformer_encoder.layers[0].self_attn.dropout == 0.1
    x = fill.hash_tensor((6, 1, 40), 811, 1.0).to(DEV)
    labels = torch.tensor([0, 1, 1, 0, 1, 0], device=DEV)

    def step(seed):
        HF.manual_seed(seed)
        HF.release_grads(m)
        loss = FocalLoss()(m(x), labels)
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    l1, g1 = step(5)
    l2, g2 = step(5)
    l3, g3 = step(6)
    assert bool(torch.isfinite(l1)) and all(bool(torch.isfinite(g).all()) for g in g1)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(l1, l3) and any(not torch.equal(a, b) for a, b in zip(g1, g3))


def test_main_trains_the_transformer(tmp_path, monkeypatch):
    import ecgmm.train_physionet as TP
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (Config,), {"synthetic": True, "synthetic_train_size": 24, "synthetic_val_size": 8,
                                    "synthetic_test_size": 8, "device": "cuda", "checkpoint_dir": str(tmp_path / "ck")})
    built = []
    real = TP.build_model
    monkeypatch.setattr(TP, "build_model", lambda *a, **k: built.append(real(*a, **k)) or built[-1])
    history, results, ckpt = TP.main(cfg, num_epochs=1, quiet=True, model="transformer", max_len=400)
    assert isinstance(built[-1], TP.ECGTransformer1D) and tuple(built[-1].pos_embedding.shape) == (1, 400, 128)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["val_loss"])
    assert np.isfinite(results["last"]["accuracy"]) and os.path.exists(os.path.join(ckpt, "last.pth"))
    # a torch module of the reference's layout takes the checkpoint
    sd = torch.load(os.path.join(ckpt, "last.pth"), map_location="cpu")
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(128, 4, 256), 2, enable_nested_tensor=False)
    enc.load_state_dict({k[len("transformer_encoder."):]: v for k, v in sd.items() if k.startswith("transformer_encoder.")},
                        strict=True)


def test_main_defaults_still_build_the_resnet(tmp_path, monkeypatch):
    import ecgmm.train_physionet as TP
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (Config,), {"synthetic": True, "synthetic_train_size": 16, "synthetic_val_size": 8,
                                    "synthetic_test_size": 8, "device": "cuda", "checkpoint_dir": str(tmp_path / "ck")})
    built = []
    real = TP.build_model
    monkeypatch.setattr(TP, "build_model", lambda *a, **k: built.append(real(*a, **k)) or built[-1])
    TP.main(cfg, num_epochs=1, quiet=True)
    assert type(built[-1]) is ResNet1D_SE
