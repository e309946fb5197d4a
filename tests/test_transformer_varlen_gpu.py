"""Lengths through the Transformer encoder on the GPU: a two-layer ecgmm.hip.nn.TransformerEncoder with ``lengths=`` against
torch's float64 encoder with ``src_key_padding_mask`` (the yardstick of every chain is torch-fp32-CPU's own error against
float64 on the same module, f64check.check_chain); ECGTransformer1D(time_attention=True) is deaf to its batch neighbours and to
its own padding, bit for bit; train_physionet.main(time_attention=True, use_lengths=True) trains."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.hip import nn as HN
from ecgmm.signal_model import FocalLoss
from oracle import fill

from . import f64check as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D_MODEL, NHEAD, FF, LAYERS = 64, 4, 128, 2
B, T = 4, 40
LENGTHS = [40, 17, 1, 9]


def _torch_run(enc, x, dout, pad):
    enc.zero_grad()
    x = x.clone().requires_grad_(True)
    out = enc(x, src_key_padding_mask=pad)
    (out * dout).sum().backward()
    return out.detach(), x.grad.detach(), {k: p.grad.detach() for k, p in enc.named_parameters()}


@pytest.mark.parametrize("bf", [True, False])
def test_two_layer_encoder_against_torch_float64(bf):
    layer = nn.TransformerEncoderLayer(D_MODEL, NHEAD, FF, dropout=0.0, batch_first=bf)
    te = nn.TransformerEncoder(layer, LAYERS, enable_nested_tensor=False)
    te = fill.hash_fill_module(te, "trv.").train()
    live = torch.arange(T)[None, :] < torch.tensor(LENGTHS)[:, None]                # [B, T]
    shape = (B, T, D_MODEL) if bf else (T, B, D_MODEL)
    live_x = live if bf else live.t()                                               # over the first two dims of x
    x = fill.hash_tensor(shape, 821, 1.0)
    dout = fill.hash_tensor(shape, 822, 1.0) * live_x[..., None]                    # the loss ignores the padding
    pad = ~live                                                                     # [N, S] as torch takes it
    o64, dx64, g64 = _torch_run(copy.deepcopy(te).double(), x.double(), dout.double(), pad)
    o32, dx32, g32 = _torch_run(te, x, dout, pad)
    assert float(dx64[~live_x].abs().max()) == 0                                    # torch agrees: no gradient into the padding
    ours = HN.TransformerEncoder(HN.TransformerEncoderLayer(D_MODEL, NHEAD, FF, dropout=0.0, batch_first=bf), LAYERS)
    ours.load_state_dict(te.state_dict(), strict=True)
    ours = ours.to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    out = ours(xg, lengths=LENGTHS)
    (out * dout.to(DEV)).sum().backward()
    name = "encoder bf%d " % bf
    FC.check_chain(out.detach().cpu()[live_x], o64[live_x], o32[live_x], name + "out (live rows)")
    dx = xg.grad.cpu()
    FC.check_chain(dx[live_x], dx64[live_x], dx32[live_x], name + "dx (live rows)")
    assert bool((dx[~live_x] == 0).all()), "dx is not exactly 0 in the padding"
    for k, p in ours.named_parameters():
        FC.check_chain(p.grad.cpu(), g64[k], g32[k], name + k)
    # device lengths are taken without a sync and give the same bits; without lengths the padding is attended to
    with torch.no_grad():
        again = ours(xg, lengths=torch.tensor(LENGTHS, device=DEV))
        plain = ours(xg)
    assert torch.equal(again, out)
    assert float((plain - out).detach().cpu()[live_x].abs().max()) > 1e-3


KW = dict(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128)
XLEN = [48, 20, 7, 33]


def _model(time_attention):
    from ecgmm.train_physionet import ECGTransformer1D
    torch.manual_seed(11)
    m = ECGTransformer1D(time_attention=time_attention, **KW)
    with torch.no_grad():
        m.pos_embedding.copy_(fill.hash_tensor(tuple(m.pos_embedding.shape), 831, 0.5))
    return m.to(DEV)


def _perturbed(x, i):
    """other finite values in the other three samples and in sample i's own padding"""
    y = 3.0 * fill.hash_tensor(tuple(x.shape), 833 + i, 1.0) + 0.5
    y[i, :, :XLEN[i]] = x[i, :, :XLEN[i]]
    return y


def test_time_attention_logits_depend_on_the_samples_own_live_part_only():
    x = fill.hash_tensor((4, 1, 48), 832, 1.0)
    timed, across = _model(True).eval(), _model(False).eval()
    across.load_state_dict(timed.state_dict(), strict=True)
    with torch.no_grad():
        base = timed(x.to(DEV), XLEN)
        base_across = across(x.to(DEV))
        assert bool(torch.isfinite(base).all())
        for i in range(4):
            y = _perturbed(x, i).to(DEV)
            assert torch.equal(timed(y, XLEN)[i], base[i]), "sample %d hears its neighbours or its padding" % i
            # the existing behaviour, as the contrast: attention across the batch mixes the samples
            assert not torch.equal(across(y)[i], base_across[i])
        # lengths matter: without them the padding is attended to and averaged
        assert not torch.equal(timed(x.to(DEV))[1], base[1])


def test_time_attention_training_with_dropout_is_seeded_and_finite():
    m = _model(True).train()
    assert m.transformer_encoder.layers[0].self_attn.dropout == 0.1
    x = fill.hash_tensor((4, 1, 48), 834, 1.0).to(DEV)
    labels = torch.tensor([0, 1, 1, 0], device=DEV)
    lengths = torch.tensor(XLEN, dtype=torch.int32, device=DEV)

    def step(seed):
        HF.manual_seed(seed)
        HF.release_grads(m)
        loss = FocalLoss()(m(x, lengths), labels)
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    l1, g1 = step(5)
    l2, g2 = step(5)
    l3, g3 = step(6)
    assert bool(torch.isfinite(l1)) and all(bool(torch.isfinite(g).all()) for g in g1)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(l1, l3)


def test_main_trains_with_time_attention_and_lengths(tmp_path, monkeypatch):
    import ecgmm.train_physionet as TP
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (Config,), {"synthetic": True, "synthetic_train_size": 24, "synthetic_val_size": 8,
                                    "synthetic_test_size": 8, "device": "cuda", "checkpoint_dir": str(tmp_path / "ck")})
    real_records = TP.load_records

    def short_records(*a, **k):      # the synthetic records (2000 .. 18000 samples) cut to 150 .. 400: lengths that differ
        signals, labels = real_records(*a, **k)
        return [s[:150 + (37 * i) % 251] for i, s in enumerate(signals)], labels

    monkeypatch.setattr(TP, "load_records", short_records)
    built, seen = [], []
    real = TP.build_model
    monkeypatch.setattr(TP, "build_model", lambda *a, **k: built.append(real(*a, **k)) or built[-1])
    real_forward = TP.ECGTransformer1D.forward

    def spy(self, x, lengths=None):
        seen.append(None if lengths is None else lengths.detach().cpu())
        return real_forward(self, x, lengths)

    monkeypatch.setattr(TP.ECGTransformer1D, "forward", spy)
    history, results, ckpt = TP.main(cfg, num_epochs=1, quiet=True, model="transformer", max_len=400, time_attention=True,
                                     use_lengths=True)
    m = built[-1]
    assert isinstance(m, TP.ECGTransformer1D) and m.time_attention
    assert all(layer.self_attn.batch_first for layer in m.transformer_encoder.layers)
    assert seen and all(s is not None and s.dtype == torch.int32 for s in seen)
    every = torch.cat(seen)
    assert int(every.min()) >= 150 and int(every.max()) <= 400 and every.unique().numel() > 4     # the records' own lengths
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["val_loss"])
    assert np.isfinite(results["last"]["accuracy"]) and os.path.exists(os.path.join(ckpt, "last.pth"))
