"""ecgmm.explain.attention_maps / attention_rollout on the GPU: ECGTransformer1D(time_attention=True) against torch's float64
encoder with the same ``state_dict`` -- the maps from each layer's ``self_attn(need_weights=True)``, the rollout from the
explicit matrix product of ``a I + (1 - a) Abar_l``.  The yardstick of every chain is torch-fp32-CPU's own error against
float64 on the same formulas (f64check.check_chain, 8 x).  Then the properties of the relevance, the bit identities and the
trainer's ``rollout_samples``."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from ecgmm import explain
from ecgmm.config import Config
from oracle import fill

from . import f64check as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128)
B, LEN = 3, 48
LENGTHS = [48, 31, 17]
A = 0.5


@functools.lru_cache(maxsize=None)
def _model(time_attention=True):
    from ecgmm.train_physionet import ECGTransformer1D
    m = fill.hash_fill_module(ECGTransformer1D(time_attention=time_attention, **KW), "roll.")
    with torch.no_grad():
        m.pos_embedding.copy_(fill.hash_tensor(tuple(m.pos_embedding.shape), 841, 0.5))
    return m.to(DEV).eval()


def _x():
    return fill.hash_tensor((B, 1, LEN), 842, 1.0)


class TorchEncoder(nn.Module):
    """the front and the encoder of ECGTransformer1D(time_attention=True) in plain torch, its parameter names"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv1d(1, KW["d_model"], 3, padding=1)
        self.pos_embedding = nn.Parameter(torch.zeros(1, KW["seq_len"], KW["d_model"]))
        layer = nn.TransformerEncoderLayer(KW["d_model"], KW["nhead"], KW["dim_feedforward"], dropout=0.0, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, KW["num_layers"], enable_nested_tensor=False)

    def maps(self, x, lengths, average=True):
        """-> the attention weights of every layer, [B, L, L] or [B, heads, L, L] (layer by layer, so that they can be asked for)"""
        Ln = x.shape[2]
        live = torch.arange(Ln)[None, :] < torch.tensor(lengths)[:, None]
        x = x * live[:, None, :]
        h = self.conv(x).transpose(1, 2) + self.pos_embedding[:, :Ln]
        out = []
        for layer in self.transformer_encoder.layers:
            a, w = layer.self_attn(h, h, h, key_padding_mask=~live, need_weights=True, average_attn_weights=average)
            out.append(w)
            h = layer.norm1(h + a)
            h = layer.norm2(h + layer.linear2(torch.relu(layer.linear1(h))))
        return out


def _rollout_by_product(maps, lengths, a):
    """[B, L]: per record, (1 / len) 1^T (a I + (1 - a) Abar_L) .. (a I + (1 - a) Abar_1) on its live block, 0 behind it"""
    out = torch.zeros(maps[0].shape[0], maps[0].shape[1], dtype=maps[0].dtype)
    for n, ln in enumerate(lengths):
        eye = torch.eye(ln, dtype=maps[0].dtype)
        prod = a * eye + (1 - a) * maps[-1][n, :ln, :ln]
        for w in reversed(maps[:-1]):
            prod = prod @ (a * eye + (1 - a) * w[n, :ln, :ln])
        out[n, :ln] = torch.full((ln,), 1.0 / ln, dtype=maps[0].dtype) @ prod
    return out


@functools.lru_cache(maxsize=None)
def _reference(average=True):
    """(float64 maps, torch-fp32 maps) of the torch encoder with the model's state_dict; shared, read only"""
    sd = {k: v.detach().cpu() for k, v in _model().state_dict().items() if not k.startswith("classifier")}
    t32 = TorchEncoder()
    t32.load_state_dict(sd, strict=True)
    t32 = t32.train()          # dropout is 0; training mode keeps torch off its fused inference path
    t64 = copy.deepcopy(t32).double()
    with torch.no_grad():
        return t64.maps(_x().double(), LENGTHS, average), t32.maps(_x(), LENGTHS, average)


def _live_block(w, n, ln):
    return w[n, ..., :ln, :ln].reshape(-1)


@pytest.mark.parametrize("average", [True, False])
def test_attention_maps_against_torch_float64(average):
    m64, m32 = _reference(average)
    got = explain.attention_maps(_model(), _x().to(DEV), LENGTHS, average=average)
    assert len(got) == KW["num_layers"]
    for i, w in enumerate(got):
        w = w.cpu()
        assert tuple(w.shape) == ((B, LEN, LEN) if average else (B, KW["nhead"], LEN, LEN)) and not w.requires_grad
        cat = lambda t: torch.cat([_live_block(t, n, ln) for n, ln in enumerate(LENGTHS)])
        FC.check_chain(cat(w), cat(m64[i]), cat(m32[i]), "layer %d map, average=%s" % (i, average))
        for n, ln in enumerate(LENGTHS):       # exact zeros in the padded query rows and key columns
            assert bool((w[n, ..., ln:, :] == 0).all()) and bool((w[n, ..., :, ln:] == 0).all()), (i, n)


def test_attention_maps_without_lengths_and_across_the_batch():
    """shapes and plumbing (the accuracy is held above and in tests/test_attention_maps_ops_gpu.py).  1e-5: a row of at most 48
    fp32 probabilities, each within a few 1e-7 relative of a value <= 1, summed in float32 by torch: well below 48 * 2e-7"""
    x = _x().to(DEV)
    full = explain.attention_maps(_model(), x)
    assert [tuple(w.shape) for w in full] == [(B, LEN, LEN)] * 2
    assert float((full[0].sum(-1) - 1).abs().max()) < 1e-5
    across = explain.attention_maps(_model(False), x, average=False)           # the reference's default: S = B, N = L
    assert [tuple(w.shape) for w in across] == [(LEN, KW["nhead"], B, B)] * 2
    assert float((across[1].sum(-1) - 1).abs().max()) < 1e-5
    mha = _model().transformer_encoder.layers[0].self_attn
    h = fill.hash_tensor((B, LEN, KW["d_model"]), 843, 1.0).to(DEV)
    w = mha.attention_weights(h, lengths=LENGTHS)
    wh = mha.attention_weights(h, lengths=LENGTHS, average_attn_weights=False)
    assert tuple(w.shape) == (B, LEN, LEN) and tuple(wh.shape) == (B, KW["nhead"], LEN, LEN)
    assert torch.allclose(wh.mean(1), w, atol=1e-6) and bool((w[2, 17:] == 0).all()) and bool((w[2, :, 17:] == 0).all())
    with pytest.raises(ValueError, match="need_weights"):
        mha(h, need_weights=True)


def test_attention_rollout_against_the_matrix_product_in_float64():
    m64, m32 = _reference(True)
    ref, own = _rollout_by_product(m64, LENGTHS, A), _rollout_by_product(m32, LENGTHS, A)
    got = explain.attention_rollout(_model(), _x().to(DEV), LENGTHS, residual=A)
    assert tuple(got.shape) == (B, LEN) and got.dtype == torch.float32 and not got.requires_grad
    got = got.cpu()
    live = torch.arange(LEN)[None, :] < torch.tensor(LENGTHS)[:, None]
    r = FC.check_chain(got[live], ref[live], own[live], "rollout, residual %.2f" % A)
    assert bool((got >= 0).all()), "a negative relevance"
    assert bool((got[~live] == 0).all()), "relevance behind a record's length"
    # each record's relevance sums to 1: the chain bar of every live element, added up
    allow = r.bar * (ref.abs().sum(-1) + torch.tensor(LENGTHS) * float(ref[live].pow(2).mean().sqrt()))
    sums = got.double().sum(-1)
    print("sums - 1:", (sums - 1).tolist(), "allowed:", allow.tolist())
    assert bool(((sums - 1).abs() <= allow).all())
    # another residual, and the vector of a model without lengths
    got25 = explain.attention_rollout(_model(), _x().to(DEV), LENGTHS, residual=0.25).cpu()
    FC.check_chain(got25[live], _rollout_by_product(m64, LENGTHS, 0.25)[live], _rollout_by_product(m32, LENGTHS, 0.25)[live],
                   "rollout, residual 0.25")
    plain = explain.attention_rollout(_model(), _x().to(DEV)).cpu()
    assert float((plain.double().sum(-1) - 1).abs().max()) < 1e-5 and bool((plain > 0).all())


def test_a_record_alone_gives_the_bits_it_gives_in_the_batch():
    x = _x().to(DEV)
    got = explain.attention_rollout(_model(), x, LENGTHS)
    maps = explain.attention_maps(_model(), x, LENGTHS)
    for n, ln in enumerate(LENGTHS):
        alone = explain.attention_rollout(_model(), x[n:n + 1, :, :ln].contiguous())
        assert torch.equal(alone[0], got[n, :ln]), (n, ln)
        for a, b in zip(explain.attention_maps(_model(), x[n:n + 1, :, :ln].contiguous()), maps):
            assert torch.equal(a[0], b[n, :ln, :ln]), (n, ln)
    again = explain.attention_rollout(_model(), x, torch.tensor(LENGTHS, device=DEV))
    assert torch.equal(again, got)


def test_logits_with_a_sink_are_the_logits_without():
    x = _x().to(DEV)
    for time_attention, lengths in ((True, LENGTHS), (True, None), (False, None)):
        m = _model(time_attention)
        sink = []
        with torch.no_grad():
            base = m(x, lengths) if lengths is not None else m(x)
            with_sink = m(x, lengths, attention_sink=sink)
        assert torch.equal(base, with_sink)
        assert len(sink) == KW["num_layers"]
        for rec in sink:
            assert set(rec) == {"qkv", "lse", "S", "N", "heads", "batch_first", "lengths"}
            assert not rec["qkv"].requires_grad and not rec["lse"].requires_grad
            assert (rec["S"], rec["N"]) == ((LEN, B) if time_attention else (B, LEN)) and rec["heads"] == KW["nhead"]
            assert (rec["lengths"] is None) == (lengths is None)
    # in training mode too: the sink changes neither the launches nor the Philox draws
    from ecgmm.hip import functional as HF
    m = copy.deepcopy(_model()).train()
    HF.manual_seed(3)
    a = m(x, LENGTHS)
    HF.manual_seed(3)
    b = m(x, LENGTHS, attention_sink=[])
    assert torch.equal(a, b)
    b.sum().backward()                     # the lse output is non-differentiable: the backward runs as before
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_main_writes_the_rollout_of_the_first_test_records(tmp_path, monkeypatch):
    import ecgmm.train_physionet as TP
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (Config,), {"synthetic": True, "synthetic_train_size": 16, "synthetic_val_size": 8,
                                    "synthetic_test_size": 8, "device": "cuda", "checkpoint_dir": str(tmp_path / "ck")})
    real_records = TP.load_records

    def short_records(*a, **k):      # the synthetic records cut to 100 .. 200 samples: lengths that differ
        signals, labels = real_records(*a, **k)
        return [s[:100 + (37 * i) % 101] for i, s in enumerate(signals)], labels

    monkeypatch.setattr(TP, "load_records", short_records)
    _h, _r, ckpt = TP.main(cfg, num_epochs=1, quiet=True, model="transformer", max_len=200, time_attention=True,
                           use_lengths=True, rollout_samples=2)
    z = np.load(os.path.join(ckpt, "attention_rollout.npz"))
    assert sorted(z.files) == ["labels", "lengths", "probs", "relevance"]
    assert z["relevance"].shape == (2, 200) and z["relevance"].dtype == np.float32
    assert z["lengths"].shape == (2,) and z["labels"].shape == (2,) and z["probs"].shape == (2, 2)
    assert np.all((z["lengths"] >= 100) & (z["lengths"] <= 200))
    # the file's content is plausible (the accuracy is held above): 200 fp32 terms of a sum that is 1 stay within 200 * 2^-24
    assert np.allclose(z["relevance"].sum(1), 1.0, atol=1e-4) and np.allclose(z["probs"].sum(1), 1.0, atol=1e-5)
    for i in range(2):
        assert np.all(z["relevance"][i, z["lengths"][i]:] == 0) and np.all(z["relevance"][i, :z["lengths"][i]] > 0)
