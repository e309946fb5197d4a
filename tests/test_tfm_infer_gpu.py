"""Predictor(ECGTransformer1D) on the GPU: against torch's float64 model (nn.TransformerEncoder, src_key_padding_mask for
lengths) under the chain bar of tests/f64check.py (8 x torch-fp32-CPU's own error against float64), the golden of the
reference's own class through the predictor, lengths (a record alone, NaN in the padding), refresh(), side effects, both
trainers' switch and the launch count.  The yardstick is always float64 or torch, never the code under test."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from ecgmm.config import Config
from ecgmm.inference import Predictor
from ecgmm.optim import FusedAdam
from ecgmm.signal_model import FocalLoss
from ecgmm.train_physionet import ECGTransformer1D
from oracle import fill

from . import f64check as FC
from . import tfm_infer_abi as A
from .test_transformer_gpu import _golden, _no_dropout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, LEN = 6, 40
LENGTHS = [40, 17, 1, 9, 33, 24]


class TorchRef(nn.Module):
    """ECGTransformer1D in plain torch with its attribute names (train_physionet.py:211-240 of the reference): the layers get
    [B, L, E] whatever batch_first says; lengths as src_key_padding_mask, zeroed raw padding and a masked mean"""

    def __init__(self, d_model, nhead, ff, layers, seq_len, classes, time_attention):
        super().__init__()
        self.conv = nn.Conv1d(1, d_model, 3, padding=1)
        self.pos_embedding = nn.Parameter(torch.zeros(1, seq_len, d_model))
        layer = nn.TransformerEncoderLayer(d_model, nhead, ff, dropout=0.0, batch_first=time_attention)
        self.transformer_encoder = nn.TransformerEncoder(layer, layers, enable_nested_tensor=False)
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(d_model, 64), nn.ReLU(), nn.Dropout(0.0), nn.Linear(64, classes))

    def forward(self, x, lengths=None):
        Ln = x.shape[2]
        live = None
        if lengths is not None:
            live = torch.arange(Ln)[None, :] < torch.as_tensor(lengths)[:, None]
            x = x * live[:, None, :]
        x = self.conv(x).permute(0, 2, 1) + self.pos_embedding[:, :Ln]
        if live is None:
            return self.classifier(self.transformer_encoder(x).mean(1))
        x = self.transformer_encoder(x, src_key_padding_mask=~live)
        w = live.to(x.dtype)
        return self.classifier((x * w[..., None]).sum(1) / w.sum(1, keepdim=True))


def _pair(d_model, nhead, ff, time_attention, layers=2, seq_len=LEN, classes=2, tag="tfi."):
    """(torch fp32 reference in train mode at dropout 0 -- no fast path --, our model on the device in eval mode)"""
    ref = fill.hash_fill_module(TorchRef(d_model, nhead, ff, layers, seq_len, classes, time_attention), tag).train()
    ours = ECGTransformer1D(seq_len=seq_len, num_classes=classes, d_model=d_model, nhead=nhead, num_layers=layers,
                            dim_feedforward=ff, time_attention=time_attention)
    ours.load_state_dict(ref.state_dict(), strict=True)
    return ref, ours.to(DEV).eval()


def _chain(name, got, ref, x, lengths=None):
    with torch.no_grad():
        l64 = copy.deepcopy(ref).double()(x.double(), lengths)
        l32 = ref(x, lengths)
    return FC.check_chain(got.detach().cpu(), l64, l32, name)


@pytest.mark.parametrize("d_model,nhead,ff,time_attention,lengths", [(128, 4, 256, False, None), (64, 4, 128, True, None),
                                                                      (64, 4, 128, True, LENGTHS)],
                         ids=["across-128", "time-64", "time-64-lengths"])
def test_predictor_against_torch_float64(d_model, nhead, ff, time_attention, lengths):
    ref, ours = _pair(d_model, nhead, ff, time_attention)
    x = fill.hash_tensor((B, 1, LEN), 841, 1.0)
    predict = Predictor(ours)
    got = predict(x.to(DEV)) if lengths is None else predict(x.to(DEV), lengths)
    assert got.shape == (B, 2) and not got.requires_grad
    _chain("predictor %d/%d/%d time%d%s" % (d_model, nhead, ff, time_attention, " lengths" if lengths else ""), got, ref, x, lengths)
    # the model's own eval forward is held to the same bar: both are forwards of the same network
    with torch.no_grad():
        own = ours(x.to(DEV)) if lengths is None else ours(x.to(DEV), lengths)
    _chain("model.eval() of the same", own, ref, x, lengths)
    assert torch.equal(predict.logits(x.to(DEV)) if lengths is None else predict.logits(x.to(DEV), lengths), got)


def _golden_predictor(golden_dir):
    z, sd, _ = _golden(golden_dir)
    m = _no_dropout(ECGTransformer1D(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128))
    m.load_state_dict(sd, strict=True)
    return z, Predictor(m.to(DEV).eval())


def test_golden_of_the_reference_class_through_the_predictor(golden_dir):
    z, predict = _golden_predictor(golden_dir)
    logits = predict(torch.from_numpy(z["x"]).to(DEV))
    FC.check_chain(logits.cpu(), torch.from_numpy(z["logits64"]), torch.from_numpy(z["logits32"]), "g11 logits, predictor")


def test_golden_attends_across_the_batch_through_the_predictor(golden_dir):
    """test_transformer_gpu.test_golden_attends_across_the_batch with the predictor in the model's place: batch_first = 0 is
    S = B, N = L, so adding 1 to sample 0 moves the logits of samples 1-4 by the stored amounts"""
    z, predict = _golden_predictor(golden_dir)
    x = torch.from_numpy(z["x"]).to(DEV)
    xp = x.clone()
    xp[0] += 1.0
    moved = (predict(xp) - predict(x)).cpu().double()
    l64, l64p = torch.from_numpy(z["logits64"]), torch.from_numpy(z["logits64_perturbed"])
    want = l64p - l64
    bar = FC.CHAIN_MARGIN * max(FC.chain_figure(torch.from_numpy(z["logits32"]), l64), FC.U)
    tol = bar * (l64.abs() + l64.pow(2).mean().sqrt() + l64p.abs() + l64p.pow(2).mean().sqrt())
    print("moved", moved[1:].abs().max().item(), "stored", want[1:].abs().max().item(), "tolerance", tol.max().item())
    assert float(want[1:].abs().max()) > 100 * float(tol.max()), "the golden's samples do not interact"
    assert bool(((moved - want).abs() <= tol).all()), \
        "batch_first slip: through the predictor the logits of samples 1-4 do not follow sample 0 as the reference's do"


def test_with_lengths_a_record_hears_neither_its_batch_nor_its_padding():
    _, ours = _pair(64, 4, 128, True, seq_len=48, tag="tfl.")
    predict = Predictor(ours)
    lens = [48, 20, 9, 33]
    x = fill.hash_tensor((4, 1, 48), 842, 1.0).to(DEV)
    base = predict(x, lens)
    assert bool(torch.isfinite(base).all())
    for i, n in enumerate(lens):
        alone = predict(x[i:i + 1].contiguous(), [n])
        assert torch.equal(alone[0], base[i]), "record %d alone differs from record %d in the batch" % (i, i)
    xn = x.clone()
    for i, n in enumerate(lens):
        xn[i, :, n:] = float("nan")
    assert torch.equal(predict(xn, lens), base), "NaN in the padding of x reaches the logits"
    assert torch.equal(predict(x, torch.tensor(lens, device=DEV)), base)            # device lengths: no sync, the same bits
    assert not torch.equal(predict(x)[1], base[1])                                   # lengths matter
    with pytest.raises(ValueError, match="time_attention"):
        Predictor(_pair(64, 4, 128, False, seq_len=48)[1])(x, lens)


def test_refresh_is_what_moves_the_answer():
    ref, ours = _pair(64, 4, 128, True, tag="tfr.")
    predict = Predictor(ours)
    x = fill.hash_tensor((B, 1, LEN), 843, 1.0)
    xd, labels = x.to(DEV), torch.tensor([0, 1, 1, 0, 1, 0], device=DEV)
    before = predict(xd, LENGTHS)
    blob = predict.encoder.blob
    opt = FusedAdam(ours.parameters(), lr=1e-2)
    ours.train()
    for m in ours.modules():               # dropout off: the step only has to move the weights
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(m.dropout, float):
            m.dropout = 0.0
    FocalLoss()(ours(xd, LENGTHS), labels).backward()
    opt.step()
    ours.eval()
    torch.cuda.synchronize()
    assert torch.equal(predict(xd, LENGTHS), before), "the snapshot follows the live weights"
    with torch.no_grad():
        now = ours(xd, LENGTHS)
    assert float((now - before).abs().max()) > 1e-4, "the optimizer step did not move the model"
    assert predict.refresh() is predict
    assert predict.encoder.blob is not blob and predict.encoder.blob.data_ptr() != blob.data_ptr(), "refresh() must make a NEW blob"
    after = predict(xd, LENGTHS)
    ref.load_state_dict({k: v.detach().cpu() for k, v in ours.state_dict().items()}, strict=True)
    _chain("predictor after refresh()", after, ref, x, LENGTHS)
    _chain("model.eval() after the step", now, ref, x, LENGTHS)


def test_the_predictor_leaves_the_model_alone():
    _, ours = _pair(64, 4, 128, True, tag="tfs.")
    x = fill.hash_tensor((B, 1, LEN), 844, 1.0).to(DEV)
    ours.train()
    FocalLoss()(ours(x, LENGTHS), torch.tensor([0, 1, 1, 0, 1, 0], device=DEV)).backward()
    grads = {k: p.grad.clone() for k, p in ours.named_parameters()}
    state = {k: v.clone() for k, v in ours.state_dict().items()}
    assert all(g is not None for g in grads.values())
    predict = Predictor(ours)
    out = predict(x, LENGTHS)
    predict.refresh()
    predict(x)
    assert ours.training and all(m.training for m in ours.modules())
    assert not out.requires_grad
    for k, p in ours.named_parameters():
        assert torch.equal(p.grad, grads[k]), k + ".grad changed"
    for k, v in ours.state_dict().items():
        assert torch.equal(v, state[k]), k + " changed"


def test_four_launches_per_layer_and_the_predictor_is_that_sequence():
    """the forward rebuilt call by call from the per-op entry points on the model's own parameters gives the predictor's bits
    with four calls per layer (counted through the per-op path, not profiled)"""
    for time_attention, lengths in ((False, None), (True, None), (True, LENGTHS)):
        _, ours = _pair(64, 4, 128, time_attention, layers=3, tag="tfc.")
        sd = {k: v.detach() for k, v in ours.named_parameters()}
        names = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                 "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                 "norm2.bias")
        p = dict(conv_w=sd["conv.weight"], conv_b=sd["conv.bias"], pos=sd["pos_embedding"][0].contiguous(), cw1=sd["classifier.1.weight"],
                 cb1=sd["classifier.1.bias"], cw2=sd["classifier.4.weight"], cb2=sd["classifier.4.bias"],
                 layers=[{k: sd["transformer_encoder.layers.%d.%s" % (i, n)] for k, n in zip(A.LAYER_KEYS, names)} for i in range(3)])
        x = fill.hash_tensor((B, 1, LEN), 845, 1.0).to(DEV)
        ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
        want, calls = A.per_op_forward(p, x, ln, 4, time_attention, ours.transformer_encoder.layers[0].norm1.eps)
        assert calls.per_layer == [4, 4, 4] and calls.total == 1 + 4 * 3 + 3
        got = Predictor(ours)(x, lengths)
        assert torch.equal(got, want)


class _Synth(Config):
    synthetic, synthetic_train_size, synthetic_val_size, synthetic_test_size, device = True, 24, 8, 8, "cuda"


@pytest.mark.parametrize("time_attention", [True, False], ids=["time-lengths", "across"])
def test_main_validates_and_tests_through_the_predictor(time_attention, tmp_path, monkeypatch):
    import ecgmm.inference as INF
    import ecgmm.train_physionet as TP
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (_Synth,), {"checkpoint_dir": str(tmp_path / "ck")})
    real_records = TP.load_records

    def short_records(*a, **k):      # the synthetic records (2000 .. 18000 samples) cut to 150 .. 400: lengths that differ
        signals, labels = real_records(*a, **k)
        return [s[:150 + (37 * i) % 251] for i, s in enumerate(signals)], labels

    monkeypatch.setattr(TP, "load_records", short_records)
    seen = []
    real_call = INF._TransformerPlan.__call__
    monkeypatch.setattr(INF._TransformerPlan, "__call__",
                        lambda self, x, lengths=None: seen.append(lengths is not None) or real_call(self, x, lengths))
    kw = dict(time_attention=True, use_lengths=True) if time_attention else {}
    history, results, ckpt = TP.main(cfg, num_epochs=1, quiet=True, model="transformer", max_len=400, use_predictor=True, **kw)
    assert seen and all(s == time_attention for s in seen), "the validation / test passes did not go through the plan"
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["val_loss"])
    for tag in ("best", "last"):
        assert all(np.isfinite(v) for k, v in results[tag].items() if k != "auc"), results[tag]
    assert os.path.exists(os.path.join(ckpt, "last.pth"))


def test_predict_proba_takes_the_signal_loaders_batches():
    """``(signals [B, L], labels)`` and ``((signals, lengths), labels)``, the batches of train_physionet.DeviceSignalLoader"""
    _, ours = _pair(64, 4, 128, True, tag="tfp.")
    predict = Predictor(ours)
    x = fill.hash_tensor((B, LEN), 846, 1.0).to(DEV)
    labels = torch.tensor([0, 1, 1, 0, 1, 0])
    lens = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    prob, lab, idx = predict.predict_proba([(x[:4], labels[:4]), (x[4:], labels[4:])])
    assert torch.equal(prob, torch.softmax(predict(x.unsqueeze(1)).float().cpu(), dim=1))
    assert torch.equal(lab, labels) and idx.tolist() == list(range(B))
    prob_l, _, _ = predict.predict_proba([((x[:4], lens[:4]), labels[:4]), ((x[4:], lens[4:]), labels[4:])])
    assert torch.equal(prob_l, torch.softmax(predict(x.unsqueeze(1), lens).float().cpu(), dim=1))
    assert not torch.equal(prob_l, prob)
