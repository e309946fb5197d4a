"""The contract of ``ecgmm.inference.Predictor``, stated once for every kind of plan: a call is deterministic, the answer is
that of the snapshot until ``refresh()``, a refresh makes NEW blobs and gives the bits of a newly constructed predictor, a call
leaves the model alone, and a wrong call signature is a ``TypeError``.

Shapes: the smallest input each plan's own GPU test uses, at batch 3 (an odd batch for the convolutions, a partial 16-row
tile for the row kernels: 3 rows for TabNet, 3 x 40 = 120 for the transformer); the CRNN's floors are F = 32, T = 8.
Everything here is bit equality or inequality, so there is no tolerance to choose."""
import pytest
import torch

from ecgmm.config import Config
from ecgmm.crnn import CRNN
from ecgmm.image_encoder import ResNet18
from ecgmm.inference import Predictor
from ecgmm.multimodal import ECGMultimodalModel as TabVariant
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel as MlpVariant, ResNet1D_SE
from ecgmm.tabnet import ClinicalTabNetEncoder
from ecgmm.train_image_only import ImageOnlyClassifier
from ecgmm.train_physionet import ECGTransformer1D
from oracle import fill

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3


def _transformer(time_attention):
    return ECGTransformer1D(seq_len=40, num_classes=2, d_model=64, nhead=4, num_layers=2, dim_feedforward=128,
                            time_attention=time_attention)


def _multimodal(cls, clin_dim):
    cfg = type("Cfg", (Config,), {"compute_dtype": "fp32", "clinical_input_dim": clin_dim})
    img, sig, clin, _ = fill.synthetic_batch(N, img_hw=(64, 64), sig_len=1000, clin_dim=clin_dim, salt=9)
    return cls(cfg), (img, sig, clin)


# kind -> (model, inputs, state_dict keys changed in place: a parameter and, where the model has one, a running statistic
# -- for the multimodal model one of each part the snapshot covers)
KINDS = {
    "resnet18": lambda: (ResNet18(num_classes=16, compute_dtype="fp32"), (fill.hash_tensor((N, 3, 32, 32), 701),),
                         ("conv1.weight", "bn1.running_mean")),
    "resnet1d_se": lambda: (ResNet1D_SE(1, 16, compute_dtype="fp32"), (fill.hash_tensor((N, 1, 64), 702, 1.5),),
                            ("initial.0.weight", "initial.1.running_var")),
    "image_only": lambda: (ImageOnlyClassifier(compute_dtype="fp32"), (fill.hash_tensor((N, 3, 32, 32), 703),),
                           ("image_encoder.conv1.weight", "image_encoder.bn1.running_var")),
    "crnn": lambda: (CRNN(compute_dtype="fp32"), (fill.hash_tensor((N, 1, 32, 8), 704),),
                     ("conv1.block.0.weight", "conv1.block.1.running_mean")),
    "transformer_time": lambda: (_transformer(True), (fill.hash_tensor((N, 1, 40), 705),), ("pos_embedding",)),
    "transformer_across": lambda: (_transformer(False), (fill.hash_tensor((N, 1, 40), 706),), ("conv.weight",)),
    "tabnet": lambda: (ClinicalTabNetEncoder(2, 32), (fill.hash_tensor((N, 2), 707),),
                       ("tabnet.encoder.initial_bn.weight", "tabnet.encoder.initial_bn.running_mean")),
    "multimodal_mlp": lambda: _multimodal(MlpVariant, 24) + (
        ("image_encoder.conv1.weight", "signal_encoder.initial.1.running_var", "fusion_classifier.3.bias"),),
    "multimodal_tabnet": lambda: _multimodal(TabVariant, 2) + (
        ("image_encoder.bn1.running_mean", "signal_encoder.initial.0.weight", "fusion_classifier.3.bias",
         "clinical_encoder.tabnet.encoder.initial_bn.running_var"),),
}


def _tensors(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))


def _clone(out):
    return tuple(t.clone() for t in _tensors(out))


def _blobs(predict):
    plans = [p for p in (predict.image, predict.signal, predict.clinical) if p is not None] if predict.multimodal \
        else [predict.encoder]
    return [p.blob for p in plans]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_predictor_contract(kind):
    torch.manual_seed(11)          # the models' own initialisation: every check below is bit (in)equality within this run
    model, xs, touched = KINDS[kind]()
    model = model.to(DEV).eval()
    xs = tuple(t.to(DEV) for t in xs)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    modes = [m.training for m in model.modules()]

    predict = Predictor(model)
    first, second = _clone(predict(*xs)), predict(*xs)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) and not t.requires_grad for t in first)
    assert _same(first, second), "two calls differ"

    # a call and the construction leave the model alone
    assert [m.training for m in model.modules()] == modes
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k + " changed"
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, torch.full_like(p, 0.25)), n + ".grad changed"

    # the snapshot answers until refresh()
    sd = model.state_dict()
    assert any(k.rsplit(".", 1)[-1].startswith("running_") for k in touched) == any("running_" in k for k in sd)
    with torch.no_grad():
        for k in touched:
            sd[k].mul_(1.5).add_(0.25)
    torch.cuda.synchronize()
    assert _same(predict(*xs), first), "a prepared predictor must keep answering from its snapshot"

    old = _blobs(predict)
    assert old and all(b is not None for b in old)
    assert predict.refresh() is predict
    new = _blobs(predict)
    assert len(new) == len(old)
    for a, b in zip(old, new):
        assert b is not a and b.data_ptr() != a.data_ptr(), "refresh() must make a NEW blob"
    after = _clone(predict(*xs))
    assert _same(after, Predictor(model)(*xs)), "a refreshed predictor and a new one differ"
    assert not _same(after, first), "refresh() did not move the answer"
    del old

    # the call signature
    with pytest.raises(TypeError):
        predict()
    with pytest.raises(TypeError):
        predict(*xs, xs[0], xs[0])
    if kind not in ("crnn", "transformer_time", "transformer_across"):
        with pytest.raises(TypeError, match="takes no lengths"):
            predict(*xs, lengths=[1] * N)
