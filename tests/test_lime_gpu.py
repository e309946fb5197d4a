"""ecgmm.lime_tabular and ecgmm.lime_fusion_modal_balance on the device: explanations against tests/lime_ref.py fed the
device's own perturbations and probabilities (only the fit differs, so the bounds are those of tests/lime_bounds.py), the
default predict_fn against torch on the CPU, feature selection, and the script's entry point on the synthetic data tree."""
import numpy as np
import pytest
import torch

from ecgmm import lime_fusion_modal_balance as LF
from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.lime_tabular import LimeTabularExplainer
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel
from oracle import fill, ref_models as O

from . import lime_bounds as Bd
from . import lime_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, N, B = 768, 160, 3


def _cfg(**kw):
    base = {"device": DEV, "compute_dtype": "fp32", "clinical_input_dim": 16, "batch_size": 8,
            "synthetic_train_size": 32, "synthetic_val_size": 8, "synthetic_test_size": 8}
    base.update(kw)
    return type("C", (Config,), base)


@pytest.fixture(scope="module")
def setup():
    ref = O.disable_dropout(fill.hash_fill_module(O.ECGMultimodalModel(2, 16), "mm.")).eval()
    model = ECGMultimodalModel(_cfg())
    model.load_state_dict(ref.state_dict())
    model = model.to(DEV).eval()
    predict_fn = LF.make_predict_fn(LF.FusionClassifierWrapper(model.fusion_classifier))
    bg = fill.hash_tensor((40, D), 81, 1.0).numpy()
    rows = fill.hash_tensor((B, D), 82, 1.0).to(DEV)
    return ref, predict_fn, bg, rows


def explainer(bg):
    return LimeTabularExplainer(bg, mode="classification", random_state=R.SEED)


@pytest.fixture(scope="module")
def batch(setup):
    """one explain_batch at num_features = D, with the device data behind it, shared by the tests below"""
    ref, predict_fn, bg, rows = setup
    ex = explainer(bg)
    exps, data = ex.explain_batch(rows, predict_fn, labels=(1,), num_features=D, num_samples=N, return_data=True)
    torch.cuda.synchronize()
    return ex, exps, data


def test_explain_batch_matches_the_float64_fit(batch):
    ex, exps, data = batch
    assert len(exps) == B and len(data) == 1
    d = data[0]
    Z, d2, probs = d["Z"].cpu().numpy(), d["d2"].cpu().numpy(), d["probs"].cpu().numpy().reshape(B, N, 2)
    assert (Z[:, 0] == 1).all() and (d2[:, 0] == 0).all()
    worst = {}
    for b, exp in enumerate(exps):
        w = R.kernel_weights(d2[b], ex.kernel_width).astype(np.float32)
        keep, ref = R.explain(Z[b], d2[b], probs[b, :, 1], ex.kernel_width, D, w=w)
        coef = np.zeros(D)
        feats = [f for f, _ in exp.local_exp[1]]
        assert sorted(feats) == list(range(D))
        mags = [abs(v) for _, v in exp.local_exp[1]]
        assert mags == sorted(mags, reverse=True)
        for f, v in exp.local_exp[1]:
            coef[f] = v
        got = Bd.ridge_ratios(ref, coef[None], [exp.intercept[1]], [exp.score[1]], [exp.local_pred[1]])
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
        names = exp.as_list(1)
        assert len(names) == D and isinstance(names[0][0], str) and names[0][1] == exp.local_exp[1][0][1]
    print("explain_batch worst ratios:", ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_default_predict_fn_matches_torch_cpu(setup, batch):
    ref, predict_fn, _, _ = setup
    inverse = batch[2][0]["inverse"].view(-1, D)[:512]
    got = predict_fn(inverse).cpu()
    with torch.no_grad():
        want = torch.softmax(ref.fusion_classifier(inverse.cpu()), dim=1)
    assert got.shape == want.shape and torch.allclose(got, want, atol=1e-3)
    assert torch.allclose(got.sum(1), torch.ones(got.shape[0]), atol=1e-6)


def test_explain_instance_equals_its_row_of_the_batch(setup, batch):
    _, predict_fn, bg, rows = setup
    for b in (0, B - 1):
        one = explainer(bg).explain_instance(rows[b], predict_fn, num_features=D, num_samples=N, sample_index=b)
        assert one.local_exp[1] == batch[1][b].local_exp[1]
        assert one.intercept[1] == batch[1][b].intercept[1] and one.score[1] == batch[1][b].score[1]


def test_num_features_keeps_the_largest_of_the_first_fit(setup, batch):
    _, predict_fn, bg, rows = setup
    ex, _, data = batch
    d = data[0]
    first = HF.lime_ridge(d["Z"], d["d2"], d["y"], ex.kernel_width, 0.01, want=())["coef"][:, 0].cpu().numpy()
    exps = explainer(bg).explain_batch(rows, predict_fn, num_features=10, num_samples=N)
    for b, exp in enumerate(exps):
        want = set(np.argsort(-np.abs(first[b]), kind="stable")[:10].tolist())
        assert len(exp.local_exp[1]) == 10 and {f for f, _ in exp.local_exp[1]} == want
        assert all(np.isfinite(v) for _, v in exp.local_exp[1])


def test_entry_point_writes_the_csv(tmp_path, capsys):
    import pandas as pd
    cfg = _cfg(compute_dtype="bf16", synthetic_train_size=24)
    runs = []
    for i in range(2):
        torch.manual_seed(0)
        HF.manual_seed(3)
        out = tmp_path / ("lime%d" % i) / "out.csv"
        df = LF.main(cfg, max_samples_per_class=4, num_samples=64, out_csv=str(out), quiet=i == 0)
        printed = capsys.readouterr().out
        if i == 0:
            assert printed == ""
        else:   # the last steps of the reference's flow: df.head() and the attention weights
            assert "Image_%" in printed and "Attention Weights (Softmax): Image=" in printed and "Clinical=" in printed
        assert out.exists() and len(pd.read_csv(out)) == len(df) == 8
        runs.append(df)
    df = runs[0]
    assert list(df.columns) == ["Sample_ID", "Image_%", "Signal_%", "Clinical_%", "Label"]
    assert list(df["Sample_ID"]) == list(range(1, 9))
    total = df["Image_%"] + df["Signal_%"] + df["Clinical_%"]
    assert np.allclose(total, 100.0, atol=1e-6)
    assert runs[0].equals(runs[1])
