"""ecgmm.shap_explainers and the explainer argument of ecgmm.shap_fusion_modal_balance.main on the device, against
tests/shap_ref.py within the bounds of tests/shap_bounds.py.  Expected gradients: a gate comes from float64 where float64
decides it and from the device's pre-activation where it does not (|z64| within the z bound; the share of such gates is
capped, and tests/test_shap_cpu.py shows the reference alone stays inside the cap).  Every element is checked."""
import numpy as np
import pytest
import torch

from ecgmm import shap_explainers as SE
from ecgmm import shap_fusion_modal_balance as X
from ecgmm.config import Config
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel

from . import shap_bounds as Bd
from . import shap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(**kw):
    base = {"device": DEV, "compute_dtype": "fp32", "clinical_input_dim": 16, "batch_size": 8,
            "synthetic_train_size": 32, "synthetic_val_size": 8, "synthetic_test_size": 8}
    base.update(kw)
    return type("C", (Config,), base)


def plain_head(w1, b1, w2, b2):
    H, D = w1.shape
    net = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Dropout(0.3), torch.nn.Linear(H, w2.shape[0]))
    with torch.no_grad():
        for p, v in zip(net.parameters(), (w1, b1, w2, b2)):
            p.copy_(torch.from_numpy(v))
    return net.to(DEV).eval()


@pytest.fixture(scope="module", params=R.E2E_SHAPES, ids=lambda s: "x".join(map(str, s[:5])))
def setup(request):
    B, N, D, H, C, seed = request.param
    x, bg, w1, b1, w2, b2 = R.make_inputs(B, N, D, H, C, seed)
    return (x, bg, w1, b1, w2, b2), plain_head(w1, b1, w2, b2), torch.from_numpy(x).to(DEV), torch.from_numpy(bg).to(DEV)


@pytest.mark.parametrize("nsamples", R.E2E_NSAMPLES)
def test_gradient_explainer_matches_float64_on_the_same_draws(setup, nsamples):
    (x, bg, w1, b1, w2, _), net, xd, bgd = setup
    B, N, H = len(x), len(bg), w1.shape[0]
    ex = SE.GradientExplainer(net, bgd)
    phi, var, z = ex.shap_values(xd, nsamples=nsamples, rseed=R.E2E_RSEED, return_variances=True, return_z=True)
    assert phi.dtype == np.float32 and phi.shape == var.shape == (B, x.shape[1], w2.shape[0])
    ridx, t = SE.draws_like_shap(R.E2E_RSEED, B, nsamples, N)
    p, pabs = R.points(x, bg, ridx, t)
    z64, zb = R.preact(p, w1, b1), Bd.z_bound(pabs, w1, b1, interpolated=True)
    rz = Bd.ratio(np.abs(z - z64), zb)
    undecided = np.abs(z64) <= zb
    share = float(undecided.mean())
    assert share <= R.UNDECIDED_CAP
    gates = np.where(undecided, R.gate_gradient(z), R.gate_gradient(z64))
    assert np.array_equal(gates, R.gate_gradient(z)) or rz > 1.0     # a decided gate the device got wrong shows in z
    prod, absprod, _ = R.products(x, R.f64(bg)[ridx], gates, w1, w2)
    phi64, var64 = R.mean_and_variance(prod)
    rp = Bd.ratio(np.abs(phi - phi64), Bd.phi_bound(absprod, phi64, H, ratio_gates=False))
    rv = Bd.ratio(np.abs(var - var64), Bd.var_bound(prod, absprod, var64, H))
    print("GradientExplainer B=%d N=%d nsamples=%d: undecided %.3g, worst ratios z %.3g phi %.3g var %.3g"
          % (B, N, nsamples, share, rz, rp, rv))
    assert rz <= 1.0 and rp <= 1.0 and rv <= 1.0
    # the plain call returns the same values alone, and is a function of rseed
    again = ex.shap_values(xd, nsamples=nsamples, rseed=R.E2E_RSEED)
    assert isinstance(again, np.ndarray) and np.array_equal(again, phi)


def test_deep_explainer_matches_float64_and_is_additive(setup):
    (x, bg, w1, b1, w2, b2), net, xd, bgd = setup
    B, N, D, H = len(x), len(bg), x.shape[1], w1.shape[0]
    ex = SE.DeepExplainer(net, bgd)
    fb = R.forward(bg, w1, b1, w2, b2).mean(0)
    assert ex.expected_value.shape == (w2.shape[0],) and np.abs(ex.expected_value - fb).max() < 1e-4
    phi, zx, zb = ex.shap_values(xd, return_z=True)
    dzx, dzb = Bd.z_bound(np.abs(R.f64(x)), w1, b1, False), Bd.z_bound(np.abs(R.f64(bg)), w1, b1, False)
    rz = max(Bd.ratio(np.abs(zx - R.preact(x, w1, b1)), dzx), Bd.ratio(np.abs(zb - R.preact(bg, w1, b1)), dzb))
    gap = np.abs(R.f64(zx)[:, None, :] - R.f64(zb)[None, :, :])
    assert not (np.abs(gap - R.THRESHOLD) <= 2 * Bd.U * R.THRESHOLD).any()
    branch = R.rescale_branch(zx, zb)
    rows = np.broadcast_to(R.f64(bg)[None], (B, N, D))
    prod, absprod, _ = R.products(x, rows, R.gate_rescale(zx, zb), w1, w2)
    phi64 = R.mean_and_variance(prod)[0]
    phi_b = Bd.phi_bound(absprod, phi64, H, ratio_gates=True)
    rp = Bd.ratio(np.abs(phi - phi64), phi_b)
    delta = R.forward(x, w1, b1, w2, b2) - fb
    add_b = Bd.additivity_bound(phi_b, w2, dzx, dzb, branch)
    add_err = np.abs(R.f64(phi).sum(1) - delta)
    ra = Bd.ratio(add_err, add_b)
    print("DeepExplainer B=%d N=%d: worst ratios z %.3g phi %.3g additivity %.3g (error at most %.3g, bound at most %.3g)"
          % (B, N, rz, rp, ra, add_err.max(), add_b.max()))
    assert rz <= 1.0 and rp <= 1.0 and ra <= 1.0
    assert add_err.max() < SE.DeepExplainer.ADDITIVITY_TOLERANCE      # and so inside shap's own tolerance
    assert np.array_equal(ex.shap_values(xd), phi)
    ex.expected_value = ex.expected_value + 0.1
    with pytest.raises(AssertionError, match="do not sum up"):
        ex.shap_values(xd)
    assert np.array_equal(ex.shap_values(xd, check_additivity=False), phi)


def test_wrapped_fusion_classifier_and_plain_sequential_give_the_same_numbers():
    cfg = _cfg()
    torch.manual_seed(0)
    model = ECGMultimodalModel(cfg).to(DEV).eval()
    fc = model.fusion_classifier
    wrapped = X.FusionClassifierWrapper(fc)
    plain = plain_head(*(p.detach().cpu().numpy() for p in (fc[0].weight, fc[0].bias, fc[3].weight, fc[3].bias)))
    x, bg = (torch.from_numpy(a).to(DEV) for a in R.make_inputs(3, 5, 768, 128, 2, seed=21)[:2])
    before = [(p.requires_grad, p.grad) for p in model.parameters()]
    g1 = SE.GradientExplainer(wrapped, bg).shap_values(x, nsamples=16, rseed=1)
    g2 = SE.GradientExplainer(plain, bg).shap_values(x, nsamples=16, rseed=1)
    d1, d2 = SE.DeepExplainer(wrapped, bg), SE.DeepExplainer(plain, bg)
    assert g1.shape == (3, 768, 2) and np.array_equal(g1, g2) and np.isfinite(g1).all() and np.abs(g1).max() > 0
    assert np.array_equal(d1.shap_values(x), d2.shap_values(x))
    assert np.allclose(d1.expected_value, d2.expected_value, atol=1e-5)
    after = [(p.requires_grad, p.grad) for p in model.parameters()]
    assert all(a[0] is b[0] and a[1] is b[1] for a, b in zip(before, after))
    assert all(p.requires_grad and p.grad is None for p in model.parameters())
    with pytest.raises(NotImplementedError, match="ranked_outputs"):
        d1.shap_values(x, ranked_outputs=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d1.shap_values(x.cpu())
    with pytest.raises(RuntimeError, match="training mode"):
        model.train()
        d1.shap_values(x)


@pytest.mark.parametrize("explainer", ["gradient", "deep"])
def test_entry_point_with_the_native_explainers_writes_the_csv(tmp_path, explainer, monkeypatch):
    import pandas as pd
    calls = []
    real = X.expected_gradients
    monkeypatch.setattr(X, "expected_gradients", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    cfg = _cfg(compute_dtype="bf16", synthetic_train_size=24)
    out = tmp_path / explainer / "out.csv"
    df = X.main(cfg, max_samples_per_class=4, nsamples=8, out_csv=str(out), quiet=True, explainer=explainer)
    assert not calls
    assert list(df.columns) == ["Image_%", "Signal_%", "Clinical_%", "Label", "Class", "Sample_ID"] and len(df) == 16
    assert out.exists() and len(pd.read_csv(out)) == 16
    assert np.allclose(df["Image_%"] + df["Signal_%"] + df["Clinical_%"], 100.0, atol=1e-6)
    assert list(df["Sample_ID"]) == [i // 2 + 1 for i in range(16)] and list(df["Class"]) == [0, 1] * 8


def test_entry_point_default_still_goes_through_expected_gradients(monkeypatch):
    calls = []
    real = X.expected_gradients
    monkeypatch.setattr(X, "expected_gradients", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    df = X.main(_cfg(compute_dtype="bf16", synthetic_train_size=24), max_samples_per_class=4, nsamples=2, quiet=True)
    assert len(calls) == 1 and len(df) == 16      # one test batch of 8 samples, two classes
