"""TabNet's fused eval forward at the Python level on the GPU: forward_masks / visualize_masks of ecgmm.tabnet against the
float64 reference (tests/tabnet_infer_ref.py, bounds of tests/tabnet_infer_bounds.py), Predictor(ClinicalTabNetEncoder) against
float64 and the module's own eval forward, and the multimodal TabNet Predictor with clinical_plan on and off: carried through
the head, stale until refresh(), side effects, the silent fall-backs.  The yardstick is float64 or torch, never the code under
test."""
import numpy as np
import pytest
import torch

from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.inference import Predictor, _TabNetPlan
from ecgmm.multimodal import ECGMultimodalModel as TabVariant
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel as MlpVariant
from ecgmm.optim import FusedAdam
from ecgmm.tabnet import ClinicalTabNetEncoder, TabNetNoEmbeddings
from oracle import fill, ref_models as O
from oracle import tabnet_ref as T

from . import f64check as FC
from . import tabnet_infer_bounds as TB
from . import tabnet_infer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C0 = R.cfg()       # ClinicalTabNetEncoder(2, 32): D = 2, n_d = n_a = 32, 3 steps, gamma 1.5, 2 shared + 2 independent layers
B = 33


def _encoder(tag="clin."):
    """(oracle TabNetNoEmbeddings in eval mode, our ClinicalTabNetEncoder on the device in eval mode, x)"""
    ref = fill.hash_fill_module(T.ClinicalTabNetEncoder(2, 32), tag).eval()
    ours = ClinicalTabNetEncoder(2, 32)
    ours.load_state_dict(ref.state_dict(), strict=True)
    return ref.tabnet, ours.to(DEV).eval(), R.inputs(B, 2, 3)


def _judge(ref_net, x, got, what):
    with torch.no_grad():
        r = R.reference(C0, ref_net, x, forced=got["masks"].cpu())
        rr = TB.ratios(got, r, TB.Forward(C0, r))
    print(what, "error / bound:", {n: "%.3g" % v for n, v in rr.items()})
    assert rr and max(rr.values()) <= 1.0, (what, rr)
    return r


def _state(m):
    return ({k: v.clone() for k, v in m.state_dict().items()}, {n: None if p.grad is None else p.grad.clone() for n, p in
                                                                 m.named_parameters()}, [k.training for k in m.modules()])


def _same_state(m, before):
    sd, grads, modes = before
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for n, p in m.named_parameters():
        assert (p.grad is None) == (grads[n] is None) and (p.grad is None or torch.equal(p.grad, grads[n])), n
    assert [k.training for k in m.modules()] == modes


def test_forward_masks_against_the_float64_reference_on_all_three_modules():
    ref_net, ours, x = _encoder()
    before = _state(ours)
    mexp, masks = ours.forward_masks(x.to(DEV))
    assert sorted(masks) == [0, 1, 2] and mexp.shape == (B, 2) and all(m.shape == (B, 2) for m in masks.values())
    got = dict(m_explain=mexp, masks=torch.stack([masks[s] for s in range(3)]))
    _judge(ref_net, x, got, "forward_masks")
    for mod in (ours.tabnet, ours.tabnet.encoder):       # the same launch on the same fold: the same bits
        m2, k2 = mod.forward_masks(x.to(DEV))
        assert torch.equal(m2, mexp) and all(torch.equal(k2[s], masks[s]) for s in range(3))
    _same_state(ours, before)


def test_forward_masks_folds_at_every_call_and_refuses_training_mode():
    ref_net, ours, x = _encoder()
    xd = x.to(DEV)
    first, _ = ours.forward_masks(xd)
    with torch.no_grad():                                  # move a running statistic of one use of a shared layer
        for net in (ref_net, ours.tabnet):
            net.encoder.feat_transformers[0].shared.glu_layers[0].bn.bn.running_mean += 0.25
            net.encoder.initial_bn.running_var *= 1.5
    mexp, masks = ours.forward_masks(xd)
    assert not torch.equal(mexp, first), "forward_masks answered from a stale fold"
    _judge(ref_net, x, dict(m_explain=mexp, masks=torch.stack([masks[s] for s in range(3)])), "forward_masks after a change")
    ours.train()
    with pytest.raises(RuntimeError, match="training mode"):
        ours.forward_masks(xd)
    assert ours.training and all(k.training for k in ours.modules())
    wide = TabNetNoEmbeddings(2, 32, n_d=8, n_a=8).to(DEV).eval()
    with pytest.raises(ValueError, match="n_d=8.*multiples of 16"):
        wide.forward_masks(xd)


def test_visualize_masks_file_contents_and_untouched_mode(tmp_path):
    ref_net, ours, x = _encoder()
    before = _state(ours)
    res = ours.visualize_masks(x.numpy(), None, str(tmp_path), "clin")
    z = np.load(tmp_path / "clin_masks.npz")
    assert sorted(z.files) == ["M_agg_mean", "M_explain", "feature_names", "masks", "step_mean"] == sorted(res)
    assert z["masks"].shape == (3, B, 2) and z["step_mean"].shape == (3, 2) and z["M_explain"].shape == (B, 2)
    assert z["M_agg_mean"].shape == (2,) and list(z["feature_names"]) == ["var_0", "var_1"]
    for k in z.files:
        assert np.array_equal(z[k], res[k]), k
    np.testing.assert_allclose(z["step_mean"], z["masks"].astype(np.float64).mean(1), rtol=1e-6)
    np.testing.assert_allclose(z["M_agg_mean"], z["masks"].astype(np.float64).mean(0).mean(0), rtol=1e-6)   # the reference's heat map
    np.testing.assert_allclose(z["masks"].sum(-1), 1.0, atol=1e-5)
    _judge(ref_net, x, dict(m_explain=torch.from_numpy(z["M_explain"]), masks=torch.from_numpy(z["masks"])), "visualize_masks")
    again = ours.visualize_masks(x.to(DEV), ["age", "sex"], str(tmp_path / "sub"), "t")   # a tensor, names, a new directory
    assert np.array_equal(again["masks"], res["masks"]) and list(np.load(tmp_path / "sub" / "t_masks.npz")["feature_names"]) == ["age", "sex"]
    _same_state(ours, before)
    assert not list(tmp_path.glob("*.png"))
    with pytest.raises(ValueError, match="feature names"):
        ours.visualize_masks(x, ["one"], str(tmp_path), "bad")
    ours.train()
    with pytest.raises(RuntimeError, match="training mode"):
        ours.visualize_masks(x, None, str(tmp_path), "bad")
    assert ours.training and not (tmp_path / "bad_masks.npz").exists()


def test_predictor_of_the_clinical_encoder_against_float64_and_the_modules_eval_forward():
    ref_net, ours, x = _encoder()
    xd = x.to(DEV)
    before = _state(ours)
    predict = Predictor(ours)
    z = predict(xd)
    assert z.shape == (B, 32) and torch.equal(predict.logits(xd), z)
    mexp, masks = predict.encoder.masks(xd)
    r = _judge(ref_net, x, dict(out=z, m_explain=mexp, masks=torch.stack([masks[s] for s in range(3)])), "Predictor(ClinicalTabNetEncoder)")
    with torch.no_grad():
        own, m_loss = ours(xd)                              # the module's own eval forward: ~110 launches
        r0 = R.reference(C0, ref_net, x)
        own32 = R.candidate(C0, ref_net, x)
    FC.check_chain(own.cpu(), r0.out, own32.out, "module eval forward")
    FC.check_chain(z.cpu(), r0.out, own32.out, "the plan, same yardstick")
    assert abs(float(m_loss) - float(r0.row_entropy.mean()) / 3) < 1e-5
    assert float((z - own).abs().max()) < 1e-3 * max(1.0, float(r.out.abs().max()))
    _same_state(ours, before)
    with pytest.raises(ValueError, match=r"\[B, 2\]"):
        predict(torch.zeros(4, 3, device=DEV))
    with pytest.raises(TypeError, match="one input"):
        predict(xd, xd)


def _multimodal(variant="tab"):
    cfg = type("Cfg", (Config,), {"compute_dtype": "fp32"})
    if variant == "tab":
        ref, net, clin_in = T.multimodal_tabnet_model(2), TabVariant(cfg), 2
    else:
        ref, net, clin_in = O.ECGMultimodalModel(2, 24), MlpVariant(cfg), 24
    net.load_state_dict(fill.hash_fill_module(ref, "mm.").state_dict(), strict=True)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    img, sig, clin, lab = fill.synthetic_batch(4, img_hw=(64, 64), sig_len=1000, clin_dim=clin_in, salt=9)
    return ref, net.to(DEV), [t.to(DEV) for t in (img, sig, clin)], lab.to(DEV)


def test_multimodal_predictor_with_the_clinical_plan_against_without():
    ref, net, xs, _ = _multimodal()
    net.eval()
    before = _state(net)
    on, off = Predictor(net, clinical_plan=True), Predictor(net, clinical_plan=False)
    assert isinstance(on.clinical, _TabNetPlan) and off.clinical is None
    a, b = on(*xs), off(*xs)
    torch.cuda.synchronize()
    # the clinical features themselves: within the derived bound of float64
    z = on.clinical(xs[2])
    mexp, masks = on.clinical.masks(xs[2])
    _judge(ref.clinical_encoder.tabnet, xs[2].cpu(), dict(out=z, m_explain=mexp, masks=torch.stack([masks[s] for s in range(3)])),
           "clinical branch of the multimodal predictor")
    for n, (o, p) in enumerate(zip(a, b)):                # carried through the head: the bar of the g9 golden test
        assert float((o - p).abs().max()) < 1e-3, n
    assert torch.equal(on(*xs)[3], a[3])
    _same_state(net, before)
    net.train()
    with pytest.raises(RuntimeError, match="the clinical branch runs the model's own forward, which is in training mode"):
        on(*xs)


def test_clinical_plan_is_stale_until_refresh_after_an_optimizer_step():
    _, net, xs, lab = _multimodal()
    net.eval()
    predict = Predictor(net, clinical_plan=True)
    old_z, old = predict.clinical(xs[2]).clone(), predict(*xs)[3].clone()
    net.train()
    opt = FusedAdam(net.parameters(), lr=1e-2)
    out = net(*xs)
    (HF.cross_entropy(out[3], lab) + 0.1 * out[4]).backward()
    opt.step()                                              # weights AND running statistics moved
    torch.cuda.synchronize()
    net.eval()
    assert torch.equal(predict.clinical(xs[2]), old_z), "a prepared clinical plan must keep answering from its snapshot"
    assert torch.equal(predict(*xs)[3], old)
    predict.refresh()
    new_z = predict.clinical(xs[2])
    with torch.no_grad():
        want_z = net.clinical_encoder(xs[2])[0]
        want = net(*xs)[3]
    assert float((new_z - want_z).abs().max()) < 1e-3 * max(1.0, float(want_z.abs().max()))
    assert float((new_z - old_z).abs().max()) > 1e-3
    assert float((predict(*xs)[3] - want).abs().max()) < 1e-3 * max(1.0, float(want.abs().max()))


def test_the_mlp_variant_and_a_narrow_tabnet_fall_back_silently():
    _, mlp, xs, _ = _multimodal("mlp")
    mlp.eval()
    p = Predictor(mlp, clinical_plan=True)
    assert p.clinical is None
    assert torch.equal(p(*xs)[3], Predictor(mlp, clinical_plan=False)(*xs)[3])
    _, net, xs, _ = _multimodal()
    net.clinical_encoder.tabnet = TabNetNoEmbeddings(input_dim=2, output_dim=32, n_d=8, n_a=8, n_steps=3, gamma=1.5).to(DEV)
    net.eval()
    p = Predictor(net, clinical_plan=True)
    assert p.clinical is None                               # n_d = 8 is outside the fused path: the module's own forward
    with torch.no_grad():
        want = net(*xs)[3]
    assert float((p(*xs)[3] - want).abs().max()) < 1e-3


def test_explain_main_writes_the_clinical_masks_of_its_samples(tmp_path):
    from ecgmm import explain
    cfg = type("Tiny", (Config,), {"compute_dtype": "fp32", "synthetic": True, "synthetic_train_size": 8, "synthetic_val_size": 4,
                                   "synthetic_test_size": 4, "batch_size": 4, "device": "cuda", "clinical_input_dim": 2})
    files = explain.main(cfg, out_dir=str(tmp_path), samples=1, quiet=True, model_cls=TabVariant)
    assert [f.rsplit("/", 1)[1] for f in files] == ["gradcam_0.png", "gradcam_0_overlay.png", "clinical_masks.npz"]
    z = np.load(files[-1])
    assert z["masks"].shape == (3, 1, 2) and z["M_explain"].shape == (1, 2)
    np.testing.assert_allclose(z["masks"].sum(-1), 1.0, atol=1e-5)
