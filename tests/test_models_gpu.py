"""End-to-end parity of the encoder plans and the full multimodal model against the CPU oracle
(oracle/ref_models.py) and the committed goldens.  fp32 compute: logits within 1e-3 (north_star);
bf16 compute: stated looser tolerances."""
import numpy as np
import pytest
import torch

from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.image_encoder import ResNet18
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel, ResNet1D_SE
from ecgmm.optim import FusedAdam
from oracle import fill, ref_models as O

from .util import DEV, dev, rel_err, switches

pytestmark = pytest.mark.gpu


def _disable_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _grads(model):
    return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


def _compare_grads(mine, ref, tol, skip=()):
    gm, bad = _grads(mine), []
    for k, p in ref.named_parameters():
        if p.grad is None or any(s in k for s in skip):
            continue
        e = rel_err(gm[k], p.grad)
        if not e < tol:
            bad.append((k, e))
    assert not bad, bad


# Conv1d biases feed straight into BatchNorm: their true gradient is exactly zero and both sides
# produce rounding noise, so they are excluded from relative comparisons (checked absolutely below).
SIG_BIAS_SKIP = ("initial.0.bias", "conv1.bias", "conv2.bias", "downsample.0.bias")


@pytest.mark.parametrize("cd,tol_out,tol_grad", [("fp32", 2e-4, 2e-3)])
def test_resnet1d_ptbxl_train_step_vs_reference_golden(golden_dir, cd, tol_out, tol_grad):
    """g2 was produced by the REFERENCE's ResNet1D_SE class with the reference's best_ptbxl.pth."""
    g2 = np.load(f"{golden_dir}/g2_ptbxl_train.npz")
    sd = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/best_ptbxl_tensors.npz").items()}
    net = ResNet1D_SE(1, 2, compute_dtype=cd)
    net.load_state_dict(sd, strict=True)
    net = _disable_dropout(net).to(DEV).train()
    x = dev(fill.hash_tensor((4, 1, 2476), 91, 1.5))
    y = dev(torch.tensor([0, 1, 1, 0]))
    logits = net(x)
    loss = HF.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    assert (logits.detach().cpu() - torch.from_numpy(g2["logits"])).abs().max() < tol_out
    assert abs(loss.item() - float(g2["loss"])) < tol_out
    bad = []
    for k, p in net.named_parameters():
        ref = torch.from_numpy(g2["grad." + k])
        if any(s in k for s in SIG_BIAS_SKIP):
            assert p.grad.abs().max().item() < (1e-3 if cd == "fp32" else 0.5), k
            continue
        e = rel_err(p.grad.cpu(), ref)
        if not e < tol_grad:
            bad.append((k, e))
    assert not bad, bad
    for k, v in net.state_dict().items():
        if "running" in k:
            assert torch.allclose(v.cpu(), torch.from_numpy(g2["buf." + k]), rtol=5e-3 if cd == "fp32" else 0.05,
                                  atol=1e-4 if cd == "fp32" else 5e-3), k


def test_resnet1d_eval_vs_reference_golden(golden_dir):
    g1 = np.load(f"{golden_dir}/g1_ptbxl_eval.npz")
    sd = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/best_ptbxl_tensors.npz").items()}
    net = ResNet1D_SE(1, 2, compute_dtype="fp32")
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    for Ln in (2476, 5000):
        x = dev(fill.hash_tensor((4, 1, Ln), 77 + Ln, 1.5))
        with torch.no_grad():
            out = net(x)
        assert (out.cpu() - torch.from_numpy(g1[f"logits_{Ln}"])).abs().max() < 1e-3


@pytest.mark.parametrize("cd,tol_out,tol_grad", [("fp32", 1e-3, 5e-3)])
@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (2, 3, 96, 160)])
def test_resnet18_train_vs_oracle(cd, tol_out, tol_grad, shape):
    ref = fill.hash_fill_module(O.ResNet18(num_classes=256), "r18.").train()
    net = ResNet18(num_classes=256, compute_dtype=cd)
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV).train()
    x = fill.hash_tensor(shape, 607)
    f_ref = ref(x)
    f_ref.square().mean().backward()
    f = net(dev(x))
    f.square().mean().backward()   # (torch elementwise on the 256-d features: host-side test glue)
    torch.cuda.synchronize()
    assert (f.detach().cpu() - f_ref.detach()).abs().max() < tol_out * max(1.0, f_ref.abs().max().item())
    _compare_grads(net, ref, tol_grad)
    sd_m, sd_r = net.state_dict(), ref.state_dict()
    for k in sd_r:
        if "running" in k:
            assert torch.allclose(sd_m[k].cpu(), sd_r[k], rtol=2e-3 if cd == "fp32" else 0.05,
                                  atol=1e-4 if cd == "fp32" else 5e-3), k
        if "num_batches" in k:
            assert int(sd_m[k]) == int(sd_r[k])


def test_resnet18_eval_golden_g6(golden_dir):
    g6 = np.load(f"{golden_dir}/g6_resnet18.npz")
    ref = fill.hash_fill_module(O.ResNet18(num_classes=256), "r18.")
    net = ResNet18(num_classes=256, compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV).eval()
    with torch.no_grad():
        f = net(dev(fill.hash_tensor((2, 3, 224, 224), 606)))
        f2 = net(dev(fill.hash_tensor((1, 3, 250, 2500), 606)))   # the reference's full-resolution lead image
    assert (f.cpu() - torch.from_numpy(g6["feat_224"])).abs().max() < 1e-3
    assert (f2.cpu() - torch.from_numpy(g6["feat_250x2500"])).abs().max() < 1e-3


def _build_pair(cd):
    cfg = type("Cfg", (Config,), {})
    cfg.compute_dtype, cfg.clinical_input_dim = cd, 16
    ref = O.disable_dropout(fill.hash_fill_module(O.ECGMultimodalModel(2, 16), "mm."))
    net = ECGMultimodalModel(cfg)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, _disable_dropout(net).to(DEV)


@pytest.mark.parametrize("cd,tol", [("fp32", 1e-3), ("bf16", 0.06)])
def test_multimodal_eval_and_train_logits_vs_golden_g5(golden_dir, cd, tol):
    g5 = np.load(f"{golden_dir}/g5_multimodal.npz")
    ref, net = _build_pair(cd)
    img, sig, clin, lab = fill.synthetic_batch(8, salt=5)
    names = ("img_logits", "sig_logits", "clin_logits", "fusion_logits", "var_loss", "soft_w")
    net.eval()
    with torch.no_grad():
        out = net(dev(img), dev(sig), dev(clin))
    for n, o in zip(names, out):
        assert (o.cpu() - torch.from_numpy(g5["eval." + n])).abs().max() < tol, n
    net.train()
    out = net(dev(img), dev(sig), dev(clin))
    loss = HF.cross_entropy(out[3], dev(lab)) + 0.1 * out[4]
    loss.backward()
    torch.cuda.synchronize()
    for n, o in zip(names, out):
        assert (o.detach().cpu() - torch.from_numpy(g5["train." + n])).abs().max() < tol, n
    assert abs(loss.item() - float(g5["train.loss"])) < tol
    if cd == "fp32":
        for k, p in net.named_parameters():
            gn = float(g5["gnorm." + k])
            if p.grad is None:
                assert gn == 0.0, k   # branch heads are not in the loss (train.py:78)
                continue
            if any(s in k for s in SIG_BIAS_SKIP):
                continue
            assert abs(p.grad.norm().item() - gn) < 5e-3 * gn + 1e-6, (k, p.grad.norm().item(), gn)
        for k in ("fusion_classifier.0.weight", "attention_fusion.weights", "signal_encoder.layer3.se.fc.0.weight",
                  "clinical_encoder.0.weight", "signal_encoder.initial.0.weight"):
            assert rel_err(dict(net.named_parameters())[k].grad.cpu(), torch.from_numpy(g5["grad." + k])) < 5e-3, k


@pytest.mark.parametrize("tag", ["pmb", "tab"])
def test_multimodal_vs_reference_object_golden_g9(golden_dir, tag):
    """g9 = outputs, loss, gradients and 3-step Adam losses of the REFERENCE's own ECGMultimodalModel objects
    (multimodal_paper_modal_balance.py:197-354 with its 24-wide clinical MLP; multimodal.py:333-469 with widths
    512 / 128 / 32 and the TabNet branch), hash-filled -- oracle/make_golden.py imports the reference files themselves.
    fp32 compute path: all six outputs within 1e-3, every head / fusion / clinical gradient, the loss trajectory."""
    from ecgmm.multimodal import ECGMultimodalModel as TabVariant
    from oracle import tabnet_ref as T
    g9 = np.load(f"{golden_dir}/g9_reference_composition.npz")
    cfg = type("Cfg", (Config,), {"compute_dtype": "fp32"})          # clinical width: the reference's own (24 / 2)
    if tag == "pmb":
        ref, net, clin_in = O.ECGMultimodalModel(2, 24), ECGMultimodalModel(cfg), 24
    else:
        ref, net, clin_in = T.multimodal_tabnet_model(2), TabVariant(cfg), 2
    net.load_state_dict(fill.hash_fill_module(ref, "mm.").state_dict(), strict=True)
    net = _disable_dropout(net).to(DEV)
    img, sig, clin, lab = fill.synthetic_batch(8, clin_dim=clin_in, salt=9)
    names = ("img_logits", "sig_logits", "clin_logits", "fusion_logits", "var_loss", "soft_w")
    net.eval()
    with torch.no_grad():
        out = net(dev(img), dev(sig), dev(clin))
    for n, o in zip(names, out):
        assert (o.cpu() - torch.from_numpy(g9[f"{tag}.eval.{n}"])).abs().max() < 1e-3, n
    net.train()
    opt = FusedAdam(net.parameters(), lr=1e-4)
    losses = []
    for it in range(3):
        opt.zero_grad()
        out = net(dev(img), dev(sig), dev(clin))
        loss = HF.cross_entropy_plus(out[3], dev(lab), out[4], 0.1)
        loss.backward()
        if it == 0:
            torch.cuda.synchronize()
            for n, o in zip(names, out):
                assert (o.detach().cpu() - torch.from_numpy(g9[f"{tag}.train.{n}"])).abs().max() < 1e-3, n
            for k, p in net.named_parameters():
                if k == "clinical_encoder.0.bias":      # feeds BatchNorm: true gradient 0, rounding noise on both sides
                    assert p.grad.abs().max().item() < 1e-6
                elif f"{tag}.grad.{k}" in g9.files:
                    assert rel_err(p.grad.cpu(), torch.from_numpy(g9[f"{tag}.grad.{k}"])) < 5e-3, k
                elif f"{tag}.gnorm.{k}" in g9.files and not any(s in k for s in SIG_BIAS_SKIP):
                    gn = float(g9[f"{tag}.gnorm.{k}"])
                    assert abs(p.grad.norm().item() - gn) < 5e-3 * gn + 1e-6, (k, p.grad.norm().item(), gn)
                else:
                    assert p.grad is None or any(s in k for s in SIG_BIAS_SKIP), k
        opt.step()
        losses.append(loss.item())
    assert np.allclose(losses, g9[f"{tag}.adam3"], atol=2e-3), (losses, g9[f"{tag}.adam3"])


@pytest.mark.parametrize("frozen", [False, True])
def test_multimodal_three_adam_steps_vs_golden_g5(golden_dir, frozen):
    """train.py:60-81 step (zero_grad / forward / CE + 0.1 var / backward / Adam) x3, fp32."""
    g5 = np.load(f"{golden_dir}/g5_multimodal.npz")
    _, net = _build_pair("fp32")
    if frozen:   # train.py:35-40
        for enc in (net.image_encoder, net.signal_encoder, net.clinical_encoder):
            for p in enc.parameters():
                p.requires_grad = False
    net.train()
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    img, sig, clin, lab = [dev(t) for t in fill.synthetic_batch(8, salt=5)]
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = net(img, sig, clin)
        loss = HF.cross_entropy(out[3], lab) + 0.1 * out[4]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    ref = g5["adam3.frozen" if frozen else "adam3.unfrozen"]
    assert np.allclose(losses, ref, atol=2e-3), (losses, ref)
    assert losses[2] < losses[0]


# ---------------------------------------------------------------------------------------------------
# bf16 trunks.  bf16 storage of activations / inter-layer gradients perturbs deep-layer gradients by
# tens of percent on ANY implementation (BatchNorm backward subtracts large common modes), so the
# yardstick is torch's own CPU bf16 autocast of the oracle: the HIP bf16 path must deviate from the
# fp32 oracle by no more than 1.3x what torch's bf16 autocast does (+2 % absolute slack).
# ---------------------------------------------------------------------------------------------------
def _dev_vs_autocast(make_ref, make_net, x, loss_of, keys):
    def run_ref(autocast):
        ref = make_ref()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            f = ref(x)
        loss_of(f.float()).backward()
        return f.detach().float(), {k: p.grad.clone() for k, p in ref.named_parameters()}
    f32, g32 = run_ref(False)
    f16, g16 = run_ref(True)
    net = make_net()
    f = net(dev(x))
    loss_of(f, gpu=True).backward()
    torch.cuda.synchronize()
    gm = _grads(net)
    assert rel_err(f.detach().cpu(), f32) < 1.3 * rel_err(f16, f32) + 0.02
    bad = []
    for k in keys:
        mine, theirs = rel_err(gm[k], g32[k]), rel_err(g16[k], g32[k])
        if not mine < 1.3 * theirs + 0.02:
            bad.append((k, mine, theirs))
    assert not bad, bad


@pytest.fixture(params=["default", "everywhere"])
def conv_kernel_choice(request):
    """default: the plans pick kernels/fusions by their size rules (small test shapes -> general kernels, separate passes);
    everywhere: the halo conv kernel, the ring wgrad kernel and the fused BatchNorm-backward reductions wherever applicable,
    and the stem by recompute (csrc/conv_stem_fused.hip: an option, off by default)"""
    from ecgmm.hip import lib as L
    everywhere = dict(ECGMM_CONV_HALO=2, ECGMM_WGRAD_RING=2, ECGMM_BN_FUSE_MIN_M=0, ECGMM_STEM_RECOMPUTE=1)
    with switches(L.lib(), **(everywhere if request.param == "everywhere" else {})):
        yield request.param


@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (8, 3, 128, 96)])
def test_resnet18_bf16_no_worse_than_torch_autocast(shape, conv_kernel_choice):
    sd = fill.hash_fill_module(O.ResNet18(num_classes=256), "r18.").state_dict()
    r = fill.hash_tensor((shape[0], 256), 99)

    def make_ref():
        m = O.ResNet18(num_classes=256); m.load_state_dict(sd); return m.train()

    def make_net():
        m = ResNet18(num_classes=256, compute_dtype="bf16"); m.load_state_dict(sd); return m.to(DEV).train()

    def loss_of(f, gpu=False):
        return (f * (dev(r) if gpu else r)).sum()

    keys = [k for k in sd if k.endswith("weight") and ("conv" in k or "downsample.0" in k or k == "fc.weight")]
    _dev_vs_autocast(make_ref, make_net, fill.hash_tensor(shape, 607), loss_of, keys)


def test_resnet1d_bf16_no_worse_than_torch_autocast(golden_dir):
    sd = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/best_ptbxl_tensors.npz").items()}
    y = torch.tensor([0, 1, 1, 0, 1, 0])

    def make_ref():
        m = O.ResNet1D_SE(1, 2); m.load_state_dict(sd); return O.disable_dropout(m).train()

    def make_net():
        m = ResNet1D_SE(1, 2, compute_dtype="bf16"); m.load_state_dict(sd); return _disable_dropout(m).to(DEV).train()

    def loss_of(f, gpu=False):
        return HF.cross_entropy(f, dev(y)) if gpu else torch.nn.functional.cross_entropy(f, y)

    keys = [k for k in sd if k.endswith("weight") and k.count(".") >= 1 and sd[k].dim() >= 2]
    _dev_vs_autocast(make_ref, make_net, fill.hash_tensor((6, 1, 2476), 91, 1.5), loss_of, keys)


def test_sig12_focal_onecycle_three_steps_vs_reference_golden_g3(golden_dir):
    """g3: the REFERENCE's 12-lead ResNet1D_SE + FocalLoss + Adam + OneCycleLR (train_signal_12_af.py:238-275),
    3 steps: same lr / beta1 schedule (OneCycleLR rewrites both every step) and loss trajectory."""
    from ecgmm.signal_model import FocalLoss
    g3 = np.load(f"{golden_dir}/g3_sig12_steps.npz")
    ref = fill.hash_fill_module(O.ResNet1D_SE(12, 2), "sig12.")
    net = ResNet1D_SE(12, 2, compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = _disable_dropout(net).to(DEV).train()
    x, y = dev(fill.hash_tensor((8, 12, 5000), 555, 1.5)), dev(torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]))
    opt = FusedAdam(net.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, steps_per_epoch=4, epochs=30)
    crit = FocalLoss(alpha=1.0, gamma=2.0)
    losses = []
    for i in range(3):
        assert abs(opt.param_groups[0]["lr"] - g3["lrs"][i]) < 1e-12
        assert abs(opt.param_groups[0]["betas"][0] - g3["beta1s"][i]) < 1e-9
        opt.zero_grad()
        loss = crit(net(x), y)
        loss.backward()
        opt.step()
        sch.step()
        losses.append(loss.item())
    assert np.allclose(losses, g3["losses"], atol=1e-3), (losses, g3["losses"])
    net.eval()
    with torch.no_grad():
        fin = net(x)
    assert (fin.cpu() - torch.from_numpy(g3["final_logits"])).abs().max() < 5e-3


def test_entry_points_run_on_gpu(tmp_path, monkeypatch):
    """train.py (frozen encoders, as train.py:35-40), train_image_only.py and train_signal_12_af.py run a tiny
    synthetic epoch end to end: loaders, freeze, step, validation, checkpoints, test metrics."""
    import ecgmm.train as T
    import ecgmm.train_image_only as TI
    import ecgmm.train_signal_12_af as TS
    monkeypatch.chdir(tmp_path)
    cfg = type("Tiny", (Config,), {})
    cfg.img_height = cfg.img_width = 64
    cfg.signal_length, cfg.clinical_input_dim = 1000, 16
    cfg.synthetic_train_size, cfg.synthetic_val_size, cfg.synthetic_test_size, cfg.batch_size = 16, 8, 8, 8
    cfg.device, cfg.compute_dtype, cfg.checkpoint_dir = "cuda", "bf16", str(tmp_path / "ck")
    import ecgmm.train_paper_modal_balance as TP
    import os
    for main, tabnet in ((lambda: T.main(cfg, freeze_encoders=True, num_epochs=2, quiet=True), True),     # train.py:14,35-40
                         (lambda: TP.main(cfg, num_epochs=2, quiet=True), False)):   # train_paper_modal_balance.py:13,29
        hist, results, ckpt = main()
        assert len(hist) == 2 and {"best", "last"} <= set(results) and 0.0 <= results["last"]["accuracy"] <= 1.0
        assert {"last.pth", "best.pth", "epoch1.pth"} <= set(os.listdir(ckpt))
        sd = torch.load(os.path.join(ckpt, "last.pth"), map_location="cpu")
        assert "image_encoder.layer4.1.bn2.running_var" in sd and "attention_fusion.weights" in sd
        assert any(k.startswith("clinical_encoder.tabnet") for k in sd) == tabnet
    for k in ("img_height", "img_width", "synthetic_train_size", "synthetic_val_size", "synthetic_test_size", "batch_size",
              "checkpoint_dir", "device"):
        monkeypatch.setattr(TI.Config, k, getattr(cfg, k), raising=False)
    h2, _ = TI.main(num_epochs=1, quiet=True)
    assert len(h2) == 1 and h2[0][0] == h2[0][0]
    h3, _ = TS.main(epochs=1, batch_size=8, length=1000, quiet=True)
    assert len(h3) == 1 and h3[0][0] == h3[0][0]


def test_multimodal_full_resolution_lead_image_train_step_vs_oracle():
    """the reference's un-resized 250x2500 lead images (dataset_image.py:67-70, README:37) through
    the same kernels: non-square maps 125x1250 -> 63x625 -> 32x313 -> 16x157 -> 8x79, fp32 parity at B=2."""
    ref, net = _build_pair("fp32")
    img = fill.hash_tensor((2, 3, 250, 2500), 808)
    _, sig, clin, lab = fill.synthetic_batch(2, salt=8)
    ref.train()
    out_ref = ref(img, sig, clin)
    O.multimodal_loss(out_ref, lab).backward()
    net.train()
    out = net(dev(img), dev(sig), dev(clin))
    (HF.cross_entropy(out[3], dev(lab)) + 0.1 * out[4]).backward()
    torch.cuda.synchronize()
    assert (out[3].detach().cpu() - out_ref[3].detach()).abs().max() < 1e-3
    for k in ("image_encoder.conv1.weight", "image_encoder.layer2.0.downsample.0.weight",
              "image_encoder.layer4.1.conv2.weight", "fusion_classifier.0.weight"):
        g_ref = dict(ref.named_parameters())[k].grad
        assert rel_err(dict(net.named_parameters())[k].grad.cpu(), g_ref) < 2e-2, k   # 4M-term fp32 sums, B=2 BatchNorm


def test_adam_skips_parameters_without_gradient_and_sinks_refuse_double_writes():
    """train.py:78 puts only fusion_logits (+ var_loss) in the loss: the three branch classifiers get no gradient and
    torch.optim.Adam leaves them at their initial values (they must not be updated from uninitialised
    memory).  And a second backward into unconsumed sinks raises instead of silently dropping the first gradient."""
    from ecgmm.optim import FusedAdam
    ref, net = _build_pair("fp32")
    net.train()
    heads = {k: p.detach().clone() for k, p in net.named_parameters() if "_classifier." in k and "fusion" not in k}
    assert len(heads) == 6
    opt = FusedAdam(net.parameters(), lr=1e-2)
    img, sig, clin, lab = (dev(t) for t in fill.synthetic_batch(8, salt=31))
    for _ in range(3):
        opt.zero_grad()
        out = net(img, sig, clin)
        (HF.cross_entropy(out[3], lab) + 0.1 * out[4]).backward()
        opt.step()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    for k, v in heads.items():
        assert params[k].grad is None and torch.equal(params[k].detach(), v), k
    assert not torch.equal(params["fusion_classifier.0.weight"].detach().cpu(),
                           dict(ref.named_parameters())["fusion_classifier.0.weight"].detach())
    # a gradient written by an earlier backward but not by the current one is zeroed, not re-applied
    opt.zero_grad()
    out = net(img, sig, clin)
    HF.cross_entropy(out[0], lab).backward()          # image branch only: fusion head gets nothing this time
    before = params["fusion_classifier.3.bias"].grad.clone()
    assert before.abs().sum() > 0
    opt.step()
    assert params["fusion_classifier.3.bias"].grad.abs().sum() == 0
    # double write without zero_grad()/step() in between
    out = net(img, sig, clin)
    loss = HF.cross_entropy(out[3], lab)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="gradient sink written twice"):
        loss.backward()
    HF.release_grads(net)
