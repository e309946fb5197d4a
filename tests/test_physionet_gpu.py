"""PhysioNet-2017 single-lead path on the GPU: filtfilt + z-score and gather + augment kernels against scipy / numpy in
float64, the device loader against the reference pipeline restated here, three training steps against the CPU oracle, both
entry points end to end.  Every test prints the figure it asserts on (run with -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.signal
import torch
from scipy.io import savemat

from ecgmm import preprocess as PP
from ecgmm import train_physionet as TP
from ecgmm import train_physionet_multi as TM
from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.multimodal_paper_modal_balance import ResNet1D_SE
from ecgmm.optim import FusedAdam
from ecgmm.signal_model import FocalLoss
from oracle import fill, ref_models as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-5          # the bar tests/test_dataset_gpu.py holds the existing signal kernel to
BAND = scipy.signal.butter(4, [16 / 150, 149 / 150], "band")


def _ref_pre(x32, b, a, zscore=True, eps=1e-8):
    """train_physionet.py:23-45 in float64: filtfilt (default odd padding, lfilter_zi) -> (x - mean) / (std + eps)."""
    y = scipy.signal.filtfilt(b, a, np.asarray(x32, dtype=np.float64), axis=-1)
    if zscore:
        y = (y - y.mean(-1, keepdims=True)) / (y.std(-1, keepdims=True) + eps)
    return y


def _fz_raw(x32, b, a, zscore=True, eps=1e-8):
    """the C entry point with a NaN-filled output: every element must be written"""
    x = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DEV)
    out = torch.full_like(x, float("nan"))
    dbl = lambda v: (C.c_double * len(v))(*[float(t) for t in v])
    zi = PP.lfilter_zi(b, a)
    L.check(L.lib().ecgmm_signal_filter_zscore(ptr(x), ptr(out), x.shape[0], x.shape[1], dbl(b), dbl(a), dbl(zi), len(a) - 1,
                                               int(zscore), eps, stream()), "signal_filter_zscore")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _records(S, Ln, salt):
    x = fill.hash_tensor((S, Ln), salt, 1.0).numpy().astype(np.float64)
    t = np.arange(Ln) / 300.0
    x += 0.8 * np.exp(8.0 * (np.cos(2 * np.pi * 1.2 * t) - 1.0)) + 0.3 * np.sin(2 * np.pi * 0.4 * t)   # beats + wander
    return x.astype(np.float32)


def test_filter_zscore_64x3000_against_float64_scipy():
    x = _records(64, 3000, 101)
    x[5, 2714:] = 0.0          # zero-padded short records (pad_sequences 'post')
    x[6, 900:] = 0.0
    x[7, :] = 0.0              # constant zero: 0 / (0 + 1e-8) = 0 in the reference
    b, a = BAND
    ref = _ref_pre(x, b, a)
    got = _fz_raw(x, b, a)
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"filter_zscore [64, 3000] band-pass: max |diff| {err:.3g}")
    assert err <= BAR
    assert np.all(ref[7] == 0.0) and np.all(got[7] == 0.0)
    one = _fz_raw(x[:1], b, a)
    assert np.array_equal(one[0], got[0])              # S = 1 equals row 0 of S = 64 bit for bit
    # the Python wrapper, with its own filter design, gives the same bits
    via = PP.filter_zscore(torch.from_numpy(x).to(DEV), *PP.butter_bandpass(4, 16 / 150, 149 / 150)).cpu().numpy()
    assert np.abs(via.astype(np.float64) - ref).max() <= BAR
    pre = TP.preprocess_signal(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.array_equal(pre, via)


_FILTERS = {2: scipy.signal.butter(1, [0.1, 0.6], "band"), 5: scipy.signal.butter(5, 0.3), 8: BAND}


@pytest.mark.parametrize("zscore", [True, False])
@pytest.mark.parametrize("n", [2, 5, 8])
@pytest.mark.parametrize("Ln", [200, 3000, 9000, 18000])
def test_filter_zscore_lengths_orders(Ln, n, zscore):
    b, a = _FILTERS[n]
    assert len(a) == n + 1
    x = _records(8, Ln, 200 + n)
    ref = _ref_pre(x, b, a, zscore)
    got = _fz_raw(x, b, a, zscore)
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"filter_zscore L={Ln} n={n} zscore={zscore}: max |diff| {err:.3g}")
    assert err <= BAR


def test_filter_zscore_helpers_and_refusals():
    x = _records(3, 3000, 77)
    xd = torch.from_numpy(x).to(DEV)
    z = TP.z_score_normalize(xd).cpu().numpy()
    x64 = x.astype(np.float64)
    assert np.abs(z - (x64 - x64.mean(-1, keepdims=True)) / (x64.std(-1, keepdims=True) + 1e-8)).max() <= BAR
    bp = TP.bandpass_filter(xd).cpu().numpy()
    assert np.abs(bp - scipy.signal.filtfilt(*BAND, x64, axis=-1)).max() <= BAR
    assert TP.preprocess_signal(xd.reshape(3, 1, 3000)).shape == (3, 1, 3000)
    with pytest.raises(RuntimeError, match="LDS"):
        PP.filter_zscore(torch.zeros(1, 20000, device=DEV), *BAND)         # largest L at order 8: 19850
    with pytest.raises(RuntimeError, match="padlen"):
        PP.filter_zscore(torch.zeros(1, 27, device=DEV), *BAND)
    with pytest.raises(RuntimeError, match="order"):
        PP.filter_zscore(torch.zeros(1, 3000, device=DEV), *scipy.signal.butter(5, [0.1, 0.5], "band"))   # order 10


# ---------------------------------------------------------------------------------------------------------------------
# gather + augment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ln", [3000, 3001, 1022, 5])
def test_gather_plain_is_bit_identical(Ln):
    src = fill.hash_tensor((100, Ln), 31, 2.0).to(DEV)
    index = torch.from_numpy(np.array([(7 * i * i + 3) % 100 for i in range(37)] + [99, 0, 0, 99], dtype=np.int64))
    out = TP.gather_augment(src, index)
    assert torch.equal(out, src[index.to(DEV)])
    assert torch.equal(TP.gather_augment(src, index.to(DEV)), out)


def test_gather_refuses_out_of_range_index_on_the_host():
    src = fill.hash_tensor((10, 64), 32).to(DEV)
    for bad in ([0, 10], [-1, 3]):
        with pytest.raises(IndexError):
            TP.gather_augment(src, torch.tensor(bad, dtype=torch.int64))
        with pytest.raises(IndexError):
            TP.gather_augment(src, torch.tensor(bad, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        TP.gather_augment(src, torch.tensor([1], dtype=torch.int32))


def _augmented(B=4096, Ln=3000, seed_offset=(1234, 7)):
    src = fill.hash_tensor((B, Ln), 41, 1.0).to(DEV)
    out, dec = TP.gather_augment(src, torch.arange(B), augment=True, return_decisions=True, seed_offset=seed_offset)
    torch.cuda.synchronize()
    return src.cpu().numpy(), out.cpu().numpy(), dec.cpu().numpy()


def test_augment_exact_reconstruction_and_rates():
    B, Ln = 4096, 3000
    src, out, dec = _augmented(B, Ln)
    assert not np.isnan(out).any()
    bits = dec[:, 3].astype(np.int64)
    f_noise, f_scale, f_roll = (bits & 1) > 0, (bits & 2) > 0, (bits & 4) > 0
    scale, shift = dec[:, 1], dec[:, 2].astype(np.int64)
    assert np.array_equal(dec[:, 0], f_noise.astype(np.float32))
    assert np.all(scale[~f_scale] == 1.0) and np.all(shift[~f_roll] == 0) and np.all(dec[:, 2] == shift)
    # (i) undo the roll (out[(t + shift) mod L] = v[t]) and the scale
    unrolled = np.stack([np.roll(out[i], -shift[i]) for i in range(B)])
    clean = src * scale[:, None]                                  # fp32 multiply, as the kernel's
    d = np.abs(unrolled[~f_noise] - clean[~f_noise])
    assert np.all(d <= np.spacing(np.abs(clean[~f_noise])))       # 1 ulp of the scale multiply
    resid = unrolled[f_noise].astype(np.float64) / scale[f_noise, None].astype(np.float64) - src[f_noise].astype(np.float64)
    n = resid.size
    assert n > 5_000_000
    # (ii) rates: conditions from the sample sizes
    band = 5 * np.sqrt(0.25 / B)
    for name, f in (("noise", f_noise), ("scale", f_scale), ("roll", f_roll)):
        print(f"flag {name}: frequency {f.mean():.4f}")
        assert abs(f.mean() - 0.5) <= band
    for fa, fb in ((f_noise, f_scale), (f_noise, f_roll), (f_scale, f_roll)):
        assert abs(np.corrcoef(fa, fb)[0, 1]) <= 5 / np.sqrt(B)
    rolled = shift[f_roll]
    assert rolled.min() >= -10 and rolled.max() <= 9 and set(rolled.tolist()) == set(range(-10, 10))
    sc = scale[f_scale].astype(np.float64)
    assert sc.min() >= np.float32(0.8) and sc.max() < np.float32(1.2)
    assert abs(sc.mean() - 1.0) <= 5 * (0.4 / np.sqrt(12)) / np.sqrt(sc.size)
    mean, std = resid.mean(), resid.std()
    r = resid - resid.mean(-1, keepdims=True)
    lag1 = (r[:, 1:] * r[:, :-1]).sum() / (r * r).sum()
    print(f"noise residual: n {n} mean {mean:.3g} std {std:.6f} lag-1 autocorrelation {lag1:.3g}")
    assert abs(mean) <= 5 * 0.01 / np.sqrt(n)
    assert abs(std - 0.01) <= 0.01 * 0.01
    assert abs(lag1) < 5 / np.sqrt(n)


def test_augment_determinism_and_row_independence():
    Ln = 3000
    src = fill.hash_tensor((600, Ln), 43, 1.0).to(DEV)
    idx = torch.from_numpy(np.array([(11 * i + 5) % 600 for i in range(512)], dtype=np.int64))
    kw = dict(augment=True, return_decisions=True)
    a, da = TP.gather_augment(src, idx, seed_offset=(99, 3), **kw)
    b, db = TP.gather_augment(src, idx, seed_offset=(99, 3), **kw)
    assert torch.equal(a, b) and torch.equal(da, db)
    c, dc = TP.gather_augment(src, idx, seed_offset=(99, 4), **kw)
    assert not torch.equal(a, c) and not torch.equal(da, dc)
    e, _ = TP.gather_augment(src, idx, seed_offset=(100, 3), **kw)
    assert not torch.equal(a, e)
    small, ds = TP.gather_augment(src, idx[:8], seed_offset=(99, 3), **kw)
    assert torch.equal(small, a[:8]) and torch.equal(ds, da[:8])      # row i does not depend on B or on the other rows
    # an odd length takes the element-wise store path: same decisions, same per-row rule
    src2 = fill.hash_tensor((64, 1021), 44, 1.0).to(DEV)
    o2, d2 = TP.gather_augment(src2, torch.arange(64), seed_offset=(99, 3), **kw)
    assert torch.equal(d2, da[:64]) and not torch.isnan(o2).any()
    # the module-level Philox state advances per call and replays under manual_seed
    HF.manual_seed(5)
    x1, x2 = TP.augment_signal(src[:32]), TP.augment_signal(src[:32])
    HF.manual_seed(5)
    y1 = TP.augment_signal(src[:32])
    assert torch.equal(x1, y1) and not torch.equal(x1, x2)


# ---------------------------------------------------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------------------------------------------------
def _write_tree(root, n=48, seed=11):
    """a small challenge-shaped tree: NAME.mat + NAME.hea, REFERENCE.csv with all four labels, lengths 2000 .. 18000"""
    data = root / "training2017"
    data.mkdir(parents=True)
    rng = np.random.RandomState(seed)
    names = ["N"] * 20 + ["AF"] * 10 + ["O"] * 14 + ["~"] * 4
    rng.shuffle(names)
    rows, signals = [], {}
    for i, lab in enumerate(names[:n]):
        rec = f"A{i:05d}"
        length = int(rng.randint(2000, 18001))
        t = np.arange(length) / 300.0
        x = 0.9 * np.exp(8.0 * (np.cos(2 * np.pi * (1.0 + 0.3 * rng.rand()) * t) - 1.0)) + 0.05 * rng.randn(length)
        val = np.round(x * 1000).astype(np.int16)
        savemat(str(data / f"{rec}.mat"), {"val": val.reshape(1, -1)})
        (data / f"{rec}.hea").write_text(f"{rec} 1 300 {length}\n{rec}.mat 16+24 1000/mV 16 0 {val[0]} 0 0 ECG\n")
        rows.append(f"{rec},{lab}")
        signals[rec] = val.astype(np.float64) / 1000.0
    (root / "REFERENCE.csv").write_text("\n".join(rows) + "\n")
    cfg = type("Tree", (Config,), {"synthetic": False, "physionet_dir": str(root), "physionet_data_dir": str(data),
                                   "physionet_label_file": str(root / "REFERENCE.csv"), "device": "cuda",
                                   "compute_dtype": "fp32", "checkpoint_dir": str(root / "ck")})
    return cfg, rows, signals


def _reference_splits(rows, signals, label_map, split, seed):
    """train_physionet.py:91-118 + :72-86 restated: labels, stratified split, pad, filtfilt, z-score, float32"""
    from sklearn.model_selection import train_test_split
    keep = [r.split(",") for r in rows if r.split(",")[1] in label_map]
    labels = np.array([label_map[lab] for _, lab in keep])
    sigs = [signals[rec] for rec, _ in keep]
    idx = np.arange(len(keep))
    tr, tmp, _, tmp_y = train_test_split(idx, labels, test_size=split[0], stratify=labels, random_state=seed)
    va, te = train_test_split(tmp, test_size=split[1], stratify=tmp_y, random_state=seed)
    out = []
    for part in (tr, va, te):
        pad = np.zeros((len(part), 3000), dtype=np.float32)
        for j, i in enumerate(part):
            k = min(len(sigs[i]), 3000)
            pad[j, :k] = sigs[i][:k]
        out.append((_ref_pre(pad, *BAND).astype(np.float32), labels[part]))
    return out


@pytest.mark.parametrize("module", ["binary", "multi"])
def test_loader_matches_the_reference_pipeline(tmp_path, module):
    cfg, rows, signals = _write_tree(tmp_path)
    if module == "binary":
        loaders = TP.get_signalonly_dataloaders(cfg, batch_size=8, augment=False)
        refs = _reference_splits(rows, signals, TP.LABEL_MAP, TP.SPLIT, cfg.seed)
    else:
        loaders = TM.get_signalonly_dataloaders(cfg, batch_size=8)
        refs = _reference_splits(rows, signals, TM.LABEL_MAP, TM.SPLIT, cfg.seed)
    worst = 0.0
    for loader, (ref_x, ref_y), shuffled in zip(loaders, refs, (True, False, False)):
        assert len(loader.dataset) == len(ref_y) and len(loader) == (len(ref_y) + 7) // 8
        xs, ys = zip(*[(x.cpu().numpy(), y.cpu().numpy()) for x, y in loader])
        assert all(x.shape == (min(8, len(ref_y) - 8 * k), 3000) and x.dtype == np.float32 for k, x in enumerate(xs))
        order = loader.last_order.numpy()
        if shuffled:
            assert sorted(order.tolist()) == list(range(len(ref_y))) and not np.array_equal(order, np.arange(len(ref_y)))
        else:
            assert np.array_equal(order, np.arange(len(ref_y)))
        assert np.array_equal(np.concatenate(ys), ref_y[order])                       # labels and order exact
        worst = max(worst, np.abs(np.concatenate(xs).astype(np.float64) - ref_x[order]).max())
    print(f"loader ({module}) vs the reference pipeline: max |diff| {worst:.3g}")
    assert worst <= BAR


def test_train_loader_augments_only_in_the_binary_script(tmp_path):
    cfg, _, _ = _write_tree(tmp_path)
    HF.manual_seed(cfg.seed)
    tr, va, _ = TP.get_signalonly_dataloaders(cfg, batch_size=8)
    assert tr.dataset.augment and not va.dataset.augment
    x, _ = next(iter(tr))
    plain = tr.dataset.signals[tr.last_order[:8].to(DEV)]
    assert x.shape == plain.shape and not torch.equal(x, plain)       # 8 rows, 7/8 chance each of a visible change
    assert not TM.get_signalonly_dataloaders(cfg, batch_size=8)[0].dataset.augment


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


@pytest.mark.parametrize("nc", [2, 3])
def test_three_steps_focal_adam_onecycle_against_the_oracle(nc):
    """ResNet1D_SE fp32 at [8, 1, 3000]: logits < 1e-3, loss trajectory within 2e-3 (the bars g3 / the fp32 path carry)"""
    ref = O.disable_dropout(fill.hash_fill_module(O.ResNet1D_SE(1, nc), f"pn{nc}.")).train()
    net = ResNet1D_SE(1, nc, compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = _no_dropout(net).to(DEV).train()
    opt_r = torch.optim.Adam(ref.parameters(), lr=1e-3)
    sch_r = torch.optim.lr_scheduler.OneCycleLR(opt_r, max_lr=1e-3, steps_per_epoch=4, epochs=30)
    opt = FusedAdam(net.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, steps_per_epoch=4, epochs=30)
    crit_r, crit = O.FocalLoss(1.0, 2.0), FocalLoss(alpha=1.0, gamma=2.0)
    for step in range(3):
        x = fill.hash_tensor((8, 3000), 700 + step, 1.7)
        y = torch.from_numpy((np.arange(8) * (step + 1) + step) % nc).long()
        opt_r.zero_grad()
        out_r = ref(x.unsqueeze(1))
        loss_r = crit_r(out_r, y)
        loss_r.backward()
        opt_r.step()
        sch_r.step()
        opt.zero_grad()
        out = net(x.to(DEV).unsqueeze(1))
        loss = crit(out, y.to(DEV))
        loss.backward()
        opt.step()
        sch.step()
        dl = (out.detach().cpu() - out_r.detach()).abs().max().item()
        print(f"nc={nc} step {step}: max |dlogit| {dl:.3g} loss {loss.item():.6f} vs {loss_r.item():.6f}")
        assert dl < 1e-3
        assert abs(loss.item() - loss_r.item()) <= 2e-3


def test_entry_points_train_on_a_data_tree(tmp_path, monkeypatch):
    from ecgmm.inference import Predictor
    monkeypatch.chdir(tmp_path)
    cfg, _, _ = _write_tree(tmp_path)
    for mod, nc in ((TP, 2), (TM, 3)):
        history, results, ckpt = mod.main(cfg, num_epochs=2, quiet=True)
        assert len(history) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in history)
        assert os.path.exists(os.path.join(ckpt, "last.pth")) and os.path.exists(os.path.join(ckpt, "best.pth"))
        assert any(f.startswith("best_signal_only_epoch") for f in os.listdir(ckpt))
        for tag in ("best", "last"):
            assert all(np.isfinite(results[tag][k]) for k in ("accuracy", "f1", "auc")), results
        sd = torch.load(os.path.join(ckpt, "last.pth"), map_location="cpu")
        O.ResNet1D_SE(1, nc).load_state_dict(sd, strict=True)            # same keys and shapes as the reference's class
    model = ResNet1D_SE(num_classes=3, compute_dtype="fp32")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    x = TP.preprocess_signal(torch.from_numpy(_records(8, 3000, 55)).to(DEV)).unsqueeze(1)
    with torch.no_grad():
        want = model(x)
    got = Predictor(model)(x)
    assert (got - want).abs().max() < 1e-3 * max(1.0, float(want.abs().max()))   # the inference tests' fp32 bar


def test_entry_point_runs_without_data(tmp_path, monkeypatch):
    """Config.synthetic: generated variable-length records; validation and test through the Predictor"""
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (Config,), {"synthetic": True, "synthetic_train_size": 24, "synthetic_val_size": 8,
                                    "synthetic_test_size": 8, "device": "cuda", "checkpoint_dir": str(tmp_path / "ck")})
    history, results, ckpt = TP.main(cfg, num_epochs=1, quiet=True, use_predictor=True)
    assert len(history) == 1 and np.isfinite(history[0]["val_loss"]) and np.isfinite(results["last"]["accuracy"])
