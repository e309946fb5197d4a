"""Log-spectrogram kernel and the train_physionet2 path on the GPU: the kernel against scipy.signal.stft in float64, zero
padding, bit equality, the device loader against the reference pipeline restated here, three training steps against the nn
restatement of the CRNN in float64, the entry point on a data tree and on synthetic records.  Every test prints the figure
it asserts on (run with -s)."""
import functools
import os

import numpy as np
import pytest
import scipy.signal
import torch
from scipy.io import savemat

from ecgmm import spectrogram as SG
from ecgmm import train_physionet2 as T2
from ecgmm.config import Config
from ecgmm.crnn import CRNN, FocalLoss
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.optim import FusedAdam
from oracle import fill

from . import crnn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-5          # the absolute bar tests/test_physionet_gpu.py holds the signal kernels to


def _ref_spec(x, hop=32, window="tukey"):
    """train_physionet2.py:30-34 in float64"""
    z = scipy.signal.stft(np.asarray(x, dtype=np.float64), fs=300, window=window, nperseg=64, noverlap=64 - hop)[2]
    return np.log1p(np.abs(z))


@functools.lru_cache(maxsize=None)
def _records(S, Ln, salt):
    """beats + wander + hash noise, |x| of a few units (the inputs of tests/test_physionet_gpu.py, restated)"""
    x = fill.hash_tensor((S, Ln), salt, 1.0).numpy().astype(np.float64)
    t = np.arange(Ln) / 300.0
    x += 0.8 * np.exp(8.0 * (np.cos(2 * np.pi * 1.2 * t) - 1.0)) + 0.3 * np.sin(2 * np.pi * 0.4 * t)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV)


def _table(window="tukey"):
    return torch.from_numpy(SG.stft_table(window).astype(np.float32)).to(DEV).contiguous()


def _raw(x32, hop=32, window="tukey"):
    """the C entry point with a NaN-filled output: every element must be written"""
    x = _dev(x32)
    S, Ln = x.shape
    T = L.lib().ecgmm_log_spectrogram_frames(Ln, 64, hop)
    assert T > 0
    out = torch.full((S, 33, T), float("nan"), device=DEV)
    L.check(L.lib().ecgmm_log_spectrogram(ptr(x), S, Ln, ptr(_table(window)), 64, hop, ptr(out), T, stream()),
            "log_spectrogram")
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel against scipy
# ---------------------------------------------------------------------------------------------------------------------
_SHAPES = [(2, 64, 32, 3), (2, 65, 32, 4), (2, 95, 32, 4), (2, 96, 32, 4), (2, 97, 32, 5),   # boundary, tail padding, T
           (2, 224, 32, 8), (2, 1216, 32, 39), (1, 3000, 32, 95), (3, 3000, 32, 95), (70, 3000, 32, 95),
           (2, 9000, 32, 283), (2, 18286, 32, 573), (1, 20011, 32, 627),                      # beyond the filter kernel's LDS limit
           (2, 97, 16, 8), (2, 1000, 16, 64), (2, 97, 64, 3), (2, 1000, 64, 17)]


@pytest.mark.parametrize("S,Ln,hop,T", _SHAPES)
def test_kernel_against_float64_scipy(S, Ln, hop, T):
    x = _records(S, Ln, 300 + hop)
    ref = _ref_spec(x, hop)
    got = _raw(x, hop)
    assert got.shape == ref.shape == (S, 33, T)
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"log_spectrogram S={S} L={Ln} hop={hop} (T={T}): max |diff| {err:.3g}, max |ref| {ref.max():.3g}")
    assert err <= BAR


def test_kernel_with_a_coefficient_array_as_window():
    x = _records(2, 1000, 411)
    w = scipy.signal.get_window("hann", 64)
    ref = _ref_spec(x, 32, w)
    got = _raw(x, 32, w)
    assert got.shape == ref.shape and not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"log_spectrogram hann coefficients L=1000: max |diff| {err:.3g}")
    assert err <= BAR
    via = SG.compute_log_spectrogram(_dev(x), window=w).cpu().numpy()
    assert np.array_equal(via, got)
    assert np.abs(got - _raw(x, 32)).max() > 1e-3          # and the window does reach the kernel


# ---------------------------------------------------------------------------------------------------------------------
# 2. zero padding
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_padded_rows_give_their_own_spectrogram_then_exact_zeros():
    lengths = [2714, 3000, 3001, 4096, 4500, 5999, 6000]
    x = np.array(_records(8, 6000, 523))
    for i, n in enumerate(lengths):
        x[i, n:] = 0.0
    x[7, :] = 0.0
    got = _raw(x)
    assert got.shape == (8, 33, 189) and not np.isnan(got).any()
    worst = 0.0
    for i, n in enumerate(lengths):
        ref = _ref_spec(x[i, :n])                       # the record alone, as the reference transforms it
        Tn = ref.shape[1]
        assert Tn == SG.stft_frames(n)
        worst = max(worst, np.abs(got[i, :, :Tn].astype(np.float64) - ref).max())
        assert np.all(got[i, :, Tn:] == 0.0), (i, n)    # np.pad of the spectrogram: exact zeros
    print(f"zero-padded rows vs per-record scipy: max |diff| {worst:.3g}; tails and the all-zero row exactly 0")
    assert worst <= BAR
    assert np.all(got[7] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_run_or_on_the_batch():
    x = _records(70, 3000, 332)
    a, b = _raw(x), _raw(x)
    assert np.array_equal(a, b)
    one = _raw(x[:1])
    assert np.array_equal(one[0], a[0])
    print("two runs equal bit for bit; S = 1 equals row 0 of S = 70")
    x3 = _dev(x[:6].reshape(2, 3, 3000))
    via = SG.compute_log_spectrogram(x3)
    assert via.shape == (2, 3, 33, 95) and via.dtype == torch.float32
    assert np.array_equal(via.cpu().numpy().reshape(6, 33, 95), a[:6])
    with pytest.raises(ValueError, match="shorter"):
        SG.compute_log_spectrogram(torch.zeros(2, 63, device=DEV))
    with pytest.raises(ValueError, match="nperseg"):
        SG.compute_log_spectrogram(x3, nperseg=128, noverlap=64)
    with pytest.raises(ValueError, match="window"):
        SG.compute_log_spectrogram(x3, window="hann")


# ---------------------------------------------------------------------------------------------------------------------
# 4. loader
# ---------------------------------------------------------------------------------------------------------------------
def _write_tree(root, seed=13):
    """a small challenge-shaped tree: NAME.mat + NAME.hea, REFERENCE.csv with all four labels, 40 records of 2000 .. 6000"""
    data = root / "training2017"
    data.mkdir(parents=True)
    rng = np.random.RandomState(seed)
    names = ["N"] * 16 + ["AF"] * 10 + ["O"] * 10 + ["~"] * 4
    rng.shuffle(names)
    rows, signals = [], {}
    for i, lab in enumerate(names):
        rec = f"A{i:05d}"
        length = int(rng.randint(2000, 6001))
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


def _reference_pipeline(rows, signals, seed):
    """train_physionet2.py:128-161 restated: labels, per-record log-spectrogram, np.pad to max_time, stack, two splits"""
    from sklearn.model_selection import train_test_split
    label_map = {"N": 0, "AF": 1, "O": 1}
    keep = [r.split(",") for r in rows if r.split(",")[1] in label_map]
    y = np.array([label_map[lab] for _, lab in keep])
    specs = [np.expand_dims(_ref_spec(signals[rec]), axis=0) for rec, _ in keep]
    max_time = max(s.shape[2] for s in specs)
    X = np.stack([np.pad(s, ((0, 0), (0, 0), (0, max_time - s.shape[2])), mode="constant") for s in specs])
    idx = np.arange(len(y))
    tr, tmp, _, tmp_y = train_test_split(idx, y, test_size=0.2, stratify=y, random_state=seed)
    va, te = train_test_split(tmp, test_size=0.5, stratify=tmp_y, random_state=seed)
    return X, y, (tr, va, te)


def test_loader_matches_the_reference_pipeline(tmp_path):
    cfg, rows, signals = _write_tree(tmp_path)
    X, y, parts = _reference_pipeline(rows, signals, cfg.seed)
    lmax = max(len(signals[r.split(",")[0]]) for r in rows if not r.endswith("~"))
    assert X.shape == (36, 1, 33, SG.stft_frames(lmax))
    B = 8
    loaders = T2.get_spectrogram_dataloaders(cfg, batch_size=B)
    worst = 0.0
    for loader, part, shuffled in zip(loaders, parts, (True, False, False)):
        n = len(part)
        assert len(loader.dataset) == n and len(loader) == (n + B - 1) // B
        assert np.array_equal(loader.dataset.indices.cpu().numpy(), part)                # the split itself, exact
        xs, ys = zip(*[(xb.cpu().numpy(), yb.cpu().numpy()) for xb, yb in loader])
        assert all(xb.shape == (min(B, n - B * k), 1, 33, X.shape[3]) and xb.dtype == np.float32 for k, xb in enumerate(xs))
        order = loader.last_order.numpy()
        if shuffled:
            assert sorted(order.tolist()) == list(range(n)) and not np.array_equal(order, np.arange(n))
        else:
            assert np.array_equal(order, np.arange(n))
        assert np.array_equal(np.concatenate(ys), y[part][order])                        # labels and order exact
        worst = max(worst, np.abs(np.concatenate(xs).astype(np.float64) - X[part][order]).max())
    print(f"loader vs the reference pipeline: splits {[len(p) for p in parts]}, max |diff| {worst:.3g}")
    assert [len(p) for p in parts] == [28, 4, 4]
    assert worst <= BAR
    # the chunked upload is the one-launch result, bit for bit
    recs = [signals[r.split(",")[0]] for r in rows if not r.endswith("~")]
    assert torch.equal(T2.build_spectrograms(recs, DEV, chunk=7), loaders[0].dataset.spectrograms)


# ---------------------------------------------------------------------------------------------------------------------
# 5. three training steps
# ---------------------------------------------------------------------------------------------------------------------
def test_three_steps_on_device_spectrograms_against_the_float64_restatement():
    """fp32 CRNN on compute_log_spectrogram of [4, 1216] records vs tests/crnn_ref.py in float64 on the scipy spectrogram:
    logits < 1e-3, losses within 2e-3 at every step (the bars tests/test_crnn_gpu.py carries for this model)"""
    torch.manual_seed(5)
    ref = R.CRNN()
    ref.classifier[2].p = 0.0
    net = CRNN(compute_dtype="fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net.classifier[2].p = 0.0
    ref, net = ref.double().train(), net.to(DEV).train()
    opt_r = torch.optim.Adam(ref.parameters(), lr=1e-3)
    opt = FusedAdam(net.parameters(), lr=1e-3)
    crit = FocalLoss()
    for step in range(3):
        x = _records(4, 1216, 800 + step)
        lab = torch.from_numpy((np.arange(4) * (step + 1) + step) % 2).long()
        opt_r.zero_grad()
        out_r = ref(torch.from_numpy(_ref_spec(x)).unsqueeze(1))
        loss_r = R.focal_loss(out_r, lab)
        loss_r.backward()
        opt_r.step()
        opt.zero_grad()
        spec = SG.compute_log_spectrogram(_dev(x)).unsqueeze(1)
        assert spec.shape == (4, 1, 33, 39)
        out = net(spec)
        loss = crit(out, lab.to(DEV))
        loss.backward()
        opt.step()
        dl = (out.detach().cpu().double() - out_r.detach()).abs().max().item()
        print(f"step {step}: max |dlogit| {dl:.3g} loss {loss.item():.6f} vs {loss_r.item():.6f}")
        assert dl < 1e-3
        assert abs(loss.item() - loss_r.item()) <= 2e-3


# ---------------------------------------------------------------------------------------------------------------------
# 6. / 7. the entry point
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_trains_on_a_data_tree(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg, _, _ = _write_tree(tmp_path)
    history, results, ckpt = T2.main(cfg, num_epochs=2, batch_size=16, quiet=True)
    print(history, results)
    assert len(history) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in history)
    assert os.path.exists(os.path.join(ckpt, "last.pth")) and os.path.exists(os.path.join(ckpt, "best.pth"))
    for tag in ("best", "last"):      # the test split holds both classes (stratified 2 + 2), so the AUC is defined
        assert all(np.isfinite(results[tag][k]) for k in ("accuracy", "f1", "auc")), results
    sd = torch.load(os.path.join(ckpt, "last.pth"), map_location="cpu")
    R.CRNN().load_state_dict(sd, strict=True)              # same keys and shapes as the reference's class


class _ShortSynthetic(Config):
    synthetic, synthetic_train_size, synthetic_val_size, synthetic_test_size = True, 24, 8, 8
    physionet2_max_len = 6000        # T = 189: the generated records run to 18000 samples
    device, compute_dtype = "cuda", "bf16"


def test_entry_point_runs_without_data(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = type("Synth", (_ShortSynthetic,), {"checkpoint_dir": str(tmp_path / "ck")})
    history, results, ckpt = T2.main(cfg, num_epochs=1, quiet=True)
    print(history, results)
    assert len(history) == 1 and np.isfinite(history[0]["val_loss"]) and np.isfinite(history[0]["val_acc"])
    assert np.isfinite(results["last"]["accuracy"])
