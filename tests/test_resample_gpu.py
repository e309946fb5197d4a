"""Fourier resampling from Python on the GPU: resample_signal and preprocess_resampled against the float64 chain stage by
stage, load_records(target_fs=...) on a small record tree with headers at three rates, and one training epoch on that tree.
Every test prints the figure it asserts on (run with -s)."""
import numpy as np
import pytest
import torch
from scipy.io import savemat

from ecgmm import preprocess as PP
from ecgmm import train_physionet as TP
from ecgmm.config import Config
from oracle import fill

from . import iir_ref as IR
from . import resample_bounds as RB
from . import resample_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _records(S, Ln, salt, fs):
    x = fill.hash_tensor((S, Ln), salt, 0.05).numpy().astype(np.float64)
    t = np.arange(Ln) / float(fs)
    x += 0.8 * np.exp(8.0 * (np.cos(2 * np.pi * 1.2 * t) - 1.0)) + 0.3 * np.sin(2 * np.pi * 0.4 * t)   # beats + wander
    return x.astype(np.float32)


def test_resample_signal_and_preprocess_resampled_against_the_float64_chain():
    """band-pass at 500 Hz (tests/iir_ref.py) -> resample 1000 -> 600 (tests/resample_ref.py) -> z-score, each stage checked
    on the stored output of the stage before it"""
    x = _records(4, 1000, 501, 500)
    xd = torch.from_numpy(x).to(DEV)
    band = IR._design("band", 4, (16 / 250, 149 / 250))
    # stage 1: the filter at orig_fs
    f = TP.bandpass_filter(xd, 16, 149, 500, 4)
    r1 = IR.case_ref(band, x)
    w1 = IR.worst(f.cpu().numpy(), r1.ref, r1.dseq)
    print("band-pass at 500 Hz: worst ratio %.3g" % w1)
    assert not r1.refusable and w1 <= 1.0
    # stage 2: resample_signal on the stored filter output
    y = TP.resample_signal(f, 500, 300)
    assert y.shape == (4, 600) and y.dtype == torch.float32
    f64 = f.cpu().numpy().astype(np.float64)
    RB.check_rows(y.cpu().numpy(), RR.resample_ref(f64, 600), f64, [(1000, 600)] * 4, "resample_signal 500 -> 300 Hz")
    assert torch.equal(y, PP.resample(f, 600)) and torch.equal(y, PP.resample(f, ratio=300 / 500))
    # stage 3: the z-score on the stored resampled rows
    z = TP.z_score_normalize(y)
    y64 = y.cpu().numpy().astype(np.float64)
    ref3 = IR.zscore_ld(y64)
    own = (y64 - y64.mean(-1, keepdims=True)) / (y64.std(-1, keepdims=True) + 1e-8)
    d3 = float(np.abs(own.astype(IR.LD) - ref3).max())
    w3 = IR.worst(z.cpu().numpy(), ref3.astype(np.float64), d3)
    print("z-score: worst ratio %.3g" % w3)
    assert w3 <= 1.0
    # the three steps as one call are these three launches
    assert torch.equal(TP.preprocess_resampled(xd, 500, 300), z)
    assert torch.equal(TP.preprocess_resampled(xd.reshape(2, 2, 1000), 500, 300), z.reshape(2, 2, 600))
    assert TP.resample_signal(xd, 300, 300) is xd


def test_python_lengths_form():
    x = _records(3, 300, 502, 500)
    lengths = [300, 17, 256]
    xn = x.copy()
    for s, n in enumerate(lengths):
        xn[s, n:] = np.nan
    out, nums = PP.resample(torch.from_numpy(xn).to(DEV), ratio=0.6, lengths=lengths)
    assert out.shape == (3, 180) and nums.dtype == torch.int32 and nums.tolist() == [180, 10, 153]
    ref, _ = RR.resample_lengths_ref(xn, lengths, 0.6)
    RB.check_rows(out.cpu().numpy(), ref, [np.nan_to_num(r.astype(np.float64)) for r in xn], list(zip(lengths, nums.tolist())),
                  "PP.resample with lengths")
    assert bool((out[1, 10:] == 0).all()) and bool((out[2, 153:] == 0).all())
    with pytest.raises(ValueError):
        PP.resample(torch.from_numpy(x).to(DEV), ratio=0.6, lengths=[300, 0, 256])      # HF.check_lengths: 1 <= len <= L
    with pytest.raises(ValueError):
        PP.resample(torch.from_numpy(x).to(DEV), ratio=0.6, lengths=[300, 301, 256])


RATES = (300, 500, 250)


def _write_tree(tmp_path, n=30, seed=5):
    root = tmp_path / "physionet"
    data = root / "training2017"
    data.mkdir(parents=True)
    rng = np.random.RandomState(seed)
    names = (["N"] * 14 + ["AF"] * 7 + ["O"] * 9)[:n]
    rng.shuffle(names)
    rows, signals, rates = [], [], []
    for i, lab in enumerate(names):
        rec, fs = f"A{i:05d}", RATES[i % 3]
        length = int(rng.randint(700, 1501))
        t = np.arange(length) / float(fs)
        x = 0.9 * np.exp(8.0 * (np.cos(2 * np.pi * (1.0 + 0.3 * rng.rand()) * t) - 1.0)) + 0.05 * rng.randn(length)
        val = np.round(x * 1000).astype(np.int16)
        savemat(str(data / f"{rec}.mat"), {"val": val.reshape(1, -1)})
        (data / f"{rec}.hea").write_text(f"{rec} 1 {fs} {length}\n{rec}.mat 16+24 1000/mV 16 0 {val[0]} 0 0 ECG\n")
        rows.append(f"{rec},{lab}")
        signals.append(val.astype(np.float64) / 1000.0)
        rates.append(fs)
    (root / "REFERENCE.csv").write_text("\n".join(rows) + "\n")
    cfg = type("Tree", (Config,), {"synthetic": False, "physionet_dir": str(root), "physionet_data_dir": str(data),
                                   "physionet_label_file": str(root / "REFERENCE.csv"), "device": "cuda",
                                   "compute_dtype": "fp32", "checkpoint_dir": str(root / "ck")})
    return cfg, signals, rates


def test_load_records_moves_every_record_to_the_target_rate(tmp_path):
    cfg, signals, rates = _write_tree(tmp_path)
    plain, labels0 = TP.load_records(cfg)
    got, labels = TP.load_records(cfg, target_fs=300)
    assert np.array_equal(labels, labels0) and len(got) == len(signals) == 30
    worst = 0.0
    for i, (raw, fs) in enumerate(zip(signals, rates)):
        assert np.array_equal(plain[i], raw)
        assert got[i].dtype == np.float64 and got[i].ndim == 1
        assert len(got[i]) == int(len(raw) * (300 / fs))
        if fs == 300:
            assert np.array_equal(got[i], raw), "a record already at the target rate must come back as it was read"
            continue
        x32 = raw.astype(np.float32).astype(np.float64)      # what the upload holds
        num = len(got[i])
        ref = RR.resample_ref(x32, num)
        r = RB.ratio_report(got[i], ref, RB.bound(ref, x32, len(raw), num), "record %d" % i)
        worst = max(worst, r.ratio)
        assert r.ok, str(r)
    print("load_records(target_fs=300): worst ratio %.3g over the 500 Hz and 250 Hz records" % worst)


def test_main_trains_one_epoch_on_a_tree_of_mixed_rates(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg, _, _ = _write_tree(tmp_path)
    history, results, _ = TP.main(cfg, num_epochs=1, quiet=True, target_fs=300, max_len=1000)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["val_loss"])
    assert np.isfinite(results["last"]["accuracy"])
    cfg2 = type("TreeFs", (cfg,), {"physionet_target_fs": 300})
    loaders = TP.get_signalonly_dataloaders(cfg, batch_size=8, augment=False, max_len=1000, target_fs=300)
    assert sum(len(ld.dataset) for ld in loaders) == 30
    history2, _, _ = TP.main(cfg2, num_epochs=1, quiet=True, max_len=1000)      # Config.physionet_target_fs alone
    assert len(history2) == 1 and np.isfinite(history2[0]["train_loss"])
