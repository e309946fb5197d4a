"""Shared by tests/test_ptbxl_cpu.py and tests/test_ptbxl_gpu.py: WFDB format-16 records written to disk, a PTB-XL style
data tree, and the reference's ``__getitem__`` (train_signal_only_ptb.py:40-53) restated with numpy / scipy in float64."""
import csv
import os

import numpy as np
from scipy.signal import butter, filtfilt

LEADS = ["I", "II", "III", "AVR", "AVL", "AVF", "V1", "V2", "V3", "V4", "V5", "V6"]


def make_frames(seed, R, T, nsig):
    """int16 frames [R, T, nsig] with negative samples, gains that differ per record and channel, baselines != 0"""
    rng = np.random.RandomState(seed)
    gain = np.round(rng.uniform(300.0, 2500.0, size=(R, nsig)), 1)
    base = rng.randint(-400, 401, size=(R, nsig))
    base[base == 0] = -23
    t = np.arange(T) / 500.0
    d = np.empty((R, T, nsig), dtype=np.int16)
    for r in range(R):
        for c in range(nsig):
            mv = (rng.uniform(0.4, 1.5) * np.sign(rng.randn()) * np.exp(8.0 * (np.cos(2 * np.pi * rng.uniform(0.9, 2.0) * t) - 1.0))
                  + 0.3 * np.sin(2 * np.pi * 0.3 * t + rng.rand() * 6.28) + 0.03 * rng.randn(T))
            d[r, :, c] = np.clip(np.round(mv * gain[r, c]) + base[r, c], -32767, 32767).astype(np.int16)
    assert (d < 0).any()
    return d, gain, base.astype(np.int64)


def write_record(path, frames, gain, base, fmt="16", init=None, checksum=None, fs=500):
    """``path`` without extension; frames int16 [T, nsig] -> path.hea + path.dat as wfdb.wrsamp lays them out"""
    T, nsig = frames.shape
    name = os.path.basename(path)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    frames.astype("<i2").tofile(path + ".dat")
    lines = [f"{name} {nsig} {fs} {T}"]
    for c in range(nsig):
        cs = int(frames[:, c].astype(np.int64).sum() % 65536) if checksum is None else checksum[c]
        iv = int(frames[0, c]) if init is None else init[c]
        lines.append(f"{name}.dat {fmt} {gain[c]}({int(base[c])})/mV 16 0 {iv} {cs} 0 {LEADS[c % 12]}")
    with open(path + ".hea", "w") as f:
        f.write("\n".join(lines) + "\n# written by the test suite\n")


def reference_item(p_lead, length=2476, step=2, order=5):
    """train_signal_only_ptb.py:44-52 on one lead's float64 p_signal"""
    x = p_lead[::step]
    x = x - np.convolve(x, np.ones(200) / 200, mode="same")
    b, a = butter(order, 40 / (0.5 * 250), btype="low")
    x = filtfilt(b, a, x)
    return x[:length] if len(x) > length else np.concatenate([x, np.zeros(length - len(x))])


SCP = ["{'AFIB': 100.0}", "{'SR': 100.0, 'NORM': 80.0}", "{'STACH': 100.0}", "{'AFIB': 100.0, 'SR': 100.0}",
       "{'SBRAD': 100.0}", "{'AFIB': 50.0, 'SR': 100.0}"]          # labels 1 0 0 1 0 0


def write_tree(root, n=24, dropped=3, seed=5):
    """``n`` labelled twelve-lead records (5000 frames, one of 3000 for the pad branch) + ``dropped`` rows whose label is 2
    (no files behind them), ptbxl_database.csv.  -> (frames list, gains, baselines, labels) of the kept rows, in csv order."""
    rows, kept = [], []
    for i in range(n):
        T = 3000 if i == 7 else 5000
        d, gain, base = make_frames(seed * 1000 + i, 1, T, 12)
        rel = f"records500/00000/{i + 1:05d}_hr"
        write_record(os.path.join(root, rel), d[0], gain[0], base[0])
        scp = SCP[i % len(SCP)]
        rows.append(dict(ecg_id=i + 1, patient_id=100 + i, scp_codes=scp, filename_lr=rel.replace("500", "100").replace("hr", "lr"),
                         filename_hr=rel))
        kept.append((d[0], gain[0], base[0], int("'AFIB': 100.0" in scp)))
        if i < dropped:
            rows.append(dict(ecg_id=1000 + i, patient_id=1, scp_codes="{'NORM': 100.0}", filename_lr="x", filename_hr="missing"))
    with open(os.path.join(root, "ptbxl_database.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    return kept
