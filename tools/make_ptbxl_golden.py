"""Generate tests/golden/g10_ptbxl_preprocess.npz -- run ONLY where the reference checkout exists (default /root/reference,
or ECGMM_REFERENCE), never on the GPU machine.

The expected values come from the reference's OWN ``evaluation_signal.preprocess_signal`` (imported, matplotlib on Agg):
the same remove_baseline_drift -> lowpass_filter(40, 250, 5) -> crop / pad to 2476 that train_signal_only_ptb.py:46-52 applies
after ``wfdb.rdsamp(path, channels=[1])`` and ``[::2]``.  Stored: the int16 frames as a WFDB format-16 ``.dat`` holds them,
the header's gains and baselines, and the float64 results -- data only, no reference text."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ECGMM_REFERENCE", "/root/reference")
LEAD = 1


def _frames(rng, n, T):
    """ECG-like 12-lead records in ADC units: beats, wander, noise; per record and lead gains, non-zero baselines"""
    t = np.arange(T) / 500.0
    gain = np.round(rng.uniform(400.0, 2000.0, size=(n, 12)), 1)
    base = rng.randint(-300, 301, size=(n, 12))
    base[base == 0] = 17
    d = np.empty((n, T, 12), dtype=np.int16)
    for r in range(n):
        phase = 2 * np.pi * rng.uniform(0.9, 1.8) * t + 0.2 * np.cumsum(rng.randn(T)) * 0.1
        beat = np.exp(8.0 * (np.cos(phase) - 1.0))
        for c in range(12):
            mv = rng.uniform(-1.5, 1.5) * beat + 0.3 * np.sin(2 * np.pi * 0.25 * t + rng.rand() * 6.28) + 0.03 * rng.randn(T)
            d[r, :, c] = np.clip(np.round(mv * gain[r, c]) + base[r, c], -32767, 32767).astype(np.int16)
    return d, gain, base


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        from evaluation_signal import preprocess_signal
    finally:
        os.chdir(cwd)
    rng = np.random.RandomState(2476)
    d, gain, base = _frames(rng, 4, 5000)
    ds, gain_s, base_s = _frames(rng, 1, 1500)
    p = (d[:, :, LEAD] - base[:, None, LEAD]) / gain[:, None, LEAD]          # wfdb's p_signal of lead II
    y = np.stack([preprocess_signal(p[r][::2]) for r in range(4)])
    ps = (ds[:, :, LEAD] - base_s[:, None, LEAD]) / gain_s[:, None, LEAD]
    y_short = np.stack([preprocess_signal(ps[0][::2])])
    assert y.shape == (4, 2476) and y.dtype == np.float64 and y_short.shape == (1, 2476)
    assert (y_short[0, 750:] == 0).all() and (d < 0).any()
    out = os.path.join(ROOT, "tests", "golden", "g10_ptbxl_preprocess.npz")
    np.savez_compressed(out, frames=d, gain=gain, baseline=base.astype(np.int32), y=y, frames_short=ds, gain_short=gain_s,
                        baseline_short=base_s.astype(np.int32), y_short=y_short, lead=np.int32(LEAD))
    print(out, os.path.getsize(out), "bytes; max |y|", np.abs(y).max())


if __name__ == "__main__":
    main()
