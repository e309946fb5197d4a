"""Fourier resampling, the part that needs no GPU: the direct-sum reference against scipy.signal.resample, the length rule
and the workspace query of the C ABI, every host refusal, the header's sampling rate and the record reader."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import savemat

from ecgmm import preprocess as PP
from ecgmm import train_physionet as TP
from ecgmm.config import Config
from ecgmm.hip import lib as L

from . import resample_bounds as RB
from . import resample_ref as RR

ERR_SHAPE = 1
# down / up / equal; m even and odd in both directions; num = 1; N = 1; primes; the PTB-XL record
REF_CASES = [(17, 9), (16, 9), (16, 8), (16, 10), (15, 20), (16, 24), (16, 25), (9, 16), (10, 10), (2, 1), (1, 3), (3, 2),
             (2, 4), (1, 1), (7, 1), (8, 1), (101, 61), (61, 101), (257, 154), (256, 307), (513, 615), (5000, 3000)]


def _rows(N, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(N).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("N,num", REF_CASES, ids=lambda v: str(v))
def test_reference_is_scipy_resample(N, num):
    from scipy.signal import resample
    x = _rows(N, 100 + N + num)
    ref = RR.resample_ref(x, num)
    sci = resample(x, num)
    assert ref.shape == sci.shape == (num,)
    bnd = RB.f64_bound(x, N, num)
    err = float(np.max(np.abs(ref.astype(np.float64) - sci)))
    print("N=%d num=%d  max |ref - scipy| %.3g  fp64 bound %.3g" % (N, num, err, bnd))
    assert err <= bnd
    if num == N:
        assert np.array_equal(ref.astype(np.float64), x)


def test_reference_simple_cases():
    x = _rows(12, 3)
    assert np.allclose(RR.resample_ref(x, 1).astype(np.float64), x.mean(), rtol=0, atol=1e-15)     # num = 1: the mean
    assert np.allclose(RR.resample_ref(np.array([2.5]), 3).astype(np.float64), 2.5, rtol=0, atol=0)   # N = 1: a constant
    c = RR.resample_ref(np.full(16, 0.75), 25).astype(np.float64)
    assert np.max(np.abs(c - 0.75)) < 1e-15
    assert np.array_equal(RR.resample_ref(np.zeros(9), 16).astype(np.float64), np.zeros(16))


def test_reference_with_lengths_is_the_reference_on_each_trimmed_row():
    rng = np.random.RandomState(8)
    x = rng.randn(6, 40)
    lengths = [0, 1, 2, 17, 40, 43]
    x_nan = x.copy()
    for s, n in enumerate(lengths):
        x_nan[s, max(min(n, 40), 0):] = np.nan
    for ratio in (0.6, 1.2):
        out, nums = RR.resample_lengths_ref(x_nan, lengths, ratio)
        assert out.shape == (6, int(40 * ratio))
        for s, n in enumerate(lengths):
            n = min(n, 40)
            num = int(n * ratio)
            assert nums[s] == num
            assert np.all(out[s, num:] == 0)
            if n >= 1 and num >= 1:
                assert np.array_equal(out[s, :num], RR.resample_ref(x[s, :n], num))
            else:
                assert np.all(out[s] == 0)


@pytest.mark.parametrize("target,orig", [(300, 500), (300, 250), (250, 300), (300, 360), (300, 1000)])
def test_resample_len_is_pythons_int(target, orig):
    lib = L.lib()
    ratio = target / orig
    n = np.arange(1, 20001)
    want = np.array([int(int(v) * (target / orig)) for v in n])
    got = np.array([lib.ecgmm_signal_resample_len(int(v), ratio) for v in n])
    assert np.array_equal(got, want)
    assert PP.resample_len(5000, 300 / 500) == 3000 and RR.resample_len(5000, 300 / 500) == 3000


def test_resample_len_refusals():
    lib = L.lib()
    for n, ratio in ((-1, 0.6), (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf")), (2 ** 30, 4.0)):
        assert lib.ecgmm_signal_resample_len(n, ratio) == -1
        assert b"signal_resample_len" in lib.ecgmm_last_error()
    assert lib.ecgmm_signal_resample_len(0, 0.6) == 0 and lib.ecgmm_signal_resample_len(1, 0.6) == 0
    with pytest.raises(ValueError, match="signal_resample_len"):
        PP.resample_len(-3, 0.6)


def test_workspace_query_without_a_gpu():
    lib = L.lib()
    assert lib.ecgmm_signal_resample_workspace(1, 1, 1) == 16
    assert lib.ecgmm_signal_resample_workspace(256, 5000, 3000) == 256 * 1501 * 16
    assert lib.ecgmm_signal_resample_workspace(3, 3000, 5000) == 3 * 1501 * 16
    assert lib.ecgmm_signal_resample_workspace(2, 65536, 65536) == 2 * 32769 * 16
    for S, Ln, T in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (1, 65537, 10), (1, 10, 65537), (-1, 10, 10)):
        assert lib.ecgmm_signal_resample_workspace(S, Ln, T) == 0
        assert b"signal_resample_workspace" in lib.ecgmm_last_error()


def test_entry_point_host_refusals():
    """every refusal returns before a launch, so made-up non-null pointers are never dereferenced"""
    lib = L.lib()
    p = C.c_void_p(4096)          # non-null, 16-byte aligned, never touched
    big = 1 << 40

    def call(x=p, S=2, Ln=100, lengths=None, num=60, ratio=0.0, out=p, T_out=60, out_lengths=None, ws=p, nb=big):
        return lib.ecgmm_signal_resample(x, S, Ln, lengths, num, ratio, out, T_out, out_lengths, ws, nb, None)

    refused = [dict(x=None), dict(out=None), dict(ws=None), dict(S=0), dict(Ln=0), dict(Ln=65537), dict(T_out=65537, num=65537),
               dict(num=0), dict(num=-3), dict(num=61), dict(T_out=0), dict(out_lengths=p), dict(nb=2 * 31 * 16 - 1), dict(nb=0),
               dict(ws=C.c_void_p(4104)),
               dict(lengths=p, num=0, ratio=0.6, T_out=59), dict(lengths=p, num=60, ratio=0.6), dict(lengths=p, num=0, ratio=0.0),
               dict(lengths=p, num=0, ratio=-0.6), dict(lengths=p, num=0, ratio=float("nan")),
               dict(lengths=p, num=0, ratio=float("inf")), dict(lengths=p, num=0, ratio=1e9, T_out=65536),
               dict(lengths=p, num=0, ratio=700.0, T_out=65536)]
    for kw in refused:
        assert call(**kw) == ERR_SHAPE, kw
        assert b"signal_resample" in lib.ecgmm_last_error(), kw


def test_python_refusals():
    x = torch.zeros(2, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.resample(x, 60)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.resample(x, ratio=0.6, lengths=[100, 50])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TP.resample_signal(x, 500, 300)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TP.preprocess_resampled(x, 500, 300)
    with pytest.raises(ValueError, match="exactly one"):
        PP.resample(x)
    with pytest.raises(ValueError, match="exactly one"):
        PP.resample(x, 60, ratio=0.6)
    with pytest.raises(ValueError, match="lengths needs ratio"):
        PP.resample(x, 60, lengths=[100, 50])
    with pytest.raises(ValueError, match="L >= 1"):
        PP.resample(torch.zeros(2, 0), 60)
    for bad in ((0, 300), (500, 0), (-500, 300), (float("nan"), 300), (500, float("inf"))):
        with pytest.raises(ValueError, match="sampling rates"):
            TP.resample_signal(x, *bad)
    with pytest.raises(NotImplementedError, match="preprocess_resampled"):
        TP.preprocess_signal(x, orig_fs=500, target_fs=300)


def test_resample_signal_at_equal_rates_returns_its_argument():
    x = torch.zeros(2, 100)          # a CPU tensor: the identity touches no device
    assert TP.resample_signal(x, 300, 300) is x
    assert TP.resample_signal(x, 500.0, 500) is x
    assert TP.resample_signal(x, 300) is x


def _write_record(dirname, name, val, fs):
    savemat(os.path.join(dirname, name + ".mat"), {"val": np.asarray(val, dtype=np.int16).reshape(1, -1)})
    with open(os.path.join(dirname, name + ".hea"), "w") as f:
        f.write(f"{name} 1 {fs} {len(val)} 2013-01-01 00:00:00\n")
        f.write(f"{name}.mat 16+24 1000/mV 16 0 {int(val[0])} 0 0 ECG\n")


def test_read_fs(tmp_path):
    val = np.arange(50)
    _write_record(tmp_path, "A1", val, 300)
    _write_record(tmp_path, "A2", val, 500)
    _write_record(tmp_path, "A3", val, "257.5/100(3)")
    np.save(tmp_path / "A4.npy", val.astype(np.float64))
    assert TP.read_fs(str(tmp_path / "A1")) == 300.0
    assert TP.read_fs(str(tmp_path / "A2")) == 500.0
    assert TP.read_fs(str(tmp_path / "A3")) == 257.5
    assert TP.read_fs(str(tmp_path / "A4")) is None and TP.read_fs(str(tmp_path / "A4.npy")) is None


def test_load_records_without_target_fs_is_unchanged(tmp_path):
    rng = np.random.RandomState(2)
    vals = {"A1": (rng.randint(-900, 900, size=700), 300, "N"), "A2": (rng.randint(-900, 900, size=810), 500, "AF"),
            "A3": (rng.randint(-900, 900, size=640), 250, "~")}
    for name, (val, fs, _) in vals.items():
        _write_record(tmp_path, name, val, fs)
    with open(tmp_path / "REFERENCE.csv", "w") as f:
        for name, (_, _, lab) in vals.items():
            f.write(f"{name},{lab}\n")
    cfg = type("Cfg", (Config,), dict(synthetic=False, physionet_data_dir=str(tmp_path),
                                      physionet_label_file=str(tmp_path / "REFERENCE.csv"), device="cpu"))
    for kw in ({}, {"target_fs": None}):
        signals, labels = TP.load_records(cfg, **kw)
        assert labels.tolist() == [0, 1] and [len(s) for s in signals] == [700, 810]
        assert np.array_equal(signals[0], vals["A1"][0] / 1000.0) and np.array_equal(signals[1], vals["A2"][0] / 1000.0)
    # a target rate every header already has: nothing is resampled, no device is touched
    only300 = type("Cfg300", (cfg,), {})
    with open(tmp_path / "REFERENCE.csv", "w") as f:
        f.write("A1,N\n")
    signals, _ = TP.load_records(only300, target_fs=300)
    assert np.array_equal(signals[0], vals["A1"][0] / 1000.0)
    assert Config.physionet_target_fs is None


def test_load_records_imports_no_hip_library():
    code = ("import sys, ecgmm.train_physionet as TP\n"
            "from ecgmm.hip import lib as L\n"
            "cfg = type('C', (TP.Config,), dict(synthetic=True, synthetic_train_size=4, synthetic_val_size=2, synthetic_test_size=2))\n"
            "s, y = TP.load_records(cfg, target_fs=None)\n"
            "assert len(s) == 8 and L._lib is None, 'load_records loaded the HIP library'\n")
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
