"""Log-spectrogram, host side: the window, the frame count and the twiddle table against scipy / float64, the C entry point's
refusals, the C-ABI table, the CPU-tensor refusal, the trainer's import.  No GPU.  Every test prints the figure it asserts on
(run with -s)."""
import ctypes

import numpy as np
import pytest
import scipy.signal
import torch

from ecgmm import spectrogram as SG
from ecgmm.hip import lib as L


def test_tukey_window_matches_scipy():
    err = np.abs(SG.tukey_window(64) - scipy.signal.get_window("tukey", 64)).max()
    print(f"tukey_window(64) vs scipy.signal.get_window: max |diff| {err:.3g}")
    assert err <= 1e-15
    w = SG.tukey_window(64)
    assert w.dtype == np.float64 and w[0] == 0.0 and abs(w.sum() - 48.0) <= 1e-12
    for M, alpha in ((64, 0.25), (64, 0.0), (64, 1.0), (63, 0.5), (16, 0.9)):
        e = np.abs(SG.tukey_window(M, alpha) - scipy.signal.get_window(("tukey", alpha), M)).max()
        print(f"tukey_window({M}, {alpha}): max |diff| {e:.3g}")
        assert e <= 1e-15


def _scipy_frames(n, hop):
    x = np.zeros(n)
    return scipy.signal.stft(x, fs=300, window="tukey", nperseg=64, noverlap=64 - hop)[2].shape[1]


_LENGTHS = [(n, 32) for n in list(range(64, 201)) + [2714, 3000, 9000, 18286, 20011]] + \
           [(n, hop) for hop in (16, 64) for n in (64, 65, 97, 127, 128, 129, 1000, 18286)]


def test_frame_count_matches_scipy():
    lib = L.lib()
    for n, hop in _LENGTHS:
        want = _scipy_frames(n, hop)
        assert SG.stft_frames(n, 64, 64 - hop) == want, (n, hop)
        assert lib.ecgmm_log_spectrogram_frames(n, 64, hop) == want, (n, hop)
    print(f"{len(_LENGTHS)} (length, hop) pairs: stft_frames and ecgmm_log_spectrogram_frames equal scipy's frame count")
    assert SG.stft_frames(9000) == 283 and SG.stft_frames(18286) == 573
    assert scipy.signal.stft(np.zeros(9000), fs=300, window="tukey", nperseg=64, noverlap=32)[2].shape[0] == 33


def test_frame_count_refusals():
    lib = L.lib()
    for args, word in (((3000, 128, 32), b"nperseg"), ((3000, 64, 0), b"hop"), ((3000, 64, 65), b"hop"),
                       ((63, 64, 32), b"length")):
        assert lib.ecgmm_log_spectrogram_frames(*args) == 0
        assert word in lib.ecgmm_last_error(), (args, lib.ecgmm_last_error())
    assert lib.ecgmm_log_spectrogram_frames(2**31 - 1, 64, 1) == 0 and b"frames" in lib.ecgmm_last_error()
    with pytest.raises(ValueError, match="nperseg"):
        SG.stft_frames(3000, nperseg=128, noverlap=64)
    with pytest.raises(ValueError, match="shorter"):
        SG.stft_frames(63)
    with pytest.raises(ValueError, match="noverlap"):
        SG.stft_frames(3000, noverlap=64)


def test_table_matches_the_float64_formula():
    for name, w in (("tukey", scipy.signal.get_window("tukey", 64)), ("hann", scipy.signal.get_window("hann", 64))):
        got = SG.stft_table("tukey" if name == "tukey" else w)
        assert got.shape == (33, 64, 2) and got.dtype == np.float64
        k, j = np.arange(33)[:, None], np.arange(64)[None, :]
        ref = (w / w.sum())[None, :] * np.exp(-2j * np.pi * j * k / 64)
        err = max(np.abs(got[..., 0] - ref.real).max(), np.abs(got[..., 1] - ref.imag).max())
        print(f"stft_table({name}) vs w / sum(w) * exp(-2 pi i j k / 64): max |diff| {err:.3g}")
        # the reference's argument 2 pi j k / 64 reaches 198 unreduced: half an ulp of it (1.4e-14) moves cos / sin by as
        # much, times the largest w / sum(w) = 1 / 32 (hann) -> 4.4e-16; the table reduces j k mod 64 in integers first
        assert err <= 1e-15
        # and the table IS scipy's transform: Z = table . frame for a random frame
        x = np.random.RandomState(3).randn(64)
        z_ref = np.fft.rfft(w * x) / w.sum()
        z = (got[..., 0] @ x) + 1j * (got[..., 1] @ x)
        assert np.abs(z - z_ref).max() <= 1e-15


def test_window_argument_refusals():
    with pytest.raises(ValueError, match="window"):
        SG.stft_table("hann")
    with pytest.raises(ValueError, match="coefficients"):
        SG.stft_table(np.ones(32))
    with pytest.raises(ValueError, match="non-zero sum"):
        SG.stft_table(np.zeros(64))


def test_entry_point_refuses_on_the_host_with_the_named_word():
    lib = L.lib()
    p = ctypes.c_void_p(256)       # never dereferenced: every refusal comes before the launch
    T = lib.ecgmm_log_spectrogram_frames(3000, 64, 32)
    assert T == 95
    cases = [("nperseg != 64", (p, 2, 3000, p, 128, 32, p, T, None), b"nperseg"),
             ("hop = 0", (p, 2, 3000, p, 64, 0, p, T, None), b"hop"),
             ("hop = 65", (p, 2, 3000, p, 64, 65, p, T, None), b"hop"),
             ("L = 63", (p, 2, 63, p, 64, 32, p, 3, None), b"length"),
             ("wrong T", (p, 2, 3000, p, 64, 32, p, T + 1, None), b"frames"),
             ("null x", (None, 2, 3000, p, 64, 32, p, T, None), b"null"),
             ("null table", (p, 2, 3000, None, 64, 32, p, T, None), b"null"),
             ("null out", (p, 2, 3000, p, 64, 32, None, T, None), b"null"),
             ("S = 0", (p, 0, 3000, p, 64, 32, p, T, None), b"S >= 1")]
    for what, args, word in cases:
        rc = lib.ecgmm_log_spectrogram(*args)
        msg = lib.ecgmm_last_error()
        print(f"{what}: code {rc}, {msg.decode()}")
        assert rc != 0 and word in msg, what


def test_symbols_are_declared_bound_and_exported():
    for name in ("ecgmm_log_spectrogram_frames", "ecgmm_log_spectrogram"):
        assert name in L.SIGNATURES and name in L.LATER_SYMBOLS
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)


def test_cpu_tensors_are_refused():
    x = torch.zeros(2, 3000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SG.compute_log_spectrogram(x)


def test_trainer_imports_without_a_gpu():
    from ecgmm import train_physionet as TP
    from ecgmm import train_physionet2 as T2
    assert T2.load_records is TP.load_records and T2.split_indices is TP.split_indices and T2.LABEL_MAP is TP.LABEL_MAP
    for name in ("build_spectrograms", "SpectrogramDataset", "DeviceSpectrogramLoader", "get_spectrogram_dataloaders", "main"):
        assert callable(getattr(T2, name))
    with pytest.raises(ValueError, match="fewer than"):
        T2.build_spectrograms([np.zeros(3000), np.zeros(40)], "cpu")
