"""Log-spectrogram of the reference's train_physionet2.py:30-34 on the device:
``np.log1p(np.abs(scipy.signal.stft(signal, fs, window, nperseg, noverlap)[2]))`` for a whole batch of records in one launch
(csrc/spectrogram.hip).  scipy's defaults are part of the definition: the periodic Tukey(0.5) window, ``boundary='zeros'``
(``nperseg / 2`` zeros in front and behind), ``padded=True`` (the tail zero-padded to a whole number of hops), the one-sided
spectrum scaled by ``1 / sum(window)``.  The window and the DFT twiddles reach the kernel as one host-built table, so nothing
here needs scipy at run time.

A record zero-padded at the end gives its own spectrogram followed by exact zeros (``log1p(0) = 0``), so one launch over a
zero-padded ``[S, Lmax]`` array is "STFT per record, then ``np.pad`` the spectrogram along time" (train_physionet2.py:138-153).
"""
import numpy as np
import torch

from .hip import lib as L
from .hip.functional import _require_cuda, ptr, stream

NPERSEG = 64            # the only segment length the kernel is built for: F = NPERSEG / 2 + 1 = 33 bins
_TABLES = {}            # (window key, nperseg, device) -> [33, 64, 2] fp32 on that device


def tukey_window(M, alpha=0.5):
    """== ``scipy.signal.get_window(('tukey', alpha), M)``: the periodic (``fftbins=True``) Tukey window, i.e. the symmetric
    window of M + 1 points without its last one.  float64 [M]."""
    M = int(M)
    if M < 1:
        return np.array([], dtype=np.float64)
    if alpha <= 0:
        return np.ones(M, dtype=np.float64)
    n = np.arange(0, M + 1)
    if alpha >= 1.0:
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / M))[:-1]          # the Hann window
    width = int(np.floor(alpha * M / 2.0))
    n1, n2, n3 = n[0:width + 1], n[width + 1:M - width], n[M - width:]
    w1 = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * n1 / alpha / M)))
    w2 = np.ones(n2.shape)
    w3 = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * n3 / alpha / M)))
    return np.concatenate((w1, w2, w3))[:-1]


def _hop(nperseg, noverlap):
    nperseg, noverlap = int(nperseg), int(noverlap)
    if nperseg != NPERSEG:
        raise ValueError(f"log-spectrogram: nperseg={nperseg} is not supported; the kernel is built for nperseg={NPERSEG} "
                         "(33 frequency bins, what the CRNN takes)")
    if not 0 <= noverlap < nperseg:
        raise ValueError(f"log-spectrogram: noverlap={noverlap} must be in 0..{nperseg - 1} (scipy: noverlap < nperseg)")
    return nperseg - noverlap


def stft_frames(L_, nperseg=NPERSEG, noverlap=32):
    """Number of STFT frames scipy returns for a record of ``L_`` samples: ``ceil(L_ / hop) + 1``, hop = nperseg - noverlap."""
    hop = _hop(nperseg, noverlap)
    if L_ < nperseg:
        raise ValueError(f"log-spectrogram: a record of {L_} samples is shorter than nperseg={nperseg}; scipy would shrink "
                         "the segment (another number of bins) or raise, here the length is refused")
    return -(-int(L_) // hop) + 1


def _window(window, nperseg):
    if isinstance(window, str):
        if window != "tukey":
            raise ValueError(f"log-spectrogram: window {window!r} is not known by name; pass 'tukey' (the reference's) or an "
                             f"array of {nperseg} coefficients")
        return tukey_window(nperseg, 0.5)
    w = np.asarray(window, dtype=np.float64)
    if w.shape != (nperseg,):
        raise ValueError(f"log-spectrogram: a window array must have nperseg={nperseg} coefficients, got shape {w.shape}")
    if not np.isfinite(w).all() or w.sum() == 0:
        raise ValueError("log-spectrogram: the window must be finite with a non-zero sum (the spectrum is scaled by 1 / sum)")
    return w


def stft_table(window="tukey", nperseg=NPERSEG):
    """The kernel's operand in float64: ``table[k, j] = w[j] / sum(w) * (cos, -sin)(2 pi j k / nperseg)``, [F, nperseg, 2]."""
    w = _window(window, nperseg)
    k = np.arange(nperseg // 2 + 1)[:, None]
    j = np.arange(nperseg)[None, :]
    ang = 2.0 * np.pi * ((j * k) % nperseg) / nperseg       # the argument reduced exactly, in integers
    scale = (w / w.sum())[None, :]
    return np.stack((scale * np.cos(ang), -scale * np.sin(ang)), axis=-1)


def _device_table(window, nperseg, device):
    key = (window if isinstance(window, str) else _window(window, nperseg).tobytes(), nperseg, str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(stft_table(window, nperseg).astype(np.float32)).to(device).contiguous()
    return _TABLES[key]


def compute_log_spectrogram(signal, fs=300, window="tukey", nperseg=NPERSEG, noverlap=32):
    """train_physionet2.py:30-34 for a CUDA float tensor ``[..., L]`` -> ``[..., 33, T]`` fp32, T = :func:`stft_frames`.
    ``window``: 'tukey' or an array of ``nperseg`` coefficients; ``fs`` only scales scipy's axes and is unused."""
    _require_cuda(signal, "compute_log_spectrogram")
    hop = _hop(nperseg, noverlap)
    shape = signal.shape
    if signal.dim() < 1:
        raise ValueError("compute_log_spectrogram: signal must have a time axis")
    T = stft_frames(shape[-1], nperseg, noverlap)
    x = signal.reshape(-1, shape[-1]).float().contiguous()
    S, Ln = x.shape
    if S < 1:
        raise ValueError("compute_log_spectrogram: no records")
    table = _device_table(window, nperseg, x.device)
    out = torch.empty(S, nperseg // 2 + 1, T, dtype=torch.float32, device=x.device)
    L.check(L.lib().ecgmm_log_spectrogram(ptr(x), S, Ln, ptr(table), nperseg, hop, ptr(out), T, stream()), "log_spectrogram")
    return out.reshape(*shape[:-1], nperseg // 2 + 1, T)
