"""ECG signal pre-processing on the GPU with the reference's function names:
``remove_baseline_drift`` + ``lowpass_filter`` = ``preprocess_signal`` (dataset.py:81-95;
train_signal_12_af.py:19-34), optionally preceded by the per-column StandardScaler of
dataset.py:195-200.  The reference runs these per sample in DataLoader workers with numpy/scipy in
float64; here a whole batch is filtered by one HIP kernel (fp64 arithmetic, fp32 result).

Filter design is done natively on the host (no scipy at run time): digital Butterworth low-pass by
bilinear transform of the analog prototype, and ``lfilter_zi``'s steady-state initial conditions.
"""
import ctypes as C

import numpy as np
import torch

from .hip import lib as L
from .hip.functional import _PhiloxState, _Scratch, _require_cuda, check_lengths, ptr, stream
from .training import ResidentLoader


def butter_lowpass(order, wn):
    """== scipy.signal.butter(order, wn, 'low') (b, a): poles of the analog prototype on the unit circle,
    frequency pre-warping, bilinear transform with fs = 2."""
    k = np.arange(order)
    p = np.exp(1j * np.pi * (2 * k + order + 1) / (2 * order))
    fs = 2.0
    warped = 2 * fs * np.tan(np.pi * wn / fs)
    p = warped * p
    gain = warped ** order
    fs2 = 2 * fs
    p_d = (fs2 + p) / (fs2 - p)
    k_d = gain * np.real(1 / np.prod(fs2 - p))
    b = k_d * np.real(np.poly(-np.ones(order)))
    a = np.real(np.poly(p_d))
    return b, a


def butter_bandpass(order, low, high):
    """== scipy.signal.butter(order, [low, high], 'band') (b, a), 2*order + 1 coefficients each: analog low-pass prototype
    -> band-pass transform about sqrt(w1 w2) with bandwidth w2 - w1 (pre-warped edges) -> bilinear transform with fs = 2
    -> polynomial coefficients.  The steps and their order are scipy's (buttap, lp2bp_zpk, bilinear_zpk, zpk2tf)."""
    if not (0.0 < low < high < 1.0):
        raise ValueError(f"butter_bandpass: need 0 < low < high < 1 (fractions of Nyquist), got {low}, {high}")
    fs = 2.0
    p = -np.exp(1j * np.pi * np.arange(-order + 1, order, 2) / (2 * order))
    w1, w2 = 2 * fs * np.tan(np.pi * low / fs), 2 * fs * np.tan(np.pi * high / fs)
    bw, wo = w2 - w1, np.sqrt(w1 * w2)
    p_lp = p * bw / 2
    root = np.sqrt(p_lp.astype(complex) ** 2 - wo ** 2)
    p_bp = np.concatenate((p_lp + root, p_lp - root))
    z_bp = np.zeros(order)
    k_bp = bw ** order
    fs2 = 2 * fs
    z_d = np.append((fs2 + z_bp) / (fs2 - z_bp), -np.ones(order))
    p_d = (fs2 + p_bp) / (fs2 - p_bp)
    k_d = k_bp * np.real(np.prod(fs2 - z_bp) / np.prod(fs2 - p_bp))
    b = k_d * np.real(np.poly(z_d))
    a = np.real(np.poly(p_d))
    return b, a


def filter_zscore(x, b, a, zscore=True, eps=1e-8):
    """z_score_normalize(scipy.signal.filtfilt(b, a, x)) per record of a CUDA float tensor [..., L] in one launch (fp64
    arithmetic, fp32 result; train_physionet.py:23-45).  Orders 1..8 (up to 9 coefficients); ``zscore=False`` stops after
    the filter.  A record must fit one CU's LDS: L <= 19904 - 3*(len(b) + len(a)) samples, longer ones are refused."""
    _require_cuda(x, "filter_zscore")
    b, a = np.atleast_1d(np.asarray(b, dtype=np.float64)), np.atleast_1d(np.asarray(a, dtype=np.float64))
    n = max(len(a), len(b))
    b, a = np.pad(b, (0, n - len(b))) / a[0], np.pad(a, (0, n - len(a))) / a[0]
    if n < 2:
        raise ValueError("filter_zscore: the transfer function needs at least two coefficients")
    zi = lfilter_zi(b, a)
    shape = x.shape
    x2 = x.reshape(-1, shape[-1]).float().contiguous()
    S, Ln = x2.shape
    out = torch.empty_like(x2)
    dbl = lambda v: (C.c_double * len(v))(*[float(t) for t in v])
    L.check(L.lib().ecgmm_signal_filter_zscore(ptr(x2), ptr(out), S, Ln, dbl(b), dbl(a), dbl(zi), n - 1, int(bool(zscore)),
                                               float(eps), stream()), "signal_filter_zscore")
    return out.reshape(shape)


def resample_len(n, ratio):
    """Samples of a record of ``n`` samples resampled by ``ratio = target_fs / orig_fs``: the library's
    ``(int)((double)n * ratio)``, which is the reference's ``int(len(signal) * (target_fs / orig_fs))``.  Needs no GPU."""
    r = L.lib().ecgmm_signal_resample_len(int(n), float(ratio))
    if r < 0:
        raise ValueError(L.lib().ecgmm_last_error().decode())
    return r


def resample(x, num=None, *, ratio=None, lengths=None):
    """``scipy.signal.resample(x, num)`` (Fourier method) per record of a CUDA float tensor [..., L]: fp64 arithmetic, fp32
    result, deterministic (csrc/resample.hip; train_physionet.py:35-39).  Exactly one of ``num`` and ``ratio``:

    ``num``                 every record goes L -> num; -> [..., num].  ``num == L`` returns the records' own bits.
    ``ratio``               every record goes L -> ``resample_len(L, ratio)``.
    ``ratio`` + ``lengths`` one length per record (``HF.check_lengths``): record s is resampled over its own first
                            ``lengths[s]`` samples (the rest of the row is never read) to ``resample_len(lengths[s], ratio)``
                            samples, followed by exact zeros; -> ([..., T_out], out_lengths int32 on the device),
                            ``T_out = resample_len(L, ratio)``.
    L and the output length are at most 65536."""
    if (num is None) == (ratio is None):
        raise ValueError("resample: give exactly one of num and ratio")
    if lengths is not None and ratio is None:
        raise ValueError("resample: lengths needs ratio (every record gets its own number of samples)")
    if x.dim() < 1 or x.shape[-1] < 1 or x.numel() < 1:
        raise ValueError(f"resample: x must be [..., L] with L >= 1 and at least one record, got {tuple(x.shape)}")
    _require_cuda(x, "resample")
    shape = x.shape
    x2 = x.reshape(-1, shape[-1]).float().contiguous()
    S, Ln = x2.shape
    if ratio is not None:
        ratio = float(ratio)
        if not (np.isfinite(ratio) and ratio > 0):
            raise ValueError(f"resample: ratio={ratio} must be finite and > 0")
        T_out = resample_len(Ln, ratio)
    else:
        T_out = int(num)
    if T_out < 1:
        raise ValueError(f"resample: the output needs at least one sample (L={Ln}, num={T_out})")
    lens = None
    if lengths is not None:
        lens = check_lengths(lengths, S, Ln).to(x2.device).contiguous()
    lib = L.lib()
    nb = lib.ecgmm_signal_resample_workspace(S, Ln, T_out)
    if nb == 0:
        raise ValueError(lib.ecgmm_last_error().decode())
    ws = _Scratch.get("resample", nb, x2.device)
    out = torch.empty(S, T_out, dtype=torch.float32, device=x2.device)
    out_len = torch.empty(S, dtype=torch.int32, device=x2.device) if lens is not None else None
    L.check(lib.ecgmm_signal_resample(ptr(x2), S, Ln, ptr(lens), 0 if lens is not None else T_out,
                                      ratio if lens is not None else 0.0, ptr(out), T_out, ptr(out_len), ptr(ws), ws.numel(),
                                      stream()), "signal_resample")
    out = out.reshape(*shape[:-1], T_out)
    return out if lens is None else (out, out_len.reshape(shape[:-1]))


def lfilter_zi(b, a):
    """== scipy.signal.lfilter_zi: initial state of the transposed direct-form-II filter for a unit step."""
    b, a = np.asarray(b, dtype=np.float64) / a[0], np.asarray(a, dtype=np.float64) / a[0]
    n = len(a)
    comp = np.zeros((n - 1, n - 1))
    comp[0] = -a[1:]
    comp[1:, :-1] = np.eye(n - 2)
    return np.linalg.solve(np.eye(n - 1) - comp.T, b[1:] - a[1:] * b[0])


def preprocess_signal(raw_signal, window_size=200, cutoff=0.05, fs=1.0, order=5, scaler_mean=None, scaler_scale=None):
    """raw_signal: CUDA float tensor [..., L] (e.g. [B, L] or [B, leads, L]); returns the same shape, float32."""
    _require_cuda(raw_signal, "preprocess_signal")
    shape = raw_signal.shape
    x = raw_signal.reshape(-1, shape[-1]).float().contiguous()
    S, Ln = x.shape
    b, a = butter_lowpass(order, cutoff / (0.5 * fs))
    zi = lfilter_zi(b, a)
    out = torch.empty_like(x)
    lib = L.lib()
    nb = lib.ecgmm_signal_preprocess_workspace(S, Ln, order)
    ws = _Scratch.get("preprocess", nb, x.device)
    dbl = lambda v: (C.c_double * len(v))(*[float(t) for t in v])
    sm = None if scaler_mean is None else torch.as_tensor(scaler_mean, dtype=torch.float32, device=x.device).contiguous()
    ss = None if scaler_scale is None else torch.as_tensor(scaler_scale, dtype=torch.float32, device=x.device).contiguous()
    L.check(lib.ecgmm_signal_preprocess(ptr(x), ptr(out), S, Ln, ptr(sm), ptr(ss), int(window_size), dbl(b), dbl(a),
                                        dbl(zi), int(order), ptr(ws), ws.numel(), stream()), "signal_preprocess")
    return out.reshape(shape)


def remove_baseline_drift(signal, window_size=200):
    """signal - moving average ('same' convolution): the first half of preprocess_signal (order-1 pass-through
    is not expressible, so this helper runs the kernel with an identity filter b=[1,0], a=[1,0])."""
    _require_cuda(signal, "remove_baseline_drift")
    shape = signal.shape
    x = signal.reshape(-1, shape[-1]).float().contiguous()
    S, Ln = x.shape
    out = torch.empty_like(x)
    lib = L.lib()
    ws = _Scratch.get("preprocess", lib.ecgmm_signal_preprocess_workspace(S, Ln, 1), x.device)
    one = (C.c_double * 2)(1.0, 0.0)
    zi = (C.c_double * 1)(0.0)
    L.check(lib.ecgmm_signal_preprocess(ptr(x), ptr(out), S, Ln, None, None, int(window_size), one, one, zi, 1,
                                        ptr(ws), ws.numel(), stream()), "remove_baseline_drift")
    return out.reshape(shape)


def preprocess_i16(raw, channels, gain, baseline, step=2, out_len=None, window_size=200, cutoff=40, fs=250, order=5):
    """WFDB format-16 frames -> the PTB-XL trainer's rows in one launch (train_signal_only_ptb.py:40-53): per record and
    channel ``rdsamp`` decode ``(d - baseline) / gain`` in float64 (-32768 -> NaN) -> ``[::step]`` -> remove_baseline_drift
    -> lowpass_filter(cutoff, fs, order) -> ``[:out_len]`` or zero padding up to ``out_len``.

    raw: CUDA int16 [R, T, nsig], the ``.dat`` payloads as on disk; channels: up to 16 signal numbers; gain (float64) and
    baseline (int) [R, len(channels)], host or device.  -> fp32 [R, len(channels), out_len] (default: all ceil(T / step))."""
    _require_cuda(raw, "preprocess_i16")
    if raw.dtype != torch.int16 or raw.dim() != 3 or not raw.is_contiguous():
        raise ValueError("preprocess_i16: raw must be a contiguous int16 [R, T, nsig] tensor")
    R, T, nsig = raw.shape
    chan = [int(c) for c in channels]
    nc = len(chan)
    if not 1 <= nc <= 16:
        raise ValueError(f"preprocess_i16: 1 to 16 channels per launch, got {nc}")
    step = int(step)
    if step < 1:
        raise ValueError(f"preprocess_i16: step must be >= 1, got {step}")
    out_len = -(-T // step) if out_len is None else int(out_len)
    g = torch.as_tensor(np.asarray(gain.cpu() if torch.is_tensor(gain) else gain, dtype=np.float64)).reshape(-1)
    bl = torch.as_tensor(np.asarray(baseline.cpu() if torch.is_tensor(baseline) else baseline).astype(np.int32)).reshape(-1)
    if g.numel() != R * nc or bl.numel() != R * nc:
        raise ValueError(f"preprocess_i16: gain and baseline must hold {R} x {nc} entries")
    if not bool(torch.isfinite(g).all()) or bool((g == 0).any()):
        raise ValueError("preprocess_i16: gains must be finite and non-zero")
    g, bl = g.to(raw.device).contiguous(), bl.to(raw.device).contiguous()
    b, a = butter_lowpass(order, cutoff / (0.5 * fs))
    zi = lfilter_zi(b, a)
    out = torch.empty(R, nc, max(out_len, 1), dtype=torch.float32, device=raw.device)
    dbl = lambda v: (C.c_double * len(v))(*[float(t) for t in v])
    L.check(L.lib().ecgmm_signal_preprocess_i16(ptr(raw), R, T, nsig, (C.c_int * nc)(*chan), nc, ptr(g), ptr(bl), step,
                                                ptr(out), out_len, int(window_size), dbl(b), dbl(a), dbl(zi), int(order),
                                                stream()), "signal_preprocess_i16")
    return out


def weight_cdf(weights):
    """Checks of ``torch.multinomial`` (no negative, non-finite or all-zero weights) -> (float64 inclusive prefix sum,
    last index of positive weight)."""
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
    if w.size < 1:
        raise ValueError("weighted_sample: no weights")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weighted_sample: weights must be finite and non-negative (invalid multinomial distribution)")
    if not (w > 0).any():
        raise ValueError("weighted_sample: the weights sum to 0 (invalid multinomial distribution)")
    cdf = np.cumsum(w)
    if not np.isfinite(cdf[-1]):
        raise ValueError("weighted_sample: the sum of the weights is not finite")
    return cdf, int(np.nonzero(w > 0)[0][-1])


def weighted_sample(cdf, last_positive, count, seed_offset=None, return_uniforms=False):
    """``count`` indices drawn with replacement, P(j) proportional to weight j, in one launch.  cdf: CUDA float64 [n] from
    :func:`weight_cdf`.  Randomness: the Philox stream of ``ecgmm.hip.functional`` advanced by one counter block per call,
    or ``seed_offset=(seed, offset)``.  -> int64 [count] on the device (and the float64 uniforms the draws used)."""
    _require_cuda(cdf, "weighted_sample")
    if cdf.dtype != torch.float64 or cdf.dim() != 1 or not cdf.is_contiguous():
        raise ValueError("weighted_sample: cdf must be a contiguous float64 vector")
    count = int(count)
    out = torch.empty(max(count, 1), dtype=torch.int64, device=cdf.device)
    u = torch.empty(max(count, 1), dtype=torch.float64, device=cdf.device) if return_uniforms else None
    seed, off = _PhiloxState.take(1) if seed_offset is None else seed_offset
    L.check(L.lib().ecgmm_weighted_sample(ptr(cdf), cdf.numel(), int(last_positive), ptr(out), ptr(u), count, int(seed),
                                          int(off), stream()), "weighted_sample")
    return (out, u) if return_uniforms else out


def gather_augment(src, index, augment=False, p=0.5, sigma=0.01, scale=(0.8, 1.2), shift=(-10, 10),
                   return_decisions=False, seed_offset=None, check_index=True):
    """``out[i] = augment_signal(src[index[i]])`` in one launch; ``augment=False`` is the plain gather.

    src: CUDA fp32 [n, L]; index: int64 [B], on the host (checked there, then uploaded) or on the device (checked with one
    device read unless ``check_index=False``).  Randomness comes from the Philox stream of ``ecgmm.hip.functional``
    (``manual_seed``), advanced by one counter block per call; ``seed_offset=(seed, offset)`` pins it instead.
    -> out [B, L] (and the decision record [B, 4]: noise flag, scale or 1, shift or 0, decisions as bits 1 / 2 / 4)."""
    _require_cuda(src, "gather_augment")
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("gather_augment: src must be a contiguous float32 [n, L] tensor")
    index = torch.as_tensor(index)
    if index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
        raise ValueError("gather_augment: index must be a non-empty int64 vector")
    n, Ln = src.shape
    if check_index:
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= n:
            raise IndexError(f"gather_augment: index range [{lo}, {hi}] outside the {n} rows of src")
    index = index.to(src.device).contiguous()
    B = index.numel()
    out = torch.empty(B, Ln, dtype=torch.float32, device=src.device)
    dec = torch.empty(B, 4, dtype=torch.float32, device=src.device) if return_decisions else None
    seed, off = (0, 0)
    if augment:
        seed, off = _PhiloxState.take(1) if seed_offset is None else seed_offset
    L.check(L.lib().ecgmm_signal_gather_augment(ptr(src), n, Ln, ptr(index), B, ptr(out), ptr(dec), int(bool(augment)),
                                                float(p), float(sigma), float(scale[0]), float(scale[1]), int(shift[0]),
                                                int(shift[1]), int(seed), int(off), stream()), "signal_gather_augment")
    return (out, dec) if return_decisions else out


class PTBXLLoader(ResidentLoader):
    """Batches ``(signals [B, leads, length], labels [B])`` of a dataset whose ``signals`` [n, leads, length] fp32 and
    ``labels`` [n] are resident on the device (``PTBXLSignalDataset``, ``DigitizedECGDataset``), one plain gather launch each.
    Under a ``sampler`` the epoch has ``len(sampler)`` samples and ``last_order`` holds the indices it drew."""

    def __init__(self, dataset, batch_size=16, shuffle=False, generator=None, drop_last=False, sampler=None):
        super().__init__(dataset, batch_size, shuffle, generator, drop_last, sampler)

    def batch(self, idx):
        ds = self.dataset
        x = gather_augment(ds.signals.view(len(ds), -1), idx, augment=False, check_index=False)
        return x.view(idx.numel(), *ds.signals.shape[1:]), ds.labels[idx]
