"""scipy.signal.resample(x, num) (Fourier method) of a real record, restated as the two direct sums the kernels of
csrc/resample.hip evaluate, in long double (as tests/iir_ref.py does) and without any FFT:

    X[k] = sum_n x[n] e^{-2 pi i k n / N},   k < K = m // 2 + 1,   m = min(N, num)
    y[j] = (X[0] + sum_{1 <= k < K} w_k 2 Re(X[k] e^{2 pi i k j / num})) / N
    w_k = 1, except at k = m / 2 with m even: the term is 2 Re X[k] (-1)^j when num < N and
          Re X[k] cos(pi N j / num) when num > N

which is scipy's Y = rfft(x)[:m // 2 + 1] zero-extended to num // 2 + 1 bins, Y[m / 2] doubled (real part, down) or halved
(up) for even m, y = irfft(Y, num) * num / N.  The phases k n mod N are reduced in integers.  num == N is the identity."""
import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))
CHUNK = 128


def _unit(r, n):
    """cos, sin of 2 pi r / n for integer arrays r in [0, n), long double"""
    ang = (LD(2) * PI) * r.astype(LD) / LD(n)
    return np.cos(ang), np.sin(ang)


def resample_ref(x, num, dtype=LD):
    """x: real [N] -> long double [num], or rows [R, N] -> [R, num] (the rows share the twiddles)"""
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    single = x.ndim == 1
    x = np.atleast_2d(x)
    N, num = x.shape[1], int(num)
    assert x.ndim == 2 and N >= 1 and num >= 1
    if num == N:
        return x[0].copy() if single else x.copy()
    m = min(N, num)
    K = m // 2 + 1
    n = np.arange(N, dtype=np.int64)
    Xre, Xim = np.zeros((K, len(x)), dtype=dtype), np.zeros((K, len(x)), dtype=dtype)
    for k0 in range(0, K, CHUNK):
        k = np.arange(k0, min(K, k0 + CHUNK), dtype=np.int64)
        c, s = _unit((k[:, None] * n[None, :]) % N, N)
        for i, row in enumerate(x):
            Xre[k0:k0 + len(k), i] = (c * row[None, :]).sum(axis=1)
            Xim[k0:k0 + len(k), i] = -(s * row[None, :]).sum(axis=1)
    even = m % 2 == 0
    Kg = K - 1 if even else K          # bins 1 .. Kg - 1 take the general term
    kg = np.arange(1, Kg, dtype=np.int64)
    y = np.zeros((len(x), num), dtype=dtype)
    for j0 in range(0, num, CHUNK):
        j = np.arange(j0, min(num, j0 + CHUNK), dtype=np.int64)
        cg, sg = _unit((j[:, None] * kg[None, :]) % num, num) if len(kg) else (None, None)
        ce, _ = _unit(((K - 1) * j) % num, num)
        for i in range(len(x)):
            acc = np.full(len(j), Xre[0, i], dtype=dtype)
            if len(kg):
                acc = acc + LD(2) * (cg * Xre[None, kg, i] - sg * Xim[None, kg, i]).sum(axis=1)
            if even and num < N:
                acc = acc + LD(2) * Xre[K - 1, i] * np.where(j % 2 == 0, LD(1), LD(-1))
            elif even:
                acc = acc + Xre[K - 1, i] * ce
            y[i, j0:j0 + len(j)] = acc / LD(N)
    return y[0] if single else y


def resample_len(n, ratio):
    """the reference's ``int(len(signal) * (target_fs / orig_fs))`` with ``ratio`` the Python float ``target_fs / orig_fs``"""
    return int(n * ratio)


def resample_lengths_ref(x, lengths, ratio, T_out=None):
    """x [S, L] (anything behind a row's length, NaN included), lengths clamped to [0, L] -> (long double [S, T_out] with
    exact zeros from each row's own num on, int [S] of those nums); T_out defaults to resample_len(L, ratio)"""
    x = np.asarray(x, dtype=np.float64)
    S, L = x.shape
    T_out = resample_len(L, ratio) if T_out is None else T_out
    out = np.zeros((S, T_out), dtype=LD)
    nums = np.zeros(S, dtype=np.int64)
    for s in range(S):
        n = min(max(int(lengths[s]), 0), L)
        nums[s] = resample_len(n, ratio)
        if n >= 1 and nums[s] >= 1:
            out[s, :nums[s]] = resample_ref(x[s, :n], nums[s])
    return out, nums
