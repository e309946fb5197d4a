"""Accuracy contract of the Fourier resampler (csrc/resample.hip): for output element j of a row of N samples resampled to num,

    |got - ref| <= u |ref| + g64(N + 2 K + C_RESAMPLE) A + FLOOR,      K = min(N, num) // 2 + 1,
    A = ((2 K - 1) / N) sum_n |x[n]|,     g64(k) = k 2^-53 / (1 - k 2^-53),     u = 2^-24 (tests/f64check.U)

ref is the long-double direct sum of tests/resample_ref.py.  u |ref| is the one rounding of the float64 result to fp32, FLOOR
half the spacing of the fp32 subnormals (where that rounding is absolute).  The middle term is the float64 arithmetic:

  A      y[j] is a sum of 2 K - 1 real terms (X[0] and two per bin k >= 1), each a product of some x[n], one unit-modulus
         analysis twiddle, one unit-modulus synthesis twiddle, and 1 / N.  With |Re(X w)| <= |X| <= sum |x| (Cauchy-Schwarz
         on (Re X, Im X) . (cos, -sin), which also bounds the two products the kernel adds up separately) the magnitudes of
         all terms sum to at most A.  The even-m bin (2 Re X (-1)^j down, Re X cos up) counts as two terms and is at most that.
  chain  every term goes through: the analysis accumulation, N fused multiply-adds in ascending n; the synthesis
         accumulation, two fused multiply-adds per bin, 2 (K - 1); then X[0] + 2 acc, the even-m term (at most two
         roundings) and the division by N: 2 K + 2 in all.  The conversions fp32 -> fp64 and the factors 2 are exact.
  C_TW   what one twiddle adds, in units of 2^-53 of its modulus 1.  A twiddle is the product of two table entries.
         An entry is sincospi(rem / (2 N)) with integers 0 <= rem <= N / 2: the division rounds the argument (<= 1/4) once,
         which turns the point by at most (pi / 4) 2^-53; sincospi is ASSUMED to return each component within K_SINCOSPI
         ulp (one ulp of a value below 1 is at most 2^-53; quarter turns are exact), sqrt(2) K_SINCOSPI in modulus.  The
         complex product (two products and one add per component, or a fused form with fewer roundings) adds at most
         2 sqrt(2) 2^-53.  C_TW = ceil(2 (pi / 4 + sqrt(2) K_SINCOSPI) + 2 sqrt(2)).
  C_RESAMPLE = 2 C_TW + 2: one twiddle per stage, and the 2 of the chain above that N + 2 K leaves out.

K_SINCOSPI is an assumption declared by name, as K_SIG and K_LOG of tests/f64check.py are; nothing here is fitted to what
the kernel returns.  The worst ratios measured on the MI355X are recorded in DESIGN.md section 29."""
import math

import numpy as np
import torch

from .f64check import U, Report, _ratio, _unravel

U64 = 2.0 ** -53
K_SINCOSPI = 2.0             # assumed: fp64 sincospi within 2 ulp per component
C_TW = math.ceil(2.0 * (math.pi / 4.0 + math.sqrt(2.0) * K_SINCOSPI) + 2.0 * math.sqrt(2.0))
C_RESAMPLE = 2 * C_TW + 2
FLOOR = 2.0 ** -150          # half the spacing of the fp32 subnormals


def g64(k):
    """(1 + 2^-53)^k - 1 <= k 2^-53 / (1 - k 2^-53)"""
    return k * U64 / (1.0 - k * U64)


def term_sum(x, N, num):
    """A of a row: x float64 [N]"""
    K = min(N, num) // 2 + 1
    return (2 * K - 1) / N * float(np.abs(np.asarray(x, dtype=np.float64)[:N]).sum())


def f64_bound(x, N, num):
    """the float64 part of the bound: g64(N + 2 K + C_RESAMPLE) A"""
    K = min(N, num) // 2 + 1
    return g64(N + 2 * K + C_RESAMPLE) * term_sum(x, N, num)


def bound(ref, x, N, num):
    """the whole bound of one row's outputs: ref long double / float64 [num], x float64 [N] -> float64 [num]"""
    return U * np.abs(np.asarray(ref, dtype=np.float64)) + f64_bound(x, N, num) + FLOOR


def ratio_report(got, ref, bnd, name):
    """Report (tests/f64check.py) of the worst |got - ref| / bnd; the accumulation figure is the worst error beyond the fp32
    rounding u |ref| in units of the float64 part of the bound"""
    got = torch.as_tensor(np.asarray(got, dtype=np.float64))
    refd = torch.as_tensor(np.asarray(ref, dtype=np.float64))
    bnd = torch.as_tensor(np.asarray(bnd, dtype=np.float64))
    err = (got - refd).abs()
    ratio = _ratio(err, bnd)
    if ratio.numel() == 0:
        return Report(name, 0.0, ())
    flat = int(torch.argmax(ratio))
    beyond = (err - U * refd.abs()).clamp_min(0) / (bnd - U * refd.abs()).clamp_min(1e-300)
    beyond = beyond[torch.isfinite(beyond)]
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, refd.shape), float(beyond.max()) if beyond.numel() else 0.0)


def check_rows(got, refs, xs, shapes, name):
    """got [S, >= num] fp32, refs / xs: per row the reference [num_s] and the float64 samples; shapes: per row (N_s, num_s).
    Prints the report, asserts ratio <= 1, returns it."""
    worst = Report(name, 0.0, ())
    for s, (N, num) in enumerate(shapes):
        if N < 1 or num < 1:
            continue
        ref = np.asarray(refs[s])[:num]
        r = ratio_report(np.asarray(got[s])[:num], ref, bound(ref, xs[s], N, num), name)
        if r.ratio >= worst.ratio:
            worst = Report(name, r.ratio, (s,) + tuple(r.where), max(worst.kappa_seen, r.kappa_seen))
        else:
            worst.kappa_seen = max(worst.kappa_seen, r.kappa_seen)
    print(worst)
    assert worst.ok, str(worst)
    return worst
