"""Reference and bound of the filtfilt front end (csrc/preprocess.hip, csrc/physionet.hip), shared by
tests/test_iir_ref_cpu.py and tests/test_iir_f64_gpu.py.  No GPU here, and no scipy in the arithmetic: scipy designs the
filters (butter, lfilter_zi for the kernels' operands) and supplies the float64 ``filtfilt`` whose distance from the long-double
one is the reference's own noise ``d_seq``.

Reference.  ``filtfilt_ld`` is scipy.signal.filtfilt's default method in 80-bit long double: odd extension by
3 * len(a) samples, the steady-state ``lfilter_zi`` state scaled by the first sample, transposed direct form II forward,
the same on the reversed signal, crop.  ``baseline_ld`` is ``x - np.convolve(x, ones / window, 'same')`` as a difference of
long-double prefix sums, ``zscore_ld`` the population z-score.

Bound, per element of a row (u = 2^-24):

    |got - ref| <= ulp32(ref) / 2  +  max(u * max|ref row|, 16 * d_seq)

  * ulp32(ref) / 2: the fp32 store of the result;
  * u * max|ref row|: the contract -- float64 arithmetic may add at most one fp32 half-ulp at the row's scale;
  * 16 * d_seq: takes over only where the reference's own float64 (scipy's sequential direct form) is worse than that; 16 is
    the margin for another rounding order (FMA contraction, another association) over the reference's noise.

A case is REFUSABLE iff 16 * d_seq > u * min over rows of max|ref row|: there float64 itself cannot promise the contract.
Every other case must be served and must meet the bound.  None of these figures comes from what the kernels return.

``chunk_scheme_f64`` restates the kernels' chunked scheme in float64 numpy (zero-state pass, A^C from unit states, the chain,
true-state pass, C = ceil(E / nl) | 1) for any number of active lanes nl; nl = 1 is the sequential pass.  ``lane_rule`` restates
the host rule of the C entry points that picks nl from (a, E)."""
import math
from collections import namedtuple

import numpy as np
import scipy.signal

from oracle import fill

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "tests/iir_ref.py needs an extended-precision np.longdouble (eps <= 2^-63) as its reference arithmetic; this platform's "
    "long double has eps = %g" % float(np.finfo(LD).eps))
U = 2.0 ** -24
MARGIN_SEQ = 16.0


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def _norm(b, a, dtype):
    b, a = np.atleast_1d(np.asarray(b, dtype=dtype)), np.atleast_1d(np.asarray(a, dtype=dtype))
    n = max(len(a), len(b))
    b = np.concatenate([b, np.zeros(n - len(b), dtype=dtype)]) / a[0]
    a = np.concatenate([a, np.zeros(n - len(a), dtype=dtype)]) / a[0]
    return b, a


def zi_steady(b, a):
    """lfilter_zi in the dtype of b: the state of the transposed direct form II at rest under a unit step, by the recurrence
    zi[0] = (sum b[1:] - b[0] sum a[1:]) / sum a,  zi[k] = (1 + a[1] + .. + a[k]) zi[0] - sum_{j<=k} (b[j] - a[j] b[0])"""
    n = len(a)
    zi = np.zeros(n - 1, dtype=b.dtype)
    if n < 2:
        return zi
    B = b[1:] - a[1:] * b[0]
    zi[0] = B.sum() / a.sum()
    asum, csum = a[0], b.dtype.type(0)
    for k in range(1, n - 1):
        asum = asum + a[k]
        csum = csum + B[k - 1]
        zi[k] = asum * zi[0] - csum
    return zi


def _lfilter(b, a, x, z):
    """transposed direct form II along the last axis of x [R, E] from the state z [N, R] (changed in place) -> y [R, E]"""
    y = np.empty_like(x)
    b0, b1, a1 = b[0], b[1:, None], a[1:, None]
    nxt = np.zeros_like(z)
    for k in range(x.shape[1]):
        e = x[:, k]
        yk = b0 * e + z[0]
        nxt[:-1] = z[1:]
        nxt[-1] = 0
        z[...] = b1 * e + nxt - a1 * yk
        y[:, k] = yk
    return y


def _filtfilt(b, a, x, dtype, ext_shift=0, back_state_from_input=False):
    """filtfilt in ``dtype``.  The two switches make the deliberately wrong variants of tests/test_iir_ref_cpu.py: the odd
    extension reflected one sample off, and the backward pass started from zi * x_ext[0] instead of zi * forward[-1]."""
    b, a = _norm(b, a, dtype)
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    pad = 3 * len(a)
    assert x.shape[1] > pad + ext_shift, "filtfilt: the record must be longer than padlen = 3 * len(a)"
    s = ext_shift
    left = 2 * x[:, :1] - x[:, pad + s:s:-1]
    right = 2 * x[:, -1:] - x[:, -2 - s:-pad - 2 - s:-1]
    ext = np.concatenate([left, x, right], axis=1)
    zi = zi_steady(b, a)[:, None]
    f = _lfilter(b, a, ext, zi * ext[None, :, 0])
    start = ext[None, :, 0] if back_state_from_input else f[None, :, -1]
    g = _lfilter(b, a, np.ascontiguousarray(f[:, ::-1]), zi * start)
    return g[:, ::-1][:, pad:-pad]


def filtfilt_ld(b, a, x, keep_ld=False):
    """scipy.signal.filtfilt(b, a, x, axis=-1) (default padding and method) in long double, vectorised over the rows of x
    [R, L] (float64 or long double in); float64 out unless ``keep_ld``."""
    y = _filtfilt(b, a, x, LD)
    return y if keep_ld else y.astype(np.float64)


def baseline_ld(x, window, shift=0):
    """x - np.convolve(x, ones(window) / window, 'same') per row, long double in and out: the window of element i is
    [i - bk, i + fw] with fw = (window - 1) // 2, bk = window - 1 - fw, zeros outside the record.  ``shift`` moves the window
    (the wrong variant of the CPU test)."""
    x = np.atleast_2d(np.asarray(x, dtype=LD))
    Ln = x.shape[1]
    fw = (window - 1) // 2
    bk = window - 1 - fw
    cs = np.concatenate([np.zeros((x.shape[0], 1), dtype=LD), np.cumsum(x, axis=1)], axis=1)
    i = np.arange(Ln) + shift
    hi = np.clip(i + fw + 1, 0, Ln)
    lo = np.clip(i - bk, 0, Ln)
    return x - (cs[:, hi] - cs[:, lo]) / LD(window)


def zscore_ld(y, eps=1e-8):
    """(y - mean) / (std + eps) per row with the population standard deviation, long double in and out"""
    y = np.atleast_2d(np.asarray(y, dtype=LD))
    m = y.mean(axis=1, keepdims=True)
    sd = np.sqrt(((y - m) ** 2).mean(axis=1, keepdims=True))
    return (y - m) / (sd + LD(eps))


# ---------------------------------------------------------------------------------------------------------------------
# bound
# ---------------------------------------------------------------------------------------------------------------------
def ratio(err, bound):
    """worst err / bound (the convention of tests/attn_bounds.ratio): an element whose bound is 0 must be exact, and a NaN /
    inf error is infinitely bad"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def half_ulp32(ref):
    r32 = np.abs(np.asarray(ref, dtype=np.float64)).astype(np.float32)
    return 0.5 * np.spacing(r32).astype(np.float64)


def bound(ref, dseq):
    """the per-element bound of the module docstring for ref [R, L] (float64)"""
    ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    row = np.abs(ref).max(axis=1, keepdims=True)
    return half_ulp32(ref) + np.maximum(U * row, MARGIN_SEQ * dseq)


def refusable(ref, dseq):
    ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    return bool(MARGIN_SEQ * dseq > U * np.abs(ref).max(axis=1).min())


def worst(got, ref, dseq):
    """worst |got - ref| / bound over all elements"""
    ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    return ratio(np.abs(got - ref), bound(ref, dseq))


# ---------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------
Design = namedtuple("Design", "name kind order wn b a N")      # N = len(a) - 1, the order the kernels are instantiated on
LOW_WN = (0.02, 0.04, 0.1, 0.32)
BAND_WIDE = (16 / 150, 149 / 150)
BAND_NARROW = (0.02, 0.06)
LENGTHS = ("min", 250, 1000, 5000)      # E < 64 so C = 1; then C = 5, 17 and about 79 at 64 lanes


def _design(kind, order, wn):
    b, a = scipy.signal.butter(order, wn, "low" if kind == "low" else "band")
    if kind == "low":
        name = "low%d_wn%g" % (order, wn)
    else:
        name = "band%d_%s" % (order, "wide" if wn == BAND_WIDE else "narrow")
    return Design(name, kind, order, wn, np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64), len(a) - 1)


def designs():
    out = [_design("low", o, w) for o in range(1, 9) for w in LOW_WN]
    out += [_design("band", o, BAND_WIDE) for o in range(1, 5)]
    out += [_design("band", o, BAND_NARROW) for o in range(2, 5)]
    return out


def find(name):
    return next(d for d in designs() if d.name == name)


def length(design, Ln):
    return 3 * (design.N + 1) + 1 if Ln == "min" else int(Ln)


def rows(Ln, salt, n=3):
    """the grid's records [n, Ln], fp32: the project's hash noise on a slow sine"""
    x = fill.hash_tensor((n, Ln), salt, 1.0).numpy().astype(np.float64)
    x += 0.5 * np.sin(np.arange(Ln) / 37.0 + np.arange(n)[:, None])
    return x.astype(np.float32)


Ref = namedtuple("Ref", "x ref dseq refusable")


def case_ref(design, x32, window=None, zscore=False, eps=1e-8, x64=None):
    """Long-double reference of one call on the fp32 rows x32 (or the float64 rows x64, for decoded int16 frames), the
    float64 noise d_seq of the same pipeline with scipy / numpy, and whether the case is refusable.
    window: the moving-average baseline in front (the preprocess entry points); zscore: behind (filter_zscore)."""
    x = np.atleast_2d(np.asarray(x32, dtype=np.float64) if x64 is None else np.asarray(x64, dtype=np.float64))
    u_ld, u64 = x.astype(LD), x
    if window is not None:
        u_ld = baseline_ld(x, window)
        u64 = np.stack([r - np.convolve(r, np.ones(window) / window, mode="same") for r in x])
    y_ld = _filtfilt(design.b, design.a, u_ld, LD)
    y64 = scipy.signal.filtfilt(design.b, design.a, u64, axis=-1)
    if zscore:
        y_ld = zscore_ld(y_ld, eps)
        y64 = (y64 - y64.mean(-1, keepdims=True)) / (y64.std(-1, keepdims=True) + eps)
    ref = y_ld.astype(np.float64)
    dseq = float(np.abs(y64.astype(LD) - y_ld).max())
    return Ref(x32, ref, dseq, refusable(ref, dseq))


def grid():
    """[(design, Ln, salt)]: 39 designs x 4 lengths"""
    out = []
    for i, d in enumerate(designs()):
        for j, Ln in enumerate(LENGTHS):
            out.append((d, length(d, Ln), 7000 + 10 * i + j))
    return out


_GRID_REFS = {}


def grid_ref(design, Ln, salt):
    """the filter-only reference of a grid case, computed once per process"""
    key = (design.name, Ln, salt)
    if key not in _GRID_REFS:
        _GRID_REFS[key] = case_ref(design, rows(Ln, salt))
    return _GRID_REFS[key]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' scheme in float64 numpy
# ---------------------------------------------------------------------------------------------------------------------
def _power_unit_states(a, C):
    """A^C as the kernels build it: column j = C zero-input steps from the unit state e_j"""
    N = len(a) - 1
    z = np.eye(N)                      # z[i, j]: state i of column j
    for _ in range(C):
        y = z[0].copy()
        nxt = np.vstack([z[1:], np.zeros((1, N))])
        z = nxt - a[1:, None] * y
    return z


def _chunk_pass(b, a, zi, B, nl, M):
    """one direction over B [R, E] in place"""
    R, E = B.shape
    N = len(a) - 1
    C = (-(-E // nl)) | 1
    nch = -(-E // C)
    full = E // C                       # chunks that hand a state on
    st = np.zeros((nch, N, R))
    b0, b1, a1 = b[0], b[1:, None, None], a[1:, None, None]

    def run(z, chunks, write):
        # z [N, chunks, R]; all chunks step together
        for k in range(C):
            idx = np.arange(chunks) * C + k
            ok = idx < E
            e = np.zeros((chunks, R))
            e[ok] = B[:, idx[ok]].T
            y = b0 * e + z[0]
            nxt = np.concatenate([z[1:], np.zeros((1, chunks, R))])
            znew = b1 * e + nxt - a1 * y
            z = np.where(ok[None, :, None], znew, z)
            if write:
                B[:, idx[ok]] = y[ok].T
        return z

    if nl > 1:
        zend = run(np.zeros((N, full, R)), full, False)
        st[:full] = zend.transpose(1, 0, 2)
    z = zi[:, None] * B[:, 0][None, :]
    entry = np.zeros((nch, N, R))
    for t in range(nch):
        entry[t] = z
        if nl > 1:
            acc = st[t].copy()
            for j in range(N):          # acc += m[i][j] * z[j], j ascending, as the kernels accumulate
                acc = acc + M[:, j][:, None] * z[j][None, :]
            z = acc
    run(entry.transpose(1, 0, 2).copy(), nch, True)


def chunk_scheme_f64(b, a, zi, u, nl=64):
    """The chunked filtfilt of signal_preprocess_lds_kernel / signal_filter_zscore_kernel in float64 numpy on u [R, L]
    (float64, baseline already removed) with nl active lanes; zi as the kernels receive it (scipy.signal.lfilter_zi)."""
    b, a = _norm(b, a, np.float64)
    zi = np.asarray(zi, dtype=np.float64)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    N = len(a) - 1
    pad = 3 * (N + 1)
    R, Ln = u.shape
    B = np.empty((R, Ln + 2 * pad))
    B[:, pad:pad + Ln] = u
    k = np.arange(pad)
    B[:, k] = 2.0 * B[:, pad:pad + 1] - B[:, pad + (pad - k)]
    B[:, pad + Ln + k] = 2.0 * B[:, pad + Ln - 1:pad + Ln] - B[:, pad + Ln - 2 - k]
    E = B.shape[1]
    C = (-(-E // nl)) | 1
    M = _power_unit_states(a, C) if nl > 1 else None
    _chunk_pass(b, a, zi, B, nl, M)
    Brev = np.ascontiguousarray(B[:, ::-1])
    _chunk_pass(b, a, zi, Brev, nl, M)
    return Brev[:, ::-1][:, pad:pad + Ln]


# ---------------------------------------------------------------------------------------------------------------------
# the host rule of the C entry points, restated
# ---------------------------------------------------------------------------------------------------------------------
LANES = (64, 32, 16, 8, 4, 2)
RULE_K = 8.0           # see DESIGN "Lane rule": predicted relative error = RULE_K * 2^-53 * G * P(nl)
RULE_MARGIN = 8.0


def growth(a, E, lanes=LANES):
    """G = max over 0 <= k <= E of max|A^k| and P[nl] = max|A^C(nl)|, C(nl) = ceil(E / nl) | 1, with A the zero-input
    transition of the transposed direct form II, all in float64 from the unit states, as the host computes them"""
    a = np.asarray(a, dtype=np.float64) / a[0]
    N = len(a) - 1
    want = {nl: (-(-E // nl)) | 1 for nl in lanes}
    z = np.eye(N)
    G, P = 1.0, {}
    for k in range(1, E + 1):
        y = z[0].copy()
        z = np.vstack([z[1:], np.zeros((1, N))]) - a[1:, None] * y
        m = float(np.abs(z).max())
        if not math.isfinite(m):
            m = math.inf
        G = max(G, m)
        for nl, C in want.items():
            if C == k:
                P[nl] = m
    for nl, C in want.items():
        P.setdefault(nl, math.inf)      # C > E cannot happen for nl >= 2 and E >= 2; kept total
    return G, P


def predicted(G, P):
    return RULE_K * 2.0 ** -53 * G * P


def lane_rule(a, E):
    """the largest nl whose predicted relative error stays RULE_MARGIN below 2^-24, else 1 (the sequential pass)"""
    G, P = growth(a, E)
    for nl in LANES:
        if predicted(G, P[nl]) * RULE_MARGIN <= U:
            return nl
    return 1
