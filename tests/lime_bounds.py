"""Error bounds of csrc/lime.hip against tests/lime_ref.py, derived in the manner of tests/f64check.py:
u = 2^-24, g_K = K u / (1 - K u).  Every bound is the derived worst case; none is fitted to what the kernels give.

Assumed constants (named, not derived): the fp64 library functions of the device (exp, normcdf, normcdfinv) and the fp64
sums of up to a few thousand terms are taken to be accurate to E_FUNC = 2^-46 relative -- 128 ulp of fp64, two decimal
orders above what such functions deliver, and 2^-22 of the fp32 rounding next to which it always stands.

Perturbation value  x = fl32(mean + std * z), z = Phi^-1(q), q = Phi(a) + u (Phi(b) - Phi(a)):
    an absolute error dq in q moves z by dq / phi(z); q <= 1 and is known to E_FUNC, so
    |x - ref| <= u |ref|                                     the fp32 rounding of the result
                 + std * E_FUNC / phi(z)                      the function error carried through the inverse CDF
                 + E_FUNC (|mean| + std |z|)                  the final fp64 operations
                 + u max(|min|, |max|)                        ONLY where the stored value is one of the clamp limits
                                                              fl32(min), fl32(max), which may lie that far from min, max

Weights  w = fl32(exp(-d2 / (2 kw^2))) evaluated in fp64:  |w - ref| <= (u + E_FUNC (1 + d2 / (2 kw^2))) ref

Ridge, per sample and label.  With G = Z^T W Z, s = Z^T w, A = G - s s^T / W + alpha I, b = Zc^T W yc (float64, rebuilt from
the device's own Z, stored w and y), the device forms
    A^ = fl32(G^ - s s^T / W + alpha I),  G^ the fp32 MFMA accumulation of exact products over N (any order):
        |A^ - A| <= dA = g_N G + u (|A| + g_N G) + E_FUNC (G + s s^T / W)
    (the centring is a rank-one correction in fp64 AFTER the Gram, so the Gram error g_N G enters uncentred: that is the
    price of exact products, and it is what the bound carries)
    b^ = fl32(b in fp64):  |b^ - b| <= db = u |b| + E_FUNC (Z^T W |y| + s |ybar|)
and solves A^ x = b^ by Cholesky and two triangular solves in fp32, for which (Higham, Accuracy and Stability, Thm 10.3 and
10.4)  (A^ + dA2) beta^ = b^,  |dA2| <= g_{3K+1} |R^T| |R|  (g_{K+1} |R^T||R| for the factorisation plus g_K |R^T||R| per
triangular solve, to first order; R from the float64 factor).  Hence componentwise
    |A beta^ - b| <= rb = (dA + g_{3K+1} |R^T||R|) |beta^| + db
    |beta^ - beta| <= fb = |A^-1| rb
and, with m = s / W, evaluated by the device in fp64 from the stored beta^ and rounded once:
    intercept = ybar - m . beta:      m . fb + u |intercept| + E_FUNC (|ybar| + m . |beta^|)
    local_pred = intercept + sum beta: |1 - m| . fb + u |local_pred| + E_FUNC (|ybar| + (1 + m) . |beta^|)
    score = 1 - res / tot, pred_n = intercept + z_n . beta so |dpred| <= dp = |Zc| fb:
        (sum_n w (2 |y - pred| dp + dp^2)) / tot + u |score| + E_FUNC (1 + res / tot)
"""
import numpy as np

U = 2.0 ** -24
E_FUNC = 2.0 ** -46


def g_k(K):
    return K * U / (1.0 - K * U)


def ratio(err, bound):
    """worst err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def value_bound(ref, z, mean, std, lo, hi, clamped):
    """clamped: the elements whose stored value equals one of the fp32 clamp limits"""
    phi = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    with np.errstate(divide="ignore", over="ignore"):
        carried = np.where(std <= 1e-11, 0.0, std * E_FUNC / phi)
    clamp = np.where(clamped, U * np.maximum(np.abs(lo), np.abs(hi)), 0.0)
    return U * np.abs(ref) + carried + E_FUNC * (np.abs(mean) + std * np.abs(z)) + clamp


def weight_bound(ref, d2, kernel_width):
    return (U + E_FUNC * (1.0 + np.asarray(d2, dtype=np.float64) / (2 * kernel_width ** 2))) * ref


class RidgeBounds:
    """the bounds above for one sample; ref: lime_ref.RidgeRef (float64), beta_hat [L, K] the coefficients under test"""

    def __init__(self, ref, beta_hat):
        N, K = ref.Z.shape
        s = ref.m * ref.W
        outer = np.outer(s, s) / ref.W
        live = (ref.Zc != 0).any(0)                   # a column of equal entries: the device's row / column is exact
        mask = np.outer(live, live)
        dA = (g_k(N) * ref.G + U * (np.abs(ref.A) + g_k(N) * ref.G) + E_FUNC * (ref.G + outer)) * mask
        R = np.linalg.cholesky(ref.A).T
        dA = dA + g_k(3 * K + 1) * (np.abs(R.T) @ np.abs(R))
        absy = np.abs(ref.y)
        db = U * np.abs(ref.b) + E_FUNC * (ref.Z.T @ (ref.w[:, None] * absy.T) + np.outer(s, np.abs(ref.ybar)))
        ab = np.abs(beta_hat)                         # [L, K]
        self.residual = (dA @ ab.T + db).T            # [L, K]
        self.forward = (np.abs(np.linalg.inv(ref.A)) @ self.residual.T).T
        m, fb = ref.m, self.forward
        self.intercept = fb @ m + U * np.abs(ref.intercept) + E_FUNC * (np.abs(ref.ybar) + ab @ m)
        self.local_pred = fb @ np.abs(1 - m) + U * np.abs(ref.local_pred) + E_FUNC * (np.abs(ref.ybar) + ab @ (1 + m))
        dp = fb @ np.abs(ref.Zc).T                    # [L, N]
        dres = (ref.w * (2 * np.abs(ref.y - ref.pred) * dp + dp * dp)).sum(1)
        self.score = dres / ref.tot + U * np.abs(ref.score) + E_FUNC * (1 + ref.res / ref.tot)


def ridge_ratios(ref, beta_hat, intercept=None, score=None, local_pred=None):
    """{quantity: worst |error| / bound} of a fit against ref (float64): the residual |A beta^ - b|, beta^, and the
    statistics that are given"""
    bd = RidgeBounds(ref, beta_hat)
    out = {"residual": ratio(np.abs(ref.A @ beta_hat.T - ref.b).T, bd.residual),
           "coef": ratio(np.abs(beta_hat - ref.beta), bd.forward)}
    for k, v in (("intercept", intercept), ("score", score), ("local_pred", local_pred)):
        if v is not None:
            out[k] = ratio(np.abs(np.asarray(v, dtype=np.float64) - getattr(ref, k)), getattr(bd, k))
    return out
