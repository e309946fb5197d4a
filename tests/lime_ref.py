"""Float64 restatement of what csrc/lime.hip computes (lime tabular 0.2.x with the defaults the reference's call hits), in
numpy / scipy / sklearn.  lime itself is not installed; DESIGN.md section 21 is the specification this file follows.
Nothing here calls the HIP library."""
import numpy as np

from .philox_ref import MASK, philox4x32_10, u53  # noqa: F401  (the one host copy; test_lime_cpu.py holds it to the known answers)

SEED = 20261019          # the Philox seed of the GPU tests (chosen on the CPU: tests/test_lime_cpu.py checks its uniforms)


def crafted_background():
    """columns: 0 distinct quartiles, 1 tied quartiles, 2 constant, 3 a value exactly on a quartile, 4 an empty bin"""
    rng = np.random.default_rng(5)
    M = 42
    bg = np.zeros((M, 5), dtype=np.float32)
    bg[:, 0] = rng.normal(size=M)
    bg[:, 1] = np.where(np.arange(M) < 30, 2.0, rng.normal(size=M) + 5)      # 25 % and 50 % both fall on 2.0
    bg[:, 2] = 0.75
    bg[:, 3] = np.arange(M)
    # sorted[0 .. 20] = 0 and the median is interpolated half way to sorted[21]: the bin (0, median] is empty
    bg[:, 4] = np.where(np.arange(M) < 21, 0.0, 5.0 + np.arange(M))
    return bg


def perturb_uniforms(seed, offset, b, n, f):
    """(u_bin, u_val) of element (b, n, f) -- b already includes b0 -- at the counter documented in include/ecgmm.h"""
    b, n, f = (np.asarray(v, dtype=np.uint64) for v in (b, n, f))
    c3 = np.uint64(0x40000000) | (b << np.uint64(12)) | f
    r = philox4x32_10((seed & MASK, (seed >> 32) & MASK), (offset & MASK, (offset >> 32) & MASK, n, c3))
    return u53(r[0], r[1]), u53(r[2], r[3])


def draw_bins(u, cdf, nbins):
    """first j with cdf[j] > u * cdf[nbins - 1]; the last bin of positive frequency where rounding leaves none.
    u [..., D], cdf [D, S], nbins [D] -> int bins [..., D]"""
    D, S = cdf.shape
    total = cdf[np.arange(D), nbins - 1]
    t = u * total
    valid = np.arange(S)[None, :] < nbins[:, None]
    hit = (cdf > t[..., None]) & valid
    first = hit.argmax(-1)
    prev = np.concatenate([np.zeros((D, 1)), cdf[:, :-1]], axis=1)
    positive = (cdf > prev) & valid
    last = S - 1 - positive[:, ::-1].argmax(-1)
    return np.where(hit.any(-1), first, last)


def truncnorm_value(u, mean, std, lo, hi):
    """scipy.stats.truncnorm.ppf(u, a, b, loc, scale) in float64, with the two degenerate cases of the specification:
    std the bare 1e-11 offset -> mean, a == b -> the common point.  Also returns z = (value - mean) / std."""
    from scipy.stats import truncnorm
    a, b = (lo - mean) / std, (hi - mean) / std
    bare, point = std <= 1e-11, a == b
    ok = ~(bare | point)
    v = np.where(bare, mean, mean + std * a)
    if ok.any():
        v = v.copy()
        v[ok] = truncnorm.ppf(u[ok], a[ok], b[ok], loc=mean[ok], scale=std[ok])
    return v, (v - mean) / std


def kernel_weights(d2, kernel_width):
    return np.sqrt(np.exp(-np.asarray(d2, dtype=np.float64) / kernel_width ** 2))


class RidgeRef:
    """(Zc^T W Zc + alpha I) beta = Zc^T W yc with w-weighted centring, for one sample.  Z [N, K] 0/1, w [N], y [L, N];
    dtype float64 is the reference, float32 the same arithmetic in numpy fp32 (Gram, Cholesky and solves)."""

    def __init__(self, Z, w, y, alpha, dtype=np.float64):
        Z, w, y = np.asarray(Z, dtype=np.float64), np.asarray(w, dtype=np.float64), np.atleast_2d(np.asarray(y, dtype=np.float64))
        self.Z, self.w, self.y, self.alpha = Z, w, y, alpha
        self.W = w.sum()
        self.m = (w[:, None] * Z).sum(0) / self.W
        equal = (Z == Z[0]).all(0)                    # a column of equal entries: its weighted mean is that entry, exactly
        self.m[equal] = Z[0, equal]
        self.ybar = (y * w).sum(1) / self.W
        self.Zc = Z - self.m
        self.G = Z.T @ (w[:, None] * Z)
        self.A = self.Zc.T @ (w[:, None] * self.Zc) + alpha * np.eye(Z.shape[1])
        self.b = self.Zc.T @ (w[:, None] * (y - self.ybar[:, None]).T)          # [K, L]
        if dtype == np.float64:
            self.beta = np.linalg.solve(self.A, self.b).T                         # [L, K]
        else:
            import scipy.linalg as sl
            Z32, w32 = Z.astype(np.float32), w.astype(np.float32)
            G32 = Z32.T @ (w32[:, None] * Z32)
            s = (w[:, None] * Z).sum(0)
            A32 = (G32.astype(np.float64) - np.outer(s, s) / self.W + alpha * np.eye(Z.shape[1])).astype(np.float32)
            A32[equal, :] = 0                         # a column of equal entries is centred exactly, as on the device
            A32[:, equal] = 0
            A32[equal, equal] = alpha
            c = sl.cho_factor(A32, lower=True)
            self.beta = sl.cho_solve(c, self.b.astype(np.float32)).T.astype(np.float64)
        self.finish(self.beta)

    def finish(self, beta):
        """intercept, local_pred and the weighted R^2 of the coefficients beta [L, K]"""
        self.intercept = self.ybar - beta @ self.m
        self.local_pred = self.intercept + beta.sum(1)
        pred = self.intercept[:, None] + beta @ self.Z.T
        self.res = (self.w * (self.y - pred) ** 2).sum(1)
        self.tot = (self.w * (self.y - self.ybar[:, None]) ** 2).sum(1)
        self.score = 1.0 - self.res / self.tot
        self.pred = pred
        return self


def sklearn_ridge(Z, w, y, alpha):
    """coef [L, K], intercept [L], score [L] of sklearn's Ridge(alpha, fit_intercept=True) with sample_weight = w"""
    from sklearn.linear_model import Ridge
    coef, icpt, score = [], [], []
    for yl in np.atleast_2d(y):
        r = Ridge(alpha=alpha, fit_intercept=True, solver="cholesky").fit(Z, yl, sample_weight=w)
        coef.append(r.coef_)
        icpt.append(r.intercept_)
        score.append(r.score(Z, yl, sample_weight=w))
    return np.array(coef), np.array(icpt), np.array(score)


def explain(Z, d2, y, kernel_width, num_features, w=None):
    """lime's explain_instance_with_data for one sample from given perturbations: Z [N, D], d2 [N], y [N] (one label);
    w: the kernel weights to use instead of the float64 ones.  -> kept columns (sorted), RidgeRef of the final alpha = 1 fit"""
    w = kernel_weights(d2, kernel_width) if w is None else w
    D = Z.shape[1]
    if num_features >= D:
        return np.arange(D), RidgeRef(Z, w, y, 1.0)
    first = RidgeRef(Z, w, y, 0.01)
    keep = np.sort(np.argsort(-np.abs(first.beta[0] * Z[0]), kind="stable")[:num_features])
    return keep, RidgeRef(Z[:, keep], w, y, 1.0)


def ridge_case(N, K, L, bins, seed):
    """Z [N, K] with row 0 all ones, column 1 all ones (its centred column is zero), columns 2 and 3 equal (a duplicated
    pair); d2 = the zeros of each row; y [L, N] a noisy linear response in (0, 1)"""
    rng = np.random.default_rng(seed)
    Z = (rng.integers(0, bins, size=(N, K)) == 0).astype(np.uint8)
    Z[0] = 1
    if K > 3:
        Z[:, 1] = 1
        Z[:, 3] = Z[:, 2]
    d2 = (Z == 0).sum(1).astype(np.int32)
    beta = rng.normal(size=(L, K)) * 0.02
    y = 0.5 + beta @ (Z.T - 1.0 / bins) + 0.01 * rng.normal(size=(L, N))
    return Z, d2, np.clip(y, 0.0, 1.0).astype(np.float32)
