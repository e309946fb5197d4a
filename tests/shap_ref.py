"""float64 numpy restatement of the two SHAP estimators of csrc/shap.hip for Linear(D, H) -> ReLU -> Linear(H, C)
(DESIGN section 22), and of the ingredients of the bounds in tests/shap_bounds.py.

Layout: x [B, D], bg [N, D], W1 [H, D], b1 [H], W2 [C, H]; pairs (b, k) with background row ridx[b, k]; every per-pair
array is [B, K, ...].  Results are [B, D, C] like the device's.  Inputs are taken as given (fp32 values) and promoted."""
import numpy as np

THRESHOLD = 1e-6   # shap's constant: below it the rescale ratio gives way to the plain ReLU gradient


def f64(a):
    return np.asarray(a, dtype=np.float64)


def make_inputs(B, N, D, H, C, seed):
    """weights uniform in +-1/sqrt(fan-in) (torch's Linear default), standard-normal x and bg, all fp32"""
    rng = np.random.default_rng(seed)
    w1 = rng.uniform(-1, 1, (H, D)) / np.sqrt(D)
    b1 = rng.uniform(-1, 1, H) / np.sqrt(D)
    w2 = rng.uniform(-1, 1, (C, H)) / np.sqrt(H)
    b2 = rng.uniform(-1, 1, C) / np.sqrt(H)
    x, bg = rng.normal(size=(B, D)), rng.normal(size=(N, D))
    return tuple(a.astype(np.float32) for a in (x, bg, w1, b1, w2, b2))


def make_draws(B, N, K, seed):
    """ridx int32 [B, K] with repeated rows, t fp32 [B, K] in [0, 1) with t[:, 0] = 0 and (K > 1) t[:, 1] = 1"""
    rng = np.random.default_rng(seed)
    ridx = rng.integers(0, N, (B, K)).astype(np.int32)
    if K > 2:
        ridx[:, 2] = ridx[:, 0]
    t = rng.uniform(size=(B, K)).astype(np.float32)
    t[:, 0] = 0.0
    if K > 1:
        t[:, 1] = 1.0
    return ridx, t


def points(x, bg, ridx, t):
    """p = t x + (1 - t) bg_r, and |t x| + |(1 - t) bg_r| for the bound; [B, K, D]"""
    x, bg, t = f64(x), f64(bg), f64(t)[..., None]
    a, b = t * x[:, None, :], (1.0 - t) * bg[ridx]
    return a + b, np.abs(a) + np.abs(b)


def preact(p, w1, b1):
    return f64(p) @ f64(w1).T + f64(b1)


def forward(x, w1, b1, w2, b2):
    return np.maximum(preact(x, w1, b1), 0.0) @ f64(w2).T + f64(b2)


def gate_gradient(z):
    return (f64(z) > 0).astype(np.float64)


def rescale_branch(zx, zb):
    """True where the plain gradient replaces the ratio; zx [B, H], zb [N, H] -> [B, N, H]"""
    return np.abs(f64(zx)[:, None, :] - f64(zb)[None, :, :]) < THRESHOLD


def gate_rescale(zx, zb):
    zx, zb = f64(zx)[:, None, :], f64(zb)[None, :, :]
    dz = zx - zb
    small = np.abs(dz) < THRESHOLD
    ratio = (np.maximum(zx, 0.0) - np.maximum(zb, 0.0)) / np.where(small, 1.0, dz)
    return np.where(small, (zb > 0).astype(np.float64), ratio)


def products(x, rows, gates, w1, w2):
    """the per-pair products G_c * (x_b - bg_r) [B, K, C, D], and the same with every factor replaced by its magnitude.
    rows [B, K, D]: the background row of each pair; gates [B, K, H]."""
    w1, w2, g = f64(w1), f64(w2), f64(gates)
    diff = f64(x)[:, None, :] - f64(rows)
    G = (g[:, :, None, :] * w2[None, None]) @ w1
    Ga = (np.abs(g)[:, :, None, :] * np.abs(w2)[None, None]) @ np.abs(w1)
    return G * diff[:, :, None, :], Ga * np.abs(diff)[:, :, None, :], G


def mean_and_variance(prod):
    """phi [B, D, C] and shap's variance: the population variance over the pairs divided by sqrt(K)"""
    K = prod.shape[1]
    return prod.mean(1).transpose(0, 2, 1), (prod.var(1) / np.sqrt(K)).transpose(0, 2, 1)


def expected_gradients(x, bg, ridx, t, w1, b1, w2, gates=None):
    """-> phi, var [B, D, C]; gates [B, K, H] replace 1[z > 0] where given"""
    if gates is None:
        gates = gate_gradient(preact(points(x, bg, ridx, t)[0], w1, b1))
    return mean_and_variance(products(x, f64(bg)[ridx], gates, w1, w2)[0])


def deeplift(x, bg, w1, b1, w2, gates=None):
    """-> phi [B, D, C]: the rescale rule against every background row, averaged"""
    B, N = len(x), len(bg)
    if gates is None:
        gates = gate_rescale(preact(x, w1, b1), preact(bg, w1, b1))
    rows = np.broadcast_to(f64(bg)[None], (B, N, bg.shape[1]))
    return mean_and_variance(products(x, rows, gates, w1, w2)[0])[0]


# the inputs of the end-to-end tests (tests/test_shap_gpu.py), shared with the cap on undecided gates that
# tests/test_shap_cpu.py asserts for them: (B, N, D, H, C, input seed); nsamples and the draws' seed
E2E_SHAPES = [(3, 5, 768, 128, 2, 11), (8, 100, 672, 128, 2, 12)]
E2E_NSAMPLES = (16, 200)
E2E_RSEED = 7
# the cases of tests/test_shap_ops_gpu.py: (B, N, K, D, H, C)
OPS_CASES = [(3, 5, 7, 70, 20, 3), (2, 1, 50, 33, 5, 1), (1, 9, 129, 100, 17, 2), (2, 9, 65, 260, 130, 8),
             (16, 100, 200, 768, 128, 2), (4, 100, 200, 672, 128, 2)]
UNDECIDED_CAP = 2e-3   # share of gates whose float64 pre-activation lies within the z bound, at the head shapes


def ops_inputs(case):
    B, N, K, D, H, C = case
    return make_inputs(B, N, D, H, C, seed=100 + D), make_draws(B, N, K, seed=200 + D)
