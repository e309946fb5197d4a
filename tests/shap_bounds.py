"""Error bounds of csrc/shap.hip against tests/shap_ref.py, derived in the manner of tests/lime_bounds.py and
tests/f64check.py: u = 2^-24, g_K = K u / (1 - K u), u64 = 2^-53.  Every bound is the derived worst case; none is fitted to
what the kernels give.

Pre-activation  z^ = fl(chain_d W1[h, d] p^_d) + b1: an fmaf chain over the D columns from 0 (D roundings; the columns the
    kernel pads are exact zeros) and the bias add, so given the fp32 point p^
        |z^ - (W1 p^ + b1)| <= g_(D+1) (|W1| |p^| + |b1|).
    DeepLIFT rows: p^ is the row itself.  Expected gradients: p^ = fl(fl(t x) + fl(fl(1 - t) bg)) carries at most three
    roundings on either term, |p^ - p| <= g_3 pa with pa = |t x| + |(1 - t) bg|, and |p^| <= (1 + g_3) pa, hence
        |z^ - z| <= g_(D+1) ((1 + g_3) |W1| pa + |b1|) + g_3 |W1| pa.

Rescale ratio given the STORED zx, zb: fl(fl(relu zx - relu zb) / fl(zx - zb)), three roundings: |g^ - g| <= g_3 |g|.

phi given the gates g (the device's own: exact 0 / 1, or the ratio above).  Per pair and class the device forms
    s_h = fl(g^_h W2[c, h])      exact for a 0 / 1 gate, one rounding otherwise (on top of the three of g^)
    G_d = chain_h W1[h, d] s_h   an fmaf chain over H terms from 0: H roundings
    q_d = fl(G_d fl(x_d - bg_d)) two roundings
so with A = sum_h |W1[h, d]| |W2[c, h]| |g_h| |x_d - bg_d| the product is off by at most e = g_n A, n = H + 2 (0 / 1 gates)
or H + 6 (ratio gates).  The pair sum and the division by K are fp64 ((K + 2) u64 mean_k A: nothing visible, carried
anyway), the result is rounded once to fp32:
    |phi^ - phi| <= (1 + u) (mean_k e + (K + 2) u64 mean_k A) + u |phi|.

var = Var_k(q) / sqrt(K).  With m the mean and a_k = e_k + mean_k e the error of a centred product,
    |Var(q^) - Var(q)| = |mean_k ((q^ - m^) - (q - m)) ((q^ - m^) + (q - m))| <= mean_k a_k (2 |q_k - m| + a_k);
the device evaluates E[q^2] - m^2 in fp64 from fp64 sums (squares of fp32 values are exact in fp64): both terms carry
(K + 4) u64 relative, so 2 (K + 4) u64 (E[q^2] + m^2) absolute; then / sqrt(K) and one fp32 rounding:
    |var^ - var| <= (1 + u) (mean_k a_k (2 |q_k - m| + a_k) + 2 (K + 4) u64 (E[q^2] + m^2)) / sqrt(K) + u |var|.

Additivity of DeepLIFT against the float64 network: with gates from stored z^ = z + dz the ratio satisfies
g (z^x - z^b) = relu z^x - relu z^b exactly, |g| <= 1 and relu is 1-Lipschitz, so per hidden unit
    |g (zx - zb) - (relu zx - relu zb)| <= 2 (|dzx| + |dzb|),   and <= 2 (1e-6 + |dzx| + |dzb|) on the threshold branch;
weighted by |W2[c, h]|, summed over h and averaged over the background it adds to the sum over d of the phi bound.
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def g_k(K):
    return K * U / (1.0 - K * U)


def ratio(err, bound):
    """worst err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def z_bound(pabs, w1, b1, interpolated):
    """pabs [..., D]: |row|, or |t x| + |(1 - t) bg| of an interpolated point"""
    D = w1.shape[1]
    aw, ab = np.abs(np.asarray(w1, dtype=np.float64)), np.abs(np.asarray(b1, dtype=np.float64))
    carried = pabs @ aw.T
    if interpolated:
        return g_k(D + 1) * ((1.0 + g_k(3)) * carried + ab) + g_k(3) * carried
    return g_k(D + 1) * (carried + ab)


def product_error(absprod, H, ratio_gates):
    """e [B, K, C, D] from the magnitude products of shap_ref.products"""
    return g_k(H + (6 if ratio_gates else 2)) * absprod


def phi_bound(absprod, phi64, H, ratio_gates):
    """[B, D, C]"""
    K = absprod.shape[1]
    e = product_error(absprod, H, ratio_gates).mean(1) + (K + 2) * U64 * absprod.mean(1)
    return (1.0 + U) * e.transpose(0, 2, 1) + U * np.abs(phi64)


def var_bound(prod, absprod, var64, H, ratio_gates=False):
    """[B, D, C]"""
    K = prod.shape[1]
    e = product_error(absprod, H, ratio_gates)
    a = e + e.mean(1, keepdims=True)
    m = prod.mean(1, keepdims=True)
    dvar = (a * (2.0 * np.abs(prod - m) + a)).mean(1)
    e64 = 2.0 * (K + 4) * U64 * ((prod * prod).mean(1) + m[:, 0] ** 2)
    return (1.0 + U) * ((dvar + e64) / np.sqrt(K)).transpose(0, 2, 1) + U * np.abs(var64)


def additivity_bound(phi_b, w2, dzx, dzb, branch):
    """[B, C]: phi_b [B, D, C] the phi bound, dzx [B, H] / dzb [N, H] the z bounds, branch [B, N, H] the threshold branch"""
    per = 2.0 * (dzx[:, None, :] + dzb[None, :, :] + 1e-6 * branch)          # [B, N, H]
    return phi_b.sum(1) + (per @ np.abs(np.asarray(w2, dtype=np.float64)).T).mean(1)
