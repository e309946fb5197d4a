"""Error bounds of csrc/transformer_infer.hip against tests/tfm_infer_ref.py, derived in the manner of tests/attn_bounds.py:
u = 2^-24, g_K = K u / (1 - K u).  Every bound is the derived worst case; none is fitted to what the kernels give.

Assumed constant (named, not derived): the reciprocal square root is within K_RSQRT ulp = 2 K_RSQRT u relative (stated as
K_EXP of attn_bounds is).

Pre-norm sum z (a dot in any order, the bias, the residual):
    linear_res_ln   e_i = g_{K+2} (|res_i| + |b_i| + sum_k |a_k| |w_ik|)
    ffn_res_ln      hidden:  eps_j = g_{E+1} (|b1_j| + sum_k |x_k| |w1_jk|);  ReLU is 1-Lipschitz and passes it unchanged;
                    e_i = sum_j eps_j |w2_ij| + g_{ff+2} (|x_i| + |b2_i| + sum_j (h_j + eps_j) |w2_ij|)

Through the normalisation, s = sqrt(var + eps), zhat = (z - mu) / s in float64.  A perturbation dz with |dz_i| <= e_i moves
y_i = gamma_i zhat_i + beta_i at first order by  gamma_i / s (dz_i - mean(dz) - zhat_i mean(zhat dz)):
    prop_i = |gamma_i| / s (e_i + mean(e) + |zhat_i| mean(|zhat| e)) (1 + 4 r),        r = max_i e_i / s,
the factor covering the second-order terms as long as r < R_MAX = 2^-5 (every case is held to that: `r` is returned).

The op's own arithmetic on the perturbed values, D_i = |z_i - mu| + e_i + mean(e):
    the mean (E additions in any order and the division):   dmu = g_{E+1} (mean|z| + mean(e));
    the centring:   one rounding, (1 + u);
    the sum of squares (the square, E additions, the division: g_{E+2}, halved by the root), the addition of eps (u), the
        reciprocal square root (2 K_RSQRT u) and the second-order effect of the shifted mean, (dmu / s)^2:
        rel_s = g_{E+2} / 2 + u + 2 K_RSQRT u + (dmu / s)^2;
    the scale (one rounding of d rstd) and the shift (one rounding of the fused multiply-add):
        T_i = (D_i + dmu) (1 + u)^2 (1 + rel_s) - D_i
        own_i = (1 + 4 r) (|gamma_i| / s T_i + u (|gamma_i| / s (D_i + T_i) + |beta_i|))
bound = prop + own."""
import torch

from .attn_bounds import U, g_k, ratio  # noqa: F401 -- ratio is what the tests judge with

K_RSQRT = 2.0                # assumed: the reciprocal square root within 2 ulp = 4 u relative
R_MAX = 2.0 ** -5


def prenorm_linear(f):
    """e [R, E] of a tfm_infer_ref.LinearResLn"""
    return g_k(f.K + 2) * f.A


def prenorm_ffn(f):
    """e [R, E] of a tfm_infer_ref.FfnResLn"""
    eh = g_k(f.E + 1) * f.Ah
    w2a = f.w2.abs().t()
    return eh @ w2a + g_k(f.ff + 2) * (f.x.abs() + f.b2.abs() + (f.h + eh) @ w2a)


def through_norm(n, e):
    """(bound [R, E], r) of a tfm_infer_ref.Norm whose pre-norm sum is known within e"""
    E = n.z.shape[1]
    s, zh = n.s, n.zhat.abs()
    ga, be = n.gamma.abs(), n.beta.abs()
    me = e.mean(-1, keepdim=True)
    r = (e / s).amax(-1, keepdim=True)
    prop = ga / s * (e + me + zh * (zh * e).mean(-1, keepdim=True)) * (1 + 4 * r)
    D = (n.z - n.mu).abs() + e + me
    dmu = g_k(E + 1) * (n.z.abs().mean(-1, keepdim=True) + me)
    rel_s = g_k(E + 2) / 2 + U + 2 * K_RSQRT * U + (dmu / s) ** 2
    T = (D + dmu) * (1 + U) ** 2 * (1 + rel_s) - D
    own = (1 + 4 * r) * (ga / s * T + U * (ga / s * (D + T) + be))
    return prop + own, float(r.max())


def linear_res_ln(f):
    return through_norm(f.n, prenorm_linear(f))


def ffn_res_ln(f):
    return through_norm(f.n, prenorm_ffn(f))
