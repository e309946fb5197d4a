"""Error bounds of csrc/attention.hip against tests/attn_ref.py, derived in the manner of tests/f64check.py:
u = 2^-24, g_K = K u / (1 - K u).  Every bound is the derived worst case; none is fitted to what the kernels give.

Assumed constants (named, not derived): expf returns its argument's exponential to K_EXP u relative and logf its logarithm
to K_LOG u relative (the device library documents 1 ulp = 2 u for both; K_SIG / K_LOG of f64check are stated the same way).

Notation: d = head_dim, S keys, T = ceil(S / 16) key tiles, A_s = scale |q| . |k| the magnitude sum of a score.

Scores.  s^ = fl(fl_dot_d(q, k) * scale^), scale^ = fl(1 / sqrtf(d)):  |s^ - s| <= ds = g_{d+3} A_s
    (a dot of length d in any order, the rounding of scale^ counted as 2 u, the multiplication).
    Row quantities: Delta_i = max_j ds_ij, R_i = max_j s_ij - min_j s_ij + 2 Delta_i (the largest |s^_ij - m| the kernel can
    form, m being a running maximum of the same row).

Forward.  The output is  o_ic = (sum_j e_ij v_jc) / (sum_j e_ij),  e_ij = expf(s^_ij - m_t) * (the rescale factors of the
    later tiles).  The factors multiply numerator and denominator alike, so their FUNCTION error cancels in the quotient and
    only the rounding of each multiplication stays.  Mathematically the quotient does not depend on m, so
      - the score error moves the softmax by at most exp(2 Delta_i) relative (numerator exp(+-Delta), denominator likewise);
      - each e_ij carries (K_EXP + R_i) u relative: the function and the rounding of the subtraction s^ - m;
      - numerator: S products accumulated in any order, T rescale multiplications, the dropout scale (3 u: 1 / (1 - p)
        rounded twice and the product, only when p > 0) and the final division: K_num = S + T + 1 (+ 3);
      - denominator: S terms summed in any order and T rescale multiply-adds: K_den = S + 2 T.
    |out - ref| <= expm1(g_{K_num} + g_{K_den} + 2 (K_EXP + R_i) u + 2 Delta_i) * A_out,   A_out = sum_j Pd_ij |v_jc|.
    lse^ = fl(m + logf(l^)):  |lse^ - lse| <= Delta_i + expm1(g_{K_den} + (K_EXP + R_i) u) + K_LOG u log(S) + u |lse|
    (l^ in [1, S] times (1 + its relative error); the last term is the final addition).

Backward, from the STORED out, lse and dout (float64 evaluation of the same formulas in attn_ref.Backward):
    p^_ij = expf(s^_ij - lse_i):   relative  ep_ij = expm1(ds_ij + (|s_ij| + ds_ij + |lse_i|) u + K_EXP u)
    dP^_ij = fl_dot_d(dout_i, v_j) (* 1 / (1 - p)):   |.| <= e_dP = g_{d+3} A_dP          A_dP = |dout| . |v| (* 1 / (1 - p))
    D^_i = fl_dot_d(dout_i, out_i):                    |.| <= e_D = g_d A_D
    dS^ = p^ (dP^ - D^):   e_dS = (ep + g_2) A_dS + (1 + ep) P (e_dP + e_D),    A_dS = P (|dP| + |D|)
    dQ_ic = scale^ sum_j dS_ij k_jc   (a dot over S, the scale as above):  scale (e_dS |k|) + g_{S+3} scale (|dS| |k|)
    dK_jc = scale^ sum_i dS_ij q_ic   (a dot over S):                      scale (e_dS^T |q|) + g_{S+3} scale (|dS|^T |q|)
    dV_jc = sum_i Pd^_ij dout_ic      (a dot over S):                      ((ep + g_3 [p > 0]) Pd)^T |dout| + g_S (Pd^T |dout|)
"""
import math

import torch

U = 2.0 ** -24
K_EXP = 2.0                  # assumed: expf within one ulp = 2 u relative
K_LOG = 2.0                  # assumed: logf within one ulp = 2 u relative (as f64check.K_LOG)


def g_k(K):
    return K * U / (1.0 - K * U)


def ratio(err, bound):
    """worst err / bound; an element whose bound is 0 must be exact; a NaN / inf error is infinitely bad"""
    err, bound = err.double(), bound.double()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def seen_units(got, ref, A):
    """the constant actually seen: worst |got - ref| in units of u A over the elements with A > 0 (the measured K)"""
    A = A.double()
    k = torch.where(A > 0, (got.double() - ref).abs() / (U * A).clamp_min(1e-300), torch.zeros_like(A))
    k = k[torch.isfinite(k)]
    return float(k.max()) if k.numel() else 0.0


class ForwardBounds:
    """out [N, heads, S, d] and lse [N, heads, S] bounds of an attn_ref.Forward"""

    def __init__(self, f):
        S, d = f.S, f.d
        T = (S + 15) // 16
        ds = g_k(d + 3) * f.As
        self.ds = ds
        self.delta = ds.amax(-1)
        self.R = f.s.amax(-1) - f.s.amin(-1) + 2 * self.delta
        drop = 3 if f.keep is not None else 0
        self.K_num, self.K_den = S + T + 1 + drop, S + 2 * T
        rel = torch.expm1(g_k(self.K_num) + g_k(self.K_den) + 2 * (K_EXP + self.R) * U + 2 * self.delta)
        self.rel = rel
        self.out = rel[..., None] * f.Aout
        self.lse = (self.delta + torch.expm1(g_k(self.K_den) + (K_EXP + self.R) * U) + K_LOG * U * math.log(max(S, 2)) +
                    U * f.lse.abs())


class BackwardBounds:
    """dq, dk, dv [N, heads, S, d] bounds of an attn_ref.Backward"""

    def __init__(self, b):
        f = b.f
        S, d = f.S, f.d
        drop = f.keep is not None
        ds = g_k(d + 3) * f.As
        ep = torch.expm1(ds + (f.s.abs() + ds + b.lse.abs()[..., None]) * U + K_EXP * U)
        e_dP = g_k(d + 3) * b.AdP
        e_D = g_k(d) * b.AD
        e_dS = (ep + g_k(2)) * b.AdS + (1 + ep) * b.P * (e_dP + e_D[..., None])
        gs = g_k(S + 3)
        self.dq = f.scale * (e_dS @ f.k.abs() + gs * (b.dS.abs() @ f.k.abs()))
        self.dk = f.scale * (e_dS.transpose(-1, -2) @ f.q.abs() + gs * (b.dS.abs().transpose(-1, -2) @ f.q.abs()))
        epd = (ep + (g_k(3) if drop else 0.0)) * b.Pd
        self.dv = epd.transpose(-1, -2) @ b.do.abs() + g_k(S) * (b.Pd.transpose(-1, -2) @ b.do.abs())
