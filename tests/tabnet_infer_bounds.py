"""Forward error bounds of csrc/tabnet_infer.hip against tests/tabnet_infer_ref.py, derived in the manner of
tests/tfm_infer_bounds.py and the TabNet section of tests/f64check.py: u = 2^-24, g_K = K u / (1 - K u).  Every bound is the
derived worst case of the arithmetic; none is fitted to what the kernel gives.  Every map of the network is Lipschitz, so no
element is excluded from a value check.

Assumed constants (named, not derived): K_SIG (|sigmoid' - sigmoid| <= K_SIG u) and K_LOG (logf within K_LOG u relative) of
f64check; K_FOLD = 5: the scale s = gamma / sqrt(rv + eps) is one addition (u) and a root and a division ASSUMED within one ulp
= 2 u each (hipcc rounds both correctly by default, which is half of that).

Fold.        W'^ = fl(s^ W):  |W'^ - W'| <= g_{K_FOLD+1} |W'|.     b'^ = fma(-rm, s^, beta), one rounding:
             |b'^ - b'| <= g_{K_FOLD+1} |rm s| + g_1 |b'|.         A gamma of 0 gives s^ = 0 and a zero row, exactly.
initial_bn   xn^ = fma(x, scale^, shift^):  e = (|x| g_{K_FOLD} |scale| + d_shift) (1 + u) + u |xn|.
Linear       z = W' a + b' on an input known within e_a (aa = |a| + e_a), an fmaf chain over K (the padding adds exact zeros) and
             the addition of the bias:
                 e_z = |W'| e_a + g_{K_FOLD+1} |W'| aa + d_b + g_{K+1} ((1 + g_{K_FOLD+1}) |W'| aa + |b'| + d_b)
GLU          o = A sigmoid(G): the sigmoid is 1/4-Lipschitz, dsg = e_G / 4 + K_SIG u;
                 e_o = e_A (sigmoid(G) + dsg) + |A| dsg, plus the rounding of the product u (|o| + e_o).
Residual     h' = fl(fl(h + o) c), c = fl(sqrt(0.5)):  e = c (e_h + e_o) (1 + g_3) + g_3 |h'|.
Prior        zp = fl(z p):  e_zp = (e_z (|p| + e_p) + |z| e_p) (1 + u) + u |zp|.
Sparsemax    p(x) = max(x - tau(x), 0) obeys |dp_i| <= 2 max_j |dx_j| (tau is 1-Lipschitz in the max norm).  The kernel's own
             arithmetic: the row maximum is subtracted first (one rounding of a value <= R~, the row's range plus twice the input
             error: a perturbation u R~ of the input); each round computes tau^ = (sum_S - 1) / |S| over at most D values of
             magnitude <= R~, |tau^ - tau(S)| <= E = g_{D+2} (R~ + 1).  With rounding tau^ still grows from round to round up to
             2 E, so an element dropped in any round lies at most 2 E above the final tau^, and an element kept lies above it:
             the result is the exact sparsemax of an input moved by at most 3 E, with tau off by one more E.  Hence
                 e_M = 2 max_j e_zp_j + 2 u R~ + 7 E + u M.
             An entry whose float64 value has zp_i - tau <= -(2 max_j e_zp_j + 2 u R~ + 7 E) must come out as exactly 0.0
             (`zero_thr`), one with M_i above that threshold must be positive.
Entropy      f(M) = M log(M + eps): |f'| <= |log(lo + eps)| + 1 on [lo, ...], lo = max(M - e_M, 0);
                 e_f = e_M (|log(lo + eps)| + 1) + (M + e_M) g_{K_LOG+2} (|log(lo + eps)| + 1)
             (the addition of eps, logf, the product); the sum over n_steps D terms: + g_{n_steps D + 2} sum (|f| + e_f).
Prior update p' = fl(p fl(gamma - M)):  e_q = e_M + u (|q| + e_M);  e_p' = (e_p (|q| + e_q) + |p| e_q) (1 + u) + u |p'|.
Masked input mx = fl(M xn):  e = (e_M (|xn| + e_xn) + M e_xn) (1 + u) + u |mx|.
d, sums      ReLU is 1-Lipschitz: e_d = e_h.  sum of the steps' d: sum e_d + g_{n_steps} (sum d + sum e_d).  The row sum of d
             (n_d terms): e_imp = sum_j e_d + g_{n_d+2} (imp + sum_j e_d).  M_explain += M imp:
             e = e_M (imp + e_imp) + M e_imp per step, + g_{n_steps+1} (M_explain + its e) for the fused multiply-adds.
out          final_mapping is copied, not folded: e_out = |Wf| e_dsum + g_{n_d+1} |Wf| (dsum + e_dsum).

Forced references.  Propagating by |W'| multiplies an error by the row sums of |W'| in every layer, about 7 on the test
weights, so over the 4 (n_steps + 1) + n_steps layers of the whole chain the bound of a late mask passes 1 and says nothing.
The masks are OUTPUTS, so the reference may take the candidate's own masks as given (tabnet_infer_ref.reference(forced=...)):
everything downstream of step s's mask then uses exactly the fp32 numbers the kernel used, e_M = 0 there, and each compared
element carries the error of one FeatTransformer and one attentive layer only.  Every element of every output is still
compared with a float64 value; the bound of step s's mask is the one above with e_p the rounding of the prior recurrence
alone."""
import math

import torch

from .attn_bounds import U, g_k, ratio  # noqa: F401 -- ratio is what the tests judge with
from .f64check import K_LOG, K_SIG

K_FOLD = 5.0


def fold_weight(W):
    return g_k(K_FOLD + 1) * W.abs()


def fold_bias(b, rms):
    return g_k(K_FOLD + 1) * rms + g_k(1) * b.abs()


def _linear(a, e_a, W, b, rms):
    K = (W.shape[1] + 15) // 16 * 16
    Wa = W.abs().t()
    aa = a.abs() + e_a
    mag = aa @ Wa
    db = fold_bias(b, rms)
    gf = g_k(K_FOLD + 1)
    return e_a @ Wa + gf * mag + db + g_k(K + 1) * ((1 + gf) * mag + b.abs() + db)


def _feat(c, layers, e_a):
    W_ = c.n_d + c.n_a
    cs = math.sqrt(0.5)
    e_h = None
    for l, y in enumerate(layers):
        e_z = _linear(y.a, e_a, y.W, y.b, y.rms)
        e_A, e_G = e_z[:, :W_], e_z[:, W_:]
        dsg = e_G / 4 + K_SIG * U
        e_o = e_A * (torch.sigmoid(y.G) + dsg) + y.A.abs() * dsg
        e_o = e_o + U * (y.o.abs() + e_o)
        e_h = e_o if l == 0 else cs * (e_h + e_o) * (1 + g_k(3)) + g_k(3) * y.h.abs()
        e_a = e_h
    return e_h


class Forward:
    """bounds of a tabnet_infer_ref.reference: out [B, out_dim], masks [n_steps, B, D], m_explain [B, D], row_entropy [B],
    zero_thr [n_steps, B, 1]"""

    def __init__(self, c, r):
        D = c.D
        sc, sh, rms0 = r.folds.bn0
        e_xn = (r.x.abs() * g_k(K_FOLD) * sc.abs() + fold_bias(sh, rms0)) * (1 + U) + U * r.xn.abs()
        e_h = _feat(c, r.ft[0], e_xn)
        eps = torch.tensor(c.epsilon, dtype=torch.float64)
        e_p = torch.zeros_like(r.xn)
        e_dsum = torch.zeros_like(r.dsum)
        e_mexp = torch.zeros_like(r.xn)
        e_ent = torch.zeros_like(r.row_entropy)
        ent_mag = torch.zeros_like(r.row_entropy)
        masks, thr = [], []
        for s, st in enumerate(r.steps):
            e_z = _linear(st.att, e_h[:, c.n_d:], st.W, st.b, st.rms)
            e_zp = (e_z * (st.prior.abs() + e_p) + st.z.abs() * e_p) * (1 + U) + U * st.zp.abs()
            emax = e_zp.amax(1, keepdim=True)
            Rt = st.zp.amax(1, keepdim=True) - st.zp.amin(1, keepdim=True) + 2 * emax
            E = g_k(D + 2) * (Rt + 1)
            row = 2 * emax + 2 * U * Rt + 7 * E
            e_M = row + U * st.M
            masks.append(e_M)
            thr.append(row)
            M = st.Mu                       # what everything downstream uses: the candidate's own mask when forced
            if r.forced:
                e_M = torch.zeros_like(e_M)
            slope = torch.log(torch.clamp(M - e_M, min=0) + eps).abs() + 1
            e_f = e_M * slope + (M + e_M) * g_k(K_LOG + 2) * slope
            e_ent = e_ent + e_f.sum(1)
            ent_mag = ent_mag + (st.term.abs() + e_f).sum(1)
            q = c.gamma - M
            e_q = e_M + U * (q.abs() + e_M)
            e_p = (e_p * (q.abs() + e_q) + st.prior.abs() * e_q) * (1 + U) + U * st.prior_next.abs()
            e_mx = (e_M * (r.xn.abs() + e_xn) + M * e_xn) * (1 + U) + U * st.mx.abs()
            e_h = _feat(c, r.ft[s + 1], e_mx)
            e_d = e_h[:, :c.n_d]
            e_dsum = e_dsum + e_d
            sd = e_d.sum(1, keepdim=True)
            e_imp = sd + g_k(c.n_d + 2) * (st.imp + sd)
            e_mexp = e_mexp + e_M * (st.imp + e_imp) + M * e_imp
        n = len(r.steps)
        e_dsum = e_dsum + g_k(n) * (r.dsum + e_dsum)
        Wf = r.final.abs().t()
        self.out = e_dsum @ Wf + g_k(c.n_d + 1) * ((r.dsum + e_dsum) @ Wf)
        self.masks = torch.stack(masks)
        self.zero_thr = torch.stack(thr)
        self.m_explain = e_mexp + g_k(n + 1) * (r.m_explain + e_mexp)
        self.row_entropy = e_ent + g_k(n * D + 2) * ent_mag


def certain(r, b):
    """(zero, positive): boolean [n_steps, B, D] of the mask entries that the float64 reference decides beyond the bound"""
    zp = torch.stack([st.zp for st in r.steps])
    tau = torch.stack([st.tau for st in r.steps])
    return zp - tau <= -b.zero_thr, zp - tau > b.zero_thr


def ratios(got, r, b):
    """worst |got - ref| / bound per output of a dict got = {out, masks, m_explain, row_entropy} (absent keys skipped)"""
    ref = dict(out=r.out, masks=r.masks, m_explain=r.m_explain, row_entropy=r.row_entropy)
    return {k: ratio((got[k].double().cpu() - ref[k]).abs(), getattr(b, k)) for k in ref if got.get(k) is not None}
