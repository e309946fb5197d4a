"""float64 restatement and error bounds of the attention maps and the rollout step of csrc/attention.hip
(ecgmm_mha_weights, ecgmm_mha_rollout_step), from the kernels' own stored ``qkv`` and stored ``lse`` (the pattern of
tests/attn_ref.py and tests/attn_bounds.py).  Every attention-batch element is restated ALONE, trimmed to its own length, and
scattered into padded tensors whose padding is zero (tests/attn_varlen_ref.py): a padded position does not exist for the
reference, so NaN in the padded rows of ``qkv`` / ``v`` never reaches it.

    P[n,h,i,j] = exp(scale q_i . k_j - lse[n,h,i])                       the per-head map
    Abar[n,i,j] = (1 / heads) sum_h P[n,h,i,j]                           the head average
    y[n,j] = a v[n,j] + (1 - a) (1 / heads) sum_h sum_i v[n,i] P[n,h,i,j]   one rollout step of the row vector v

Bounds.  u = 2^-24, g_K = K u / (1 - K u), K_EXP as assumed in tests/attn_bounds.py; nothing is fitted to what the kernels give.
TINY = 2^-126, the smallest normal fp32: a result below it may be rounded to a subnormal or flushed, an absolute term.
  per head   p^ = expf(fl(fl_dot_d(q, k) scale^) - lse): the relative error ep of attn_bounds.BackwardBounds,
             ep = expm1(ds + (|s| + ds + |lse|) u + K_EXP u), ds = g_{d+3} A_s.        |p^ - P| <= ep P + TINY
  average    heads - 1 additions in a fixed order, then the product with fl(1 / heads) (its rounding and the product's: 2 u):
             |a^ - Abar| <= (1 / heads) (sum_h ep_h P_h + g_{heads+1} sum_h (1 + ep_h) P_h) + 2 TINY
  row sums   sum_j P[n,h,i,j] = exp(lse_true - lse_stored): off 1 by at most expm1(e_lse), e_lse the bound of the forward's
             lse (attn_bounds.ForwardBounds); the sum itself is taken in float64, so
             |sum_j p^_ij - 1| <= sum_j (element bound)_ij + expm1(e_lse_i)              (average: the mean over the heads)
  rollout    T_j = sum_h sum_i v_i P_hij is a dot of length heads S accumulated in some order, every term carrying ep:
             e_T = sum |v_i| ep P + g_{heads S} sum |v_i| (1 + ep) P + heads S max|v| TINY.  Then four roundings on the way to
             B = fl(1 - a) * (T^ * fl(1 / heads)) (two roundings of constants, two products), the product a v and the final
             addition (an fma makes these two one; both are counted):
             |y^ - y| <= ((1 - a) / heads) (e_T (1 + g_4) + g_4 |T|_abs) (1 + u) + u a |v_j| (1 + u) + u (a |v_j| + ((1 - a) / heads) |T|_abs) + TINY
             with |T|_abs = sum |v_i| P.
  mass       sum_j y_j - sum_i v_i = ((1 - a) / heads) sum_h sum_i v_i (rowsum_hi - 1) + the element errors:
             <= sum_j (rollout bound)_j + ((1 - a) / heads) sum_h sum_i |v_i| expm1(e_lse_hi)
"""
import numpy as np
import torch

from . import attn_bounds as AB
from . import attn_ref as AR
from . import attn_varlen_ref as VR

U, K_EXP, g_k = AB.U, AB.K_EXP, AB.g_k
TINY = 2.0 ** -126


def f32(x):
    """the fp32 value the C ABI receives for a Python float (residual)"""
    return float(np.float32(x))


class Maps:
    """P, ep [N, heads, S, S], lse and its forward bound e_lse [N, heads, S], live [N, S]; zeros in the padding.
    ``lse``: the stored fp32 [N, heads, S] of the forward, or None = the exact float64 log-sum-exp (the mathematics alone)."""

    def __init__(self, qkv, lse, S, N, heads, batch_first, lengths=None):
        E = qkv.shape[1] // 3
        self.S, self.N, self.heads, self.d, self.batch_first = S, N, heads, E // heads, bool(batch_first)
        self.lens = [S] * N if lengths is None else VR.clamp(lengths, S)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64)
        self.P, self.ep, self.s = z(N, heads, S, S), z(N, heads, S, S), z(N, heads, S, S)
        self.lse, self.e_lse = z(N, heads, S), z(N, heads, S)
        self.live = torch.arange(S)[None, :] < torch.tensor(self.lens)[:, None]
        stored = None if lse is None else lse.double().reshape(N, heads, S)
        for n, ln in enumerate(self.lens):
            if ln == 0:
                continue
            f = AR.Forward(qkv[VR.rows(S, N, n, ln, self.batch_first)], ln, 1, heads, self.batch_first)
            l = f.lse[0] if stored is None else stored[n, :, :ln]
            ds = g_k(self.d + 3) * f.As[0]
            self.s[n, :, :ln, :ln] = f.s[0]
            self.P[n, :, :ln, :ln] = torch.exp(f.s[0] - l[..., None])
            self.ep[n, :, :ln, :ln] = torch.expm1(ds + (f.s[0].abs() + ds + l.abs()[..., None]) * U + K_EXP * U)
            self.lse[n, :, :ln] = l
            self.e_lse[n, :, :ln] = AB.ForwardBounds(f).lse[0]

    # ---- values
    def average(self):
        return self.P.sum(1) / self.heads

    def weights(self, per_head):
        return self.P if per_head else self.average()

    def _v(self, v):
        """v [N, S] with the padding (which may hold NaN) replaced by 0, float64"""
        return torch.where(self.live, v.double(), torch.zeros((), dtype=torch.float64))

    def rollout_step(self, v, a):
        """-> y [N, S] float64"""
        a, v = f32(a), self._v(v)
        return a * v + (1.0 - a) * torch.einsum("ni,nij->nj", v, self.average())

    def matrix(self, a):
        """a I + (1 - a) Abar on the live positions [N, S, S] (zero rows and columns in the padding)"""
        a = f32(a)
        return a * torch.diag_embed(self.live.double()) + (1.0 - a) * self.average()

    # ---- bounds
    def weights_bound(self, per_head):
        if per_head:
            return self.ep * self.P + TINY * (self.P > 0)
        h = self.heads
        b = ((self.ep * self.P).sum(1) + g_k(h + 1) * ((1 + self.ep) * self.P).sum(1)) / h
        return b + 2 * TINY * (b > 0)

    def rowsum_bound(self, per_head):
        e = torch.expm1(self.e_lse)
        return self.weights_bound(per_head).sum(-1) + (e if per_head else e.mean(1))

    def rollout_bound(self, v, a):
        a, v = f32(a), self._v(v).abs()
        h, K = self.heads, self.heads * self.S
        T = torch.einsum("ni,nhij->nj", v, self.P)
        eT = (torch.einsum("ni,nhij->nj", v, self.ep * self.P) + g_k(K) * torch.einsum("ni,nhij->nj", v, (1 + self.ep) * self.P) +
              K * float(v.max()) * TINY)
        c = (1.0 - a) / h
        b = (c * (eT * (1 + g_k(4)) + g_k(4) * T) + U * a * v) * (1 + U) + U * (a * v + c * T) + TINY
        return b * self.live

    def mass_bound(self, v, a):
        a, va = f32(a), self._v(v).abs()
        slack = (1.0 - a) / self.heads * torch.einsum("ni,nhi->n", va, torch.expm1(self.e_lse))
        return self.rollout_bound(v, a).sum(-1) + slack


def head_average_fp32(per_head):
    """the kernel's head average restated in fp32 on the CPU: the heads 0, 1, .. added in that order, then one multiplication
    by the fp32 1 / heads.  per_head [N, heads, S, S] fp32 -> [N, S, S] fp32, to be met bit for bit."""
    assert per_head.dtype == torch.float32
    heads = per_head.shape[1]
    acc = per_head[:, 0].clone()
    for h in range(1, heads):
        acc = acc + per_head[:, h]
    return acc * torch.tensor(np.float32(1.0) / np.float32(heads))


def torch_weights(qkv, lengths, S, N, heads, batch_first, average):
    """torch's own float64 attention weights (multi_head_attention_forward, need_weights=True; identity projections, the
    packed projection is the input) with key_padding_mask[n, s] = s >= lengths[n] -> [N, S, S] or [N, heads, S, S].  Its padded
    QUERY rows still attend to the live keys (compare the live rows only)."""
    E = qkv.shape[1] // 3
    x = qkv.double().reshape(N, S, 3 * E).transpose(0, 1) if batch_first else qkv.double().reshape(S, N, 3 * E)
    eye = torch.eye(E, dtype=torch.float64)
    mask = None if lengths is None else torch.arange(S)[None, :] >= torch.tensor(VR.clamp(lengths, S))[:, None]
    _, w = torch.nn.functional.multi_head_attention_forward(
        x[..., :E], x[..., E:2 * E], x[..., 2 * E:], E, heads, in_proj_weight=None, in_proj_bias=None, bias_k=None,
        bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=eye, out_proj_bias=None, training=False,
        key_padding_mask=mask, need_weights=True, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye,
        v_proj_weight=eye, average_attn_weights=average)
    return w


def rollout_by_matrices(mats, v):
    """the explicit rollout: v (row vectors [N, S]) times the product of the layers' matrices, LAST layer first:
    v_0 = v_L M_L M_{L-1} .. M_1, with the S x S product formed first (what the vector recursion avoids)"""
    prod = mats[-1]
    for m in reversed(mats[:-1]):
        prod = prod @ m
    return torch.einsum("ni,nij->nj", v.double(), prod)
