"""float64 restatement of csrc/attention.hip, from the kernel's own stored inputs (the pattern of tests/lime_ref.py).

Forward: from the packed projection ``qkv`` [rows, 3E] (fp32 as stored) and, optionally, the keep mask [N, heads, S, S].
Backward: from ``qkv``, the STORED ``out`` and ``lse`` of the forward and ``dout`` -- the probabilities are rebuilt as
exp(scale * q.k - lse) and D = dout . out exactly as the kernels rebuild them, in float64.  Row index of (s, n):
s * N + n (batch_first = False) or n * S + s (batch_first = True).  Besides the values every result carries the magnitude
sums the bounds of tests/attn_bounds.py are stated in (|q| |k|^T and so on)."""
import math

import torch


def split_heads(t, S, N, heads, batch_first):
    """[rows, heads * d] -> [N, heads, S, d] (float64)"""
    d = t.shape[1] // heads
    t = t.double().reshape(N, S, heads, d) if batch_first else t.double().reshape(S, N, heads, d).transpose(0, 1)
    return t.permute(0, 2, 1, 3)


def merge_heads(t, batch_first):
    """[N, heads, S, d] -> [rows, heads * d]"""
    N, heads, S, d = t.shape
    t = t.permute(0, 2, 1, 3)            # [N, S, heads, d]
    if not batch_first:
        t = t.transpose(0, 1)            # [S, N, heads, d]
    return t.reshape(S * N, heads * d)


class Forward:
    """q, k, v [N, heads, S, d]; s the scaled scores, As = scale |q| |k|^T; lse [N, heads, S]; P the softmax, Pd the
    probabilities after dropout; out [N, heads, S, d] and out_rows [rows, E]; Aout = Pd |v|."""

    def __init__(self, qkv, S, N, heads, batch_first, keep=None, p=0.0):
        E = qkv.shape[1] // 3
        self.S, self.N, self.heads, self.d, self.batch_first, self.p = S, N, heads, E // heads, batch_first, float(p)
        self.q, self.k, self.v = (split_heads(qkv[:, i * E:(i + 1) * E], S, N, heads, batch_first) for i in range(3))
        self.scale = 1.0 / math.sqrt(self.d)
        self.s = self.q @ self.k.transpose(-1, -2) * self.scale
        self.As = self.q.abs() @ self.k.abs().transpose(-1, -2) * self.scale
        self.lse = torch.logsumexp(self.s, dim=-1)
        self.P = torch.exp(self.s - self.lse[..., None])
        self.keep = None if keep is None else keep.double().reshape(N, heads, S, S)
        self.Pd = self.P if self.keep is None else self.P * self.keep / (1.0 - self.p)
        self.out = self.Pd @ self.v
        self.Aout = self.Pd @ self.v.abs()
        self.out_rows = merge_heads(self.out, batch_first)


class Backward:
    """dq, dk, dv [N, heads, S, d] and dqkv [rows, 3E] from the stored out [rows, E], lse [N, heads, S] and dout [rows, E]."""

    def __init__(self, qkv, out, lse, dout, S, N, heads, batch_first, keep=None, p=0.0):
        f = Forward(qkv, S, N, heads, batch_first, keep, p)
        self.f = f
        inv = 1.0 if f.keep is None else 1.0 / (1.0 - f.p)
        m = 1.0 if f.keep is None else f.keep
        self.lse = lse.double().reshape(N, heads, S)
        self.P = torch.exp(f.s - self.lse[..., None])
        self.Pd = self.P * m * inv
        self.do = split_heads(dout, S, N, heads, batch_first)
        o = split_heads(out, S, N, heads, batch_first)
        self.D = (self.do * o).sum(-1)
        self.AD = (self.do.abs() * o.abs()).sum(-1)
        self.dP = self.do @ f.v.transpose(-1, -2) * m * inv
        self.AdP = self.do.abs() @ f.v.abs().transpose(-1, -2) * m * inv
        self.dS = self.P * (self.dP - self.D[..., None])
        self.AdS = self.P * (self.dP.abs() + self.D.abs()[..., None])
        self.dq = self.dS @ f.k * f.scale
        self.dk = self.dS.transpose(-1, -2) @ f.q * f.scale
        self.dv = self.Pd.transpose(-1, -2) @ self.do
        self.dqkv = torch.cat([merge_heads(t, batch_first) for t in (self.dq, self.dk, self.dv)], dim=1)


def torch_attention(qkv, S, N, heads, batch_first):
    """the same forward through torch.nn.functional.multi_head_attention_forward in float64: identity projections (the
    packed projection is the input), [rows, E]"""
    E = qkv.shape[1] // 3
    x = qkv.double().reshape(N, S, 3 * E).transpose(0, 1) if batch_first else qkv.double().reshape(S, N, 3 * E)
    eye = torch.eye(E, dtype=torch.float64)
    out, _ = torch.nn.functional.multi_head_attention_forward(
        x[..., :E], x[..., E:2 * E], x[..., 2 * E:], E, heads, in_proj_weight=None, in_proj_bias=None, bias_k=None,
        bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=eye, out_proj_bias=None, training=False,
        need_weights=False, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    return (out.transpose(0, 1) if batch_first else out).reshape(S * N, E)      # [S, N, E] -> rows
