"""float64 reference of the attention kernels with lengths (ecgmm_mha_forward_varlen / ecgmm_mha_backward_varlen): every
attention-batch element ``n`` ALONE, trimmed to its own length, through tests/attn_ref.py (``S = lengths[n]``, ``N = 1``), and
the results scattered into padded tensors whose padding is zero.  Nothing here knows about masks: a padded position simply does
not exist for the reference.  ``lengths`` are clamped to ``[0, S]`` as the kernels clamp them; an element of length 0 has no
reference (``None``) and only zeros.  The yardstick of this reference itself is torch's float64
``multi_head_attention_forward(key_padding_mask=...)`` (:func:`torch_masked`, tests/test_attention_varlen_cpu.py)."""
import torch

from . import attn_ref as AR


def clamp(lengths, S):
    return [min(max(int(v), 0), S) for v in lengths]


def rows(S, N, n, length, batch_first):
    """row indices of positions 0 .. length-1 of element n in a [S * N, ...] tensor"""
    s = torch.arange(length)
    return n * S + s if batch_first else s * N + n


def _keep_of(keep, n, ln):
    return None if keep is None else keep[n:n + 1, :, :ln, :ln]


def forward_alone(qkv, lengths, S, N, heads, batch_first, keep=None, p=0.0):
    """-> [attn_ref.Forward of element n alone (S = its length, N = 1), or None at length 0]; ``keep`` [N, heads, S, S] is the
    keep mask of the padded launch, sliced to [:len, :len]"""
    out = []
    for n, ln in enumerate(clamp(lengths, S)):
        out.append(None if ln == 0 else
                   AR.Forward(qkv[rows(S, N, n, ln, batch_first)], ln, 1, heads, batch_first, _keep_of(keep, n, ln), p))
    return out


def backward_alone(qkv, out, lse, dout, lengths, S, N, heads, batch_first, keep=None, p=0.0):
    """-> [attn_ref.Backward of element n alone from the STORED out [S * N, E] and lse [N, heads, S], or None]"""
    res = []
    lse = lse.reshape(N, heads, S)
    for n, ln in enumerate(clamp(lengths, S)):
        if ln == 0:
            res.append(None)
            continue
        r = rows(S, N, n, ln, batch_first)
        res.append(AR.Backward(qkv[r], out[r], lse[n, :, :ln].reshape(-1), dout[r], ln, 1, heads, batch_first,
                               _keep_of(keep, n, ln), p))
    return res


def scatter_forward(fs, lengths, S, N, heads, batch_first):
    """-> (out [S * N, E], lse [N, heads, S]) float64, zeros in the padding"""
    E = next(f for f in fs if f is not None).out_rows.shape[1]
    out = torch.zeros(S * N, E, dtype=torch.float64)
    lse = torch.zeros(N, heads, S, dtype=torch.float64)
    for n, (f, ln) in enumerate(zip(fs, clamp(lengths, S))):
        if f is not None:
            out[rows(S, N, n, ln, batch_first)] = f.out_rows
            lse[n, :, :ln] = f.lse[0]
    return out, lse


def scatter_backward(bs, lengths, S, N, batch_first):
    """-> dqkv [S * N, 3E] float64, zeros in the padding"""
    E3 = next(b for b in bs if b is not None).dqkv.shape[1]
    dqkv = torch.zeros(S * N, E3, dtype=torch.float64)
    for n, (b, ln) in enumerate(zip(bs, clamp(lengths, S))):
        if b is not None:
            dqkv[rows(S, N, n, ln, batch_first)] = b.dqkv
    return dqkv


def live_rows(lengths, S, N, batch_first):
    """bool [S * N]: the row is a live position"""
    m = torch.zeros(S * N, dtype=torch.bool)
    for n, ln in enumerate(clamp(lengths, S)):
        m[rows(S, N, n, ln, batch_first)] = True
    return m


def torch_masked(qkv, dout, lengths, S, N, heads, batch_first):
    """torch's own float64 attention with key_padding_mask[n, s] = s >= lengths[n] and its autograd with dout zeroed in the
    padding -> (out [S * N, E], dqkv [S * N, 3E]); padded rows hold whatever torch computes there.  Needs lengths >= 1."""
    E = qkv.shape[1] // 3
    q = qkv.double().clone().requires_grad_(True)
    x = q.reshape(N, S, 3 * E).transpose(0, 1) if batch_first else q.reshape(S, N, 3 * E)
    eye = torch.eye(E, dtype=torch.float64)
    mask = torch.arange(S)[None, :] >= torch.tensor(clamp(lengths, S))[:, None]
    out, _ = torch.nn.functional.multi_head_attention_forward(
        x[..., :E], x[..., E:2 * E], x[..., 2 * E:], E, heads, in_proj_weight=None, in_proj_bias=None, bias_k=None,
        bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=eye, out_proj_bias=None, training=False,
        key_padding_mask=mask, need_weights=False, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye,
        v_proj_weight=eye)
    out = (out.transpose(0, 1) if batch_first else out).reshape(S * N, E)
    g = dout.double() * live_rows(lengths, S, N, batch_first)[:, None]
    (out * g).sum().backward()
    return out.detach(), q.grad.detach()
