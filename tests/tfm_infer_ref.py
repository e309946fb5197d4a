"""float64 restatement of the two fused layer tails of csrc/transformer_infer.hip, from the operands the kernels read:

    linear_res_ln :  y = LayerNorm(res + a W^T + b; gamma, beta, eps)
    ffn_res_ln    :  y = LayerNorm(x + relu(x W1^T + b1) W2^T + b2; gamma, beta, eps)

with the sums of magnitudes tests/tfm_infer_bounds.py builds its bounds from, the seeded operand generator shared by the CPU
and the GPU tests, and torch-fp32 candidates with named slips (what the bounds must reject)."""
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass
class Norm:
    z: torch.Tensor        # pre-norm sum                       [R, E] float64
    mu: torch.Tensor       # its row mean                       [R, 1]
    s: torch.Tensor        # sqrt(biased variance + eps)        [R, 1]
    zhat: torch.Tensor     # (z - mu) / s                       [R, E]
    y: torch.Tensor        # zhat * gamma + beta                [R, E]
    gamma: torch.Tensor
    beta: torch.Tensor


def layer_norm64(z, gamma, beta, eps):
    z, gamma, beta = z.double(), gamma.double(), beta.double()
    mu = z.mean(-1, keepdim=True)
    s = ((z - mu).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    zhat = (z - mu) / s
    return Norm(z, mu, s, zhat, zhat * gamma + beta, gamma, beta)


@dataclass
class LinearResLn:
    n: Norm
    A: torch.Tensor        # |res| + |b| + |a| |W|^T            [R, E]
    K: int


def linear_res_ln(a, w, b, res, gamma, beta, eps):
    a, w, b, res = a.double(), w.double(), b.double(), res.double()
    z = res + a @ w.t() + b
    return LinearResLn(layer_norm64(z, gamma, beta, eps), res.abs() + b.abs() + a.abs() @ w.abs().t(), a.shape[1])


@dataclass
class FfnResLn:
    n: Norm
    h: torch.Tensor        # relu(x W1^T + b1)                  [R, ff]
    Ah: torch.Tensor       # |b1| + |x| |W1|^T                  [R, ff]
    x: torch.Tensor
    w2: torch.Tensor
    b2: torch.Tensor
    E: int
    ff: int


def ffn_res_ln(x, w1, b1, w2, b2, gamma, beta, eps):
    x, w1, b1, w2, b2 = x.double(), w1.double(), b1.double(), w2.double(), b2.double()
    h = torch.relu(x @ w1.t() + b1)
    z = x + h @ w2.t() + b2
    return FfnResLn(layer_norm64(z, gamma, beta, eps), h, b1.abs() + x.abs() @ w1.abs().t(), x, w2, b2, x.shape[1], w1.shape[0])


# ---- operands -----------------------------------------------------------------------------------------------------------
def linear_case(R, K, E, scale=1.0, seed=0, small_var=False):
    """Gaussian operands of linear_res_ln (fp32, CPU).  scale: the input scale of a and res.  small_var: rows whose pre-norm
    sum is a constant plus noise of standard deviation 1e-3 (the product and the bias scaled away), where eps decides."""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    a, w, b, res = scale * rn(R, K), rn(E, K) / K ** 0.5, 0.1 * rn(E), scale * rn(R, E)
    if small_var:
        a, b, res = 1e-5 * a, 1e-5 * b, 1.0 + 1e-3 * rn(R, E)
    return dict(a=a, w=w, b=b, res=res, gamma=1.0 + 0.1 * rn(E), beta=0.1 * rn(E))


def ffn_case(R, E, ff, scale=1.0, seed=0, small_var=False):
    g = torch.Generator().manual_seed(2000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, w1, b1, w2, b2 = scale * rn(R, E), rn(ff, E) / E ** 0.5, 0.1 * rn(ff), rn(E, ff) / ff ** 0.5, 0.1 * rn(E)
    if small_var:
        x, w2, b2 = 1.0 + 1e-3 * rn(R, E), 1e-5 * w2, 1e-5 * b2
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=1.0 + 0.1 * rn(E), beta=0.1 * rn(E))


# ---- torch-fp32 candidates, with named slips ------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).float()


def _ln32(z, gamma, beta, eps, slip):
    if slip == "half_stats":
        half = z[:, :z.shape[1] // 2]
        mu, var = half.mean(-1, keepdim=True), half.var(-1, unbiased=False, keepdim=True)
        return (z - mu) / (var + eps).sqrt() * gamma + beta
    if slip == "bf16_prenorm":
        z = _bf16(z)
    return F.layer_norm(z, (z.shape[1],), gamma, beta, 0.0 if slip == "no_eps" else eps)


def linear_candidate(c, eps, slip=None):
    """torch's fp32 evaluation of linear_res_ln on a linear_case; slip: None, "no_residual", "no_bias", "half_stats", "no_eps",
    "bf16_prenorm" """
    z = F.linear(c["a"], c["w"], None if slip == "no_bias" else c["b"])
    if slip != "no_residual":
        z = z + c["res"]
    return _ln32(z, c["gamma"], c["beta"], eps, slip)


def ffn_candidate(c, eps, slip=None):
    """torch's fp32 evaluation of ffn_res_ln on an ffn_case; slip: None, "no_residual", "no_bias" (b2), "no_relu", "half_stats",
    "no_eps", "bf16_prenorm" """
    h = F.linear(c["x"], c["w1"], c["b1"])
    if slip != "no_relu":
        h = torch.relu(h)
    z = F.linear(h, c["w2"], None if slip == "no_bias" else c["b2"])
    if slip != "no_residual":
        z = z + c["x"]
    return _ln32(z, c["gamma"], c["beta"], eps, slip)
