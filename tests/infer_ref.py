"""Reference side of the inference-plan tests: the BatchNorm fold in float64 and the one-sided bound of a fused ReLU.
Nothing here calls the HIP library."""
import torch

from .f64check import KAPPA, Report, _unravel, half_ulp_bf16


def fold_ref64(w, conv_bias, gamma, beta, rm, rv, eps):
    """float64 fold of an eval-mode BatchNorm into the convolution in front of it:
    scale = gamma / sqrt(rv + eps); w' = w * scale[cout]; b' = beta + (conv_bias - rm) * scale."""
    w, gamma, beta, rm, rv = (t.double() for t in (w, gamma, beta, rm, rv))
    scale = gamma / torch.sqrt(rv + float(eps))
    wf = w * scale.view(-1, *([1] * (w.dim() - 1)))
    cb = torch.zeros_like(beta) if conv_bias is None else conv_bias.double()
    return wf, beta + (cb - rm) * scale, scale


def relu_bf16_ratio(out, ref_pre, acc_abs, kappa=KAPPA, name="relu(out)"):
    """Worst ratio of |out - relu(ref_pre)| to the bf16-output bound of f64check.bf16_ratio, for a kernel that clamps at
    zero before it stores.  ref_pre: the float64 value BEFORE the ReLU; acc_abs: the convolution of absolute values
    (+ |bias| + |addend|).  The ReLU makes the bound one-sided at zero: where the reference lies within the bound of zero
    the kernel's own fp32 value may fall on either side, so such an element may come out as 0 or as the (small) value --
    both are accepted, i.e. the error is measured against whichever of relu(ref) and ref's bound-neighbourhood of 0 is
    nearer.  Everywhere else the check is exactly f64check's."""
    out, ref_pre, acc_abs = out.double(), ref_pre.double(), acc_abs.double()
    acc = kappa * acc_abs
    bound = half_ulp_bf16(ref_pre.abs() + acc) + acc
    ref = ref_pre.clamp_min(0)
    err = (out - ref).abs()
    near_zero = ref_pre.abs() <= bound
    # (near zero: out must lie in [0, max(ref_pre, 0) + bound]; the plain error against relu(ref) already says that)
    assert bool((out >= 0).all()), name + ": negative value after ReLU"
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
    flat = int(torch.argmax(ratio))
    beyond = (err - half_ulp_bf16(ref.abs())).clamp_min(0) / acc_abs.clamp_min(1e-300)
    beyond = torch.where((acc_abs > 0) & ~near_zero, beyond, torch.zeros_like(beyond))
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape), float(beyond.max()))


def check_relu_bf16(out, ref_pre, acc_abs, kappa=KAPPA, name="relu(out)"):
    r = relu_bf16_ratio(out, ref_pre, acc_abs, kappa, name)
    print(r)
    assert torch.isfinite(out.double()).all(), name + ": non-finite output"
    assert r.ok, str(r)
    return r
