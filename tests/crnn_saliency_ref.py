"""Float64 restatement of ecgmm_crnn_gradcam (include/ecgmm.h, csrc/gradcam.hip) for the CRNN saliency tests: Grad-CAM of the
CRNN's last ConvBlock from the front end's output and the gradient of a logit w.r.t. it, both in the sequence layout
[B][Tp][C * Fp] (feature c * Fp + f), with live steps and live frames.  Pure torch on whichever device the operands live
on; nothing here calls the HIP library.  tests/test_crnn_saliency_cpu.py holds it to textbook Grad-CAM taken with hooks.

gradcam_bound: the per-element error an fp32 evaluation of the same chain may show, in tests/f64check.py's style (g_k(K)
times the sum of magnitudes, K counted from the kernel's own chain; see the function)."""
import torch
import torch.nn.functional as F

from .f64check import U, g_k


def _live(steps, B, Tp, device):
    if steps is None:
        return torch.ones(B, Tp, dtype=torch.bool, device=device)
    return torch.arange(Tp, device=device)[None, :] < steps.to(device).long()[:, None]


def gradcam_parts(seq, dseq, steps, C, absval=False):
    """a [B][C], the coarse map before the ReLU m_raw [B][Fp][Tp] (0 behind steps) and, with ``absval``, the same sums of
    magnitudes.  Values behind ``steps`` are never read (they may be NaN)."""
    B, Tp, feat = seq.shape
    Fp = feat // C
    live = _live(steps, B, Tp, seq.device)[:, :, None, None]
    zero = torch.zeros((), dtype=torch.float64, device=seq.device)
    A = torch.where(live, seq.double().view(B, Tp, C, Fp), zero)        # A[b][t][c][f]
    G = torch.where(live, dseq.double().view(B, Tp, C, Fp), zero)
    if absval:
        A, G = A.abs(), G.abs()
    a = G.sum((1, 3)) / (Tp * Fp)
    m = torch.einsum("bc,btcf->bft", a, A)
    return a, m


def gradcam_ref(seq, dseq, steps, frames, C, F_, T):
    """cam [B][F_][T] float64: a, m = relu(.), m / max m (all zero where the maximum is 0), F.interpolate bilinear with
    align_corners=False from (Fp, Tp) to (F_, T), columns t >= frames[b] zeroed"""
    _, m = gradcam_parts(seq, dseq, steps, C)
    m = m.clamp_min(0)
    mx = m.amax((1, 2), keepdim=True)
    m = torch.where(mx > 0, m / torch.where(mx > 0, mx, torch.ones_like(mx)), torch.zeros_like(m))
    cam = F.interpolate(m[:, None], size=(F_, T), mode="bilinear", align_corners=False)[:, 0]
    if frames is not None:
        dead = torch.arange(T, device=cam.device)[None, :] >= frames.to(cam.device).long()[:, None]
        cam = cam.masked_fill(dead[:, None, :], 0.0)
    return cam


# The kernel's chain, rounding by rounding (csrc/gradcam.hip):
#   a[b][c]     a sum of Tp * Fp terms in some fixed order (at most Tp * Fp - 1 additions on any term's path), times the
#               fp32 constant 1 / (Tp * Fp), itself rounded:                                   Tp * Fp + 1 roundings
#   m[b][f][t]  a dot product of C terms, each a[c] * seq (one rounding, or none under fma) and at most C - 1 additions:
#                                                                                              C roundings
#               so |m - m_ref| <= g_k(Tp * Fp + 1 + C) * M_abs, M_abs = sum_c |a|_abs[c] * |seq|, |a|_abs the mean of |dseq|
#               (the ReLU is 1-Lipschitz)
#   normalise   m / max, a true division: 1 rounding (and max / max is exactly 1).  The maximum's own error e_max <= the
#               largest bound(m) of the record, and moves every quotient by cam_ref * e_max / max.
#   upsample    top = c00 * (1 - lw) + c01 * lw, bot likewise, out = top * (1 - lh) + bot * lh: on any operand's path a
#               weight (1 - l: 1 rounding; l itself is exact to 1 ulp: +1), two products and two additions: 6 roundings
#               of values in [0, 1]; the blend is a convex combination, so it carries the coarse errors through without
#               growing them: the error of an output pixel <= the blend of its four corners' errors + g_k(6) * blend.
K_NORM = 1
K_BLEND = 6


def gradcam_bound(seq, dseq, steps, frames, C, F_, T):
    """per-element |cam - gradcam_ref| allowed, [B][F_][T] float64 (0 behind ``frames`` and for an all-zero map of exact
    zeros: those must be exact).  A record whose maximum is not separated from its own error bound has no bound (inf): the
    all-zero decision could go either way; the tests' inputs keep clear of it."""
    B, Tp, feat = seq.shape
    Fp = feat // C
    _, m_raw = gradcam_parts(seq, dseq, steps, C)
    _, m_abs = gradcam_parts(seq, dseq, steps, C, absval=True)
    e_m = g_k(Tp * Fp + 1 + C) * m_abs                                   # [B][Fp][Tp]
    m = m_raw.clamp_min(0)
    mx = m.amax((1, 2), keepdim=True)
    e_max = e_m.amax((1, 2), keepdim=True)
    safe = torch.where(mx > 0, mx, torch.ones_like(mx))
    q = torch.where(mx > 0, m / safe, torch.zeros_like(m))
    # |m' / mx' - m / mx| <= (e_m + q * e_max) / mx', mx' >= mx - e_max
    low = torch.where(mx > e_max, mx - e_max, torch.ones_like(mx))
    e_q = torch.where(mx > 0, (e_m + q * e_max) / low + g_k(K_NORM) * q, torch.zeros_like(m))
    # a maximum inside its own error: undecidable (inf), unless every magnitude is 0 (then everything is exactly 0)
    unsure = (mx <= e_max) & (e_max > 0)
    e_q = torch.where(unsure.expand_as(e_q), torch.full_like(e_q, float("inf")), e_q)
    up = lambda v: F.interpolate(v[:, None], size=(F_, T), mode="bilinear", align_corners=False)[:, 0]
    e = up(torch.where(torch.isfinite(e_q), e_q, torch.zeros_like(e_q))) + g_k(K_BLEND) * up(q)
    # the kernel's fp32 source coordinate (dst + 0.5) * (in / out) - 0.5 carries three roundings (the ratio, the product, the
    # subtraction; lam = src - floor is exact) of a value below max(Tp, Fp), float64's none: a blend weight moves by at most
    # 4 u * max(Tp, Fp, 2) per axis (one spare), and the output by that times the spread of its corners (<= 1), two axes
    e = e + 8 * U * max(Tp, Fp, 2)
    e = torch.where(unsure.expand(B, F_, T), torch.full_like(e, float("inf")), e)
    zero_map = (mx <= 0) & (e_max <= 0)
    e = torch.where(zero_map.expand(B, F_, T), torch.zeros_like(e), e)
    if frames is not None:
        dead = torch.arange(T, device=e.device)[None, :] >= frames.to(e.device).long()[:, None]
        e = e.masked_fill(dead[:, None, :], 0.0)
    return e
