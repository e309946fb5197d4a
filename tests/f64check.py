"""Float64 checker for the bf16 conv kernels.

With the operands rounded to bf16, every product x * w is exact in float64 and so is any sum of a few million of them to
well below a bf16 ulp: a float64 convolution of the same operands is the exact answer.  What a kernel may deviate by is
then known per element:

  bf16 outputs (y, dx):   |out - ref| <= half_ulp_bf16(|ref| + kappa * A) + kappa * A
                          A = (|x| * |w|) [+ |bias|]  or  (|dy| *T |w|) [+ |addend|]: the same convolution of absolute
                          values.  The first term is the rounding of the stored output (half an ulp of the bf16 binade the
                          value lies in), the second the kernel's fp32 accumulation.
  fp32 weight gradients:  |dw - ref| <= eps * rms(ref) + tau * (|x|^T |dy|),  and  ||dw - ref|| <= 1e-5 ||ref||
  BatchNorm partial rows: column sums of the rows the kernel wrote against float64 sums of the reference, within the
                          accumulation bound summed over the column plus sigma times the sum of magnitudes.

The reference is autograd of F.conv2d in float64, chunked over the batch, on whichever device the operands live on
(torch's own im2col + GEMM there: MIOpen has no float64 path).  Nothing here calls the HIP library.

KAPPA, EPS_DW and SIGMA were calibrated on the MI355X with tests/test_conv_layers_f64_gpu.py: each is at most 4x the largest
value measured over every layer of the benchmarked step (below).  TAU_DW is set by torch's CPU fp32 weight gradient, whose
serial sums are longer than the kernels' split-K chunks.  The mutation test in tests/test_f64check.py shows that they still reject a zeroed tile, a neighbour's tile, a missing K slice,
a wrong image-border row, a 4-ulp error and (dw) a missing tile or a split-K chunk counted twice.
"""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

# Calibrated on the MI355X (every test of tests/test_conv_layers_f64_gpu.py), each at most 4x the largest value measured there:
# fp32 accumulation of bf16 products, relative to the convolution of absolute values (measured 7.6e-8, 1-D block 0 dx)
KAPPA = 3.0e-7
# fp32 weight gradients: floor relative to rms(ref) (measured max |err| / rms 8.6e-7, ResNet18 layer 4) ...
EPS_DW = 3.4e-6
# ... and the accumulation term relative to |x|^T |dy| (measured 1.8e-7, ResNet18 stem).  The one constant above 4x: torch's
# own fp32 weight gradient on the CPU, which the checker must accept, sums 2304 pixels serially and reaches 1.13e-6
TAU_DW = 1.4e-6
# fp32 summation of BatchNorm partial rows, relative to the column's sum of magnitudes (measured 1.0e-7, MODE-1 rows)
SIGMA = 4.0e-7
DW_REL_L2 = 1e-5


def half_ulp_bf16(v):
    """half an ulp of the bf16 binade |v| lies in (0 where v == 0): 2^(e - 9) for |v| = m * 2^e, m in [0.5, 1)"""
    v = v.abs().double()
    e = torch.frexp(v).exponent
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 9), torch.zeros_like(v))


@dataclass
class ConvRef:
    y: torch.Tensor          # conv(x, w) + bias                                    [N, Cout, OH, OW] float64
    dx: torch.Tensor         # conv^T(dy, w) + addend                               [N, Cin, H, W]
    dw: torch.Tensor         # x^T dy                                               [Cout, Cin, R, S]
    ay: torch.Tensor         # |x| * |w| + |bias|
    adx: torch.Tensor        # |dy| *T |w| + |addend|
    adw: torch.Tensor        # |x|^T |dy|


def conv_ref64(x, w, dy, stride=1, padding=(1, 1), bias=None, addend=None, chunk=32):
    """float64 y, dx, dw of F.conv2d and the same of |x|, |w|, |dy| (the accumulation bounds), chunked over the batch.
    x [N, Cin, H, W], w [Cout, Cin, R, S], dy [N, Cout, OH, OW] (any float dtype, values taken as given) on any device;
    dy may be None (forward only).  bias [Cout] is added to y, addend [N, Cin, H, W] to dx."""
    N = x.shape[0]
    w64 = w.double()
    b64 = None if bias is None else bias.double()
    outs = {k: [] for k in ("y", "dx", "ay", "adx")}
    dw = torch.zeros_like(w64)
    adw = torch.zeros_like(w64)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        for absval in (False, True):
            xc = x[lo:hi].double()
            wc = w64
            bc = b64
            if absval:
                xc, wc = xc.abs(), wc.abs()
                bc = None if bc is None else bc.abs()
            xc = xc.requires_grad_(dy is not None)
            wc = wc.detach().requires_grad_(dy is not None)
            y = F.conv2d(xc, wc, bc, stride=stride, padding=padding)
            if dy is not None:
                g = dy[lo:hi].double()
                y.backward(g.abs() if absval else g)
                d = xc.grad
                if addend is not None:
                    a = addend[lo:hi].double()
                    d = d + (a.abs() if absval else a)
                outs["adx" if absval else "dx"].append(d.detach())
                (adw if absval else dw).add_(wc.grad)
            outs["ay" if absval else "y"].append(y.detach())
    cat = {k: torch.cat(v) if v else None for k, v in outs.items()}
    return ConvRef(cat["y"], cat["dx"], dw if dy is not None else None, cat["ay"], cat["adx"],
                   adw if dy is not None else None)


@dataclass
class Report:
    name: str
    ratio: float             # worst |err| / bound (<= 1 passes)
    where: tuple             # (image, channel, pixel row, pixel column) of the worst element (index tuple for dw)
    kappa_seen: float = 0.0  # worst |err| beyond the rounding term, over the accumulation bound (the measured kappa / tau)

    @property
    def ok(self):
        return self.ratio <= 1.0

    def __str__(self):
        return "%-34s worst ratio %.3g at %s (accumulation term %.3g)" % (self.name, self.ratio, self.where, self.kappa_seen)


def _unravel(flat, shape):
    idx = []
    for s in reversed(shape):
        idx.append(int(flat % s))
        flat //= s
    return tuple(reversed(idx))


def bf16_ratio(out, ref, acc_abs, kappa=KAPPA, name="out"):
    """worst ratio of |out - ref| to the bf16-output bound; out, ref, acc_abs: same shape (NCHW)"""
    out, ref, acc_abs = out.double(), ref.double(), acc_abs.double()
    err = (out - ref).abs()
    acc = kappa * acc_abs
    bound = half_ulp_bf16(ref.abs() + acc) + acc
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
    flat = int(torch.argmax(ratio))
    worst = float(ratio.reshape(-1)[flat])
    # the accumulation error the worst-over-rounding element shows, in units of the |.| convolution
    beyond = (err - half_ulp_bf16(ref.abs())).clamp_min(0) / acc_abs.clamp_min(1e-300)
    beyond = torch.where(acc_abs > 0, beyond, torch.zeros_like(beyond))
    return Report(name, worst, _unravel(flat, ref.shape), float(beyond.max()))


def check_bf16(out, ref, acc_abs, kappa=KAPPA, name="out"):
    r = bf16_ratio(out, ref, acc_abs, kappa, name)
    print(r)
    assert torch.isfinite(out.double()).all(), name + ": non-finite output"
    assert r.ok, str(r)
    return r


def dw_ratio(dw, ref, acc_abs, eps=EPS_DW, tau=TAU_DW, name="dw"):
    dw, ref, acc_abs = dw.double(), ref.double(), acc_abs.double()
    err = (dw - ref).abs()
    floor = eps * float(ref.pow(2).mean().sqrt())
    bound = floor + tau * acc_abs
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
    flat = int(torch.argmax(ratio))
    # measured constants, each term on its own: max |err| / (|x|^T |dy|) and max |err| / rms(ref)
    seen = float((err / acc_abs.clamp_min(1e-300)).max())
    r = Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape), seen)
    r.eps_seen = float(err.max()) / max(floor / eps, 1e-300)
    r.rel_l2 = float((dw - ref).norm() / ref.norm().clamp_min(1e-300))
    return r


def check_dw(dw, ref, acc_abs, eps=EPS_DW, tau=TAU_DW, name="dw"):
    r = dw_ratio(dw, ref, acc_abs, eps, tau, name)
    print(r, " rel L2 %.3g, max|err| / rms %.3g" % (r.rel_l2, r.eps_seen))
    assert torch.isfinite(dw.double()).all(), name + ": non-finite weight gradient"
    assert r.rel_l2 <= DW_REL_L2, "%s: relative L2 error %.3g > %g" % (name, r.rel_l2, DW_REL_L2)
    assert r.ok, str(r)
    return r


def colsum_ratio(got, want, slack, mag, sigma=SIGMA, name="rows"):
    """got, want [C]: column sums (kernel rows, float64 reference); slack [C]: what the per-element accumulation bound
    allows for the column; mag [C]: sum of magnitudes of the summands (the fp32 summation term)"""
    got, want = got.double(), want.double()
    err = (got - want).abs()
    bound = slack.double() + sigma * mag.double()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
    c = int(torch.argmax(ratio))
    seen = float(((err - slack.double()).clamp_min(0) / mag.double().clamp_min(1e-300)).max())
    return Report(name, float(ratio[c]), ("channel", c), seen)


def check_colsums(got, want, slack, mag, sigma=SIGMA, name="rows"):
    r = colsum_ratio(got, want, slack, mag, sigma, name)
    print(r)
    assert torch.isfinite(got.double()).all(), name + ": non-finite partial rows"
    assert r.ok, str(r)
    return r


def stats_ref(ref, kappa=KAPPA):
    """reference column sums of a forward's statistics rows (sum y, sum y^2 over N, H, W) and their slack: the rows are
    taken from the fp32 accumulators, so each value may be off by kappa * A (not by the bf16 rounding)"""
    y, a = ref.y, kappa * ref.ay
    dims = (0, 2, 3)
    s1, s2 = y.sum(dims), (y * y).sum(dims)
    slack1 = a.sum(dims)
    slack2 = (2 * y.abs() * a + a * a).sum(dims)
    return (s1, s2), (slack1, slack2), (y.abs().sum(dims), (y * y).sum(dims))


def check_stats(rows, ref, name="stats"):
    """rows [n][2][C] fp32 as the kernel wrote them"""
    rows = rows.double()
    (s1, s2), (k1, k2), (m1, m2) = stats_ref(ref)
    check_colsums(rows[:, 0].sum(0), s1, k1, m1, name=name + " sum y")
    check_colsums(rows[:, 1].sum(0), s2, k2, m2, name=name + " sum y^2")


def bnred_ref(dx_stored, y, coef, mask=None):
    """float64 sums of the BatchNorm-backward reduction over what a dgrad stored: g = [relu mask] * dx,
    (sum g, sum g * (y - mean)) per channel.  dx_stored, y, mask: [N, C, H, W]; coef [4][C] (scale, shift, mean, invstd).
    mask None: the mask is bn(y) > 0.  Returns the sums, their slack (elements whose mask is decided within fp32 rounding
    of zero may go either way) and the sums of magnitudes."""
    d, yv = dx_stored.double(), y.double()
    sc, sh, mu = (coef[i].double().view(1, -1, 1, 1) for i in range(3))
    if mask is None:
        z = yv * sc + sh
        m = z > 0
        unsure = z.abs() <= 1e-6 * ((yv * sc).abs() + sh.abs())
    else:
        m = mask.double() > 0
        unsure = torch.zeros_like(m)
    g = torch.where(m, d, torch.zeros_like(d))
    dev = yv - mu
    dims = (0, 2, 3)
    sums = (g.sum(dims), (g * dev).sum(dims))
    u = unsure.double()
    slack = ((d.abs() * u).sum(dims), (d.abs() * dev.abs() * u).sum(dims))
    mags = (g.abs().sum(dims), (g * dev).abs().sum(dims))
    return sums, slack, mags


def check_bnred(rows, dx_stored, y, coef, mask=None, name="bnred"):
    rows = rows.double()
    sums, slack, mags = bnred_ref(dx_stored, y, coef, mask)
    check_colsums(rows[:, 0].sum(0), sums[0], slack[0], mags[0], name=name + " sum g")
    check_colsums(rows[:, 1].sum(0), sums[1], slack[1], mags[1], name=name + " sum g(y-mu)")
