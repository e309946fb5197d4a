"""Float64 checkers: the bf16 conv kernels (below), the BatchNorm / pooling passes, the fp32 dense tails, the LSTM
recurrence, the TabNet clinical branch, the ops that run only inside the encoder launch plans, the fp32-operand conv
kernels, the two elementwise passes of the inference plans and the Grad-CAM map kernels of the two ResNet encoders (their own
sections further down, each with its bounds derived in a header comment).


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
import copy
import functools
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
    """half an ulp of the bf16 binade |v| lies in (0 where v == 0): 2^(e - 9) for |v| = m * 2^e, m in [0.5, 1).
    Below the smallest normal number 2^-126 bf16 is evenly spaced by 2^-133 (its subnormals share fp32's exponent range), so
    the half ulp stays at 2^-134 there.  (Found by tests/test_infer_chain_gpu.py: a squeeze-excite gate that saturates to a
    subnormal fp32 value gives a subnormal product, which the device rounds to the nearest bf16 subnormal as torch does.)"""
    v = v.abs().double()
    e = torch.frexp(v).exponent.clamp_min(-125)
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


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm and pooling passes (csrc/elementwise.hip, csrc/bn_eval_bwd.hip), tensors channels-last: [M rows][C] for the
# BatchNorm passes, [N][H][W][C] for the pooling passes.  Operands are taken as given (bf16-rounded where the kernel
# reads bf16), a pass that consumes another pass's fp32 output (coef rows, partial rows, pooled / idx, dbeta / dgamma)
# gets that output as its given input, and the float64 evaluation of the same formula is the exact answer.
#
#   stored tensors (out, dy, dz):  |got - ref| <= round_T(|ref| + g_K * A) + g_K * A
#       A: the same expression on absolute values, g_K = K u / (1 - K u), u = 2^-24, K = the number of fp32 roundings on
#       the longest operand-to-result path (an fma only removes one), round_T = half_ulp_bf16 (bf16) or u |.| (fp32)
#   sums (partial rows, dgamma, dbeta, dbias):  colsum_ratio with sigma = g_K, K = the per-element roundings plus the
#       longest chain of fp32 additions: ceil(M / (rows * rpi)) in the thread + rpi in the block fold (chain_len; rows as
#       the library reports them, rpi = threads / (C / vec)) + 1 where a double sum is rounded to fp32 at the end
#   coef: the sum bounds carried through mean = s1 / M, var = s2 / M - mean^2, invstd = 1 / sqrt(var + eps) (coef_ref)
#
# Every K below is the derived worst case, none is tightened; measured on the MI355X over tests/test_bn_pool_f64_gpu.py
# the worst ratio to these bounds is recorded in that file's docstring.  All of them accept torch's own fp32 evaluation
# of the same formulas on the CPU, stored as fp32 and as bf16 (tests/test_f64check.py: test_bn_pool_checkers_accept_torch_fp32
# for the statistics, coef, K_ACT, K_DZ, K_DZXHAT, K_DY and the sums; test_eval_backward_checker_accepts_torch_fp32 for
# K_EVAL_DY; test_pool_checkers_accept_torch for K_AFFINE and K_POOL_DZ; test_fused_stem_backward_checker_accepts_torch_fp32
# for K_POOL_RED and K_POOL_DY).
# ----------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
# |y * scale + shift| decided within this many roundings of zero: the mask / the all-zero window may go either way
K_AFFINE = 2                 # y * scale, + shift
# out = relu((y * scale + shift) * gate + (res * rscale + rshift)): y * scale, + shift, * gate, [res * rscale, + rshift,] + -> 4
# on the path from y, 3 from res; the stored rounding is round_T
K_ACT = 4
# dz = dout * gate + addc: 2
K_DZ = 2
# xhat = (y - mean) * invstd: 2;  dz * xhat: K_DZ + 2 + 1
K_DZXHAT = K_DZ + 3
# dy = k1 * ((dz - k2) - xhat * k3), k2 = (float)(s1 / M) against dbeta / M: 2, k1 = gamma * invstd: 1.
#   from dz: 2 + sub + sub + mul = 5;  from xhat or k3: 2 + mul + sub + mul = 5;  from k2: 2 + sub + sub + mul = 5
K_DY = 5
# eval mode: dy = dz * scale: K_DZ + 1
K_EVAL_DY = K_DZ + 1
# fused stem backward: dy = k1 * z + (bn * y + an), z = up to 4 routed terms (3 adds), bn = -(k1 * k3) * invstd,
# an = -(k1 * k2) - bn * mean.  Longest path, from k3 (2 roundings of its own): k1 * k3, * invstd, bn * mean, an's subtraction,
# (bn * y) + an, + k1 * z = 2 + 6 = 8
K_POOL_DY = 8
# its reduction: g * (p - beta) * (1 / scale), beta = shift + mean * scale: 2, p - beta: 1, g *: 1, 1 / scale: 1, * rsc: 1 -> 6
K_POOL_RED = 6
# max-pool backward: up to four routed terms, three additions
K_POOL_DZ = 3
UNSURE_CAP = 1e-4


def g_k(K):
    """(1 + u)^K - 1 <= K u / (1 - K u)"""
    return K * U / (1.0 - K * U)


def round_T(v, bf16):
    return half_ulp_bf16(v) if bf16 else U * v.abs().double()


def chain_len(M, rows, C, vec, threads):
    """longest chain of fp32 additions behind one column of `rows` partial rows: the thread's own rows, then the fold of
    the block's rpi threads that share the channel chunk (vec = 8 bf16 / 4 fp32 channels per thread)"""
    rpi = threads // (C // vec)
    return -(-M // (rows * rpi)) + rpi


def _ratio(err, bound):
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))


def stored_ratio(got, ref, acc_abs, K, bf16, name="out", skip=None):
    """worst ratio of |got - ref| to the stored-tensor bound; skip: elements left out (unsure ReLU masks)"""
    got, ref, acc_abs = got.double(), ref.double(), acc_abs.double()
    err = (got - ref).abs()
    acc = g_k(K) * acc_abs
    ratio = _ratio(err, round_T(ref.abs() + acc, bf16) + acc)
    seen = torch.where(acc_abs > 0, (err - round_T(ref, bf16)).clamp_min(0) / (U * acc_abs).clamp_min(1e-300), torch.zeros_like(err))
    if skip is not None:
        ratio, seen = ratio.masked_fill(skip, 0.0), seen.masked_fill(skip, 0.0)
    flat = int(torch.argmax(ratio))
    seen = seen[torch.isfinite(seen)]
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape), float(seen.max()) if seen.numel() else 0.0)


def check_stored(got, ref, acc_abs, K, bf16, name="out", skip=None):
    """(the accumulation term printed is the error beyond the stored rounding in units of u * A: the measured K)"""
    r = stored_ratio(got, ref, acc_abs, K, bf16, name, skip)
    print(r)
    assert r.ok, str(r)
    return r


def check_sum(got, want, mag, K, name, slack=None):
    return check_colsums(got, want, torch.zeros_like(mag) if slack is None else slack, mag, sigma=g_k(K), name=name)


def check_unsure(unsure, name):
    share = float(unsure.double().mean())
    assert share <= UNSURE_CAP, "%s: %.3g of the elements have a ReLU mask decided inside fp32 rounding" % (name, share)
    return share


def per_row(v, rows_per_sample, M):
    """[N][C] per-sample values -> [M][C]"""
    return v.double().repeat_interleave(rows_per_sample, 0)[:M]


def colstats_ref(y):
    """(sum y, sum y^2) over the rows of y [M][C] and the sums of magnitudes"""
    y = y.double()
    return (y.sum(0), (y * y).sum(0)), (y.abs().sum(0), (y * y).sum(0))


def check_colstats(rows, y, K, name="col_stats"):
    """rows [n][2][C] as the kernel wrote them; K = chain_len(...); y * y is one more rounding"""
    (s1, s2), (m1, m2) = colstats_ref(y)
    rows = rows.double()
    a = check_sum(rows[:, 0].sum(0), s1, m1, K, name + " sum y")
    b = check_sum(rows[:, 1].sum(0), s2, m2, K + 1, name + " sum y^2")
    return max(a.ratio, b.ratio)


def f32(v):
    """a Python float as the fp32 value the kernel receives"""
    return float(torch.tensor(v, dtype=torch.float32))


@dataclass
class CoefRef:
    val: dict                # scale, shift, mean, invstd, rm, rv: float64 [C]
    bound: dict              # the allowed |error| of each


def coef_ref(s1, s2, M, gamma, beta, eps, rm0=None, rv0=None, momentum=0.1, ds1=None, ds2=None):
    """BatchNorm finalize in float64 from the column sums s1, s2 [C] known to within ds1, ds2 (None: exact), with the
    allowed error of every output.  The kernel sums the rows and forms mean / var / invstd in double (relative 2^-50
    covers it) and rounds to fp32 where it stores:
      mean   : ds1 / M, + 1 rounding
      var    : dvar = ds2 / M + (2 |mean| + ds1 / M) ds1 / M       <- the term that grows with mean^2 / var
      invstd : relative 1 / sqrt(1 - dvar / (var + eps)) - 1  (= 0.5 dvar / (var + eps) to first order), + 1 rounding
      scale  = gamma * invstd: + 1;   shift = beta - mean * scale: mean (1), scale (2), product, difference
      running_mean = (1 - m) * rm0 + m * mean: 3 roundings on either path;  running_var likewise from the unbiased
      variance var * M / (M - 1) (var itself for M == 1)."""
    s1, s2, g, b = s1.double(), s2.double(), gamma.double(), beta.double()
    z = torch.zeros_like(s1)
    ds1 = z if ds1 is None else ds1.double()
    ds2 = z if ds2 is None else ds2.double()
    tiny = 2.0 ** -50
    eps, mom = f32(eps), f32(momentum)
    mean = s1 / M
    dm = ds1 / M + tiny * mean.abs()
    ex2 = s2 / M
    var = (ex2 - mean * mean).clamp_min(0)
    dvar = ds2 / M + (2 * mean.abs() + dm) * dm + tiny * (ex2.abs() + mean * mean)
    w = var + eps
    invstd = 1.0 / w.sqrt()
    t = dvar / w
    rel = torch.where(t < 1, 1.0 / (1 - t).clamp_min(1e-300).sqrt() - 1, torch.full_like(t, float("inf")))
    d_inv = invstd * (rel + g_k(1) * (1 + rel))
    scale = g * invstd
    d_scale = g.abs() * invstd * (rel + g_k(2) * (1 + rel))
    d_mean = dm + U * (mean.abs() + dm)
    shift = b - mean * scale
    prod, d_prod = (mean * scale).abs(), mean.abs() * d_scale + scale.abs() * d_mean + d_mean * d_scale
    d_shift = d_prod + g_k(2) * (b.abs() + prod + d_prod)
    val = dict(scale=scale, shift=shift, mean=mean, invstd=invstd)
    bound = dict(scale=d_scale, shift=d_shift, mean=d_mean, invstd=d_inv)
    if rm0 is not None:
        unb = var * M / (M - 1) if M > 1 else var
        d_unb = dvar * M / (M - 1) if M > 1 else dvar
        val["rm"] = (1 - mom) * rm0.double() + mom * mean
        bound["rm"] = mom * dm + g_k(3) * ((1 - mom) * rm0.double().abs() + mom * (mean.abs() + dm))
        val["rv"] = (1 - mom) * rv0.double() + mom * unb
        bound["rv"] = mom * d_unb + g_k(3) * ((1 - mom) * rv0.double().abs() + mom * (unb + d_unb))
    return CoefRef(val, bound)


def coef_ratio(coef, ref, rm=None, rv=None, name="coef"):
    """coef [4][C] (scale, shift, mean, invstd) as stored -> worst |err| / bound and the quantity / channel it is at"""
    got = dict(scale=coef[0], shift=coef[1], mean=coef[2], invstd=coef[3])
    if rm is not None:
        got["rm"], got["rv"] = rm, rv
    worst = Report(name, 0.0, ("", 0))
    for k, v in got.items():
        ratio = _ratio((v.double() - ref.val[k]).abs(), ref.bound[k])
        c = int(torch.argmax(ratio))
        if float(ratio[c]) >= worst.ratio:
            worst = Report(name, float(ratio[c]), (k, c))
    return worst


def check_coef(coef, ref, rm=None, rv=None, name="coef"):
    r = coef_ratio(coef, ref, rm, rv, name)
    print(r)
    assert r.ok, str(r)
    return r


def bn_act_ref(y, scale, shift, res=None, rscale=None, rshift=None, gate=None, relu=False):
    """out = relu?((y * scale + shift) * gate + res * rscale + rshift) and the same on absolute values; y, res, gate [M][C]
    (gate already per row), the coefficients [C]"""
    y = y.double()
    ref = y * scale.double() + shift.double()
    A = y.abs() * scale.double().abs() + shift.double().abs()
    if gate is not None:
        ref, A = ref * gate.double(), A * gate.double().abs()
    if res is not None:
        r = res.double()
        rs = torch.ones_like(scale.double()) if rscale is None else rscale.double()
        rb = torch.zeros_like(rs) if rshift is None else rshift.double()
        ref, A = ref + r * rs + rb, A + r.abs() * rs.abs() + rb.abs()
    return (ref.clamp_min(0) if relu else ref), A


def affine_mask(y, scale, shift):
    """the recomputed ReLU mask bn(y) > 0 and the elements whose sign fp32 may decide either way"""
    y = y.double()
    z = y * scale.double() + shift.double()
    A = y.abs() * scale.double().abs() + shift.double().abs()
    return z > 0, z.abs() <= g_k(K_AFFINE) * A


def bn_dz_ref(dout, mask=None, gate=None, addc=None):
    """dz = [mask] * dout * gate + addc and the same on absolute values (gate, addc [M][C], per row); the masked dout on
    its own is what dz_out stores, exactly"""
    d = dout.double()
    if mask is not None:
        d = torch.where(mask, d, torch.zeros_like(d))
    masked = d
    A = d.abs()
    if gate is not None:
        d, A = d * gate.double(), A * gate.double().abs()
    if addc is not None:
        d, A = d + addc.double(), A + addc.double().abs()
    return d, A, masked


def xhat_ref(y, coef):
    return (y.double() - coef[2].double()) * coef[3].double()


def bn_bwd_sums_ref(dz, A, xhat, unsure=None, dswing=None):
    """(sum dz, sum dz * xhat), the slack of the unsure elements (dswing: what flipping their mask changes dz by) and the
    sums of magnitudes"""
    sums = (dz.sum(0), (dz * xhat).sum(0))
    mags = (A.sum(0), (A * xhat.abs()).sum(0))
    if unsure is None:
        z = torch.zeros_like(sums[0])
        return sums, (z, z), mags
    sw = dswing.abs() * unsure.double()
    return sums, (sw.sum(0), (sw * xhat.abs()).sum(0)), mags


def bn_dy_ref(dz, A, xhat, k1, k2, k3):
    """dy = k1 * (dz - k2 - xhat * k3) and the same on absolute values"""
    k1, k2, k3 = k1.double(), k2.double(), k3.double()
    return k1 * (dz - k2 - xhat * k3), k1.abs() * (A + k2.abs() + xhat.abs() * k3.abs())


def bn_eval_dy_ref(dz, A, scale):
    return dz * scale.double(), A * scale.double().abs()


# ---- 3x3 / stride 2 / pad 1 max-pool fused with BatchNorm + ReLU ----
def pool_taps(a, fill):
    """a [N][H][W][C] float64 -> [N][OH][OW][9][C]: the nine taps (kh * 3 + kw) of every window, `fill` outside the image"""
    N, H, W, C = a.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = torch.full((N, 2 * OH + 1, 2 * OW + 1, C), float(fill), dtype=a.dtype, device=a.device)
    p[:, 1:H + 1, 1:W + 1] = a
    return torch.stack([p[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)], dim=3)


def pool_fwd_ratio(pooled, idx, y, scale, shift, bf16, name="maxpool"):
    """pooled, idx [N][OH][OW][C] as the kernel stored them against a64 = relu(y * scale + shift) in float64:
    pooled within the stored bound (K_AFFINE) of the window maximum; idx an in-image tap whose a64 is within that bound of
    the maximum; where idx names a tap that ties the maximum exactly, it is the earliest such tap (windows holding an
    element whose sign fp32 may decide either way are left out of this last rule).
    bf16: the taps are compared as stored, i.e. after rounding to bf16 (torch's own pooling of a bf16 activation does the
    same), and the earliest tap whose ROUNDED value is the largest wins.  Its fp32 value then lies within one bf16 ulp -- two
    half ulps -- below the largest fp32 value, each of the two within the accumulation term of its a64: the tap bound is
    twice the stored bound.  (Found by tests/test_plan_replay_gpu.py: behind a BatchNorm scale below 1 several bf16 conv
    outputs land in one bf16 cell of the activation; the hash inputs of pool_inputs, scale >= 0.7 and a negative shift, never
    do.)"""
    y = y.double()
    z = y * scale.double() + shift.double()
    A = y.abs() * scale.double().abs() + shift.double().abs()
    unsure = z.abs() <= g_k(K_AFFINE) * A
    check_unsure(unsure, name)
    T, TA = pool_taps(z.clamp_min(0), float("-inf")), pool_taps(A, 0.0)
    TU = pool_taps(unsure.double(), 0.0).amax(3) > 0
    mx, acc = T.amax(3), g_k(K_AFFINE) * TA.amax(3)
    bound = round_T(mx + acc, bf16) + acc
    r_val = _ratio((pooled.double() - mx).abs(), bound)
    ix = idx.long()
    sel = T.gather(3, ix.clamp(0, 8).unsqueeze(3)).squeeze(3)
    in_range = (ix < 9) & torch.isfinite(sel)
    r_tap = torch.where(in_range, _ratio(mx - torch.where(in_range, sel, mx), 2 * bound if bf16 else bound),
                        torch.full_like(mx, float("inf")))
    first = (T == mx.unsqueeze(3)).double().argmax(3)
    late = in_range & (sel == mx) & (ix != first) & ~TU
    ratio = torch.where(late, torch.full_like(mx, float("inf")), torch.maximum(r_val, r_tap))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    flat = int(torch.argmax(ratio))
    r = Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, mx.shape))
    r.parts = dict(value=float(r_val.max()), tap=float(r_tap.max()), late_ties=int(late.sum()))
    r.ties = int(((T == mx.unsqueeze(3)).sum(3) > 1).sum())
    return r


def check_pool_fwd(pooled, idx, y, scale, shift, bf16, name="maxpool"):
    r = pool_fwd_ratio(pooled, idx, y, scale, shift, bf16, name)
    print(r, r.parts, "windows with exact ties: %d" % r.ties)
    assert r.ok, str(r) + " " + str(r.parts)
    return r


def pool_bwd_ref(dp, pooled, idx, H, W):
    """float64 scatter of dp into the taps idx names, for windows with pooled > 0: dz [N][H][W][C] and sum |terms|"""
    N, OH, OW, C = dp.shape
    dev_ = dp.device
    ix = idx.long()
    n = torch.arange(N, device=dev_).view(N, 1, 1, 1)
    h = 2 * torch.arange(OH, device=dev_).view(1, OH, 1, 1) - 1 + ix // 3
    w = 2 * torch.arange(OW, device=dev_).view(1, 1, OW, 1) - 1 + ix % 3
    c = torch.arange(C, device=dev_).view(1, 1, 1, C)
    ok = (pooled.double() > 0) & (ix < 9) & (h >= 0) & (h < H) & (w >= 0) & (w < W)
    flat = (((n * H + h) * W + w) * C + c)[ok]
    v = dp.double()[ok]
    dz = torch.zeros(N * H * W * C, dtype=torch.float64, device=dev_).index_add_(0, flat, v)
    mag = torch.zeros_like(dz).index_add_(0, flat, v.abs())
    return dz.view(N, H, W, C), mag.view(N, H, W, C)


def pool_bwd_ratio(dz, dp, pooled, idx, bf16, name="maxpool bwd"):
    """|dz - ref| <= half an ulp of the stored type + K_POOL_DZ u sum |terms|"""
    ref, mag = pool_bwd_ref(dp, pooled, idx, dz.shape[1], dz.shape[2])
    ratio = _ratio((dz.double() - ref).abs(), round_T(ref, bf16) + K_POOL_DZ * U * mag)
    flat = int(torch.argmax(ratio))
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape))


def check_pool_bwd(dz, dp, pooled, idx, bf16, name="maxpool bwd"):
    r = pool_bwd_ratio(dz, dp, pooled, idx, bf16, name)
    print(r)
    assert r.ok, str(r)
    return r


def pool_red_ref(dp, pooled, coef):
    """the fused stem backward's reduction over windows: g = dp * [pooled > 0];  sum g  and
    invstd * sum g * (pooled - beta) / scale with beta = shift + mean * scale (0 where scale == 0), and their magnitudes"""
    sc, sh, mu, inv = (coef[i].double() for i in range(4))
    p = pooled.double()
    g = torch.where(p > 0, dp.double(), torch.zeros_like(p))
    rsc = torch.where(sc != 0, 1.0 / sc, torch.zeros_like(sc))
    dims = (0, 1, 2)
    s1, s2 = g.sum(dims), (g * (p - (sh + mu * sc)) * rsc).sum(dims) * inv
    m2 = (g.abs() * (p.abs() + sh.abs() + (mu * sc).abs()) * rsc.abs()).sum(dims) * inv.abs()
    return (s1, s2), (g.abs().sum(dims), m2)


def pool_dy_ref(dz, mag, y, coef, k1, k2, k3):
    """dy of the fused stem backward as the kernel forms it: k1 * dz + (bn * y + an), an = -(k1 * k2) - bn * mean,
    bn = -(k1 * k3) * invstd; the reference is the float64 value, A follows the kernel's own (uncentred) expression"""
    mu, inv = coef[2].double(), coef[3].double()
    k1, k2, k3 = k1.double(), k2.double(), k3.double()
    yv = y.double()
    bn = -(k1 * k3) * inv
    ref = k1 * dz + bn * yv - k1 * k2 - bn * mu
    A = k1.abs() * mag + bn.abs() * yv.abs() + (k1 * k2).abs() + (bn * mu).abs()
    return ref, A


def check_bn_bwd(dout, y, coef, gamma, bf16, K_sum, dgamma, dbeta, dy=None, dz_out=None, dbias=None, K_bias=None,
                 maskref=None, gate=None, addc=None, name="bn_bwd"):
    """Every output of one BatchNorm-backward call against float64.  dout, y [M][C] as given; coef [4][C] the forward's
    stored fp32 coefficients; maskref: None, the string "y" (mask = bn(y) > 0, recomputed) or a tensor (mask = maskref > 0);
    gate, addc [M][C] per row.  K_sum = chain_len(...) of the reduction rows, K_bias that of the dy rows.
    dgamma / dbeta: K_DZXHAT / K_DZ per element + K_sum + 1 (the double sum of the rows stored as fp32).
    dy: given the kernel's own k2 = dbeta / M, k3 = dgamma / M (K_DY).  dz_out: the masked dout, exactly.
    dbias: the float64 sum of the dy values stored (K_bias + 1).  Returns {output: worst ratio}."""
    M = y.shape[0]
    unsure, mask = None, None
    if isinstance(maskref, str):
        mask, unsure = affine_mask(y, coef[0], coef[1])
        check_unsure(unsure, name)
    elif maskref is not None:
        mask = maskref.double() > 0
    dz, A, masked = bn_dz_ref(dout, mask, gate, addc)
    xh = xhat_ref(y, coef)
    swing = None if unsure is None else (dout.double() * (1 if gate is None else gate.double()))
    sums, slack, mags = bn_bwd_sums_ref(dz, A, xh, unsure, swing)
    out = {}
    if dbeta is not None:
        out["dbeta"] = check_sum(dbeta, sums[0], mags[0], K_DZ + K_sum + 1, name + " dbeta", slack[0]).ratio
        out["dgamma"] = check_sum(dgamma, sums[1], mags[1], K_DZXHAT + K_sum + 1, name + " dgamma", slack[1]).ratio
    if dz_out is not None:
        bad = (dz_out.double() != masked)
        if unsure is not None:
            bad &= ~unsure
        assert not bool(bad.any()), "%s dz_out: %d elements are not the masked gradient" % (name, int(bad.sum()))
        out["dz_out"] = 0.0
    if dy is not None:
        k1 = gamma.double() * coef[3].double()
        ref, Ady = bn_dy_ref(dz, A, xh, k1, dbeta.double() / M, dgamma.double() / M)
        out["dy"] = check_stored(dy, ref, Ady, K_DY, bf16, name + " dy", skip=unsure).ratio
    if dbias is not None:
        s = dy.double()
        out["dbias"] = check_sum(dbias, s.sum(0), s.abs().sum(0), K_bias + 1, name + " dbias").ratio
    return out


# ---- input families of tests/test_bn_pool_f64_gpu.py (hash-filled; tests/test_f64check.py verifies on the CPU that the
#      float64 reference alone keeps the unsure-mask share of each under UNSURE_CAP) ----
def _b(t, bf16):
    """tests/util.bf16_round, behind a switch (util imports the HIP library's ctypes layer; nothing in this file may, so
    that the checker and its CPU tests load without the built library)"""
    return t.to(torch.bfloat16).float() if bf16 else t


def bn_inputs(M, C, bf16, rows_per_sample=None, mean_ratios=None):
    """y, res, dout [M][C], gamma, beta, rscale, rshift [C], gate, addc [N][C] (N samples of rows_per_sample rows).
    mean_ratios: channel c gets mean = mean_ratios[c % len] * std (sign alternating) instead of 0.5"""
    from oracle import fill
    h = fill.hash_tensor
    y = h((M, C), 31, 2.0)
    if mean_ratios is None:
        y = y + 0.5
    else:
        c = torch.arange(C)
        r = torch.tensor(mean_ratios, dtype=torch.float32)[c % len(mean_ratios)]
        y = y + (r * (2.0 / 3 ** 0.5) * (1 - 2 * ((c // len(mean_ratios)) % 2).float()))[None]
    rps = rows_per_sample or M
    N = -(-M // rps)
    d = dict(y=_b(y, bf16), res=_b(h((M, C), 32), bf16), dout=_b(h((M, C), 37), bf16), gamma=1 + 0.2 * h((C,), 35),
             beta=0.1 * h((C,), 36), rscale=1 + 0.3 * h((C,), 38), rshift=0.2 * h((C,), 39), gate=0.5 + 0.4 * h((N, C), 33),
             addc=0.01 * h((N, C), 34), rps=rps, N=N)
    return d


def pool_inputs(N, C, H, W, bf16):
    """y [N][H][W][C], scale, shift [C] (shift negative enough that about a quarter of the full 3x3 windows are all zero
    after the ReLU), dp [N][OH][OW][C]; mean, invstd [C] complete a forward coef [4][C] for the fused stem backward, with
    gamma = scale / invstd"""
    from oracle import fill
    h = fill.hash_tensor
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    sc = 1 + 0.3 * h((C,), 42)
    inv = 0.8 + 0.2 * h((C,), 46)
    return dict(y=_b(h((N, H, W, C), 41, 2.0), bf16), scale=sc, shift=-1.4 * sc + 0.1 * h((C,), 43),
                dp=_b(h((N, OH, OW, C), 44), bf16), mean=0.1 * h((C,), 45), invstd=inv, gamma=sc / inv)


# ----------------------------------------------------------------------------------------------------------------------
# The fp32 dense tails (csrc/linear.hip, csrc/head.hip, csrc/head_fused.hip): Linear on its three routes, the squeeze-excite
# MLP, the fused head, LayerNorm / attention fusion, the losses and Adam.  Operands are fp32 and taken as given.
#
#   dot-product outputs stored as fp32 (Linear y / dx / dw / db, every stage of the SE MLP, ecg_rows_sum):
#       |got - ref| <= g_k(K + 2) * A        K = the reduction length, A = the same product on absolute values (+ |bias|)
#     the standard bound of an fp32 dot product summed in ANY order (Higham, Accuracy and Stability, 3.1: every summand passes
#     through at most K roundings whatever the tree); fma chains -- the f32-input MFMA -- only remove roundings.  The + 2
#     covers the bias add and one more operation (accumulate, scale, or the stored product).  ReLU keeps the bound
#     (1-Lipschitz); a sigmoid output gets 0.25 * g_k(K + 2) * A + 4 u (its Lipschitz constant; expf, the add and the divide
#     on a value <= 1).  Where A == 0 the result must be exact.  Every K is the derived worst case, none is tightened.
#   a consumer stage gets the kernel's own stored output of the producer stage as its given input (se_mlp_stages), so the
#     float64 evaluation of that one stage is the exact answer.
#   chains that are not one dot product (LayerNorm, attention fusion, var_loss, CE / focal, the head end to end, Adam):
#       m(t) = max_i |got_i - ref_i| / (|ref_i| + rms(ref_t))  against the float64 torch formulas, at most CHAIN_MARGIN x the
#     m(t) torch's own CPU fp32 run of the same formulas reaches on the same inputs, with a floor of CHAIN_MARGIN * u.  The
#     margin is 8 and not the 4 of the conv constants: the two sides differ in summation order (wave butterfly and per-wave
#     serial rows against torch's blocked sums) and in rsqrtf against 1 / sqrt, and the figure is a maximum over up to ~2e5
#     elements, where the reference run can simply be lucky.
# ----------------------------------------------------------------------------------------------------------------------
CHAIN_MARGIN = 8.0


def dot_bound(A, K, sigmoid=False):
    b = g_k(K + 2) * A.double()
    return 0.25 * b + 4 * U if sigmoid else b


def dot_ratio(got, ref, A, K, name="dot", sigmoid=False):
    """worst |got - ref| / bound of a dot-product output; got, ref, A: same shape"""
    got, ref = got.double(), ref.double()
    ratio = _ratio((got - ref).abs(), dot_bound(A, K, sigmoid))
    if ratio.numel() == 0:
        return Report(name, 0.0, ())
    flat = int(torch.argmax(ratio))
    seen = torch.where(A.double() > 0, (got - ref).abs() / (U * A.double()).clamp_min(1e-300), torch.zeros_like(ref))
    seen = seen[torch.isfinite(seen)]
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape), float(seen.max()) if seen.numel() else 0.0)


def check_dot(got, ref, A, K, name="dot", sigmoid=False):
    """(the accumulation term printed is the worst error in units of u * A: the measured K)"""
    r = dot_ratio(got, ref, A, K, name, sigmoid)
    print(r)
    assert r.ok, str(r)
    return r


def linear_ref(x, w, b=None, dz=None, act="none"):
    """float64 Linear: {name: (ref, A, K, sigmoid)} for y = act(x w^T + b) and, given dz (the gradient of the
    pre-activation), dx = dz w, dw = dz^T x, db = sum_b dz.  x [B][In], w [Out][In], b [Out] or None, dz [B][Out]."""
    x, w = x.double(), w.double()
    B, In = x.shape
    pre, A = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        pre, A = pre + b.double(), A + b.double().abs()
    y = {"none": pre, "relu": pre.clamp_min(0), "sigmoid": torch.sigmoid(pre)}[act]
    out = {"y": (y, A, In, act == "sigmoid")}
    if dz is not None:
        d = dz.double()
        out["dx"] = (d @ w, d.abs() @ w.abs(), w.shape[0], False)
        out["dw"] = (d.t() @ x, d.abs().t() @ x.abs(), B, False)
        out["db"] = (d.sum(0), d.abs().sum(0), B, False)
    return out


def se_mlp_stages(m, w1, b1, w2, b2, h, g, dg=None, ds=None, dh=None, scale=1.0):
    """The stages of the squeeze-excite MLP in float64, each from the STORED output of the stage before it:
    {stage: (ref, A, K, kind)}, kind "dot", "sigmoid" or "ds" (bound g_k(4) * |ref|).  m [N][C], w1 [CR][C], w2 [C][CR];
    h, g: what the forward stored; ds, dh: what the backward stored; scale: the fp32 value the kernel received."""
    m, w1, b1, w2, b2 = (t.double() for t in (m, w1, b1, w2, b2))
    N, C = m.shape
    CR = w1.shape[0]
    out = {"h": ((m @ w1.t() + b1).clamp_min(0), m.abs() @ w1.abs().t() + b1.abs(), C, "dot")}
    hs = h.double()
    out["g"] = (torch.sigmoid(hs @ w2.t() + b2), hs.abs() @ w2.abs().t() + b2.abs(), CR, "sigmoid")
    if dg is None:
        return out
    gs, dgd, dss, dhs = g.double(), dg.double(), ds.double(), dh.double()
    r = dgd * gs * (1 - gs)
    out["ds"] = (r, r.abs(), 0, "ds")
    mask = (hs > 0).double()
    out["dh"] = ((dss @ w2) * mask, (dss.abs() @ w2.abs()) * mask, C, "dot")
    sc = f32(scale)
    out["dm"] = ((dhs @ w1) * sc, (dhs.abs() @ w1.abs()) * abs(sc), CR, "dot")
    out["dw2"] = (dss.t() @ hs, dss.abs().t() @ hs.abs(), N, "dot")
    out["db2"] = (dss.sum(0), dss.abs().sum(0), N, "dot")
    out["dw1"] = (dhs.t() @ m, dhs.abs().t() @ m.abs(), N, "dot")
    out["db1"] = (dhs.sum(0), dhs.abs().sum(0), N, "dot")
    return out


def se_stage_ratio(got, stage, name):
    ref, A, K, kind = stage
    if kind == "ds":
        got = got.double()
        ratio = _ratio((got - ref).abs(), g_k(4) * A)
        flat = int(torch.argmax(ratio))
        return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape))
    return dot_ratio(got, ref, A, K, name, sigmoid=kind == "sigmoid")


def check_se_mlp(stages, got, name="se_mlp"):
    """got: {stage: stored tensor or None}; every stage given is checked.  Returns {stage: Report}"""
    out = {}
    for k, st in stages.items():
        if got.get(k) is None:
            continue
        r = se_stage_ratio(got[k], st, "%s %s" % (name, k))
        print(r)
        assert r.ok, str(r)
        out[k] = r
    return out


def se_inputs(N, C, CR):
    """m, w1, b1, w2, b2, dg of one SEBlock.fc (hash-filled, torch's Linear scale)"""
    from oracle import fill
    h = fill.hash_tensor
    return dict(m=h((N, C), 51) * 0.8 + 0.3, w1=h((CR, C), 52, (3.0 / C) ** 0.5), b1=h((CR,), 53, 0.1),
                w2=h((C, CR), 54, (3.0 / CR) ** 0.5), b2=h((C,), 55, 0.1), dg=h((N, C), 56))


def chain_figure(got, ref):
    """m(t) = max_i |got_i - ref_i| / (|ref_i| + rms(ref_t)); an element whose denominator is 0 must be exact"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    den = ref.abs() + float(ref.pow(2).mean().sqrt())
    return float(_ratio(err, den).max())


def chain_ratio(got, ref, own, name="chain"):
    """got: the kernel's tensor, ref: float64, own: torch's CPU fp32 run of the same formulas.  ratio = m(got) / bar,
    bar = CHAIN_MARGIN * max(m(own), u)"""
    mk, mt = chain_figure(got, ref), chain_figure(own, ref)
    bar = CHAIN_MARGIN * max(mt, U)
    r = Report(name, mk / bar, ())
    r.kernel, r.torch32, r.bar = mk, mt, bar
    return r


def check_chain(got, ref, own, name="chain"):
    r = chain_ratio(got, ref, own, name)
    print("%-34s kernel %.3g, torch fp32 %.3g, bar %.3g: ratio %.3g" % (name, r.kernel, r.torch32, r.bar, r.ratio))
    assert r.ok, "%s: m = %.3g above %g x torch fp32's own %.3g" % (name, r.kernel, CHAIN_MARGIN, r.torch32)
    return r


class HeadRef(torch.nn.Module):
    """The multimodal head (multimodal_paper_modal_balance.py:326-354) at any widths, as plain torch modules: three
    LayerNorms, three branch classifiers, attention fusion, Linear-ReLU-Linear, var_loss.  .table() lists the 19 parameters
    in the order of ecgmm_head_forward."""

    def __init__(self, dims, hidden, num_classes):
        super().__init__()
        nn = torch.nn
        D = sum(dims)
        self.dims = tuple(dims)
        self.norms = nn.ModuleList([nn.LayerNorm(d) for d in dims])
        self.cls = nn.ModuleList([nn.Linear(d, num_classes) for d in dims])
        self.aw = nn.Parameter(torch.ones(3))
        self.fnorm = nn.LayerNorm(D)
        self.fc0 = nn.Linear(D, hidden)
        self.fc3 = nn.Linear(hidden, num_classes)

    def table(self):
        t = []
        for n in self.norms:
            t += [n.weight, n.bias]
        for c in self.cls:
            t += [c.weight, c.bias]
        return t + [self.aw, self.fnorm.weight, self.fnorm.bias, self.fc0.weight, self.fc0.bias, self.fc3.weight, self.fc3.bias]

    TABLE_NAMES = ("image_norm.w", "image_norm.b", "signal_norm.w", "signal_norm.b", "clinical_norm.w", "clinical_norm.b",
                   "image_cls.w", "image_cls.b", "signal_cls.w", "signal_cls.b", "clinical_cls.w", "clinical_cls.b",
                   "fusion.weights", "fusion.norm.w", "fusion.norm.b", "fc0.w", "fc0.b", "fc3.w", "fc3.b")

    def forward(self, raws):
        """-> (image, signal, clinical, fusion logits, var_loss, softmax weights), per-row variances [3][B]"""
        f = [n(r) for n, r in zip(self.norms, raws)]
        w = torch.softmax(self.aw, 0)
        fused = self.fnorm(torch.cat([w[m] * f[m] for m in range(3)], 1))
        logits = [c(t) for c, t in zip(self.cls, f)] + [self.fc3(torch.relu(self.fc0(fused)))]
        rv = [torch.var(t, dim=1) for t in f]
        v = [t.mean() for t in rv]
        var = (v[0] - v[1]).abs() + (v[0] - v[2]).abs() + (v[1] - v[2]).abs()
        return (*logits, var, w), rv


def head_fill(head, salt=0):
    """hash fill: gammas near 1, biases small, Linear weights at torch's scale, fusion weights apart"""
    from oracle import fill
    with torch.no_grad():
        for i, p in enumerate(head.table()):
            s = 700 + 31 * salt + i
            if i == 12:
                p.copy_(torch.tensor([1.3, 0.2, 0.8]))
            elif p.dim() == 2:
                p.copy_(fill.hash_tensor(p.shape, s, (3.0 / p.shape[1]) ** 0.5))
            elif i in (0, 2, 4):     # branch gammas apart, so that the three mean variances of var_loss differ by O(1)
                p.copy_((1.0, 1.5, 0.6)[i // 2] + 0.2 * fill.hash_tensor(p.shape, s))
            elif i == 13:
                p.copy_(1 + 0.2 * fill.hash_tensor(p.shape, s))
            else:
                p.copy_(0.1 * fill.hash_tensor(p.shape, s))
    return head


def head_inputs(B, dims, num_classes):
    from oracle import fill
    raws = [fill.hash_tensor((B, d), 90 + i, 1.0 + 0.5 * i) + 0.2 * i for i, d in enumerate(dims)]
    return raws, torch.arange(B) % num_classes


HEAD_LOSSES = ("all_heads", "train_py", "signal_only", "var_only")


def head_loss(out, labels, kind, ce=F.cross_entropy):
    if kind == "all_heads":
        return ce(out[0], labels) + ce(out[1], labels) + ce(out[2], labels) + ce(out[3], labels) + 0.1 * out[4]
    if kind == "train_py":
        return ce(out[3], labels) + 0.1 * out[4]
    if kind == "signal_only":
        return ce(out[1], labels)
    return out[4] * 1.0


def head_run(head, raws, labels, kind, dtype, row_weight=None):
    """outputs, d raw x 3 and the 19 parameter gradients (None where the branch is not in the loss) of `head` evaluated in
    `dtype` on the CPU.  row_weight [B] (None = ones) weights every row's share of the loss: the cross-entropy terms are row
    sums, and var_loss enters through its own linearisation sum_m sign_m * mean_b var_m[b] (the signs of the full batch),
    whose gradient is var_loss's -- so a zero weight removes exactly that row's contribution from every gradient."""
    h = HeadRef(head.dims, head.fc0.out_features, head.fc3.out_features).to(dtype)
    h.load_state_dict({k: v.to(dtype) for k, v in head.state_dict().items()})
    rr = [r.to(dtype).clone().requires_grad_(True) for r in raws]
    out, rv = h(rr)
    if row_weight is None:
        loss = head_loss(out, labels, kind)
    else:
        wgt = row_weight.to(dtype)
        B = labels.shape[0]
        ce = lambda lg, y: (F.cross_entropy(lg, y, reduction="none") * wgt).sum() / B
        v = [t.mean().detach() for t in rv]
        sg = [torch.sign(v[0] - v[1]) + torch.sign(v[0] - v[2]), -torch.sign(v[0] - v[1]) + torch.sign(v[1] - v[2]),
              -torch.sign(v[0] - v[2]) - torch.sign(v[1] - v[2])]
        lin = sum(sg[m] * (rv[m] * wgt).sum() / B for m in range(3))
        loss = head_loss((*out[:4], lin, out[5]), labels, kind, ce)
    loss.backward()
    return [o.detach() for o in out], [r.grad for r in rr], [p.grad for p in h.table()]


# ---- cases shared by tests/test_dense_f64_gpu.py and the CPU tests of the checkers (tests/test_f64check.py) ----
# (B, In, Out) of a Linear, and what each reaches in csrc/linear.hip
LINEAR_CASES = [(16, 16, 16), (48, 80, 16), (272, 672, 128), (17, 672, 128), (7, 96, 40), (300, 10, 30), (70, 300, 30),
                (1040, 768, 2), (6, 4, 64), (6, 64, 4), (1, 16, 16)]
# (N, C, CR) of the SE MLP: every width at N = 67 (the model's four stages, an odd one and the limit), every N at (64, 4)
SE_CASES = [(67, 64, 4), (67, 128, 8), (67, 256, 16), (67, 512, 32), (67, 100, 7), (67, 1024, 64),
            (1, 64, 4), (5, 64, 4), (16, 64, 4), (17, 64, 4), (49, 64, 4), (130, 64, 4)]
SE_SCALE = 1.0 / 313            # the mean over L = 313 positions: not a power of two


def linear_inputs(B, In, Out):
    from oracle import fill
    h = fill.hash_tensor
    return h((B, In), 1), h((Out, In), 2, In ** -0.5), h((Out,), 3, 0.1), h((B, Out), 4)


# ----------------------------------------------------------------------------------------------------------------------
# The LSTM recurrence (csrc/lstm.hip: lstm_seq_fwd_kernel, lstm_seq_bwd_kernel and the GEMMs around them), fp32, operands
# taken as given.  References: torch.nn.LSTM on the CPU in float64 (the answer) and in float32 (the yardstick).
#
# (a) The LSTM is a chain, so it falls under the chain rule above -- but per slice.  A whole-tensor figure is blind to
#     magnitudes that decay in time: with the loss on h_n only, dx of the 70-step case falls from an rms of O(1e-2) at the
#     last step to 2.2e-15 at t = 0, and max|a - ref| / max|ref| accepts a backward that is wrong by 100 % over the first 60
#     steps.  So, for every time step t of a tensor with a time axis (y, dx),
#         m_t = max_i |got_i - ref_i| / (|ref_i| + rms(ref[t]))          over that step's slice
#     and every m_t <= CHAIN_MARGIN * max(u, max_t m_t(own32)): the yardstick is the MAXIMUM over the slices of torch's own
#     fp32 run, so that one lucky slice of that run cannot tighten the bar.  hn, cn, dh0, dc0 are one slice per (layer,
#     direction) (their leading axis), a parameter gradient is one slice.  No slice is skipped; the float64 reference's
#     smallest slice rms must be >= LSTM_MIN_RMS = 1e-25, far above fp32's subnormal range (the smallest over LSTM_CHAIN_CASES
#     is the 2.2e-15 above).  torch fp32's own worst per-slice figure over LSTM_CHAIN_CASES is 15 - 33 u on the CPU.
#
# (b) One step (T = 1) reads and writes only public tensors (x, h0, c0 -> y, hn, cn), so the float64 evaluation of one
#     cell is the exact answer and every output has a derived bound:
#       pre-activations   A = |x| |W_ih|^T + |b_ih| + |h0| |W_hh|^T + |b_hh|,   b = g_k(In + H + 4) * A
#                         the any-order dot-product bound of the dense section; the + 4: the stored projection, its bias
#                         and the two adds in the kernel
#       gates             d(i, f, o) = 0.25 b + E (sigmoid is 0.25-Lipschitz),   dg = b + E (tanh is 1-Lipschitz)
#       cell state        dc = |c0| df + |g| di + |i| dg + di dg + g_k(3) (|f c0| + |i g|)     (two products, one add)
#       output            dh = do + dc + E + u |h|       (|tanh c| <= 1, o <= 1; tanhf of c; the product)
#     E = K_FN * u is the absolute error of sigmoidf_ (1 / (1 + expf(-x))) and tanhf on the device, the one constant here
#     that is measured: the worst error of y / cn beyond the remaining terms, in units of what one u of E adds to the
#     bound, over every case of LSTM_STEP_* (tests/test_lstm_f64_gpu.py prints it).  K_FN is at most 4x that.
#     hn must equal y bit for bit at T = 1.
#
# Measured on the MI355X (tests/test_lstm_f64_gpu.py, 120 shapes + the saturated one): the function error seen beyond the
# remaining terms is 0.00 u at every case -- no element of y or cn leaves the derived terms alone, which are worst-case sums
# of In + H + 4 roundings where the functions contribute one or two -- so K_FN = 4 x 0 = 0 and E drops out of the bound (it
# stays in the formulas for a device whose expf / tanhf were worse).  Worst ratio to that bound: 0.143 (H = 4), 0.097
# (H = 16), 0.085 (H = 1), under 0.04 from H = 37 up, 0.0066 at the cap; torch's CPU fp32 cell: 0.16 (tests/test_f64check.py).
# Per-slice chain bar, worst ratio over LSTM_CHAIN_CASES: 0.56 (dc0 at H = 1: 10.1 u against torch fp32's 2.2 u on that
# tensor), 0.35 at the cap (dx, 40.6 u), 0.15 on the 70-step case; torch fp32's own worst slice there is 13.9 - 45.6 u.
# ----------------------------------------------------------------------------------------------------------------------
K_FN = 0.0                   # measured 0.00 u beyond the other terms (above)
LSTM_MIN_RMS = 1e-25

# (B, T, In, H, layers, bidirectional, batch_first, h0 / c0 given), the cotangents in the loss, what the case reaches
LSTM_CHAIN_CASES = [
    ((16, 70, 24, 200, 1, False, False, True), ("h",)),          # dx decays to 2.2e-15 at t = 0
    ((9, 24, 20, 132, 1, False, True, False), ("c",)),           # wave 0 alone takes a second tile
    ((17, 3, 24, 384, 1, True, True, True), ("y", "h", "c")),    # the cap: 148 224 B of LDS in the backward
    ((17, 3, 24, 128, 1, True, False, True), ("y", "h", "c")),   # exactly one tile per wave
    ((17, 3, 24, 256, 1, True, True, True), ("y", "h", "c")),    # two tiles per wave
    ((3, 5, 16, 8, 8, True, False, False), ("y",)),              # 8 layers
    ((5, 1, 12, 37, 2, True, True, True), ("y", "h", "c")),      # T = 1: the backward's `first` branch in both directions
    ((33, 4, 16, 1, 1, True, True, True), ("y", "h", "c")),      # H = 1
]
LSTM_CHAIN_IDS = ["t70_hn_only", "h132_cn_only", "h384_cap", "h128", "h256", "layers8", "t1x2", "h1"]
LSTM_STEP_H = (1, 4, 16, 37, 128, 132, 200, 256, 380, 384)
LSTM_STEP_B = (1, 16, 17)
LSTM_STEP_IN = (3, 24)


def lstm_step_case(B, In, H, bi):
    return (B, 1, In, H, 1, bi, True, True)


@functools.lru_cache(maxsize=None)
def lstm_inputs(case, wscale=1.0, xscale=1.0):
    """(torch.nn.LSTM, x, h0, c0, gy, gh, gc) of a case, seeded by its shape; cached and never modified"""
    B, T, In, H, layers, bi, bf, given = case
    torch.manual_seed(1234 + B * 7 + T)
    mod = torch.nn.LSTM(In, H, layers, batch_first=bf, bidirectional=bi)
    with torch.no_grad():
        for p in mod.parameters():
            p.mul_(wscale)
    D = 2 if bi else 1
    x = torch.randn((B, T, In) if bf else (T, B, In)) * xscale
    h0 = torch.randn(layers * D, B, H) * 0.5 if given else None
    c0 = torch.randn(layers * D, B, H) * 0.5 if given else None
    gy = torch.randn((B, T, D * H) if bf else (T, B, D * H))
    gh, gc = torch.randn(layers * D, B, H), torch.randn(layers * D, B, H)
    return mod, x, h0, c0, gy, gh, gc


def lstm_run(ins, dtype, use=("y", "h", "c")):
    """torch.nn.LSTM on the CPU in `dtype`: outputs and every gradient of sum y gy + sum h_n gh + sum c_n gc (the terms
    named in `use`).  ins = (module, x, h0, c0, gy, gh, gc), left as they are."""
    mod, x, h0, c0, gy, gh, gc = ins
    m = copy.deepcopy(mod).to(dtype)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    x = leaf(x)
    hx = None if h0 is None else (leaf(h0), leaf(c0))
    y, (hn, cn) = m(x, hx)
    loss = 0
    if "y" in use:
        loss = loss + (y * gy.to(dtype)).sum()
    if "h" in use:
        loss = loss + (hn * gh.to(dtype)).sum()
    if "c" in use:
        loss = loss + (cn * gc.to(dtype)).sum()
    loss.backward()
    out = {"y": y, "hn": hn, "cn": cn, "dx": x.grad}
    if hx is not None:
        out["dh0"], out["dc0"] = hx[0].grad, hx[1].grad
    for n, p in m.named_parameters():
        out["d" + n] = p.grad
    return {k: v.detach() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def lstm_refs(case, use=("y", "h", "c"), wscale=1.0, xscale=1.0):
    """(float64 run, float32 run) of a case on the CPU; computed once and never modified"""
    ins = lstm_inputs(case, wscale, xscale)
    return lstm_run(ins, torch.float64, use), lstm_run(ins, torch.float32, use)


def lstm_slice_dim(key, batch_first):
    """the axis a tensor of lstm_run is sliced along: time for y / dx, (layer, direction) for the states, None = one slice"""
    if key in ("y", "dx"):
        return 1 if batch_first else 0
    return 0 if key in ("hn", "cn", "dh0", "dc0") else None


def seq_slice_figures(got, ref, dim):
    """(m_t, rms(ref[t])) for every slice t along `dim` (None: the tensor is one slice)"""
    got, ref = got.double(), ref.double()
    if dim is None:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    else:
        n = ref.shape[dim]
        got, ref = got.movedim(dim, 0).reshape(n, -1), ref.movedim(dim, 0).reshape(n, -1)
    rms = ref.pow(2).mean(1, keepdim=True).sqrt()
    return _ratio((got - ref).abs(), ref.abs() + rms).amax(1), rms.reshape(-1)


def seq_chain_ratio(got, ref64, own32, time_dim, name="seq"):
    assert got.shape == ref64.shape == own32.shape, (name, got.shape, ref64.shape, own32.shape)
    mk, rms = seq_slice_figures(got, ref64, time_dim)
    mt, _ = seq_slice_figures(own32, ref64, time_dim)
    bar = CHAIN_MARGIN * max(float(mt.max()), U)
    t = int(torch.argmax(mk))
    r = Report(name, float(mk[t]) / bar, (t,))
    r.kernel, r.torch32, r.bar, r.min_rms = float(mk[t]), float(mt.max()), bar, float(rms.min())
    return r


def seq_chain_check(got, ref64, own32, time_dim, name="seq", quiet=False):
    """every slice of `got` along time_dim within CHAIN_MARGIN x the worst slice of torch's own fp32 run (header (a))"""
    r = seq_chain_ratio(got, ref64, own32, time_dim, name)
    if not quiet:
        print("%-34s worst slice %s: kernel %.3g, torch fp32 %.3g (= %.1f u), bar %.3g: ratio %.3g" %
              (name, r.where, r.kernel, r.torch32, r.torch32 / U, r.bar, r.ratio))
    assert r.min_rms >= LSTM_MIN_RMS, "%s: a slice of the float64 reference has rms %.3g" % (name, r.min_rms)
    assert r.ok, "%s: slice %s has m = %.3g above %g x torch fp32's own worst %.3g" % (name, r.where, r.kernel, CHAIN_MARGIN,
                                                                                    r.torch32)
    return r


def lstm_chain_check(out, ref64, own32, batch_first, name, keys=None, quiet=True):
    """seq_chain_check of every tensor of `out` named in keys (default: every tensor of the reference).  Returns the worst
    Report; prints one line: the worst per-slice figure next to torch fp32's own."""
    worst = None
    for k in (keys or ref64):
        r = seq_chain_check(out[k], ref64[k], own32[k], lstm_slice_dim(k, batch_first), name + " " + k, quiet)
        if worst is None or r.ratio >= worst.ratio:
            worst = r
    own = max(seq_chain_ratio(own32[k], ref64[k], own32[k], lstm_slice_dim(k, batch_first)).torch32 for k in (keys or ref64))
    print("[lstm f64] %-30s worst %.3g = %.1f u (%s, slice %s), ratio to its bar %.3g; torch fp32's own worst %.1f u" %
          (name, worst.kernel, worst.kernel / U, worst.name.split()[-1], worst.where, worst.ratio, own / U))
    return worst


def lstm_step_ref(x, h0, c0, w_ih, w_hh, b_ih, b_hh, k_fn=K_FN):
    """one LSTM cell in float64: (h, c, dh, dc), the outputs and their bounds (header (b)).  x [B][In], h0, c0 [B][H]"""
    x, h0, c0, w_ih, w_hh, b_ih, b_hh = (t.double() for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh))
    In, H = x.shape[1], h0.shape[1]
    pre = x @ w_ih.t() + b_ih + h0 @ w_hh.t() + b_hh
    A = x.abs() @ w_ih.abs().t() + b_ih.abs() + h0.abs() @ w_hh.abs().t() + b_hh.abs()
    b = g_k(In + H + 4) * A
    E = k_fn * U
    i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
    di, df, dg, do = 0.25 * b[:, :H] + E, 0.25 * b[:, H:2 * H] + E, b[:, 2 * H:3 * H] + E, 0.25 * b[:, 3 * H:] + E
    c = f * c0 + i * g
    dc = c0.abs() * df + g.abs() * di + i.abs() * dg + di * dg + g_k(3) * ((f * c0).abs() + (i * g).abs())
    h = o * torch.tanh(c)
    dh = do + dc + E + U * h.abs()
    return h, c, dh, dc


def lstm_step_ratio(out, ins, name="lstm step"):
    """y, hn, cn of a T = 1, one-layer run (out) against the float64 cell of every direction.  Report.ratio: worst
    |err| / bound; .fn_seen: the worst error beyond the bound's other terms in units of what one u of E adds (the measured
    K_FN); .hn_is_y: hn equals y bit for bit"""
    mod, x, h0, c0 = ins[:4]
    H = mod.hidden_size
    D = 2 if mod.bidirectional else 1
    xs = (x[:, 0] if mod.batch_first else x[0])
    y = out["y"].detach().cpu()
    y = y[:, 0] if mod.batch_first else y[0]
    worst = Report(name, 0.0, ())
    worst.fn_seen, worst.hn_is_y = 0.0, True
    for k in range(D):
        sfx = "_l0" + ("_reverse" if k else "")
        par = [getattr(mod, n + sfx).detach() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        h, c, dh, dc = lstm_step_ref(xs, h0[k], c0[k], *par)
        _, _, dh0_, dc0_ = lstm_step_ref(xs, h0[k], c0[k], *par, k_fn=0.0)
        _, _, dh1_, dc1_ = lstm_step_ref(xs, h0[k], c0[k], *par, k_fn=1.0)
        got_h, got_c, got_hn = y[:, k * H:(k + 1) * H].double(), out["cn"][k].detach().cpu().double(), out["hn"][k].detach().cpu()
        worst.hn_is_y = worst.hn_is_y and torch.equal(got_hn, y[:, k * H:(k + 1) * H])
        for tag, got, ref, bound, b0, b1 in (("y", got_h, h, dh, dh0_, dh1_), ("cn", got_c, c, dc, dc0_, dc1_)):
            ratio = _ratio((got - ref).abs(), bound)
            flat = int(torch.argmax(ratio))
            if float(ratio.reshape(-1)[flat]) >= worst.ratio:
                worst.ratio, worst.where = float(ratio.reshape(-1)[flat]), (tag, k) + _unravel(flat, ref.shape)
            seen = ((got - ref).abs() - b0).clamp_min(0) / (b1 - b0)
            seen = seen[torch.isfinite(seen)]
            worst.fn_seen = max(worst.fn_seen, float(seen.max()) if seen.numel() else 0.0)
    return worst


def lstm_step_check(out, ins, name="lstm step"):
    r = lstm_step_ratio(out, ins, name)
    print("[lstm step] %-30s worst ratio to the bound %.3g at %s; function error seen %.2f u; hn == y: %s" %
          (name, r.ratio, r.where, r.fn_seen, r.hn_is_y))
    assert r.hn_is_y, name + ": hn differs from y at T = 1"
    assert r.ok, str(r)
    return r


# ----------------------------------------------------------------------------------------------------------------------
# The TabNet clinical branch (csrc/tabnet.hip, bn_small_eval_bwd of csrc/bn_eval_bwd.hip, ecgmm/tabnet.py), fp32, operands
# taken as given.  Every kernel is checked on its own stored input, so the float64 evaluation of that one operation is the
# exact answer, and every mask (ReLU, sparsemax support) is taken from the kernel's stored output.  u = 2^-24, g_k as above.
#
#   sigmoid     s' = 1 / (1 + expf(-b)): |s' - s| <= E_SIG = K_SIG u, the convention of the dense section (expf, the add and the
#               divide on a value <= 1: a relative error eps of expf moves s by s (1 - s) eps <= eps / 4, the add and the divide
#               by u s each).  It is absolute, so it also holds where expf overflows (b = -100: s' = 1 / inf = 0, s = 4e-44) or
#               underflows (b = 100: s' = 1).  K_SIG = 4 is ASSUMED (expf within 2 ulp); the GLU checks print what is seen.
#   GLU fwd     out = a s':                |err| <= |a| E + u |a| (s + E)
#   GLU bwd     dz_a = g s':               |err| <= |g| E + u |g| (s + E)
#               dz_b = ((g a) s') (1 - s'): s'(1 - s') is off by <= E |1 - 2 s| + E^2 <= E + E^2, then 1 - s' and three products:
#                                          |err| <= |g a| (E + E^2) + g_k(4) |g a| (s (1 - s) + E + E^2)
#   sparsemax   z = x - max(x) in float64, sorted descending; tau_k = (S_k - 1) / k, S_k the sum of the k largest; the support
#     fwd       size k* is the last k with z_(k) > tau_k; p = max(z - tau_k*, 0).  The kernel forms v = fl(x - max) (u |z| each),
#               the serial fp32 prefix sum (every summand passes <= k roundings with its own: g_k(k + 1) A_k, A_k = the sum of
#               the k largest |z|, leaves one to spare), tau' = fl(fl(cum - 1) / k) (two roundings of |tau_k| >= 1 / k) and
#               fl(v - tau').  For the support size k the kernel settled on:
#                   dtau(k) = g_k(k + 1) A_k / k + g_k(2) (|tau_k| + g_k(k + 1) A_k / k)
#                   b_d(k)  = u |z_d| + dtau(k) + u (|z_d - tau_k| + u |z_d| + dtau(k))          (max(., 0) is 1-Lipschitz)
#               The kernel's support test fl(1 + fl(k v_(k))) > cum, divided by k, is off by at most 2 u |z_(k)| + u |tau_k| +
#               g_k(k) A_k / k <= 2 b_(k)(k): where float64 has |z_(k) - tau_k| <= 2 b_(k)(k) the test at k may go either way, and
#               the kernel (which keeps the LAST k that passes) may have settled on k or on k - 1.  tau_k <= tau_k* for every k
#               and tau_k - tau_(k-1) = (z_(k) - tau_(k-1)) / k, so such a k moves tau by that distance over k only: the output
#               is continuous and no element is skipped.  The bound of element d is the maximum over the admissible k (k* and
#               every such k, k - 1) of |max(z_d - tau_k, 0) - p_d| + b_d(k).  Row sums: |sum_d p'_d - 1| <= sum_d bound_d.
#               p >= 0; D = 1 gives exactly 1 (v = 0, tau' = -1); a lead of >= 1 gives exactly one-hot (tau' = -1, v <= -1).
#   sparsemax   support = {p' > 0} as stored; dx = dp - mean_support(dp): a serial fp32 sum of k terms and the divide
#     bwd       (dv = g_k(k) A / k, A = sum_support |dp|), then the subtract: |err| <= dv + u (|ref| + dv); 0 outside, exactly
#   entropy     term_i = fl(M_i logf(fl(M_i + eps))): the argument's rounding moves the logarithm by <= g_k(1) absolute, logf is
#     fwd       ASSUMED within K_LOG u relative (K_LOG = 2: one ulp), the product rounds once:
#                   e_i = M_i (g_k(1) + g_k(K_LOG + 1) (|L_i| + g_k(1))),  L = log(M + eps) in float64, eps as the fp32 it is
#               M_i = 0 gives 0 * logf(eps) = 0 exactly.  The kernel sums in double and rounds (sum / N) once:
#                   |err| <= (1 + u) sum_i e_i / N + u |ref|
#     bwd       dM = gs (logf(M + eps) + M / (M + eps)), gs = fl(g / N): from L: logf, add, product, gs = K_LOG + 3 roundings;
#               from q = M / (M + eps): argument, divide, add, product, gs = 5:
#                   |err| <= |g / N| (g_k(max(K_LOG + 3, 5)) (|L| + q) + g_k(1) (1 + g_k(K_LOG + 3)))
#   ecgmm_ew    MUL, ADD, RELU, RELU_BWD, SCALE, NEG_MUL, RSUB: one correctly rounded operation (or none), so the stored value
#               EQUALS the float64 result rounded to fp32 (53 >= 2 * 24 + 2 bits: no double rounding).  ADD_SCALE, PRIOR: two
#               roundings, |err| <= g_k(2) |ref|.  split_cols(_bwd): copies and masks, exact (-0.0 == 0.0).
#   bn_small    the kernel sums x and x^2 in double (ceil(N / 256) serial adds + the 8-level fold + the divide and subtract:
#     fwd       K64 = ceil(N / 256) + 11 roundings of 2^-53 on sum |x|, sum x^2) and rounds mean / invstd / the unbiased variance to
#               fp32: coef_ref above with ds1 = K64 2^-53 sum |x|, ds2 = K64 2^-53 sum x^2 gives save (mean, invstd) and the
#               running statistics with their bounds (unbiased variance, momentum as the fp32 it is; three roundings on either
#               path).  y = ((x - m') inv') g + b with the STORED m', inv' against the float64 mean / invstd:
#                   |err| <= |g| (d_mean inv + |x - mean| d_inv + d_mean d_inv) + g_k(4) (|g| (|x - mean| + d_mean) (inv + d_inv) + |b|)
#               whose first term, u |mean| inv |g| from the cast of the mean, dominates at a large mean / std.  nbt += 1 with every
#               update of the running statistics (a call that is given none leaves nbt alone).
#               Eval mode: mean = running_mean exactly, invstd = fl(1 / sqrt(running_var + eps)) (one rounding), nothing updated.
#     bwd       the kernel's stored save = (m, inv) is GIVEN.  xh = fl(fl(x - m) inv) (two roundings), the sums in double:
#               dbeta = sum dy, dgamma = sum dy xh are dot products of length N: dot_bound(A, N), A = sum |dy| [|xh|] (+ |what was
#               there| when accumulate = 1; + 2 covers the cast and that add).  dx = k (dy - S1 / N - xh S2 / N), k = fl(g inv),
#               S1, S2 the float64 sums the kernel holds to e1 = g_k(1) |S1|, e2 = g_k(1) |S2| + g_k(2) sum |dy| |xh|; the longest
#               path (xh: 2, product, subtract, product; or a divide in its place) has 5 roundings, k one more:
#                   |err| <= g_k(6) |k| (|dy| + |S1| / N + |xh| |S2| / N) + (1 + g_k(6)) |k| (e1 + |xh| e2) / N
#     eval bwd  dx = dy fl(g inv): g_k(2) |ref|.  dbeta = sum dy, dgamma = sum dy xh as above (dot_bound(A, N)).
#   ghost BN    every torch.chunk slice is one bn_small call: forward per slice from the running statistics the float64
#               reference has reached (the bound of a running statistic carries (1 - momentum) of the slice before it),
#               nbt + 1 per slice, dx per slice, dgamma / dbeta = the sum over the slices: dot_bound(A, B + slices).
#   Linear      linear_ref / check_dot of the dense section; the weight gradient of a layer used `uses` times per forward is
#               the float64 sum over its uses of dy_i^T x_i, K = uses * B (+ 2 covers the accumulate).
#
# The worst ratios measured on the MI355X (tests/test_tabnet_f64_gpu.py) are recorded in DESIGN.md, "f3 TabNet ... Checks".
# ----------------------------------------------------------------------------------------------------------------------
K_SIG = 4.0                  # assumed: |sigmoid' - sigmoid| <= 4 u (dense section)
K_LOG = 2.0                  # assumed: logf within one ulp = 2 u relative
ENT_EPS = 1e-15
EW_OPS = dict(MUL=0, ADD_SCALE=1, PRIOR=2, RELU=3, RELU_BWD=4, SCALE=5, NEG_MUL=6, ADD=7, RSUB=8)
EW_EXACT = ("MUL", "ADD", "RELU", "RELU_BWD", "SCALE", "NEG_MUL", "RSUB")
EW_ARITY = dict(MUL=2, ADD_SCALE=2, PRIOR=2, RELU=1, RELU_BWD=2, SCALE=1, NEG_MUL=2, ADD=2, RSUB=1)
EW_GRID_CAP = 4096 * 256

TAB_ROWS = (1, 255, 256, 257, 513)
SPMAX_D = (1, 2, 3, 5, 63, 64)
SPMAX_FAMILIES = ("hash", "equal", "ascending", "descending", "ties", "dominant", "shift_up", "shift_down", "prior")
GLU_D = (1, 32, 64)
BN_SMALL_N = (2, 65, 128, 255, 256, 257, 513)
BN_SMALL_C = (1, 2, 3, 64, 128)
GHOST_CASES = [(2, 128), (128, 128), (129, 128), (130, 128), (255, 128), (257, 128), (300, 128), (385, 128), (50, 16)]
SPLIT_CASES = [(1, 2, 1), (257, 5, 1), (257, 5, 2), (257, 5, 4), (513, 64, 32), (7, 64, 63)]


def _report(name, ratio, shape, seen=0.0):
    if ratio.numel() == 0:
        return Report(name, 0.0, ())
    flat = int(torch.argmax(ratio))
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, shape), seen)


def _bounded(got, ref, bound, name, unit=None):
    """Report of |got - ref| / bound; kappa_seen = the worst error in units of `unit` (u * something) where that is > 0"""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    seen = 0.0
    if unit is not None:
        s = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.zeros_like(err))
        s = s[torch.isfinite(s)]
        seen = float(s.max()) if s.numel() else 0.0
    return _report(name, _ratio(err, bound.double()), ref.shape, seen)


def _check(r):
    print(r)
    assert r.ok, str(r)
    return r


def glu_ref(z, dout=None):
    """{out, dza, dzb: (ref, bound, unit)} of the GLU gate on z [N][2 D] (a | b); unit = u |a| etc.: the sigmoid error seen"""
    z = z.double()
    D = z.shape[1] // 2
    a, b = z[:, :D], z[:, D:]
    s = torch.sigmoid(b)
    E = K_SIG * U
    out = {"out": (a * s, a.abs() * E + U * a.abs() * (s + E), U * a.abs())}
    if dout is not None:
        g = dout.double()
        ga = (g * a).abs()
        out["dza"] = (g * s, g.abs() * E + U * g.abs() * (s + E), U * g.abs())
        out["dzb"] = (g * a * s * (1 - s), ga * (E + E * E) + g_k(4) * ga * (s * (1 - s) + E + E * E), U * ga)
    return out


def check_glu(z, out, dout=None, dz=None, name="glu"):
    """out [N][D], dz [N][2 D] as stored.  Returns {output: Report}; kappa_seen of each is the sigmoid error seen in u"""
    D = z.shape[1] // 2
    ref = glu_ref(z, dout)
    got = {"out": out}
    if dz is not None:
        got["dza"], got["dzb"] = dz[:, :D], dz[:, D:]
    res = {}
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), "%s %s: NaN / inf" % (name, k)
        res[k] = _check(_bounded(t, *ref[k][:2], "%s %s" % (name, k), unit=ref[k][2]))
    return res


def sparsemax_ref(x):
    """float64 sparsemax of every row of x [N][D] and the bound of every element (header): (p, bound, kstar)"""
    x = x.double()
    N, D = x.shape
    z = x - x.amax(1, keepdim=True)
    zs = z.sort(1, descending=True).values
    ks = torch.arange(1, D + 1, dtype=torch.float64).view(1, D)
    tau = (zs.cumsum(1) - 1) / ks
    A = zs.abs().cumsum(1)
    kstar = (zs > tau).sum(1, keepdim=True)                       # >= 1: z_(1) = 0 > -1
    gk = ks * 0 + torch.tensor([g_k(k + 1) for k in range(1, D + 1)], dtype=torch.float64).view(1, D)
    dtau = gk * A / ks + g_k(2) * (tau.abs() + gk * A / ks)
    own = U * zs.abs() + dtau + U * ((zs - tau).abs() + U * zs.abs() + dtau)       # b_(k)(k)
    near = (zs - tau).abs() <= 2 * own
    cand = torch.zeros(N, D, dtype=torch.bool)
    cand.scatter_(1, kstar - 1, True)
    cand |= near
    cand[:, :-1] |= near[:, 1:]
    p = (z - tau.gather(1, kstar - 1)).clamp_min(0)
    bound = torch.zeros_like(z)
    for k in range(D):
        if not bool(cand[:, k].any()):
            continue
        tk, dk = tau[:, k:k + 1], dtau[:, k:k + 1]
        b = U * z.abs() + dk + U * ((z - tk).abs() + U * z.abs() + dk)
        tot = ((z - tk).clamp_min(0) - p).abs() + b
        bound = torch.where(cand[:, k:k + 1], torch.maximum(bound, tot), bound)
    return p, bound, kstar.reshape(-1)


def check_sparsemax(x, p, name="sparsemax"):
    """p [N][D] as stored against float64 sparsemax of the same rows; p >= 0, row sums 1, D = 1 and a lead >= 1 exact"""
    assert bool(torch.isfinite(p).all()), name + ": NaN / inf"
    ref, bound, kstar = sparsemax_ref(x)
    pd = p.double()
    assert bool((pd >= 0).all()), name + ": negative probability"
    r = _check(_bounded(p, ref, bound, name, unit=U * (1 + (x.double() - x.double().amax(1, keepdim=True)).abs())))
    rs = _check(_bounded(pd.sum(1), torch.ones(p.shape[0], dtype=torch.float64), bound.sum(1), name + " row sum"))
    if p.shape[1] == 1:
        assert bool((pd == 1).all()), name + ": D = 1 must give exactly 1"
    xs = x.double().sort(1, descending=True).values
    if p.shape[1] > 1:
        lead = (xs[:, 0] - xs[:, 1]) >= 1
        onehot = (x.double() == xs[:, :1]).double()
        assert bool((pd[lead] == onehot[lead]).all()), name + ": a lead of >= 1 must give exactly one-hot"
    r.row_sum, r.kstar = rs.ratio, kstar
    return r


def check_sparsemax_bwd(p, dp, dx, name="sparsemax bwd"):
    """dx as stored; the support is the kernel's own stored p > 0"""
    assert bool(torch.isfinite(dx).all()), name + ": NaN / inf"
    sup = p.double() > 0
    g = dp.double()
    k = sup.sum(1, keepdim=True).clamp_min(1).double()
    A = (g.abs() * sup).sum(1, keepdim=True)
    vhat = (g * sup).sum(1, keepdim=True) / k
    ref = torch.where(sup, g - vhat, torch.zeros_like(g))
    gk = torch.tensor([g_k(int(v)) for v in k.reshape(-1)], dtype=torch.float64).view(-1, 1)
    dv = gk * A / k
    bound = torch.where(sup, dv + U * (ref.abs() + dv), torch.zeros_like(g))
    return _check(_bounded(dx, ref, bound, name, unit=U * (g.abs() + A / k)))


def entropy_ref(M, eps=ENT_EPS, g=None):
    """(ref, bound) of mean_n sum_d M log(M + eps) and, given g [1], (ref, bound, unit) of its backward"""
    M = M.double()
    N = M.shape[0]
    e = f32(eps)
    Lg = torch.log(M + e)
    ei = M * (g_k(1) + g_k(K_LOG + 1) * (Lg.abs() + g_k(1)))
    ref = (M * Lg).sum() / N
    fwd = (ref.reshape(1), ((1 + U) * ei.sum() / N + U * ref.abs()).reshape(1))
    if g is None:
        return fwd, None
    gs = abs(float(g.double().reshape(-1)[0])) / N
    q = M / (M + e)
    rb = float(g.double().reshape(-1)[0]) / N * (Lg + q)
    bb = gs * (g_k(max(K_LOG + 3, 5)) * (Lg.abs() + q) + g_k(1) * (1 + g_k(K_LOG + 3)))
    return fwd, (rb, bb, U * gs * (Lg.abs() + q))


def check_entropy(M, out, eps=ENT_EPS, g=None, dM=None, name="entropy"):
    fwd, bwd = entropy_ref(M, eps, g)
    res = {}
    if out is not None:
        assert bool(torch.isfinite(out).all()), name + ": NaN / inf"
        res["out"] = _check(_bounded(out.reshape(1), fwd[0], fwd[1], name + " fwd"))
    if dM is not None:
        assert bool(torch.isfinite(dM).all()), name + " bwd: NaN / inf"
        res["dM"] = _check(_bounded(dM, bwd[0], bwd[1], name + " bwd", unit=bwd[2]))
    return res


def ew_ref(op, a, b, s):
    """(ref float64, exact?) of one ecgmm_ew op; s is the fp32 scalar the kernel receives"""
    a = a.double()
    b = None if b is None else b.double()
    s = f32(s)
    ref = {"MUL": lambda: a * b, "ADD_SCALE": lambda: (a + b) * s, "PRIOR": lambda: b * (s - a), "RELU": lambda: a.clamp_min(0),
           "RELU_BWD": lambda: torch.where(a > 0, b, torch.zeros_like(a)), "SCALE": lambda: a * s, "NEG_MUL": lambda: -a * b,
           "ADD": lambda: a + b, "RSUB": lambda: s - a}[op]()
    return ref, op in EW_EXACT


def check_ew(op, a, b, s, out, name=None):
    name = name or "ew " + op
    ref, exact = ew_ref(op, a, b, s)
    assert bool(torch.isfinite(out).all()), name + ": NaN / inf"
    if exact:
        bad = out != ref.float()
        assert not bool(bad.any()), "%s: %d elements are not the correctly rounded result (first at %d)" % (
            name, int(bad.sum()), int(bad.reshape(-1).nonzero()[0]))
        r = Report(name, 0.0, ())
        print(r)
        return r
    return _check(_bounded(out, ref, g_k(2) * ref.abs(), name, unit=U * ref.abs()))


def split_ref(x, nd, relu):
    d = x[:, :nd]
    return (d.clamp_min(0) if relu else d).contiguous(), x[:, nd:].contiguous()


def split_bwd_ref(d, gd, ga, D, nd, relu):
    N = d.shape[0]
    gx = torch.zeros(N, D, dtype=d.dtype)
    if gd is not None:
        gx[:, :nd] = torch.where(d <= 0, torch.zeros_like(gd), gd) if relu else gd
    if ga is not None:
        gx[:, nd:] = ga
    return gx


def _k64(N):
    return (-(-N // 256) + 11) * 2.0 ** -53


def bn_small_fwd_ref(x, gamma, beta, rm0, rv0, momentum, eps, training):
    """float64 BatchNorm over the rows of x [N][C]: CoefRef (mean, invstd[, rm, rv] and their bounds) and (y, |.| parts).
    gamma / beta / rm0 / rv0 may be None (training).  Eval: mean = rm0, var = rv0."""
    x = x.double()
    N, C = x.shape
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    if training:
        k = _k64(N)
        cr = coef_ref(x.sum(0), (x * x).sum(0), N, g, b, eps, rm0, rv0, momentum, ds1=k * x.abs().sum(0), ds2=k * (x * x).sum(0))
        # the exact mean / variance (two-pass) in place of the one-pass float64 values coef_ref forms: the difference is inside dvar
        mean = x.mean(0)
        cr.val["mean"] = mean
    else:
        mean = rm0.double()
        inv = 1.0 / (rv0.double() + f32(eps)).sqrt()
        cr = CoefRef(dict(mean=mean, invstd=inv), dict(mean=torch.zeros_like(mean), invstd=g_k(1) * inv * (1 + 2.0 ** -50)))
    inv, dm, di = cr.val["invstd"], cr.bound["mean"], cr.bound["invstd"]
    dev = (x - mean).abs()
    y = (x - mean) * inv * g + b
    bound = g.abs() * (dm * inv + dev * di + dm * di) + g_k(4) * (g.abs() * (dev + dm) * (inv + di) + b.abs())
    return cr, y, bound


def check_bn_small_fwd(x, gamma, beta, rm0, rv0, nbt0, momentum, eps, training, y, save, rm, rv, nbt, name="bn_small fwd",
                       carry=None):
    """y [N][C], save [2][C], rm, rv [C], nbt (int) as stored after the call (rm / rv / nbt None where null was passed).
    carry: (drm, drv) bounds on rm0 / rv0 themselves (ghost BN: the slices before).  Returns ({output: Report}, CoefRef)"""
    cr, yr, yb = bn_small_fwd_ref(x, gamma, beta, rm0, rv0, momentum, eps, training)
    res = {"y": _check(_bounded(y, yr, yb, name + " y", unit=U * (yr.abs() + 1)))}
    res["mean"] = _check(_bounded(save[0], cr.val["mean"], cr.bound["mean"], name + " save mean"))
    res["invstd"] = _check(_bounded(save[1], cr.val["invstd"], cr.bound["invstd"], name + " save invstd"))
    if training and rm is not None:
        mom = f32(momentum)
        for k, got, c in (("rm", rm, 0), ("rv", rv, 1)):
            bd = cr.bound[k] + (0 if carry is None else (1 - mom) * (1 + g_k(3)) * carry[c])
            cr.bound[k] = bd
            res[k] = _check(_bounded(got, cr.val[k], bd, name + " running " + ("mean" if k == "rm" else "var")))
    elif rm is not None:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), name + ": eval mode changed the running statistics"
    if nbt is not None:
        # nbt counts the updates of the running statistics: a training call that is given none leaves it alone
        step = 1 if training and rm0 is not None else 0
        assert int(nbt) == int(nbt0) + step, "%s: nbt %d after %d" % (name, int(nbt), int(nbt0))
    return res, cr


def bn_small_bwd_ref(x, dy, gamma, save, training, dg0=None, db0=None):
    """{dx, dgamma, dbeta: (ref, bound)} from the kernel's own stored save [2][C]; dg0 / db0: what accumulate = 1 adds to"""
    x, dy, m, inv = x.double(), dy.double(), save[0].double(), save[1].double()
    N, C = x.shape
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    xh = (x - m) * inv
    out = {}
    if training:
        S1, S2 = dy.sum(0), (dy * xh).sum(0)
        A1, A2 = dy.abs().sum(0), (dy * xh).abs().sum(0)
        k = g * inv
        e1, e2 = g_k(1) * S1.abs(), g_k(1) * S2.abs() + g_k(2) * A2
        ref = k * (dy - S1 / N - xh * S2 / N)
        bound = g_k(6) * k.abs() * (dy.abs() + S1.abs() / N + xh.abs() * S2.abs() / N) + (1 + g_k(6)) * k.abs() * (e1 + xh.abs() * e2) / N
        out["dx"] = (ref, bound)
    else:
        ref = dy * (g * inv)
        out["dx"] = (ref, g_k(2) * ref.abs())
        S1, S2 = dy.sum(0), (dy * xh).sum(0)
        A1, A2 = dy.abs().sum(0), (dy * xh).abs().sum(0)
    if dg0 is not None:
        S1, S2, A1, A2 = S1 + db0.double(), S2 + dg0.double(), A1 + db0.double().abs(), A2 + dg0.double().abs()
    out["dbeta"] = (S1, dot_bound(A1, N))
    out["dgamma"] = (S2, dot_bound(A2, N))
    return out


def check_bn_small_bwd(x, dy, gamma, save, training, dx=None, dgamma=None, dbeta=None, dg0=None, db0=None, name="bn_small bwd"):
    ref = bn_small_bwd_ref(x, dy, gamma, save, training, dg0, db0)
    res = {}
    for k, t in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        if t is not None:
            assert bool(torch.isfinite(t).all()), "%s %s: NaN / inf" % (name, k)
            res[k] = _check(_bounded(t, ref[k][0], ref[k][1], "%s %s" % (name, k), unit=U * ref[k][0].abs()))
    return res


def ghost_slices(B, vbs):
    """torch.chunk's split of B rows into ceil(B / vbs) chunks: [(i0, i1)]"""
    return [(int(c[0]), int(c[-1]) + 1) for c in torch.arange(B).chunk(-(-B // vbs) if vbs else 1)]


def check_ghost_bn(x, gamma, beta, rm0, rv0, nbt0, momentum, eps, vbs, training, y, save, rm, rv, nbt, dy=None, dx=None,
                   dgamma=None, dbeta=None, name="ghost bn", slices=None):
    """One _GhostBN call against float64 applied per torch.chunk slice, in order.  save [slices][2][C] as the forward
    stored it (taken as given by the backward).  Returns the worst ratio of each output."""
    B = x.shape[0]
    sl = slices or ghost_slices(B, vbs)
    assert save.shape[0] == len(sl), "%s: %d slices stored, torch.chunk makes %d" % (name, save.shape[0], len(sl))
    worst = {}
    up = lambda d: [worst.__setitem__(k, max(worst.get(k, 0.0), r.ratio)) for k, r in d.items()]
    r_m, r_v, carry, n = rm0, rv0, None, int(nbt0)
    last = len(sl) - 1
    sums = {"dgamma": [0.0, 0.0], "dbeta": [0.0, 0.0]}
    for j, (i0, i1) in enumerate(sl):
        # the running statistics are only visible after the last slice: the slices before it update the float64 reference
        res, cr = check_bn_small_fwd(x[i0:i1], gamma, beta, r_m, r_v, n, momentum, eps, training, y[i0:i1], save[j],
                                     rm if j == last and training else None, rv if j == last and training else None,
                                     None, "%s slice %d" % (name, j), carry)
        up(res)
        if training:
            if j != last:
                mom = f32(momentum)
                for k, c in (("rm", 0), ("rv", 1)):
                    cr.bound[k] = cr.bound[k] + (0 if carry is None else (1 - mom) * (1 + g_k(3)) * carry[c])
            r_m, r_v, carry, n = cr.val["rm"], cr.val["rv"], (cr.bound["rm"], cr.bound["rv"]), n + 1
        if dy is not None:
            ref = bn_small_bwd_ref(x[i0:i1], dy[i0:i1], gamma, save[j], training)
            if dx is not None:
                up({"dx": _check(_bounded(dx[i0:i1], *ref["dx"], "%s slice %d dx" % (name, j)))})
            for k in sums:
                sums[k][0] = sums[k][0] + ref[k][0]
                sums[k][1] = sums[k][1] + ref[k][1] / g_k(i1 - i0 + 2)          # back to A
    if not training:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), name + ": eval mode changed the running statistics"
    assert int(nbt) == n, "%s: nbt %d, expected %d (one step per slice)" % (name, int(nbt), n)
    if dy is not None:
        for k, t in (("dgamma", dgamma), ("dbeta", dbeta)):
            if t is not None:
                up({k: _check(_bounded(t, sums[k][0], dot_bound(sums[k][1], B + len(sl)), "%s %s" % (name, k)))})
    return worst


def shared_dw_ref(pairs):
    """[(x_i, dy_i)] of every use of one weight -> (ref, A, K) of sum_i dy_i^T x_i for check_dot"""
    ref = sum(dy.double().t() @ x.double() for x, dy in pairs)
    A = sum(dy.double().abs().t() @ x.double().abs() for x, dy in pairs)
    return ref, A, sum(x.shape[0] for x, _ in pairs)


# ---- input families shared by tests/test_tabnet_f64_gpu.py and the CPU tests of the checkers ----
def sparsemax_rows(N, D, family):
    """x [N][D] fp32 of one family of SPMAX_FAMILIES"""
    from oracle import fill
    h = fill.hash_tensor
    base = h((N, D), 61, 2.0)
    col = torch.arange(D, dtype=torch.float32).view(1, D)
    row = torch.arange(N, dtype=torch.float32).view(N, 1)
    if family == "hash":
        return base
    if family == "equal":
        return (h((N, 1), 62, 3.0)).expand(N, D).contiguous()
    if family in ("ascending", "descending"):        # strictly monotone, steps from 1 / 64 (most in the support) to 1 (one-hot)
        step = 2.0 ** -((row % 7))
        x = col * step + h((N, 1), 63, 1.0)
        return x if family == "ascending" else -x
    if family == "ties":
        # pairs of equal entries: with the pair values c, c - t the threshold falls between, on or next to a pair as t varies
        t = (1 + (row % 8)) / 8.0
        x = -torch.floor(col / 2) * t
        perm = torch.argsort(h((D,), 64))            # the same shuffle of the columns in every row
        return x[:, perm].contiguous()
    if family == "dominant":
        x = base.clone()
        lead = 1.0 + (row % 3) * 0.25                # a lead of exactly 1, 1.25, 1.5 over the runner-up
        j = (torch.arange(N) * 5) % D
        others = x.clone()
        others[torch.arange(N), j] = float("-inf")
        if D == 1:
            return x
        q = torch.floor(others.amax(1) * 4) / 4       # the runner-up moves onto a grid of quarters, so the lead is exact
        x = torch.minimum(x, q.view(N, 1))
        x[torch.arange(N), j] = q + lead.reshape(-1)
        return x
    if family == "shift_up":
        return base + 1e4
    if family == "shift_down":
        return base - 1e4
    if family == "prior":                            # rows multiplied by a prior in [0, 1.5^3], as the model feeds them
        return base * ((h((N, D), 65) * 0.5 + 0.5) * 1.5 ** 3)
    raise ValueError(family)


def glu_inputs(N, D, extreme=False):
    """z [N][2 D], dout [N][D]; extreme: the gate half alternates +-100 (expf overflows / underflows) with +-20 and 0 mixed in"""
    from oracle import fill
    z = fill.hash_tensor((N, 2 * D), 66, 3.0)
    if extreme:
        vals = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0, 88.8, -88.8, 104.0, -104.0])
        idx = (torch.arange(N).view(N, 1) * 3 + torch.arange(D).view(1, D)) % len(vals)
        z[:, D:] = vals[idx]
    return z, fill.hash_tensor((N, D), 67)


def entropy_inputs(N, D):
    """a sparsemax output (exact zeros, ones and values between) and the cotangent g [1]"""
    p, _, _ = sparsemax_ref(sparsemax_rows(N, D, "hash"))
    M = p.float()
    if N > 2:
        M[1] = 0.0
        M[2] = 1e-12                                  # small enough that eps = 1e-15 still moves the logarithm's argument
    return M, torch.tensor([0.7])


def ew_inputs(n):
    from oracle import fill
    a = fill.hash_tensor((n,), 68, 2.0)
    b = fill.hash_tensor((n,), 69, 2.0)
    if n > 4:
        a[1], a[2], a[3] = 0.0, -0.0, -1.5
    return a, b, 1.3


def split_inputs(N, D, nd):
    from oracle import fill
    x = fill.hash_tensor((N, D), 70, 2.0)
    x.view(-1)[0::7] = 0.0
    x.view(-1)[3::11] = -0.0
    return x, fill.hash_tensor((N, nd), 71), fill.hash_tensor((N, D - nd), 72)


def bn_small_inputs(N, C, mean_ratio=None):
    """x, dy [N][C], gamma, beta, rm0, rv0 [C]; mean_ratio: every channel gets mean = +-mean_ratio * std"""
    from oracle import fill
    h = fill.hash_tensor
    x = h((N, C), 73, 2.0) + 0.5
    if mean_ratio is not None:
        c = torch.arange(C)
        x = x + (mean_ratio * (2.0 / 3 ** 0.5) * (1 - 2 * (c % 2).float()))[None]
    return dict(x=x, dy=h((N, C), 74), gamma=1 + 0.2 * h((C,), 75), beta=0.1 * h((C,), 76), rm0=0.1 * h((C,), 77),
                rv0=1 + 0.5 * h((C,), 78), dg0=h((C,), 79), db0=h((C,), 80))


# ----------------------------------------------------------------------------------------------------------------------
# The ops that run only inside the encoder launch plans (tests/plan_replay.py): the global average pool (plain and through
# BatchNorm coefficients), its broadcast backward, the squeeze-excite gate gradient (two-pass and merged form: the same sum)
# and the dropout scaling.  Operands are taken as given; every K is the derived worst case of an fp32 sum taken in ANY
# order (each summand passes through at most as many roundings as there are summands), nothing here is calibrated.
#
#   avgpool:       out[n][c] = (sum_r x) / R [* scale + shift].  R roundings in the sum, the division: K = R + 1, and two
#                  more through the coefficients;  A = mean_r |x| [* |scale| + |shift|];  |got - ref| <= g_k(K) * A
#   bcast_rows:    out[n][r][c] = v[n][c] * scale, scale the fp32 value the kernel received: K = 1, stored as round_T
#   SE gate grad:  dg[n][c] = sum_r [mask] dout * (y * scale + shift): y * scale, + shift, the product, R in the sum:
#                  K = R + 3;  A = sum_r [mask] |dout| (|y| |scale| + |shift|)
#   dropout:       y = keep ? x * (1 / (1 - p)) : 0, p the fp32 value: 1 - p, the reciprocal, the product: K = 3
# ----------------------------------------------------------------------------------------------------------------------
K_BCAST = 1
K_DROPOUT = 3


def avgpool_ref(x, scale=None, shift=None):
    """x [N][R][C] -> (ref, A, K) of the mean over R, optionally through the per-channel affine map"""
    x = x.double()
    R = x.shape[1]
    ref, A, K = x.mean(1), x.abs().mean(1), R + 1
    if scale is not None:
        ref, A, K = ref * scale.double() + shift.double(), A * scale.double().abs() + shift.double().abs(), K + 2
    return ref, A, K


def plain_ratio(got, ref, A, K, name):
    """worst |got - ref| / (g_k(K) * A) of an fp32 output; exact where A == 0"""
    got, ref = got.double(), ref.double()
    ratio = _ratio((got - ref).abs(), g_k(K) * A.double())
    if ratio.numel() == 0:
        return Report(name, 0.0, ())
    flat = int(torch.argmax(ratio))
    seen = torch.where(A.double() > 0, (got - ref).abs() / (U * A.double()).clamp_min(1e-300), torch.zeros_like(ref))
    seen = seen[torch.isfinite(seen)]
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ref.shape), float(seen.max()) if seen.numel() else 0.0)


def check_plain(got, ref, A, K, name):
    r = plain_ratio(got, ref, A, K, name)
    print(r)
    assert r.ok, str(r)
    return r


def check_avgpool(got, x, scale=None, shift=None, name="avgpool"):
    ref, A, K = avgpool_ref(x, scale, shift)
    return check_plain(got, ref, A, K, name)


def check_bcast(got, v, R, bf16, name="bcast_rows"):
    """got [N][R][C] as stored against v [N][C] * fp32(1 / R)"""
    ref = (v.double() * f32(1.0 / R)).unsqueeze(1).expand(-1, R, -1)
    return check_stored(got, ref, ref.abs(), K_BCAST, bf16, name)


def se_gate_grad_ref(dout, mask, y, scale, shift):
    """dout, y [N][R][C], mask [N][R][C] bool -> (ref, A, K) of dg [N][C]"""
    d, yv = dout.double(), y.double()
    d = torch.where(mask, d, torch.zeros_like(d))
    z = yv * scale.double() + shift.double()
    Az = yv.abs() * scale.double().abs() + shift.double().abs()
    return (d * z).sum(1), (d.abs() * Az).sum(1), dout.shape[1] + 3


def check_se_gate_grad(got, dout, mask, y, scale, shift, name="se_gate_grad"):
    ref, A, K = se_gate_grad_ref(dout, mask, y, scale, shift)
    return check_plain(got, ref, A, K, name)


def dropout_ref(x, keep, p, A=None):
    """keep ? x / (1 - p) : 0 with p as the fp32 value the kernel received; A: the magnitude behind x (default |x|)"""
    s = 1.0 / (1.0 - f32(p))
    k = keep.double()
    return x.double() * k * s, (x.double().abs() if A is None else A.double()) * k * s


def check_dropout(got, x, keep, p, name="dropout"):
    ref, A = dropout_ref(x, keep, p)
    return check_plain(got, ref, A, K_DROPOUT, name)


def eval_coef_ref(gamma, beta, rm, rv, eps):
    """BatchNorm coefficients from the running statistics as ecg_bn_eval_coef forms them in fp32:
    invstd = 1 / sqrtf(rv + eps): the sum, the root, the division, one spare for a root that is not correctly rounded: g_k(4);
    scale = gamma * invstd: g_k(5);  shift = beta - rm * scale: the product and the difference on top of scale's error;
    mean = rm, exactly."""
    g, b, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
    inv = 1.0 / (rv + f32(eps)).sqrt()
    scale = g * inv
    d_scale = g_k(5) * scale.abs()
    shift = b - rm * scale
    d_shift = rm.abs() * d_scale + g_k(2) * (b.abs() + (rm * scale).abs() + rm.abs() * d_scale)
    return CoefRef(dict(scale=scale, shift=shift, mean=rm, invstd=inv),
                   dict(scale=d_scale, shift=d_shift, mean=torch.zeros_like(rm), invstd=g_k(4) * inv))


def check_bn_eval_bwd(dout, y, coef, bf16, K_sum, dgamma, dbeta, dy=None, dz_out=None, dbias=None, K_bias=None,
                      maskref=None, gate=None, addc=None, name="bn_eval_bwd"):
    """check_bn_bwd for the affine (eval-mode) backward: dy = dz * scale (K_EVAL_DY); dgamma / dbeta / dz_out / dbias as there"""
    unsure, mask = None, None
    if isinstance(maskref, str):
        mask, unsure = affine_mask(y, coef[0], coef[1])
        check_unsure(unsure, name)
    elif maskref is not None:
        mask = maskref.double() > 0
    dz, A, masked = bn_dz_ref(dout, mask, gate, addc)
    xh = xhat_ref(y, coef)
    swing = None if unsure is None else (dout.double() * (1 if gate is None else gate.double()))
    sums, slack, mags = bn_bwd_sums_ref(dz, A, xh, unsure, swing)
    out = {}
    if dbeta is not None:
        out["dbeta"] = check_sum(dbeta, sums[0], mags[0], K_DZ + K_sum + 1, name + " dbeta", slack[0]).ratio
        out["dgamma"] = check_sum(dgamma, sums[1], mags[1], K_DZXHAT + K_sum + 1, name + " dgamma", slack[1]).ratio
    if dz_out is not None:
        bad = (dz_out.double() != masked)
        if unsure is not None:
            bad &= ~unsure
        assert not bool(bad.any()), "%s dz_out: %d elements are not the masked gradient" % (name, int(bad.sum()))
        out["dz_out"] = 0.0
    if dy is not None:
        want, Ady = bn_eval_dy_ref(dz, A, coef[0])
        out["dy"] = check_stored(dy, want, Ady, K_EVAL_DY, bf16, name + " dy", skip=unsure).ratio
    if dbias is not None:
        s = dy.double()
        out["dbias"] = check_sum(dbias, s.sum(0), s.abs().sum(0), K_bias + 1, name + " dbias").ratio
    return out


# ----------------------------------------------------------------------------------------------------------------------
# fp32-operand convolutions (csrc/conv_igemm.hip, csrc/conv_wgrad.hip, csrc/conv_stem.hip with dtype fp32): operands taken
# as given, the float64 convolution of the same operands is the answer, outputs stored as fp32.
#
#   derived (nothing calibrated):  |out - ref| <= g_k(K + 2) * A
#       A: the same convolution of absolute values (+ |bias| + |addend|), K the number of summands -- Cs * taps for y / dx,
#       the pixel count for a weight gradient.  The dense section's dot_bound: an fp32 dot product summed in ANY order (the
#       f32-input MFMA's fma chain, split-K slabs folded afterwards), + 2 for the bias / addend add and one more operation
#       (accumulate = 1).  ReLU keeps it (1-Lipschitz).  Where A == 0 -- a pixel a stride-2 or 1x1 convolution never reads --
#       the result must be exact.
#   calibrated:  y / dx  |out - ref| <= KAPPA_F32 * A;   dw  |dw - ref| <= EPS_DW_F32 * rms(ref) + TAU_DW_F32 * A  (check_dw's form)
#       by the rule of the bf16 constants above: at most 4x the largest value measured against float64 on the MI355X over
#       tests/test_conv_edges_f64_gpu.py, unless torch's own CPU fp32 conv2d / autograd of the same operands needs more
#       (tests/test_f64check.py: test_fp32_conv_checker_accepts_torch_fp32); then torch sets the constant.
#   The assertion is the smaller of the two bounds, element by element.
#   statistics rows:  colsum_ratio, slack = the per-element bound summed over the column, sigma = g_k(chain) with the chain
#       DERIVED from conv_igemm's epilogue: a lane adds its 4 pixels (TP = 4 fragments of a 64-pixel half tile) into s1: 4
#       additions, row16_sum folds the 16 pixel lanes in 4 DPP butterfly levels: 4 more -> 8; s2 adds the rounding of v * v: 9.
#       The rows themselves are summed in double by the test: 0.  (conv_stem's per-tile rows: 2 pixels per lane + 4 levels = 6,
#       held to the same 8 / 9.)
#
# Measured on the MI355X over tests/test_conv_edges_f64_gpu.py (every fp32 case of groups a, b, d, e):
#   y / dx   max |err| / A           3.07e-7  (1x1 stride-2 input gradient, 256 summands, L = 313)   -> KAPPA_F32 = 1.2e-6
#   dw       max |err| / A           3.55e-7  (12-lead stem, 334 pixels)                             -> TAU_DW_F32 = 1.4e-6
#   dw       max |err| / rms(ref)    8.73e-7  (7x7 stem on 1x1 images)                               -> EPS_DW_F32 = 3.4e-6
# (4 x 3.55e-7 = 1.42e-6 and 4 x 8.73e-7 = 3.49e-6, rounded down, happen to land on the values of the bf16 TAU_DW and EPS_DW;
#  nothing was taken over from them.)
# torch's CPU fp32 on the operands of tests/test_f64check.py (K = 1152; 9600 pixels): y 6.1e-8, dx 9.0e-8 of A, under
#   KAPPA_F32.  Its dw errs by up to 9.7e-7 of A (a serial sum over the pixels) and 6.1e-6 of rms(ref): the second figure is ABOVE
#   EPS_DW_F32 taken alone, but the bound is the sum eps * rms + tau * A, and 9.7e-7 of A is under TAU_DW_F32 by itself, so
#   torch passes on the tau term (worst ratio 0.49) and sets no constant.
# ----------------------------------------------------------------------------------------------------------------------
KAPPA_F32 = 1.2e-6
EPS_DW_F32 = 3.4e-6
TAU_DW_F32 = 1.4e-6
STATS_CHAIN_F32 = 8          # 4 pixels per lane + the 16-lane butterfly (above)


def f32_bound(acc_abs, K, kappa=KAPPA_F32):
    """per-element bound of an fp32 y / dx: the smaller of the derived and the calibrated constant, times A"""
    return min(g_k(K + 2), kappa) * acc_abs.double()


def _f32_report(err, bound, acc_abs, name):
    """Report of |err| against a bound tensor; the accumulation term reported is max |err| / A over the elements with A > 0"""
    ratio = _ratio(err, bound)
    flat = int(torch.argmax(ratio))
    seen = torch.where(acc_abs > 0, err / acc_abs.clamp_min(1e-300), torch.zeros_like(err))
    seen = seen[torch.isfinite(seen)]
    return Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, err.shape), float(seen.max()) if seen.numel() else 0.0)


def f32_ratio(out, ref, acc_abs, K, kappa=KAPPA_F32, name="out"):
    """worst |out - ref| / bound of an fp32-operand conv output; out, ref, acc_abs: same shape.  The accumulation term
    reported is the measured kappa"""
    out, ref, acc_abs = out.double(), ref.double(), acc_abs.double()
    return _f32_report((out - ref).abs(), f32_bound(acc_abs, K, kappa), acc_abs, name)


def check_f32(out, ref, acc_abs, K, kappa=KAPPA_F32, name="out"):
    r = f32_ratio(out, ref, acc_abs, K, kappa, name)
    print(r)
    assert torch.isfinite(out.double()).all(), name + ": non-finite output"
    assert r.ok, str(r)
    return r


def dw_f32_ratio(dw, ref, acc_abs, K, eps=EPS_DW_F32, tau=TAU_DW_F32, name="dw"):
    """fp32-operand weight gradient: bound = min(g_k(K + 2) * A, eps * rms(ref) + tau * A), K = the pixel count.  The
    accumulation term reported is the measured tau; eps_seen = max |err| / rms(ref), rel_l2 for the record (not asserted:
    the per-element bound is the stricter statement and no bar for the norm has been derived)"""
    dw, ref, acc_abs = dw.double(), ref.double(), acc_abs.double()
    err = (dw - ref).abs()
    rms = float(ref.pow(2).mean().sqrt())
    r = _f32_report(err, torch.minimum(g_k(K + 2) * acc_abs, eps * rms + tau * acc_abs), acc_abs, name)
    fin = err[torch.isfinite(err)]
    r.eps_seen = (float(fin.max()) if fin.numel() else 0.0) / max(rms, 1e-300)
    r.rel_l2 = float((dw - ref).norm() / ref.norm().clamp_min(1e-300))
    return r


def check_dw_f32(dw, ref, acc_abs, K, eps=EPS_DW_F32, tau=TAU_DW_F32, name="dw"):
    r = dw_f32_ratio(dw, ref, acc_abs, K, eps, tau, name)
    print(r, " rel L2 %.3g, max|err| / rms %.3g" % (r.rel_l2, r.eps_seen))
    assert torch.isfinite(dw.double()).all(), name + ": non-finite weight gradient"
    assert r.ok, str(r)
    return r


def check_stats_f32(rows, ref, K, chain=STATS_CHAIN_F32, kappa=KAPPA_F32, name="stats"):
    """rows [n][2][C] fp32 as an fp32 forward wrote them; ref: conv_ref64 of the same operands (+ bias); K = Cs * taps"""
    rows = rows.double()
    y, b = ref.y, f32_bound(ref.ay, K, kappa)
    dims = (0, 2, 3)
    a = check_colsums(rows[:, 0].sum(0), y.sum(dims), b.sum(dims), y.abs().sum(dims), sigma=g_k(chain), name=name + " sum y")
    c = check_colsums(rows[:, 1].sum(0), (y * y).sum(dims), (2 * y.abs() * b + b * b).sum(dims), (y * y).sum(dims),
                      sigma=g_k(chain + 1), name=name + " sum y^2")
    return max(a.ratio, c.ratio)


# ----------------------------------------------------------------------------------------------------------------------
# The two elementwise passes only the inference plans run (csrc/infer_fold.hip), tensors channels-last.
#
#   relu_maxpool:   out = max(0, max over the in-image taps of the 3x3 / stride 2 / pad 1 window), H may be 1.  The kernel only
#                   compares stored values and writes one of them, or 0, so the float64 window maximum of the STORED input,
#                   clamped at 0, is the answer and the bar is exact equality.  No output carries a sign bit (a window of
#                   -0.0 or of negative values gives +0) and a NaN tap never wins: it is skipped like a tap outside the image.
#   gate_res_relu:  out = max(0, y * gate[row // rows_per_sample] + res), A = |y| |gate| + |res|: a product and a sum, two
#                   roundings of A at most whether or not the compiler contracts them -- fp32 check_f32 with K = 2 summands
#                   (g_k(4), below KAPPA_F32), bf16 the one-sided ReLU bound of tests/infer_ref.py with KAPPA unchanged (2 u
#                   is 1.2e-7 of A).  Nothing is calibrated.
# ----------------------------------------------------------------------------------------------------------------------
def relu_maxpool_ref(y):
    """y [N][H][W][C] as stored (any float dtype) -> float64 [N][OH][OW][C]: max(0, window maximum), NaN taps skipped"""
    y = y.double()
    N, H, W, C = y.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = torch.full((N, 2 * OH + 1, 2 * OW + 1, C), float("-inf"), dtype=torch.float64, device=y.device)
    p[:, 1:H + 1, 1:W + 1] = torch.where(torch.isnan(y), torch.full_like(y, float("-inf")), y)
    ref = torch.zeros((N, OH, OW, C), dtype=torch.float64, device=y.device)
    for kh in range(3):
        for kw in range(3):
            ref = torch.maximum(ref, p[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2])
    return ref


def relu_maxpool_ratio(out, y_stored, N, H, W, C, bf16, name="relu_maxpool"):
    """out [N][OH][OW][C] (or flat) as the kernel stored it against relu_maxpool_ref of the stored input: ratio 0 where
    every element is the reference exactly, is finite and has no sign bit; inf otherwise.  .bad counts the elements"""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    want = torch.bfloat16 if bf16 else torch.float32
    assert out.dtype == want and y_stored.dtype == want, "%s: tensors are not in the stored type" % name
    ref = relu_maxpool_ref(y_stored.reshape(N, H, W, C))
    got = out.reshape(N, OH, OW, C).double()
    bad = ~(got == ref) | torch.signbit(got)
    r = Report(name, 0.0, ())
    r.bad = int(bad.sum())
    if r.bad:
        r.ratio, r.where = float("inf"), _unravel(int(torch.argmax(bad.reshape(-1).to(torch.uint8))), ref.shape)
    return r


def check_relu_maxpool(out, y_stored, N, H, W, C, bf16, name="relu_maxpool"):
    r = relu_maxpool_ratio(out, y_stored, N, H, W, C, bf16, name)
    print(r, "%d elements differ" % r.bad)
    assert r.ok, "%s: %d elements are not max(0, window maximum) of the stored input, first at %s" % (name, r.bad, r.where)
    return r


def gate_res_relu_ref(y, gate, res, rows_per_sample):
    """y, res [M][C] as stored, gate [N][C] fp32 -> (the float64 value BEFORE the ReLU, A)"""
    y, res = y.double(), res.double()
    g = per_row(gate, rows_per_sample, y.shape[0])
    return y * g + res, y.abs() * g.abs() + res.abs()


def gate_res_relu_ratio(out, y, gate, res, rows_per_sample, bf16, name="gate_res_relu"):
    pre, A = gate_res_relu_ref(y, gate, res, rows_per_sample)
    out = out.reshape(pre.shape)
    if bf16:
        from .infer_ref import relu_bf16_ratio      # (infer_ref imports this module)
        return relu_bf16_ratio(out, pre, A, name=name)
    assert bool((out.double() >= 0).all()), name + ": negative value after ReLU"
    return f32_ratio(out, pre.clamp_min(0), A, 2, name=name)


def check_gate_res_relu(out, y, gate, res, rows_per_sample, bf16, name="gate_res_relu"):
    """(out >= 0 rejects NaN as well)"""
    r = gate_res_relu_ratio(out, y, gate, res, rows_per_sample, bf16, name)
    print(r)
    assert torch.isfinite(out.double()).all(), name + ": non-finite output"
    assert r.ok, str(r)
    return r


# ----------------------------------------------------------------------------------------------------------------------
# Grad-CAM of the two ResNet encoders (csrc/gradcam.hip: ecgmm_gradcam, the map kernels behind ecgmm_resnet18_gradcam and
# ecgmm_resnet1d_gradcam).  act [N][R = Hs * Ws][C] in the compute dtype and dpooled [N][C] fp32 are taken as given (a bf16
# act already rounded), and the float64 evaluation of
#     s = relu((1 / R) sum_c dpooled[n][c] act[n][r][c]),   q = s / max_r s  (all zero where the maximum is 0),
#     out = F.interpolate(q, (H, W), mode="bilinear", align_corners=False)
# is the exact answer.  Three stages, nothing calibrated:
#
#   weighted sum   e1 = g_k(C + 2) A,  A = (1 / R) sum_c |dpooled| |act|: the dot-product bound of C summands in any order
#                  (lanes stride the channels, then a wave butterfly); the + 2 are the multiplication by the fp32 value of
#                  1 / R and that value's own rounding.  ReLU is 1-Lipschitz and adds nothing.  Where dpooled itself is only
#                  known to within dd (the plan entry points: the fp32 classifier backward against its float64 value), the
#                  kernel's sum is that of dpooled + delta, |delta| <= dd:  e1 += (1 + g_k(C + 2)) (1 / R) sum_c dd |act|.
#   normalise      with m = max_r s and em = max_r e1 (a maximum moves by no more than its arguments),
#                      |s~ / m~ - s / m| = |(s~ - s) m - s (m~ - m)| / (m m~) <= (e1 + q em) / (m - em) =: d      (em < m)
#                  and the encoders' form, q~ = s~ * fl(1 / m~), rounds twice more:  e2 = d + g_k(2) (q + d).
#                  m == 0: every sum is <= 0; a sample none of whose sums fp32 can lift above 0 (|sum| > e1 everywhere) must be
#                  exactly 0.  A maximum inside its own error (m <= em) decides nothing.  No error of a map in [0, 1] may
#                  exceed 1: the bound is capped there, which is also what "decides nothing" means.
#   upsample       per axis the kernel forms src~ = (dst + 0.5) * fl(in / out) - 0.5 in fp32: dst + 0.5 is exact, the quotient,
#                  the product and the difference round once each, so |src~ - src| <= g_k(3) (|src| + 1) =: dsrc (src before
#                  the clamp at 0, which is 1-Lipschitz).  The weight lam = src~ - floor(src~) is exact.  Write f~ for the
#                  bilinear interpolant of the kernel's coarse map q~ and f for that of q:
#                      |out - f(src)| <= |f~(src) - f(src)| + |f~(src~) - f~(src)| + rounding of the lerp
#                    * the first term is the interpolant of q~ - q at the exact coordinate: a convex combination of the four
#                      neighbours' errors, at most the largest of them;
#                    * f~ is continuous and piecewise linear in each coordinate, so the second is at most dsrc times the
#                      largest slope |q~[i + 1] - q~[i]| between src and src~.  Being continuous it needs no special case
#                      where fp32 and float64 choose a different i0 at an integer boundary: the two cells agree on their
#                      common edge.  The slope is taken over the cell and its neighbours on either side (a 3 x 3 dilation of
#                      the per-node largest adjacent difference), and from q with 2 max(e2) added for q~;
#                    * the lerp c0 * fl(1 - lam) + c1 * lam rounds three times on its longest path, per axis: g_k(3) or
#                      g_k(6) times the largest of the four values.
#                  An axis with in == out has fl(in / out) = 1, src~ = dst exactly and lam = 0: c0 * 1 + c1 * 0 is c0, no
#                  rounding and no coordinate term -- with both axes so, out is the coarse map bit for bit.
#   Given the kernel's own stored coarse map (`small`), the upsample is checked on its own from it, as every consumer stage
#   in this file is (e_in = 0), and the coarse map against stages 1 and 2.
#
# What the bound can and cannot resolve: at C = 512 the first stage alone is 514 u A / m of a map in [0, 1], some hundreds of
# fp32 ulps where the channel sum cancels -- it is the standard bound, not tightened to the kernel's tree.  Lost channels, a
# neighbour's weights or maximum, swapped extents, align_corners=True, a missing -0.5, a missing ReLU and a border clamped
# one early are all orders of magnitude outside it (tests/test_gradcam_cpu.py); a few fp32 ulps on one element are resolved
# only where the derivation leaves no room: a sample that must be exactly 0, and the upsample of a stored coarse map at
# identity size.  Dropping the 1 / R scale cancels in the normalisation and is accepted, as it must be.
# Measured on the MI355X: tests/test_gradcam_f64_gpu.py, module docstring.
# ----------------------------------------------------------------------------------------------------------------------
# (N, Hs, Ws, C, H, W) -> the sample given an all-negative dpooled (None: none)
GRADCAM_CASES = {
    (2, 7, 7, 512, 224, 224): None,
    (1, 8, 79, 512, 250, 2500): None,
    (2, 1, 313, 256, 1, 5000): None,
    (3, 1, 1, 64, 5, 9): 1,
    (2, 3, 5, 70, 3, 5): 0,
    (2, 9, 11, 33, 4, 6): None,
    (5, 2, 3, 8, 7, 7): 2,
    (2, 17, 19, 16, 40, 40): None,
    (5, 2, 2, 8, 512, 512): 4,
}
# a sample meant to be nonzero has its float64 maximum at least this many times above the weighted-sum bound
GRADCAM_MARGIN = 100.0


# the salt of the operands: chosen on the float64 reference alone (tests/test_gradcam_cpu.py asserts it) so that every live
# sample of every case clears GRADCAM_MARGIN -- with R == 1 a sample has one sum, which half the salts make negative
GRADCAM_SALT = 10


def gradcam_inputs(case, bf16, salt=GRADCAM_SALT):
    """act [N][R][C] >= 0 with about half its elements 0, as behind a ReLU (bf16-rounded for bf16), dpooled [N][C] of mixed
    signs (the ReLU clips about half the positions); the case's negative sample gets -|dpooled| - 2^-10 (every weighted sum of it is <= 0)"""
    from oracle import fill
    N, Hs, Ws, C, H, W = case
    act = _b(fill.hash_tensor((N, Hs * Ws, C), 7001 + salt).clamp_min(0), bf16)
    dp = fill.hash_tensor((N, C), 7002 + salt, 0.5)
    neg = GRADCAM_CASES.get(tuple(case))
    if neg is not None:
        dp[neg] = -dp[neg].abs() - 2.0 ** -10
    return act, dp


@dataclass
class GradcamRef:
    pre: torch.Tensor        # (1 / R) sum_c dpooled * act before the ReLU           [N][R] float64
    A: torch.Tensor          # the same on absolute values
    m: torch.Tensor          # per-sample maximum of relu(pre)                        [N]
    small: torch.Tensor      # the normalised coarse map                              [N][Hs][Ws]
    out: torch.Tensor        # upsampled                                              [N][H][W]
    e_small: torch.Tensor    # allowed |error| of the coarse map (stages 1 and 2)     [N][Hs][Ws]
    e_out: torch.Tensor      # allowed |error| of the map from the operands (all three stages)
    em: torch.Tensor         # weighted-sum bound at its largest, per sample          [N]


def upsample_ref(small, H, W):
    """small [N][Hs][Ws] -> float64 [N][H][W], F.interpolate(bilinear, align_corners=False)"""
    return F.interpolate(small.double()[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]


def _axis(in_, out_, dev_):
    """float64 source coordinate of every destination index (clamped at 0), its cell i0, i1 and the coordinate error"""
    dst = torch.arange(out_, dtype=torch.float64, device=dev_)
    raw = (dst + 0.5) * (float(in_) / float(out_)) - 0.5
    src = raw.clamp_min(0)
    i0 = src.floor().long().clamp_max(in_ - 1)
    i1 = (i0 + 1).clamp_max(in_ - 1)
    dsrc = torch.zeros_like(src) if in_ == out_ else g_k(3) * (raw.abs() + 1)
    return i0, i1, dsrc


def _dilate(v):
    """largest value of the 3 x 3 neighbourhood, v [N][Hs][Ws]"""
    return F.max_pool2d(v[:, None], 3, stride=1, padding=1)[:, 0]


def upsample_bound(small, e_in, H, W):
    """allowed |out - upsample_ref(small)| of the fp32 upsample of a coarse map known to within e_in (same shape as small,
    or None: the map is the kernel's own stored input)"""
    q = small.double()
    N, Hs, Ws = q.shape
    e = torch.zeros_like(q) if e_in is None else e_in.double()
    h0, h1, dh = _axis(Hs, H, q.device)
    w0, w1, dw = _axis(Ws, W, q.device)
    cell = lambda t: torch.stack([t[:, h0][:, :, w0], t[:, h0][:, :, w1], t[:, h1][:, :, w0], t[:, h1][:, :, w1]]).amax(0)
    e4, v4 = cell(e), cell(q.abs() + e)
    K = 3 * (int(Hs != H) + int(Ws != W))
    bound = e4 + g_k(K) * v4 if K else e4
    emax2 = 2 * _dilate(e)
    z = torch.zeros_like(q)
    if Ws != W:
        d = (q[:, :, 1:] - q[:, :, :-1]).abs()
        node = torch.maximum(torch.cat([d, z[:, :, :1]], 2), torch.cat([z[:, :, :1], d], 2))
        bound = bound + dw.view(1, 1, W) * (_dilate(node) + emax2)[:, h0][:, :, w0]
    if Hs != H:
        d = (q[:, 1:] - q[:, :-1]).abs()
        node = torch.maximum(torch.cat([d, z[:, :1]], 1), torch.cat([z[:, :1], d], 1))
        bound = bound + dh.view(1, H, 1) * (_dilate(node) + emax2)[:, h0][:, :, w0]
    return bound.clamp_max(1.0)


def gradcam_ref(act, dpooled, Hs, Ws, H, W, dpooled_err=None):
    """float64 Grad-CAM of the operands as given and the allowed error of every element.  act [N][Hs * Ws][C] (any float dtype),
    dpooled [N][C]; dpooled_err [N][C]: what the kernel's dpooled may differ by from the one given here"""
    a, d = act.double(), dpooled.double()
    N, R, C = a.shape
    assert R == Hs * Ws and d.shape == (N, C)
    pre = torch.einsum("nrc,nc->nr", a, d) / R
    A = torch.einsum("nrc,nc->nr", a.abs(), d.abs()) / R
    e1 = g_k(C + 2) * A
    if dpooled_err is not None:
        e1 = e1 + (1 + g_k(C + 2)) * torch.einsum("nrc,nc->nr", a.abs(), dpooled_err.double()) / R
    s = pre.clamp_min(0)
    m, em = s.amax(1), e1.amax(1)
    live = (m > 0)[:, None]
    q = torch.where(live, s / m.clamp_min(1e-300)[:, None], torch.zeros_like(s))
    room = (m - em)[:, None]
    dq = torch.where(room > 0, (e1 + q * em[:, None]) / room.clamp_min(1e-300), torch.full_like(q, float("inf")))
    e2 = dq + g_k(2) * (q + dq)
    # m == 0: exactly zero unless fp32 may lift some sum of the sample above 0
    may_rise = ((e1 >= pre.abs()) & (e1 > 0)).any(1, keepdim=True)
    e2 = torch.where(live, e2, torch.where(may_rise, torch.ones_like(e2), torch.zeros_like(e2))).clamp_max(1.0)
    small, e_small = q.view(N, Hs, Ws), e2.view(N, Hs, Ws)
    return GradcamRef(pre, A, m, small, upsample_ref(small, H, W), e_small, upsample_bound(small, e_small, H, W), em)


def gradcam_ratio(out, ref, small=None, name="gradcam"):
    """worst |err| / bound of a map against gradcam_ref.  small None: out against the three-stage bound.  small given (the
    kernel's stored coarse map): small against stages 1 and 2, out against the float64 upsample of that stored map.
    .parts: the two ratios (small, out)"""
    N, H, W = ref.out.shape
    out = out.reshape(N, H, W).double()
    if small is None:
        ratio = _ratio((out - ref.out).abs(), ref.e_out)
        parts = dict(out=float(ratio.max()))
    else:
        sm = small.reshape(ref.small.shape).double()
        r_small = _ratio((sm - ref.small).abs(), ref.e_small)
        fin = torch.where(torch.isfinite(sm), sm, torch.zeros_like(sm))
        ratio = _ratio((out - upsample_ref(fin, H, W)).abs(), upsample_bound(fin, None, H, W))
        parts = dict(small=float(r_small.max()), out=float(ratio.max()))
        if parts["small"] > parts["out"]:
            flat = int(torch.argmax(r_small))
            r = Report(name + " (coarse map)", parts["small"], _unravel(flat, r_small.shape))
            r.parts = parts
            return r
    flat = int(torch.argmax(ratio))
    r = Report(name, float(ratio.reshape(-1)[flat]), _unravel(flat, ratio.shape))
    r.parts = parts
    return r


def gradcam_live(ref, expect_zero=()):
    """the reference alone: every sample not in expect_zero has its maximum GRADCAM_MARGIN times above the weighted-sum bound
    (never zeros against zeros), every sample in it is all zero with a bound of exactly 0.  -> smallest m / em seen"""
    worst = float("inf")
    for n in range(ref.m.shape[0]):
        if n in expect_zero:
            assert float(ref.m[n]) == 0 and float(ref.out[n].abs().max()) == 0 and float(ref.e_out[n].max()) == 0, n
        else:
            margin = float(ref.m[n] / ref.em[n].clamp_min(1e-300))
            assert margin >= GRADCAM_MARGIN, "sample %d: maximum %.3g against a bound of %.3g" % (n, float(ref.m[n]), float(ref.em[n]))
            worst = min(worst, margin)
    return worst


def check_gradcam(out, ref, small=None, name="gradcam"):
    r = gradcam_ratio(out, ref, small, name)
    print(r, r.parts)
    assert torch.isfinite(out.double()).all(), name + ": non-finite map"
    assert r.ok, str(r) + " " + str(r.parts)
    return r
