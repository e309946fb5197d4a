"""The bf16 conv kernels at the benchmarked step's layer shapes, element by element against float64 (tests/f64check.py).

Part 1 -- every distinct conv geometry of the step at batch 256 (ResNet18 on 224x224, ResNet1D_SE on 5000 samples of one
lead), called through the ABI with the arguments the encoder plans pass (csrc/plan_resnet18.hip, csrc/plan_resnet1d.hip)
and the library's switches at their defaults: forward with statistics rows (per workgroup for the 2-D layers, per 64
pixels with the Conv1d bias for the 1-D ones), input gradient without and with the residual addend, the stride-2 entries'
input gradient with the folded downsample branch, weight gradients at the default split, the two stems.  Then the other
real batch sizes where they change the tiles per workgroup (image-only 128: layers 1-2; 12 leads at 512: stem and 1-D
blocks) and the fused BatchNorm-backward reduction (MODE 1, ecgmm_conv_bwd_data_bnred) at layers 1 and 2.

Part 2 -- the persistent loop of conv_halo_kernel at moderate cost: halo launches capped to 1, 7 and 13 CUs
(ecgmm_conv_halo_cus) on 25-tile problems whose tiles span image boundaries (25 % Gk != 0 for every cap), one case per
launch_halo instantiation ecg_conv_halo (csrc/conv_halo.hip) dispatches:

  instantiation <BN, RS, MODE, NCS1, NW, PP, ST, AD>   test id (test_persistent_halo_loop[<id>-<cap>])
  <64, 9, 0, false, 4>                    w4_fwd           (ecgmm_conv_halo_w4(1))
  <64, 9, 2, false, 4>                    w4_dgrad         (ecgmm_conv_halo_w4(1))
  <64, 9, 0, true, 8, false, true>        stream_fwd       (stream form, statistics rows per workgroup)
  <64, 9, 2, true, 8, false, true>        stream_dgrad
  <64, 9, 2, true, 8, false, true, true>  stream_dgrad_add
  <64, 9, 0, true>                        ncs1_fwd_bias    (the bias keeps it off the stream form)
  <64, 9, 2, true>                        ncs1_dgrad_add   (ecgmm_conv_halo_stream(0))
  <64, 9, 1, true>                        ncs1_bnred
  <128, 9, 0, false, 8, true>             pp_fwd
  <128, 9, 2, false, 8, true>             pp_dgrad_add
  <128, 9, 1, false, 8, true>             pp_bnred_sep     (separate ReLU mask, masked store, addend)
  <128, 9, 0>                             lock_fwd         (ecgmm_conv_halo_pingpong(0))
  <128, 9, 2>                             lock_dgrad_add   (ecgmm_conv_halo_pingpong(0))
  <128, 9, 1>                             lock_bnred       (ecgmm_conv_halo_pingpong(0))
  <64, 9, 0>                              c64_fwd          (128 -> 64 channels: two K slices)
  <64, 9, 2>                              c64_dgrad_add
  <64, 9, 1>                              c64_bnred
  <128, 3, 0>                             rs3_fwd_bias     (1x3, Conv1d bias)
  <128, 3, 2>                             rs3_dgrad_add
  <128, 3, 1>                             rs3_bnred_sep
  <64, 3, 0>                              rs3_c64_fwd_bias
  <64, 3, 2>                              rs3_c64_dgrad
  <64, 3, 1>                              rs3_c64_bnred

Calibration (tests/f64check.py) from this file on the MI355X: worst fp32 accumulation term of a bf16 output 7.6e-8 of the
|.| convolution (KAPPA = 3e-7), of a weight gradient 1.8e-7 of |x|^T |dy| and 8.6e-7 of rms(dw) (EPS_DW = 3.4e-6; TAU_DW = 1.4e-6
is set by torch's CPU fp32 weight gradient, which must also pass), of the
BatchNorm partial rows 1.0e-7 of the summed magnitudes (SIGMA = 4e-7); every bf16 output's worst ratio to its bound is the
half-ulp rounding (0.98 - 0.997).  The whole module runs in about 8 s.

Every output (y, dx, dw, statistics and reduction rows) and every workspace is NaN before the launch, and y / dx carry GUARD
NaN elements behind the last valid one that must still be NaN afterwards (the helpers are shared with
tests/test_conv_edges_f64_gpu.py, which runs them in fp32 as well).

Inputs are generated on the device from fixed seeds and rounded to bf16: activations non-negative with exact zeros,
gradients signed; both with an offset per image and per channel, so that reading a neighbouring image or channel gives a
large error instead of a plausible one.
"""
import ctypes as C
import time

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from .util import DEV, switches

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BN_TAIL = 64
GUARD = 64             # NaN elements behind every y / dx: a store past the last valid element shows
TDT = {L.BF16: BF, L.F32: torch.float32}


# ------------------------------------------------------------------------------------------------ operands and calls
def _gen(shape, seed, kind, fan_in=1):
    """bf16-exact float32 tensor on the device.  act: >= 0 with exact zeros; grad: signed; w: weights"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(shape, device=DEV, generator=g)
    if kind == "w":
        return (z * (2.0 / fan_in) ** 0.5).to(BF).float()
    n, c = shape[0], shape[1]
    k = ((torch.arange(n, device=DEV).view(-1, 1) * 37 + torch.arange(c, device=DEV).view(1, -1) * 11 + seed) % 64).float()
    k = k.view(n, c, *([1] * (len(shape) - 2)))
    if kind == "act":
        t = torch.where(z > 0, z + 1.0 + k / 16, torch.zeros_like(z))
    else:
        t = z + (k - 31.5) / 16
    return t.to(BF).float()


def _nhwc(t, dt=L.BF16):
    return t.permute(0, 2, 3, 1).contiguous().to(TDT[dt])


def _nchw(t, n, h, w, c):
    return t.view(n, h, w, c).permute(0, 3, 1, 2).double()


def _pack(w, dt=L.BF16):
    """OIHW fp32 -> (forward, dgrad) packs in the compute dtype, by the library's packer (what the plans call)"""
    n = w.numel()
    f = torch.empty(n, device=DEV, dtype=TDT[dt])
    d = torch.empty(n, device=DEV, dtype=TDT[dt])
    L.check(L.lib().ecgmm_pack_conv_weight(dt, ptr(w.contiguous()), ptr(f), ptr(d), w.shape[0], w.shape[1],
                                           w.shape[2] * w.shape[3], stream()))
    return f, d


def poisoned(n, dtype):
    """n elements for a kernel to fill and GUARD more behind them, all NaN: what it leaves unwritten stays NaN (the
    checkers assert finiteness), what it writes past the end shows in the guard"""
    return torch.full((n + GUARD,), float("nan"), device=DEV, dtype=dtype)


def unguard(buf, n, name):
    torch.cuda.synchronize()
    assert torch.isnan(buf[n:].float()).all(), name + ": written past its last element"
    return buf[:n]


class Geo:
    def __init__(self, N, H, W, Cin, Cout, R, S, stride, ph, pw):
        self.N, self.H, self.W, self.Cin, self.Cout, self.R, self.S = N, H, W, Cin, Cout, R, S
        self.stride, self.ph, self.pw = stride, ph, pw
        self.OH = (H + 2 * ph - R) // stride + 1
        self.OW = (W + 2 * pw - S) // stride + 1
        self.d = L.ConvDesc(N, H, W, Cin, Cout, R, S, stride, ph, pw)

    @property
    def M(self):
        return self.N * self.OH * self.OW


def _stats_buf(g):
    rows = max(L.lib().ecgmm_conv_stats_rows(g.M), 512) + BN_TAIL
    return torch.full((rows, 2, g.Cout), float("nan"), device=DEV)


def fwd(g, x, wf, bias=None, wgrows=True, dt=L.BF16):
    """-> y [N, Cout, OH, OW] float64, statistics rows [n][2][Cout], the NaN rows behind them"""
    lib = L.lib()
    y = poisoned(g.M * g.Cout, TDT[dt])
    st = _stats_buf(g)
    if wgrows:
        n = C.c_int(0)
        L.check(lib.ecgmm_conv_fwd_wgrows(dt, C.byref(g.d), ptr(x), ptr(wf), ptr(bias), ptr(y), ptr(st), C.byref(n), 0,
                                          stream()))
        rows = n.value
    else:
        L.check(lib.ecgmm_conv_fwd(dt, C.byref(g.d), ptr(x), ptr(wf), ptr(bias), ptr(y), ptr(st), 0, stream()))
        rows = lib.ecgmm_conv_stats_rows(g.M)
    y = unguard(y, g.M * g.Cout, "y")
    assert 1 <= rows <= st.shape[0] - BN_TAIL
    return _nchw(y, g.N, g.OH, g.OW, g.Cout), st[:rows], st[rows:]


def dgrad(g, dy, wd, addend=None, dt=L.BF16):
    n = g.N * g.H * g.W * g.Cin
    dx = poisoned(n, TDT[dt])
    L.check(L.lib().ecgmm_conv_bwd_data(dt, C.byref(g.d), ptr(dy), ptr(wd), ptr(addend), ptr(dx), stream()))
    return _nchw(unguard(dx, n, "dx"), g.N, g.H, g.W, g.Cin)


def nan_workspace(nbytes):
    """a workspace of at least nbytes whose every float is NaN: a slab the kernel leaves unwritten reaches the result"""
    return torch.full((max(nbytes, 4) // 4 + 1,), float("nan"), device=DEV)


def wgrad(g, x, dy, dt=L.BF16, accumulate=0, dw=None):
    lib = L.lib()
    nb = lib.ecgmm_conv_bwd_weight_workspace(dt, C.byref(g.d))
    ws = nan_workspace(nb)
    if dw is None:
        dw = torch.full((g.Cout, g.Cin, g.R, g.S), float("nan"), device=DEV)
    L.check(lib.ecgmm_conv_bwd_weight(dt, C.byref(g.d), ptr(x), ptr(dy), ptr(dw), accumulate, ptr(ws), nb, stream()))
    torch.cuda.synchronize()
    return dw


def _check_fwd(tag, y, rows, ref):
    r = F64.check_bf16(y, ref.y, ref.ay, name=tag + " y")
    F64.check_stats(rows, ref, name=tag + " stats")
    return r


# ------------------------------------------------------------------------------------------------ part 1: layer shapes
def _body(tag, N, H, W, C_, R, bias_on, seed, wgrows):
    """stride-1 layer Cin = Cout = C_: forward (+ statistics rows), input gradient without / with the residual addend
    (conv2 / conv1 of a block), weight gradient"""
    S, ph = 3, (1 if R == 3 else 0)
    g = Geo(N, H, W, C_, C_, R, S, 1, ph, 1)
    x = _gen((N, C_, H, W), seed, "act")
    w = _gen((C_, C_, R, S), seed + 1, "w", C_ * R * S)
    dy = _gen((N, C_, H, W), seed + 2, "grad")
    add = _gen((N, C_, H, W), seed + 3, "grad")
    b = _gen((C_, 1), seed + 4, "grad").view(-1) if bias_on else None
    t0 = time.time()
    ref = F64.conv_ref64(x, w, dy, 1, (ph, 1), bias=b)
    t_ref = time.time() - t0
    xg, dyg, addg = _nhwc(x), _nhwc(dy), _nhwc(add)
    wf, wd = _pack(w)
    y, rows, tail = fwd(g, xg, wf, b, wgrows)
    out = [_check_fwd(tag, y, rows, ref)]
    out.append(F64.check_bf16(dgrad(g, dyg, wd), ref.dx, ref.adx, name=tag + " dx"))
    out.append(F64.check_bf16(dgrad(g, dyg, wd, addg), ref.dx + add.double(), ref.adx + add.double().abs(),
                              name=tag + " dx+addend"))
    out.append(F64.check_dw(wgrad(g, xg, dyg), ref.dw, ref.adw, name=tag + " dw"))
    print("%s: float64 reference %.1f s" % (tag, t_ref))
    return out


def _entry(tag, N, H, W, Cin, Cout, R, bias_on, seed, wgrows):
    """stage entry: stride-2 conv1 (3x3 / 1x3) and the 1x1 stride-2 downsample: both forwards, the input gradient of the
    two branches in one launch (ecgmm_conv_bwd_data_with_downsample, parity classes), both weight gradients"""
    ph = 1 if R == 3 else 0
    g = Geo(N, H, W, Cin, Cout, R, 3, 2, ph, 1)
    gd = Geo(N, H, W, Cin, Cout, 1, 1, 2, 0, 0)
    assert (g.OH, g.OW) == (gd.OH, gd.OW)
    x = _gen((N, Cin, H, W), seed, "act")
    w = _gen((Cout, Cin, R, 3), seed + 1, "w", Cin * R * 3)
    wdn = _gen((Cout, Cin, 1, 1), seed + 2, "w", Cin)
    dy = _gen((N, Cout, g.OH, g.OW), seed + 3, "grad")
    dyd = _gen((N, Cout, g.OH, g.OW), seed + 4, "grad")
    b = _gen((Cout, 1), seed + 5, "grad").view(-1) if bias_on else None
    bd = _gen((Cout, 1), seed + 6, "grad").view(-1) if bias_on else None
    t0 = time.time()
    ref = F64.conv_ref64(x, w, dy, 2, (ph, 1), bias=b)
    refd = F64.conv_ref64(x, wdn, dyd, 2, (0, 0), bias=bd)
    t_ref = time.time() - t0
    xg, dyg, dydg = _nhwc(x), _nhwc(dy), _nhwc(dyd)
    wf, wd = _pack(w)
    wdf, wdd = _pack(wdn)
    out = []
    y, rows, _ = fwd(g, xg, wf, b, wgrows)
    out.append(_check_fwd(tag + " conv1", y, rows, ref))
    y, rows, _ = fwd(gd, xg, wdf, bd, wgrows=False)         # (the plans' downsample forward: per-64-pixel rows)
    out.append(_check_fwd(tag + " down", y, rows, refd))
    dx = poisoned(N * H * W * Cin, BF)
    L.check(L.lib().ecgmm_conv_bwd_data_with_downsample(L.BF16, C.byref(g.d), ptr(dyg), ptr(wd), ptr(dydg), ptr(wdd),
                                                        ptr(dx), None, stream()))
    dx = unguard(dx, N * H * W * Cin, tag + " dx")
    out.append(F64.check_bf16(_nchw(dx, N, H, W, Cin), ref.dx + refd.dx, ref.adx + refd.adx, name=tag + " dx (both branches)"))
    out.append(F64.check_dw(wgrad(g, xg, dyg), ref.dw, ref.adw, name=tag + " conv1 dw"))
    out.append(F64.check_dw(wgrad(gd, xg, dydg), refd.dw, refd.adw, name=tag + " down dw"))
    print("%s: float64 reference %.1f s" % (tag, t_ref))
    return out


def _stem(tag, N, Cin, H, W, R, bias_on, seed):
    """stem conv straight from the fp32 NCHW input (7x7/2 pad 3 or k7/2 pad 3): forward with per-workgroup statistics
    rows (what the plans call for bf16) and the weight gradient"""
    lib = L.lib()
    x = _gen((N, Cin, H, W), seed, "grad")
    w = _gen((64, Cin, R, 7), seed + 1, "w", Cin * R * 7)
    b = _gen((64, 1), seed + 2, "grad").view(-1) if bias_on else None
    OH, OW = (H + 2 * (R // 2) - R) // 2 + 1, (W + 6 - 7) // 2 + 1
    dy = _gen((N, 64, OH, OW), seed + 3, "grad")
    t0 = time.time()
    ref = F64.conv_ref64(x, w, dy, 2, (R // 2, 3), bias=b)
    t_ref = time.time() - t0
    pk = torch.empty(lib.ecgmm_stem_packed_elems(Cin, R), device=DEV, dtype=BF)
    L.check(lib.ecgmm_stem_pack(L.BF16, ptr(w), ptr(pk), Cin, R, stream()))
    nrows = lib.ecgmm_stem_wg_stats_rows(N, Cin, H, W, R)
    st = torch.full((nrows + BN_TAIL, 2, 64), float("nan"), device=DEV)
    y = poisoned(N * OH * OW * 64, BF)
    L.check(lib.ecgmm_stem_fwd_wgrows(L.BF16, ptr(x), ptr(pk), ptr(b), ptr(y), ptr(st), N, Cin, H, W, R, stream()))
    y = unguard(y, N * OH * OW * 64, tag + " y")
    assert torch.isnan(st[nrows:]).all(), tag + ": statistics rows written beyond the reported count"
    out = [_check_fwd(tag, _nchw(y, N, OH, OW, 64), st[:nrows], ref)]
    nb = lib.ecgmm_stem_bwd_weight_workspace(N, Cin, H, W, R)
    ws = nan_workspace(nb)
    dw = torch.full(w.shape, float("nan"), device=DEV)
    L.check(lib.ecgmm_stem_bwd_weight(L.BF16, ptr(x), ptr(_nhwc(dy)), ptr(dw), 0, ptr(ws), nb, N, Cin, H, W, R, stream()))
    torch.cuda.synchronize()
    out.append(F64.check_dw(dw, ref.dw, ref.adw, name=tag + " dw"))
    print("%s: float64 reference %.1f s" % (tag, t_ref))
    return out


def _r18(N, upto=4):
    """(id, runner) of the ResNet18 geometries at batch N, layers 1..upto"""
    out = [] if upto < 4 else [("stem", lambda: _stem("r18 B%d stem 7x7/2" % N, N, 3, 224, 224, 7, False, 100))]
    out.append(("layer1", lambda: _body("r18 B%d layer1 56x56x64" % N, N, 56, 56, 64, 3, False, 110, True)))
    hw, c = 56, 64
    for li in range(2, upto + 1):
        def entry(hw=hw, c=c, li=li):
            return _entry("r18 B%d layer%d entry" % (N, li), N, hw, hw, c, 2 * c, 3, False, 100 + 20 * li, True)

        def body(hw=hw // 2, c=2 * c, li=li):
            return _body("r18 B%d layer%d %dx%dx%d" % (N, li, hw, hw, c), N, hw, hw, c, 3, False, 110 + 20 * li, True)
        out += [("layer%d_entry" % li, entry), ("layer%d" % li, body)]
        hw, c = hw // 2, 2 * c
    return out


def _r1d(N, leads):
    L1 = (5000 + 6 - 7) // 2 + 1
    L2 = (L1 + 2 - 3) // 2 + 1       # 1250 after the max-pool
    L3 = (L2 + 2 - 3) // 2 + 1       # 625
    L4 = (L3 + 2 - 3) // 2 + 1       # 313
    return [
        ("stem", lambda: _stem("r1d B%d x%d stem k7/2" % (N, leads), N, leads, 1, 5000, 1, True, 200)),
        ("block0", lambda: _body("r1d B%d block0 %dx64" % (N, L2), N, 1, L2, 64, 1, True, 210, False)),
        ("block1_entry", lambda: _entry("r1d B%d block1 entry" % N, N, 1, L2, 64, 128, 1, True, 220, False)),
        ("block1", lambda: _body("r1d B%d block1 %dx128" % (N, L3), N, 1, L3, 128, 1, True, 230, False)),
        ("block2_entry", lambda: _entry("r1d B%d block2 entry" % N, N, 1, L3, 128, 256, 1, True, 240, False)),
        ("block2", lambda: _body("r1d B%d block2 %dx256" % (N, L4), N, 1, L4, 256, 1, True, 250, False)),
    ]


LAYERS = ([("r18_b256_" + k, f) for k, f in _r18(256)] + [("r1d_b256_" + k, f) for k, f in _r1d(256, 1)] +
          [("r18_b128_" + k, f) for k, f in _r18(128, upto=2)] + [("r1d_b512x12_" + k, f) for k, f in _r1d(512, 12)])


def test_float64_reference_on_the_device_matches_the_cpu():
    """the device float64 path (torch's im2col + GEMM; MIOpen has no float64 kernels) against the CPU, one small chunk"""
    x = _gen((2, 64, 14, 14), 1, "act")
    w = _gen((128, 64, 3, 3), 2, "w", 576)
    dy = _gen((2, 128, 7, 7), 3, "grad")
    a = F64.conv_ref64(x, w, dy, 2, (1, 1))
    b = F64.conv_ref64(x.cpu(), w.cpu(), dy.cpu(), 2, (1, 1))
    for u, v in ((a.y, b.y), (a.dx, b.dx), (a.dw, b.dw), (a.ay, b.ay), (a.adx, b.adx), (a.adw, b.adw)):
        assert torch.allclose(u.cpu(), v, rtol=1e-12, atol=1e-12 * float(v.abs().max()))


@pytest.mark.parametrize("layer", [f for _, f in LAYERS], ids=[k for k, _ in LAYERS])
def test_layer_against_float64(layer):
    lib = L.lib()
    for on in (lib.ecgmm_conv_halo_enable, lib.ecgmm_conv_wgrad_ring_enable):
        on(1)                                  # the defaults bench.py runs with
    lib.ecgmm_conv_halo_cus(0)
    t0 = time.time()
    reps = layer()
    print("worst ratio %.3g, %.1f s" % (max(r.ratio for r in reps), time.time() - t0))


# ------------------------------------------------------------------------------- fused BatchNorm-backward reduction
def _bnred(g, dyg, wd, seed, sep, addg=None):
    """ecgmm_conv_bwd_data_bnred: dx (stored masked when sep) and its partial rows, checked against float64"""
    lib = L.lib()
    N, H, W, Ci = g.N, g.H, g.W, g.Cin
    ybn = _gen((N, Ci, H, W), seed, "grad")
    mask = _gen((N, Ci, H, W), seed + 1, "act") if sep else None
    gc = torch.Generator(device=DEV).manual_seed(seed + 2)
    coef = torch.stack([torch.rand(Ci, device=DEV, generator=gc) + 0.5, torch.randn(Ci, device=DEV, generator=gc) * 0.5,
                        torch.randn(Ci, device=DEV, generator=gc) * 0.3, torch.ones(Ci, device=DEV)]).contiguous()
    yg = _nhwc(ybn)
    mg = _nhwc(mask) if sep else yg
    rows = torch.full((512, 2, Ci), float("nan"), device=DEV)
    dx = poisoned(N * H * W * Ci, BF)
    n = C.c_int(0)
    want = lib.ecgmm_conv_bwd_data_bnred_rows(L.BF16, C.byref(g.d))
    L.check(lib.ecgmm_conv_bwd_data_bnred(L.BF16, C.byref(g.d), ptr(dyg), ptr(wd), ptr(addg), ptr(dx), ptr(yg), ptr(mg),
                                          ptr(coef), ptr(rows), C.byref(n), stream()))
    dx = unguard(dx, N * H * W * Ci, "bnred dx")
    assert n.value == want >= 1, (n.value, want)
    assert torch.isfinite(rows[:n.value]).all() and torch.isnan(rows[n.value:]).all()
    return _nchw(dx, N, H, W, Ci), rows[:n.value], ybn, mask, coef


def _check_bnred(tag, g, ref, add, out):
    dx, rows, ybn, mask, coef = out
    want, acc = ref.dx, ref.adx
    if add is not None:
        want, acc = want + add.double(), acc + add.double().abs()
    if mask is not None:                               # stored masked: exact zeros where the ReLU was off
        keep = mask.double() > 0
        want, acc = torch.where(keep, want, torch.zeros_like(want)), torch.where(keep, acc, torch.zeros_like(acc))
    F64.check_bf16(dx, want, acc, name=tag + " dx")
    F64.check_bnred(rows, dx, ybn, coef, mask, name=tag + " rows")


@pytest.mark.parametrize("layer", [(56, 64), (28, 128)], ids=["layer1", "layer2"])
def test_fused_batchnorm_reduction_at_full_size(layer):
    """MODE 1 (ecgmm_bn_fuse_min_pixels(0): the plans fuse every reduction the halo kernel can take): conv2's dgrad with
    bn1's reduction (mask = bn(y) > 0, unmasked store) and the next block's conv1 dgrad with bn2's (residual addend,
    separate mask, masked store), batch 256"""
    hw, c = layer
    lib = L.lib()
    g = Geo(256, hw, hw, c, c, 3, 3, 1, 1, 1)
    w = _gen((c, c, 3, 3), 300, "w", 9 * c)
    dy = _gen((256, c, hw, hw), 301, "grad")
    add = _gen((256, c, hw, hw), 302, "grad")
    # (input gradient only: the reference is the transposed conv of dy, as autograd of a forward of zeros)
    ref =F64.conv_ref64(torch.zeros(256, c, hw, hw, device=DEV), w, dy, 1, (1, 1))
    dyg, addg = _nhwc(dy), _nhwc(add)
    _, wd = _pack(w)
    with switches(lib, ECGMM_BN_FUSE_MIN_M=0):
        tag = "bnred B256 %dx%dx%d" % (hw, hw, c)
        _check_bnred(tag + " bn1", g, ref, None, _bnred(g, dyg, wd, 310, False))
        _check_bnred(tag + " bn2+addend", g, ref, add, _bnred(g, dyg, wd, 320, True, addg))


# ------------------------------------------------------------------------------------- part 2: the persistent loop
# id -> (Cin, Cout, R, op, toggles); op: fwd | fwd_bias | dgrad | dgrad_add | bnred | bnred_sep
HALO_CASES = {
    "w4_fwd": (64, 64, 3, "fwd", {"w4": 1}),
    "w4_dgrad": (64, 64, 3, "dgrad", {"w4": 1}),
    "stream_fwd": (64, 64, 3, "fwd", {}),
    "stream_dgrad": (64, 64, 3, "dgrad", {}),
    "stream_dgrad_add": (64, 64, 3, "dgrad_add", {}),
    "ncs1_fwd_bias": (64, 64, 3, "fwd_bias", {}),
    "ncs1_dgrad_add": (64, 64, 3, "dgrad_add", {"stream": 0}),
    "ncs1_bnred": (64, 64, 3, "bnred", {}),
    "pp_fwd": (128, 128, 3, "fwd", {}),
    "pp_dgrad_add": (128, 128, 3, "dgrad_add", {}),
    "pp_bnred_sep": (128, 128, 3, "bnred_sep", {}),
    "lock_fwd": (128, 128, 3, "fwd", {"pp": 0}),
    "lock_dgrad_add": (128, 128, 3, "dgrad_add", {"pp": 0}),
    "lock_bnred": (128, 128, 3, "bnred", {"pp": 0}),
    "c64_fwd": (128, 64, 3, "fwd", {}),
    "c64_dgrad_add": (64, 128, 3, "dgrad_add", {}),
    "c64_bnred": (64, 128, 3, "bnred", {}),
    "rs3_fwd_bias": (128, 128, 1, "fwd_bias", {}),
    "rs3_dgrad_add": (128, 128, 1, "dgrad_add", {}),
    "rs3_bnred_sep": (128, 128, 1, "bnred_sep", {}),
    "rs3_c64_fwd_bias": (128, 64, 1, "fwd_bias", {}),
    "rs3_c64_dgrad": (64, 128, 1, "dgrad", {}),
    "rs3_c64_bnred": (64, 128, 1, "bnred", {}),
}


@pytest.mark.parametrize("cap", [1, 7, 13])
@pytest.mark.parametrize("case", list(HALO_CASES))
def test_persistent_halo_loop(case, cap):
    """25 pixel tiles (6400 pixels: 16 images of 20x20, or 32 sequences of 200) on a launch capped to `cap` CUs: every
    workgroup walks several tiles (double-buffered halo, stream-form prefetch across tile boundaries) and the last round
    is ragged; tiles span image boundaries"""
    Cin, Cout, R, op, tog = HALO_CASES[case]
    lib = L.lib()
    N, H, W = (16, 20, 20) if R == 3 else (32, 1, 200)
    g = Geo(N, H, W, Cin, Cout, R, 3, 1, 1 if R == 3 else 0, 1)
    seed = 400 + 10 * list(HALO_CASES).index(case)
    x = _gen((N, Cin, H, W), seed, "act")
    w = _gen((Cout, Cin, R, 3), seed + 1, "w", Cin * R * 3)
    dy = _gen((N, Cout, H, W), seed + 2, "grad")
    add = _gen((N, Cin, H, W), seed + 3, "grad")
    b = _gen((Cout, 1), seed + 4, "grad").view(-1) if op == "fwd_bias" else None
    ref = F64.conv_ref64(x, w, dy, 1, (g.ph, 1), bias=b)
    wf, wd = _pack(w)
    tag = "halo %s cap %d" % (case, cap)
    with switches(lib, ECGMM_HALO_CUS=cap, ECGMM_HALO_W4=tog.get("w4", 0), ECGMM_HALO_STREAM=tog.get("stream", 1),
                  ECGMM_HALO_PP=tog.get("pp", 1)):
        if op.startswith("fwd"):
            y, rows, tail = fwd(g, _nhwc(x), wf, b, wgrows=True)
            ntn = 1 if Cout <= 64 else Cout // 128
            gk = max(1, min(cap * (2 if "w4" in tog else 1) // ntn, g.M // 256))
            assert rows.shape[0] == gk and torch.isnan(tail).all(), (rows.shape[0], gk)
            _check_fwd(tag, y, rows, ref)
        elif op.startswith("dgrad"):
            a = _nhwc(add) if op == "dgrad_add" else None
            dx = dgrad(g, _nhwc(dy), wd, a)
            if a is None:
                F64.check_bf16(dx, ref.dx, ref.adx, name=tag + " dx")
            else:
                F64.check_bf16(dx, ref.dx + add.double(), ref.adx + add.double().abs(), name=tag + " dx+addend")
        else:
            sep = op == "bnred_sep"
            a = add if sep else None
            _check_bnred(tag, g, ref, a, _bnred(g, _nhwc(dy), wd, seed + 5, sep, _nhwc(a) if sep else None))
