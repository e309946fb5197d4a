"""The conv kernels where they branch: ragged, partial-tile shapes, element by element against float64 (tests/f64check.py).

tests/test_conv_layers_f64_gpu.py holds the kernels to float64 at the benchmarked step's shapes, where every pixel count is a
multiple of 256, every channel count a multiple of 64 and every split-K divides evenly: the branch-free paths.  This module
runs the code that exists for everything else -- conv_igemm's generic epilogue (partial pixel / channel tiles, narrow and
scalar stores, partial K stages, every fp32 launch, the stride-2 parity classes with unequal or empty sizes, the folded
downsample tap, statistics rows over padding pixels), conv_halo at the limits of ecg_conv_halo_ok, conv_wgrad with short and
empty splits, and the stems at ragged widths and tiny images.  The shapes are the project's own: 250 x 2500 pictures give
W = 1250, 625, 313, 157, 79 down the image encoder, records of 2476 / 1000 / 999 samples and 12 leads go through the signal
encoder, and every epoch's last batch is short.

Every output (y, dx, dw, statistics rows, reduction rows) and every workspace is NaN before the launch; y and dx carry 64
guard elements that must still be NaN afterwards, and so must the statistics rows beyond the reported count.  bf16 goes
through check_bf16 / check_dw / check_stats / check_bnred / check_relu_bf16 with KAPPA, EPS_DW, TAU_DW and SIGMA unchanged;
fp32 through check_f32 / check_dw_f32 / check_stats_f32 (the smaller of the derived g_k(K + 2) * A and the calibrated bound).

Groups (test name prefix): a = conv_igemm stride 1 (ECGMM_CONV_HALO=0), b = stride 2 and the folded downsample,
c = conv_halo at its limits (ECGMM_CONV_HALO=2, ECGMM_BN_FUSE_MIN_M=0; then the same limits on its other instantiations and
under a CU cap), d = weight gradients, e = stems.

Measured on the MI355X (worst ratio to the bound per group and dtype; the bf16 figures are the half-ulp rounding of the
stored output):
  group  dtype  y / dx / dw worst ratio        statistics / reduction rows   accumulation seen (bound's constant)
  a      bf16   1.00 (half-ulp rounding)        0.066                         8.7e-9 of A (KAPPA 3e-7)
  a      fp32   0.21                            0.065                         2.6e-7 of A (c6_row_300 dx)
  b      bf16   1.00                            0.11                          2.4e-8 of A
  b      fp32   0.26                            0.078                         3.1e-7 of A (s2_1d_313 down dx)
  c      bf16   1.00                            0.37                          6.2e-8 of A
  d      bf16   0.045 (0.050 with one group)    --                            1.2e-7 of A, 4.3e-7 of rms (TAU_DW 1.4e-6, EPS_DW 3.4e-6)
  d      fp32   0.081                           --                            1.5e-7 of A, 6.7e-7 of rms
  e      bf16   1.00 (dw 0.14)                  0.11                          y 1.5e-8 of A; dw 1.9e-7 of A, 4.8e-7 of rms
  e      fp32   0.34                            0.080                         y 2.5e-7 of A; dw 3.6e-7 of A, 8.7e-7 of rms
The fp32 constants follow from the largest of these (tests/f64check.py): KAPPA_F32 = 1.2e-6 (3.07e-7 measured), TAU_DW_F32 =
1.4e-6 (3.55e-7), EPS_DW_F32 = 3.4e-6 (8.73e-7); torch's CPU fp32 needs less than each.  No case exceeded a bf16 constant and no
kernel defect was found; the halo kernel refuses W = 64 / 32 and the ring kernel W = 64 and W = 3 as their limits say.
ECGMM_WGRAD_GROUPS is read once at start-up and the library refuses to set it afterwards (asserted once): the one-group bf16
kernels run in one child process started with ECGMM_WGRAD_GROUPS=1, which takes every 3- and 9-tap case of group d through
the same helpers, with and without the ring kernel (the "one group" figure above).
The whole module (118 tests) runs in about 8 s, of which the child process is 3 s.

Operands are generated on the device from fixed seeds (the generators of tests/test_conv_layers_f64_gpu.py: activations
non-negative with exact zeros, gradients signed, an offset per image and per channel); for fp32 each value is then scaled
by 1 + r, r in [0, 2^-8), so that it fills the fp32 mantissa and zeros stay zeros.
"""
import ctypes as C

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from .infer_ref import check_relu_bf16
from .test_conv_layers_f64_gpu import (BN_TAIL, TDT, Geo, _bnred, _check_bnred, _gen, _nchw, _nhwc, _pack, _stem, dgrad, fwd,
                                       nan_workspace, poisoned, unguard, wgrad)
from .util import DEV, switch_get, switches

pytestmark = pytest.mark.gpu
DTS = [L.BF16, L.F32]
DT_IDS = ["bf16", "f32"]
NAME = {L.BF16: "bf16", L.F32: "f32"}


# ------------------------------------------------------------------------------------------------ operands and checks
def _op(shape, seed, kind, dt, fan_in=1):
    t = _gen(shape, seed, kind, fan_in)
    if dt == L.F32:      # fill the fp32 mantissa; zeros stay zeros
        g = torch.Generator(device=DEV).manual_seed(seed + 7919)
        t = t * (1 + torch.rand(shape, device=DEV, generator=g) / 256)
    return t


def _bias(c, seed, dt):
    return _op((c, 1), seed, "grad", dt).view(-1).contiguous()


def _chk(dt, out, ref, A, K, tag, relu=False):
    """y / dx against float64: K = the number of summands (fp32's derived bound)"""
    if dt == L.BF16:
        return (check_relu_bf16 if relu else F64.check_bf16)(out, ref, A, name=tag)
    if relu:
        assert bool((out >= 0).all()), tag + ": negative value after ReLU"
        ref = ref.clamp_min(0)
    return F64.check_f32(out, ref, A, K, name=tag)


def _chk_fwd(dt, tag, y, rows, tail, ref, K):
    assert torch.isnan(tail).all(), tag + ": statistics rows written beyond the reported count"
    _chk(dt, y, ref.y, ref.ay, K, tag + " y")
    if dt == L.BF16:
        F64.check_stats(rows, ref, name=tag + " stats")
    else:
        F64.check_stats_f32(rows, ref, K, name=tag + " stats")


def _chk_dw(dt, dw, ref, A, M, tag):
    if dt == L.BF16:
        return F64.check_dw(dw, ref, A, name=tag)
    return F64.check_dw_f32(dw, ref, A, M, name=tag)


def _fused(dt, g, x, wf, bias, addend, act):
    n = g.M * g.Cout
    y = poisoned(n, TDT[dt])
    L.check(L.lib().ecgmm_conv_fwd_fused(dt, C.byref(g.d), ptr(x), ptr(wf), ptr(bias), ptr(addend), ptr(y), act, stream()),
            "conv_fwd_fused")
    return _nchw(unguard(y, n, "fused y"), g.N, g.OH, g.OW, g.Cout)


def _with_down(dt, g, dy, wd, dyd, wdd):
    """ecgmm_conv_bwd_data_with_downsample without the temporary, as tests/test_ops_gpu.py calls it"""
    n = g.N * g.H * g.W * g.Cin
    dx = poisoned(n, TDT[dt])
    L.check(L.lib().ecgmm_conv_bwd_data_with_downsample(dt, C.byref(g.d), ptr(dy), ptr(wd), ptr(dyd), ptr(wdd), ptr(dx), None,
                                                        stream()))
    return _nchw(unguard(dx, n, "dx (both branches)"), g.N, g.H, g.W, g.Cin)


# ------------------------------------------------------------------------------------------------ a: conv_igemm, stride 1
# id -> (N, H, W, Cin, Cout, R, S, forward only, fused forms too).  igemm tiles: 128 pixels x 64 / 128 channels; a K stage is
# 64 bf16 / 32 fp32 reduction channels; the wide (16-byte, lane-swapped) bf16 store needs Cd % 32 == 0, the 8 / 16-byte store
# Cd % 4 == 0, anything else goes out channel by channel.
A_CASES = {
    # one pixel; Cs = 8 is one partial K stage in both dtypes; Cd = 8: narrow store, partial channel tile
    "c1_one_pixel": (1, 1, 1, 8, 8, 1, 1, False, False),
    # 297 pixels = two tiles + 41: partial last tile, tiles span images (99 pixels each), statistics rows over padding pixels
    "c2_297_pixels": (3, 9, 11, 64, 64, 3, 3, False, True),
    # forward: Cs = 96 = a whole + a partial bf16 stage, Cd = 40: no wide store, partial channel tile;
    # dgrad: Cs = 40 (partial stage in both dtypes), Cd = 96: wide store with a partial 128-channel tile
    "c3_96_to_40": (2, 7, 5, 96, 40, 3, 3, False, True),
    # Cd = 37: scalar stores (the guard elements sit right behind the last one); dgrad would have Cs = 37: refused, forward only.
    # (Its fused form is a neighbour: the addend's channel-by-channel loads, which Cd = 40 never reaches.)
    "c4_cd37_scalar": (2, 5, 6, 64, 37, 3, 3, True, True),
    # 1x3: one tile + 2 pixels; two 128-channel tiles forward, Cs = 256 in the dgrad
    "c5_1x3_130": (1, 1, 130, 128, 256, 1, 3, False, False),
    # a tile that lies inside one image row (W = 300 > 128): no row or image boundary within the tile
    "c6_row_300": (2, 3, 300, 64, 64, 3, 3, False, False),
    # 1x1: 50 pixels, one tap
    "c7_1x1_50": (2, 5, 5, 64, 128, 1, 1, False, False),
    # 1x1 on one-pixel images (Linear-shaped): 7 pixels, Cs = 96 / 40
    "c7_1x1_linear": (7, 1, 1, 96, 40, 1, 1, False, False),
}


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("case", list(A_CASES))
def test_a_igemm_stride1(case, dt):
    N, H, W, Cin, Cout, R, S, fwd_only, fused = A_CASES[case]
    ph, pw = R // 2, S // 2
    g = Geo(N, H, W, Cin, Cout, R, S, 1, ph, pw)
    seed = 1000 + 10 * list(A_CASES).index(case)
    x = _op((N, Cin, H, W), seed, "act", dt)
    w = _op((Cout, Cin, R, S), seed + 1, "w", dt, Cin * R * S)
    dy = None if fwd_only else _op((N, Cout, H, W), seed + 2, "grad", dt)
    b = _bias(Cout, seed + 4, dt)
    ref = F64.conv_ref64(x, w, dy, 1, (ph, pw), bias=b)
    xg = _nhwc(x, dt)
    wf, wd = _pack(w, dt)
    tag = "a %s %s" % (NAME[dt], case)
    Kf, Kd = Cin * R * S, Cout * R * S
    with switches(L.lib(), ECGMM_CONV_HALO=0):
        y, rows, tail = fwd(g, xg, wf, b, wgrows=False, dt=dt)
        assert rows.shape[0] == 2 * -(-g.M // 128)
        _chk_fwd(dt, tag, y, rows, tail, ref, Kf)
        if fused:
            add = _op((N, Cout, H, W), seed + 5, "grad", dt)
            ry, ay = ref.y + add.double(), ref.ay + add.double().abs()
            _chk(dt, _fused(dt, g, xg, wf, b, _nhwc(add, dt), 1), ry, ay, Kf, tag + " fused bias_addend_relu", relu=True)
            _chk(dt, _fused(dt, g, xg, wf, b, None, 0), ref.y, ref.ay, Kf, tag + " fused bias_only")
        if not fwd_only:
            add = _op((N, Cin, H, W), seed + 3, "grad", dt)
            dyg = _nhwc(dy, dt)
            _chk(dt, dgrad(g, dyg, wd, dt=dt), ref.dx, ref.adx, Kd, tag + " dx")
            _chk(dt, dgrad(g, dyg, wd, _nhwc(add, dt), dt=dt), ref.dx + add.double(), ref.adx + add.double().abs(), Kd,
                 tag + " dx+addend")


def test_a_igemm_refuses_channels_off_the_16_byte_vector():
    """the dgrad of case 4 (Cs = 37) and a wgrad with 37 channels: refused with a message, nothing written.  Every buffer has
    the geometry's real size, so a refusal that went missing would end in a failed assertion, not in a stray access."""
    lib = L.lib()
    g = Geo(2, 5, 6, 64, 37, 3, 3, 1, 1, 1)
    for dt, vec in ((L.BF16, 8), (L.F32, 4)):
        dy = torch.zeros(g.M * g.Cout, device=DEV, dtype=TDT[dt])
        x = torch.zeros(g.M * g.Cin, device=DEV, dtype=TDT[dt])
        wd = torch.zeros(g.Cout * g.Cin * 9, device=DEV, dtype=TDT[dt])
        dx = poisoned(g.M * g.Cin, TDT[dt])
        dw = poisoned(g.Cout * g.Cin * 9, torch.float32)
        nb = lib.ecgmm_conv_bwd_weight_workspace(dt, C.byref(g.d))
        ws = nan_workspace(nb)
        assert lib.ecgmm_conv_bwd_data(dt, C.byref(g.d), ptr(dy), ptr(wd), None, ptr(dx), stream()) == 1
        msg = lib.ecgmm_last_error().decode()
        assert "reduction channels 37" in msg and "multiple of %d" % vec in msg, msg
        assert lib.ecgmm_conv_bwd_weight(dt, C.byref(g.d), ptr(x), ptr(dy), ptr(dw), 0, ptr(ws), nb, stream()) == 1
        assert "multiples of %d" % vec in lib.ecgmm_last_error().decode()
        torch.cuda.synchronize()
        assert torch.isnan(dx.float()).all() and torch.isnan(dw).all() and torch.isnan(ws).all()


# ------------------------------------------------------------------------------------------------ b: stride 2
# id -> (N, H, W, Cin, Cout, R).  The stride-2 input gradient runs as four parity classes (row parity, column parity) of
# ceil / floor halves of H and W; grid.x is sized for the largest class, the others end early or are empty.
B_CASES = {
    "s2_15x13": (3, 15, 13, 64, 128, 3),        # classes of 8x7, 8x6, 7x7 and 7x6 pixels
    "s2_6x8": (2, 6, 8, 64, 128, 3),            # even sizes: four equal classes of 3x4
    "s2_2x2": (2, 2, 2, 64, 64, 3),             # one pixel per class and image
    "s2_1x1": (2, 1, 1, 64, 128, 3),            # three empty classes: Mc = 0 and the magic divisor of 0
    "s2_1d_313": (5, 1, 313, 128, 256, 1),      # 1-D: classes of 157 and 156 columns, the odd-row classes empty
    "s2_1d_2": (3, 1, 2, 64, 128, 1),           # 1-D: one column per class
}


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("case", list(B_CASES))
def test_b_stride2_and_downsample(case, dt):
    N, H, W, Cin, Cout, R = B_CASES[case]
    ph = R // 2
    g = Geo(N, H, W, Cin, Cout, R, 3, 2, ph, 1)
    gd = Geo(N, H, W, Cin, Cout, 1, 1, 2, 0, 0)
    assert (g.OH, g.OW) == (gd.OH, gd.OW)
    seed = 2000 + 10 * list(B_CASES).index(case)
    x = _op((N, Cin, H, W), seed, "act", dt)
    w = _op((Cout, Cin, R, 3), seed + 1, "w", dt, Cin * R * 3)
    wdn = _op((Cout, Cin, 1, 1), seed + 2, "w", dt, Cin)
    dy = _op((N, Cout, g.OH, g.OW), seed + 3, "grad", dt)
    dyd = _op((N, Cout, g.OH, g.OW), seed + 4, "grad", dt)
    b, bd = _bias(Cout, seed + 5, dt), _bias(Cout, seed + 6, dt)
    ref = F64.conv_ref64(x, w, dy, 2, (ph, 1), bias=b)
    refd = F64.conv_ref64(x, wdn, dyd, 2, (0, 0), bias=bd)
    xg, dyg, dydg = _nhwc(x, dt), _nhwc(dy, dt), _nhwc(dyd, dt)
    wf, wd = _pack(w, dt)
    wdf, wdd = _pack(wdn, dt)
    tag = "b %s %s" % (NAME[dt], case)
    Kf, Kd = Cin * R * 3, Cout * R * 3
    y, rows, tail = fwd(g, xg, wf, b, wgrows=False, dt=dt)
    _chk_fwd(dt, tag + " conv", y, rows, tail, ref, Kf)
    y, rows, tail = fwd(gd, xg, wdf, bd, wgrows=False, dt=dt)
    _chk_fwd(dt, tag + " down", y, rows, tail, refd, Cin)
    _chk(dt, dgrad(g, dyg, wd, dt=dt), ref.dx, ref.adx, Kd, tag + " conv dx")
    _chk(dt, dgrad(gd, dydg, wdd, dt=dt), refd.dx, refd.adx, Cout, tag + " down dx")
    _chk(dt, _with_down(dt, g, dyg, wd, dydg, wdd), ref.dx + refd.dx, ref.adx + refd.adx, Kd + Cout, tag + " dx (both branches)")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_b_1x1_stride2_alone_leaves_exact_zeros(dt):
    """(2, 9, 9, 128, 256), 1x1 / stride 2: three of the four parity classes have no tap at all -- every pixel with an odd row
    or column gets exactly 0 (A == 0 there, so both checkers demand it; asserted on its own as well)"""
    N, H, W, Cin, Cout = 2, 9, 9, 128, 256
    g = Geo(N, H, W, Cin, Cout, 1, 1, 2, 0, 0)
    x = _op((N, Cin, H, W), 2100, "act", dt)
    w = _op((Cout, Cin, 1, 1), 2101, "w", dt, Cin)
    dy = _op((N, Cout, g.OH, g.OW), 2102, "grad", dt)
    b = _bias(Cout, 2103, dt)
    ref = F64.conv_ref64(x, w, dy, 2, (0, 0), bias=b)
    wf, wd = _pack(w, dt)
    tag = "b %s 1x1s2_9x9" % NAME[dt]
    y, rows, tail = fwd(g, _nhwc(x, dt), wf, b, wgrows=False, dt=dt)
    _chk_fwd(dt, tag, y, rows, tail, ref, Cin)
    dx = dgrad(g, _nhwc(dy, dt), wd, dt=dt)
    _chk(dt, dx, ref.dx, ref.adx, Cout, tag + " dx")
    assert (dx[:, :, 1::2] == 0).all() and (dx[:, :, :, 1::2] == 0).all()
    assert (ref.adx[:, :, ::2, ::2] > 0).all()


# ------------------------------------------------------------------------------------------------ c: conv_halo at its limits
def _halo_serves(g, mode):
    """ecg_conv_halo_ok at ECGMM_CONV_HALO=2, restated: whole 256-pixel tiles, channels in 64s (128s above 64), and the tile's
    256 + 2 (pad_h W + 1) halo rows within HCAP = 384 (64-channel tiles) / 320 (128-channel tiles)"""
    Cs, Cd = (g.Cin, g.Cout) if mode == 0 else (g.Cout, g.Cin)
    if g.M % 256 or Cs % 64 or Cd % 64 or (Cd > 64 and Cd % 128):
        return False
    return 256 + 2 * (g.ph * g.W + 1) <= (320 if Cd > 64 else 384)


PAIRS = [(64, 64), (128, 128), (128, 64), (64, 128)]
# id -> (N, H, W, R, channel pairs).  M is a multiple of 256 everywhere (the halo kernel takes nothing else).
C_CASES = {
    # W = 63: 256 + 2 * 64 = 384 rows, the last width HCAP = 384 admits (64-channel tiles); 128 -> 64: the forward is served
    # (two K slices), its dgrad has 128-channel tiles (384 > 320) and must fall to igemm
    "w63": (4, 64, 63, 3, [(64, 64), (128, 64)]),
    # W = 31: 256 + 2 * 32 = 320 rows, the last for HCAP = 320 (128-channel tiles)
    "w31": (8, 32, 31, 3, PAIRS),
    # one past either limit: the halo kernel must refuse, the answer (from igemm) is held to the same bound
    "w64_refused": (4, 64, 64, 3, [(64, 64)]),
    "w32_refused": (8, 32, 32, 3, [(128, 128)]),
    # 256 one-pixel images in one tile: every tap but the centre is padding, an image boundary after every pixel
    "one_pixel_images": (256, 1, 1, 3, PAIRS),
    "2x2_images": (64, 2, 2, 3, PAIRS),
    # 15 tiles over 256 images of 15 pixels: every image but the multiples of 256 / 15 straddles a tile boundary
    "3x5_images": (256, 3, 5, 3, PAIRS),
    # 1x3
    "1x3_two_rows": (2, 1, 128, 1, PAIRS),
    "1x3_w3": (256, 1, 3, 1, PAIRS),
}
C_IDS = ["%s-%dto%d" % (k, ci, co) for k, v in C_CASES.items() for ci, co in v[4]]
C_PARAMS = [(k, ci, co) for k, v in C_CASES.items() for ci, co in v[4]]


def _bnred_unserved(g, dyg, wd, addg):
    """ecgmm_conv_bwd_data_bnred on a geometry the halo kernel refuses: *nrows = 0, no row written, dx the plain gradient"""
    lib = L.lib()
    n = g.N * g.H * g.W * g.Cin
    yg = _nhwc(_gen((g.N, g.Cin, g.H, g.W), 77, "grad"))
    coef = torch.ones(4, g.Cin, device=DEV)
    rows = torch.full((512, 2, g.Cin), float("nan"), device=DEV)
    dx = poisoned(n, TDT[L.BF16])
    nr = C.c_int(-1)
    assert lib.ecgmm_conv_bwd_data_bnred_rows(L.BF16, C.byref(g.d)) == 0
    L.check(lib.ecgmm_conv_bwd_data_bnred(L.BF16, C.byref(g.d), ptr(dyg), ptr(wd), ptr(addg), ptr(dx), ptr(yg), ptr(yg),
                                          ptr(coef), ptr(rows), C.byref(nr), stream()))
    dx = unguard(dx, n, "bnred dx")
    assert nr.value == 0 and torch.isnan(rows).all()
    return _nchw(dx, g.N, g.H, g.W, g.Cin)


# Neighbours of the cases above (the only legs of group c that move a switch besides the two the group sets): ecg_conv_halo
# dispatches other instantiations of conv_halo_kernel for the same shapes, each with its own halo-fill schedule, and at
# W = 63 / 31 every 8-row DMA piece of the HCAP rows is in use; and with the default of one workgroup per CU none of the
# shapes above makes a workgroup walk more than one tile.  id -> (case, Cin, Cout, switches): the branch it reaches
C_VARIANTS = {
    # <64, 9, 0 / 2 / 1, NCS1>: one tile at a time with the next tile's halo prefetched into the second buffer during the K
    # loop (the default sends 64 -> 64 without bias or addend to the stream form <.., ST>)
    "w63_tile_at_a_time": ("w63", 64, 64, dict(ECGMM_HALO_STREAM=0)),
    # <64, 9, 0 / 2, false, 4>: four waves, ONE halo buffer, NPW_MAX = 12 fill pieces per wave instead of 6, 3-slot weight ring
    "w63_four_waves": ("w63", 64, 64, dict(ECGMM_HALO_W4=1)),
    "one_pixel_images_four_waves": ("one_pixel_images", 64, 64, dict(ECGMM_HALO_W4=1)),
    # <64, 9, 0> with two K slices: 63 tiles over 5 workgroups -- the persistent loop's double-buffered halo at all 384 rows,
    # a ragged last round (63 % 5 = 3)
    "w63_two_slices_5cus": ("w63", 128, 64, dict(ECGMM_HALO_CUS=5)),
    # <128, 9, 0 / 2 / 1>: the lock-step K loop of the 128-channel tiles (the default is the ping-pong form <.., PP>), at all
    # 320 rows, with two K slices and with one
    "w31_lock_step": ("w31", 128, 128, dict(ECGMM_HALO_PP=0)),
    "w31_lock_step_64to128": ("w31", 64, 128, dict(ECGMM_HALO_PP=0)),
    # the persistent loop over tiles every one of which straddles images: 15 tiles over 3 workgroups (stream form: the K loop
    # runs on across tile boundaries), over 4 (ping-pong form, ragged last round), and 3 tiles of 1x3 over 2
    "3x5_images_3cus": ("3x5_images", 64, 64, dict(ECGMM_HALO_CUS=3)),
    "3x5_images_4cus_128": ("3x5_images", 128, 128, dict(ECGMM_HALO_CUS=4)),
    "1x3_w3_2cus": ("1x3_w3", 128, 128, dict(ECGMM_HALO_CUS=2)),
}


@pytest.mark.parametrize("variant", list(C_VARIANTS))
def test_c_halo_limit_variants(variant):
    case, Cin, Cout, sw = C_VARIANTS[variant]
    _halo_case(case, Cin, Cout, 3900 + 10 * list(C_VARIANTS).index(variant), sw, " " + variant)


@pytest.mark.parametrize("case,Cin,Cout", C_PARAMS, ids=C_IDS)
def test_c_halo_limits(case, Cin, Cout):
    _halo_case(case, Cin, Cout, 3000 + 10 * C_PARAMS.index((case, Cin, Cout)), {}, "")


def _halo_case(case, Cin, Cout, seed, extra, suffix):
    N, H, W, R, _ = C_CASES[case]
    lib = L.lib()
    ph = R // 2
    g = Geo(N, H, W, Cin, Cout, R, 3, 1, ph, 1)
    x = _gen((N, Cin, H, W), seed, "act")
    w = _gen((Cout, Cin, R, 3), seed + 1, "w", Cin * R * 3)
    dy = _gen((N, Cout, H, W), seed + 2, "grad")
    add = _gen((N, Cin, H, W), seed + 3, "grad")
    b = _gen((Cout, 1), seed + 4, "grad").view(-1) if R == 1 else None     # (Conv1d bias, as the signal encoder)
    ref = F64.conv_ref64(x, w, dy, 1, (ph, 1), bias=b)
    wf, wd = _pack(w)
    dyg, addg = _nhwc(dy), _nhwc(add)
    tag = "c bf16 %s %d->%d%s" % (case, Cin, Cout, suffix)
    with switches(lib, ECGMM_CONV_HALO=2, ECGMM_BN_FUSE_MIN_M=0, **extra):
        y, rows, tail = fwd(g, _nhwc(x), wf, b, wgrows=True)
        # one row per workgroup (at most M / 256 of them) from the halo kernel, 2 per 128 pixels from igemm
        igemm_rows = lib.ecgmm_conv_stats_rows(g.M)
        assert (rows.shape[0] != igemm_rows) == _halo_serves(g, 0), (rows.shape[0], igemm_rows)
        _chk_fwd(L.BF16, tag, y, rows, tail, ref, 0)
        served = _halo_serves(g, 1)
        assert (lib.ecgmm_conv_bwd_data_bnred_rows(L.BF16, C.byref(g.d)) > 0) == served
        F64.check_bf16(dgrad(g, dyg, wd), ref.dx, ref.adx, name=tag + " dx")
        radd, aadd = ref.dx + add.double(), ref.adx + add.double().abs()
        F64.check_bf16(dgrad(g, dyg, wd, addg), radd, aadd, name=tag + " dx+addend")
        if served:
            _check_bnred(tag + " bnred", g, ref, None, _bnred(g, dyg, wd, seed + 5, False))
            _check_bnred(tag + " bnred sep+addend", g, ref, add, _bnred(g, dyg, wd, seed + 6, True, addg))
        else:
            F64.check_bf16(_bnred_unserved(g, dyg, wd, None), ref.dx, ref.adx, name=tag + " bnred (unserved) dx")
            F64.check_bf16(_bnred_unserved(g, dyg, wd, addg), radd, aadd, name=tag + " bnred (unserved) dx+addend")


def test_c_halo_limit_table():
    """the cases above sit where they claim to: the last admitted width, the first refused one"""
    for (n, h, w, ci, co), want in (((4, 64, 63, 64, 64), True), ((4, 64, 64, 64, 64), False), ((8, 32, 31, 128, 128), True),
                                    ((8, 32, 32, 128, 128), False), ((4, 64, 63, 128, 64), True)):
        g = Geo(n, h, w, ci, co, 3, 3, 1, 1, 1)
        assert _halo_serves(g, 0) is want
    assert not _halo_serves(Geo(4, 64, 63, 128, 64, 3, 3, 1, 1, 1), 1)


# ------------------------------------------------------------------------------------------------ d: weight gradients
# id -> (N, H, W, Cin, Cout, R, S, stride).  pick_nsplit (csrc/conv_wgrad.hip): steps = ceil(M / kp), kp = 32 bf16 / 16 fp32
# pixels; tiles = ceil(Cout / 64) * ceil(Cin / 64); ns = min(steps, ceil(512 / groups / tiles), 512), groups = 2 for bf16 filters
# of 3 or 9 taps (1 with ECGMM_WGRAD_GROUPS=1, for 1x1 filters and for fp32); steps_per_split = ceil(steps / ns); split i takes
# steps [i * sps, (i + 1) * sps) cut at `steps`, so trailing splits are short or empty -- and must still write zeros to
# their slab, which the reduce kernel sums.  The workspace is sized for groups = 1.
# A process started with ECGMM_WGRAD_WGS=6 (leg halo_generic_wgs6 of tests/startup_legs.py) has 6 slots in place of the 512:
# ns = min(steps, ceil(6 / groups / tiles)), geometries the default never produces.  bf16 with one channel tile: ns = 3, several
# steps per split (empty_splits 3 x 100, partial_last_step 4 + 4 + 2, 15_steps 3 x 5, ring_w63 3 x 42, ring_w64_refused 43 + 43 +
# 42; w3_ring_refused has one step: ns = 1).  fp32 with one channel tile: ns = 6 (600 / 30 / 252 steps in splits of 100 / 5 / 42;
# partial_last_step 19 steps as 4 x 4 + 3 and one EMPTY split; ring_w64_refused 256 as 5 x 43 + 41; w3_ring_refused 2 steps, ns = 2).  Two tiles (partial_channel_tiles, stride2): bf16
# ns = 2 (2 + 1 and 3 + 3 steps), fp32 ns = 3 (2 + 2 + 1 and 4 + 4 + 3).  odd_steps_two_groups (16 tiles) and 1x1_stride2, 1x3_130
# (8 tiles each): ns = 1, a single split over 48, 2 and 13 steps (fp32: 96, 4 and 25) -- the slab is the result.
D_CASES = {
    # M = 9600.  bf16: 300 steps, ns = 256, sps = 2: 150 splits of 2 steps (one per group), 106 EMPTY.  groups = 1: ns = 300.
    # fp32: 600 steps, ns = 512, sps = 2: 300 used, 212 empty
    "empty_splits": (6, 40, 40, 64, 64, 3, 3, 1),
    # M = 297.  bf16: 10 steps (the last holds 9 pixels), ns = 10, sps = 1: group 1 of every workgroup has nothing.
    # fp32: 19 steps (the last holds 9), ns = 19
    "partial_last_step": (3, 9, 11, 64, 64, 3, 3, 1),
    # M = 480.  bf16: 15 steps, ns = 15, sps = 1.  fp32: 30 steps, ns = 30
    "15_steps": (5, 8, 12, 64, 64, 3, 3, 1),
    # (a neighbour: none of the listed cases gives a split an odd step count above 1)  M = 1530, tiles = 16.  bf16: 48 steps (the
    # last holds 26 pixels), ns = 16, sps = 3: group 0 takes 2 steps, group 1 takes 1.  groups = 1: ns = 32, sps = 2, 24 used, 8
    # empty.  fp32: 96 steps, ns = 32, sps = 3
    "odd_steps_two_groups": (3, 17, 30, 256, 256, 3, 3, 1),
    # M = 70, tiles = 1 x 2 (Cin = 64 + 32, Cout = 40): partial channel tiles on both sides.  bf16: 3 steps (6 pixels in the
    # last), ns = 3.  fp32: 5 steps, ns = 5
    "partial_channel_tiles": (2, 7, 5, 96, 40, 3, 3, 1),
    # stride 2: M = 3 * 8 * 7 = 168, tiles = 2.  bf16: 6 steps (8 pixels in the last), ns = 6.  fp32: 11 steps, ns = 11
    "stride2": (3, 15, 13, 64, 128, 3, 3, 2),
    # 1x1 stride 2 (one tap: one wave group in every dtype): M = 50, tiles = 8.  bf16: 2 steps, ns = 2.  fp32: 4 steps, ns = 4
    "1x1_stride2": (2, 9, 9, 128, 256, 1, 1, 2),
    # the ring kernel's limit HL + HLa + 128 <= 256 with HL = W + 1, HLa = HL rounded up to 8: W = 63 gives 64 + 64 + 128
    # (admitted), W = 64 gives 65 + 72 + 128 (refused: wgrad_kernel).  M = 4032 / 4096: 126 / 128 steps, ns = steps, sps = 1
    "ring_w63": (4, 16, 63, 64, 64, 3, 3, 1),
    "ring_w64_refused": (4, 16, 64, 64, 64, 3, 3, 1),
    # W < 4: the ring refuses.  M = 30: one partial step, ns = 1
    "w3_ring_refused": (2, 5, 3, 64, 64, 3, 3, 1),
    # 1x3, 128 -> 256 (the ring takes it at its default level): M = 390, tiles = 8.  bf16: 13 steps (6 pixels in the last),
    # ns = 13.  fp32: 25 steps, ns = 25
    "1x3_130": (3, 1, 130, 128, 256, 1, 3, 1),
}
D_MODES = [(L.BF16, "default"), (L.BF16, "ring0"), (L.F32, "default")]


def _wgrad_case(case, dt, mode, sw):
    N, H, W, Cin, Cout, R, S, st = D_CASES[case]
    ph, pw = R // 2, S // 2
    g = Geo(N, H, W, Cin, Cout, R, S, st, ph, pw)
    seed = 4000 + 10 * list(D_CASES).index(case)
    x = _op((N, Cin, H, W), seed, "act", dt)
    dy = _op((N, Cout, g.OH, g.OW), seed + 1, "grad", dt)
    ref = F64.conv_ref64(x, torch.zeros(Cout, Cin, R, S, device=DEV), dy, st, (ph, pw))
    tag = "d %s %s %s" % (NAME[dt], case, mode)
    with switches(L.lib(), **sw):
        dw = wgrad(g, _nhwc(x, dt), _nhwc(dy, dt), dt=dt)
        _chk_dw(dt, dw, ref.dw, ref.adw, g.M, tag + " dw")
        if case == "partial_last_step":       # accumulate = 1 onto a known tensor, NaN slab again
            prior = _op((Cout, Cin, R, S), seed + 2, "grad", dt)
            dw = wgrad(g, _nhwc(x, dt), _nhwc(dy, dt), dt=dt, accumulate=1, dw=prior.clone())
            _chk_dw(dt, dw, ref.dw + prior.double(), ref.adw + prior.double().abs(), g.M, tag + " dw accumulated")


@pytest.mark.parametrize("dt,mode", D_MODES, ids=["bf16", "bf16_ring0", "f32"])
@pytest.mark.parametrize("case", list(D_CASES))
def test_d_weight_gradient(case, dt, mode):
    _wgrad_case(case, dt, mode, dict(ECGMM_WGRAD_RING=0) if mode == "ring0" else {})


def test_d_one_group_switch_is_refused_after_start_up():
    """ECGMM_WGRAD_GROUPS is read once at start-up: setting it afterwards is refused with a message and changes nothing"""
    lib = L.lib()
    before = switch_get(lib, "ECGMM_WGRAD_GROUPS")
    with pytest.raises(RuntimeError, match="ECGMM_WGRAD_GROUPS is read once at start-up"):
        with switches(lib, ECGMM_WGRAD_GROUPS=1 - before):
            pass
    assert switch_get(lib, "ECGMM_WGRAD_GROUPS") == before


def _one_group_main():
    """`python -m tests.test_conv_edges_f64_gpu` under ECGMM_WGRAD_GROUPS=1: every bf16 case of D_CASES with 3 or 9 taps through
    the same wgrad / check_dw helpers, on wgrad_ring_kernel<NT, 1> where the ring serves the shape and on wgrad_kernel<bf16, NT, 1>
    (ECGMM_WGRAD_RING=0).  One 256-thread group per workgroup doubles the split count: M = 9600 gives ns = 300 of one step,
    the 256 -> 256 case ns = 32, sps = 2 with 8 empty splits.  Any failed check ends the process with a traceback."""
    assert switch_get(L.lib(), "ECGMM_WGRAD_GROUPS") == 1
    n = 0
    for case, geo in D_CASES.items():
        if geo[5] * geo[6] == 1:
            continue                          # one tap: one group whatever the switch says
        _wgrad_case(case, L.BF16, "groups1", {})
        _wgrad_case(case, L.BF16, "groups1 ring0", dict(ECGMM_WGRAD_RING=0))
        n += 2
    print("one-group weight gradients ok: %d legs" % n)


def test_d_weight_gradient_one_group_in_a_fresh_process():
    """the one-group bf16 kernels are reachable from the environment only: one child process started with
    ECGMM_WGRAD_GROUPS=1 runs _one_group_main; a failed check or a fault there is a non-zero exit status here"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_conv_edges_f64_gpu"], cwd=root, capture_output=True, text=True,
                       env=dict(os.environ, ECGMM_WGRAD_GROUPS="1"), timeout=120)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "one-group weight gradients ok: 20 legs" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ e: stems
# (N, Cin, H, W, R): output tiles are 8 x 16 pixels (R = 7) / 1 x 128 (R = 1), a workgroup walks the images of one tile position
E_CASES = [
    (1, 3, 10, 2500, 7),     # golden g6's picture height after the crop, full width: OH = 5 of a tile's 8 rows, OW = 1250 = 78 tiles + 2
    (1, 3, 50, 83, 7),       # OH = 25, OW = 42: partial tiles in both directions
    (2, 3, 7, 9, 7),         # smaller than the filter's reach: OH = 4, OW = 5
    (2, 3, 1, 1, 7),         # one pixel in, one pixel out: every tap but the centre is padding
    (2, 12, 1, 333, 1),      # 12 leads, odd length: OW = 167 = one tile + 39
    (3, 1, 1, 999, 1),       # one lead, 999 samples: OW = 500 = three tiles + 116
    (1, 1, 1, 7, 1),         # OW = 4
]
E_IDS = ["%dx%dx%dx%d" % c[:4] for c in E_CASES]


@pytest.mark.parametrize("case", E_CASES, ids=E_IDS)
def test_e_stem_bf16(case):
    """ecgmm_stem_fwd_wgrows (per-workgroup statistics rows) and ecgmm_stem_bwd_weight (NaN workspace), bf16"""
    N, Cin, H, W, R = case
    _stem("e bf16 stem %dx%dx%dx%d" % (N, Cin, H, W), N, Cin, H, W, R, R == 1, 5000 + 10 * E_CASES.index(case))


@pytest.mark.parametrize("case", E_CASES, ids=E_IDS)
def test_e_stem_f32(case):
    """ecgmm_stem_fwd (four statistics rows per tile) and ecgmm_stem_bwd_weight (NaN workspace), fp32"""
    N, Cin, H, W, R = case
    lib = L.lib()
    seed = 5100 + 10 * E_CASES.index(case)
    tag = "e f32 stem %dx%dx%dx%d" % (N, Cin, H, W)
    x = _op((N, Cin, H, W), seed, "grad", L.F32)
    w = _op((64, Cin, R, 7), seed + 1, "w", L.F32, Cin * R * 7)
    b = _bias(64, seed + 2, L.F32) if R == 1 else None
    OH, OW = (H + 2 * (R // 2) - R) // 2 + 1, (W + 6 - 7) // 2 + 1
    dy = _op((N, 64, OH, OW), seed + 3, "grad", L.F32)
    ref = F64.conv_ref64(x, w, dy, 2, (R // 2, 3), bias=b)
    pk = torch.empty(lib.ecgmm_stem_packed_elems(Cin, R), device=DEV)
    L.check(lib.ecgmm_stem_pack(L.F32, ptr(w), ptr(pk), Cin, R, stream()))
    nrows = lib.ecgmm_stem_stats_rows(N, Cin, H, W, R)
    st = torch.full((nrows + BN_TAIL, 2, 64), float("nan"), device=DEV)
    n = N * OH * OW * 64
    y = poisoned(n, torch.float32)
    L.check(lib.ecgmm_stem_fwd(L.F32, ptr(x), ptr(pk), ptr(b), ptr(y), ptr(st), N, Cin, H, W, R, stream()))
    y = _nchw(unguard(y, n, tag + " y"), N, OH, OW, 64)
    _chk_fwd(L.F32, tag, y, st[:nrows], st[nrows:], ref, Cin * R * 7)
    nb = lib.ecgmm_stem_bwd_weight_workspace(N, Cin, H, W, R)
    ws, dyg = nan_workspace(nb), _nhwc(dy, L.F32)
    dw = torch.full(w.shape, float("nan"), device=DEV)
    L.check(lib.ecgmm_stem_bwd_weight(L.F32, ptr(x), ptr(dyg), ptr(dw), 0, ptr(ws), nb, N, Cin, H, W, R, stream()))
    torch.cuda.synchronize()
    F64.check_dw_f32(dw, ref.dw, ref.adw, N * OH * OW, name=tag + " dw")


if __name__ == "__main__":
    _one_group_main()
