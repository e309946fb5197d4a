"""Per-op checks of the CRNN saliency kernels on the GPU, both compute dtypes, every output a tests/exact_abi.Guarded buffer
(NaN-prefilled between sentinel zones) and every workspace NaN-filled.

ecgmm_conv5_in1_bwd_data (csrc/crnn_front.hip) against tests/f64check.conv_ref64 of the operands as the kernel rounds them:
F64.check_f32(dx, ref.dx, ref.adx, K = 800) in both dtypes -- the output is fp32 and bf16 x bf16 products are exact in fp32,
so only the 32 x 25 = 800-term fp32 accumulation separates kernel and reference; f64check's constants as they are.  Shapes:
test_crnn_ops_gpu.py's IN1_CASES, one pixel, an image smaller than the filter, and one derived from the tiling the library
reports (ecgmm_conv5_in1_bwd_data_tile): a width that crosses two column-strip boundaries, a height that is no multiple of
the row step and spans two workgroups.  Small-integer operands must give the float64 result exactly; two runs the same bits.

ecgmm_crnn_gradcam (csrc/gradcam.hip) against tests/crnn_saliency_ref.py from the same seq / dseq.  Bound per element
(crnn_saliency_ref.gradcam_bound, f64check's g_k): the coarse map g_k(Tp * Fp + 1 + C) times its sum of magnitudes -- the
Tp * Fp-term sum and its scaling by 1 / (Tp * Fp), then the C-term dot -- carried through the division by the maximum (1
rounding, the maximum's own error as cam_ref * bound(max) / max) and the bilinear blend (6 roundings, plus the fp32 source
coordinates).  Exact: zeros behind ``frames``, an all-zero map for dseq <= 0 with seq >= 0, a coarse maximum of exactly 1.
Run with -s to see every figure."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import crnn_saliency_ref as S
from . import f64check as F64
from .exact_abi import Guarded
from .test_crnn_ops_gpu import IN1_CASES
from .util import DEV, bf16_round, dev, to_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [L.BF16, L.F32]
DT_IDS = ["bf16", "fp32"]
K_DX = 800


def tile(H):
    strip, step, rows = C.c_int(0), C.c_int(0), C.c_int(0)
    L.lib().ecgmm_conv5_in1_bwd_data_tile(H, C.byref(strip), C.byref(step), C.byref(rows))
    return strip.value, step.value, rows.value


def tiled_case():
    """two strip boundaries inside the width; a height that is no multiple of the row step and longer than one workgroup's
    rows, from the library's own tiling"""
    strip, step, _ = tile(1)
    H = next(h for h in range(3, 4096) if h % step and tile(h)[2] < h)
    return (2, H, 2 * strip + 5)


def dx_cases():
    return list(IN1_CASES) + [(1, 1, 1), (1, 3, 2), tiled_case()]


def run_dgrad(dy, w, dt):
    """dy [N,32,H,W], w [32,1,5,5] on the CPU -> dx [N,1,H,W] fp32 on the CPU, through a Guarded output"""
    N, _, H, W = dy.shape
    dyg, wg = to_nhwc(dy, dt), dev(w)
    out = Guarded(N * H * W, "f32")
    L.check(L.lib().ecgmm_conv5_in1_bwd_data(dt, ptr(dyg), ptr(wg), out.ptr, N, H, W, stream()), "conv5_in1_bwd_data")
    bits = out.done("dx")
    return torch.from_numpy(bits.view(np.float32).copy()).view(N, 1, H, W)


def test_the_tiled_case_is_what_it_is_meant_to_be():
    N, H, W = tiled_case()
    strip, step, rows = tile(H)
    assert (W - 1) // strip == 2 and W % strip and H % step and rows < H and rows % step == 0


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", range(6), ids=lambda i: "case%d" % i)
def test_conv5_in1_bwd_data_vs_float64(case, dt):
    N, H, W = dx_cases()[case]
    torch.manual_seed(300 + N * 31 + W)
    rnd = bf16_round if dt == L.BF16 else (lambda t: t)
    x = torch.randn(N, 1, H, W)
    w = torch.randn(32, 1, 5, 5) * 0.2
    dy = rnd(torch.randn(N, 32, H, W))
    ref = F64.conv_ref64(rnd(x), rnd(w), dy, padding=(2, 2))      # the kernel rounds w itself
    dx = run_dgrad(dy, w, dt)
    print((N, H, W), end=" ")
    F64.check_f32(dx, ref.dx, ref.adx, K=K_DX, name="dx")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_conv5_in1_bwd_data_exact_on_small_integers_and_rerun(dt):
    """dy in {-2..2}, w in {-1, 0, 1}: every partial sum is an integer below 2^24, so any order gives the float64 result;
    a second run gives the same bits"""
    N, H, W = tiled_case()
    torch.manual_seed(17)
    dy = torch.randint(-2, 3, (N, 32, H, W)).float()
    w = torch.randint(-1, 2, (32, 1, 5, 5)).float()
    ref = F64.conv_ref64(torch.zeros(N, 1, H, W), w, dy, padding=(2, 2))
    a, b = run_dgrad(dy, w, dt), run_dgrad(dy, w, dt)
    assert float(ref.dx.abs().max()) > 10
    assert torch.equal(a.double(), ref.dx)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_conv5_in1_bwd_data_two_runs_same_bits(dt):
    N, H, W = IN1_CASES[1]
    torch.manual_seed(23)
    dy, w = torch.randn(N, 32, H, W), torch.randn(32, 1, 5, 5)
    assert torch.equal(run_dgrad(dy, w, dt), run_dgrad(dy, w, dt))


# ---------------------------------------------------------------------------------------------------
# ecgmm_crnn_gradcam
# ---------------------------------------------------------------------------------------------------
# (B, Tp, C, Fp, F, T)
CAM_CASES = [(2, 5, 128, 4, 33, 40), (3, 1, 128, 4, 33, 8), (2, 7, 32, 5, 40, 59)]
VARIANTS = ["plain", "steps+frames", "steps=1", "frames"]


def lengths_of(case, variant):
    B, Tp, Cn, Fp, Fq, T = case
    steps = frames = None
    if variant == "steps+frames":
        steps = torch.tensor([max(1, Tp - 2 * b) for b in range(B)], dtype=torch.int32)
        steps[-1] = 1
        frames = torch.tensor([max(1, T - 7 * b) for b in range(B)], dtype=torch.int32)
        frames[-1] = 1
    elif variant == "steps=1":
        steps = torch.ones(B, dtype=torch.int32)
    elif variant == "frames":
        frames = torch.tensor([max(1, T // (b + 1) - 1) for b in range(B)], dtype=torch.int32)
    return steps, frames


@functools.lru_cache(maxsize=None)
def cam_inputs(case):
    B, Tp, Cn, Fp, Fq, T = case
    torch.manual_seed(500 + Tp * 13 + Cn)
    seq = torch.relu(torch.randn(B, Tp, Cn * Fp) + 0.3)       # behind a ReLU and a max-pool
    # mixed signs with a positive mean: every record's live part keeps a maximum well clear of its own error bound (an
    # all-zero map is a case of its own below), checked on the reference alone by gradcam_bound (finite)
    dseq = torch.randn(B, Tp, Cn * Fp) * 0.01 + 0.0008
    return seq, dseq


def run_cam(seq, dseq, steps, frames, case):
    """-> cam [B][F][T] and the normalised coarse map [B][Fp][Tp] out of the workspace, on the CPU"""
    B, Tp, Cn, Fp, Fq, T = case
    lib = L.lib()
    nws = lib.ecgmm_crnn_gradcam_workspace(B, Tp, Fp, Cn)
    assert nws >= (B * Cn + B * Fp * Tp) * 4
    ws = torch.full((nws // 4,), float("nan"), device=DEV)
    sg, dg = dev(seq), dev(dseq)
    st = None if steps is None else dev(steps)
    fr = None if frames is None else dev(frames)
    out = Guarded(B * Fq * T, "f32")
    L.check(lib.ecgmm_crnn_gradcam(ptr(sg), ptr(dg), ptr(st), ptr(fr), ptr(ws), nws, out.ptr, B, Tp, Cn, Fp, Fq, T, stream()),
            "crnn_gradcam")
    bits = out.done("cam")
    cam = torch.from_numpy(bits.view(np.float32).copy()).view(B, Fq, T)
    coarse = ws[B * Cn:B * Cn + B * Fp * Tp].view(B, Fp, Tp).cpu()
    return cam, coarse


def behind(t, steps, value):
    t = t.clone()
    if steps is not None:
        for b, n in enumerate(steps.tolist()):
            t[b, n:] = value
    return t


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CAM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_crnn_gradcam_vs_float64(case, variant):
    """K of the coarse map = Tp * Fp + 1 + C (module docstring); NaN stands behind ``steps`` in both operands"""
    B, Tp, Cn, Fp, Fq, T = case
    seq, dseq = cam_inputs(case)
    steps, frames = lengths_of(case, variant)
    seq, dseq = behind(seq, steps, float("nan")), behind(dseq, steps, float("nan"))
    cam, coarse = run_cam(seq, dseq, steps, frames, case)
    ref = S.gradcam_ref(seq, dseq, steps, frames, Cn, Fq, T)
    bound = S.gradcam_bound(seq, dseq, steps, frames, Cn, Fq, T)
    assert bool(torch.isfinite(cam).all()) and bool(torch.isfinite(bound).all())
    err = (cam.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
    print("%s %-13s worst |err| %.3g, worst |err| / bound %.3g (largest bound %.3g)"
          % (case, variant, float(err.max()), float(ratio.max()), float(bound.max())))
    assert float(ratio.max()) <= 1.0
    assert float(cam.min()) >= 0 and float(cam.max()) <= 1
    for b in range(B):
        assert float(coarse[b].max()) == 1.0, "record %d: the coarse maximum is not exactly 1" % b
        if steps is not None:
            assert bool((coarse[b, :, int(steps[b]):] == 0).all())
        if frames is not None:
            assert bool((cam[b, :, int(frames[b]):] == 0).all())
            assert float(cam[b, :, :int(frames[b])].max()) > 0


def test_crnn_gradcam_all_zero_map_and_exact_maximum():
    case = CAM_CASES[0]
    B, Tp, Cn, Fp, Fq, T = case
    seq, dseq = cam_inputs(case)
    # dseq <= 0 with seq >= 0: every weighted sum is <= 0, the map is exactly zero
    cam, coarse = run_cam(seq, -dseq.abs(), None, None, case)
    assert bool((cam == 0).all()) and bool((coarse == 0).all())
    # one record all zero, the other not
    mixed = dseq.clone()
    mixed[0] = -dseq[0].abs()
    cam, coarse = run_cam(seq, mixed, None, None, case)
    assert bool((cam[0] == 0).all()) and float(cam[1].max()) > 0 and float(coarse[1].max()) == 1.0
    # dseq >= 0 and the activation at (f, t) = (0, 0) ten times the rest: the coarse maximum sits in the corner, which the
    # upsample copies (source coordinate clamped to 0, blend weights exactly 1 and 0) -> cam[b][0][0] is exactly 1
    corner = seq.clone() + 0.1
    corner.view(B, Tp, Cn, Fp)[:, 0, :, 0] *= 10
    cam, coarse = run_cam(corner, dseq.abs(), None, None, case)
    assert bool((coarse[:, 0, 0] == 1).all()) and bool((cam[:, 0, 0] == 1).all()) and float(cam.max()) == 1.0
