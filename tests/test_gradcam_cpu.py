"""The Grad-CAM checker of tests/f64check.py (last section) on the CPU: it accepts the kernels of csrc/gradcam.hip restated in
torch fp32, operation by operation, and rejects that restatement with one defect each -- the slips the three kernels could
make without the whole-model comparison of tests/test_explain_gpu.py noticing.  Also here, because only torch is needed: the
hash-filled operands of every case of tests/test_gradcam_f64_gpu.py give the float64 reference something to compare (no
sample meant to be nonzero has its maximum near the weighted-sum bound; every sample meant to be zero is exactly zero).
No test here calls a kernel; ecgmm_gradcam's refusals (which launch nothing) are in tests/test_explain_cpu.py."""
import pytest
import torch

from . import f64check as F64

f32 = torch.float32


def _axis32(dst_n, in_, out_, corners=False, offset=True, early=False):
    """bilinear_src of csrc/gradcam.hip in fp32 tensors -> i0, i1, lam"""
    dst = torch.arange(dst_n, dtype=f32)
    if corners:
        src = dst * (torch.tensor(float(in_ - 1), dtype=f32) / torch.tensor(float(max(out_ - 1, 1)), dtype=f32))
    else:
        scale = torch.tensor(float(in_), dtype=f32) / torch.tensor(float(out_), dtype=f32)
        src = (dst + 0.5) * scale - (0.5 if offset else 0.0)
    src = src.clamp_min(0)
    last = in_ - 1 - int(early and in_ > 1)
    i0 = src.to(torch.int64).clamp_max(last)
    i1 = (i0 + 1).clamp_max(last)
    return i0, i1, src - i0.to(f32)


def analogue(act, dp, Hs, Ws, H, W, defect=None):
    """-> (small [N][Hs][Ws], out [N][H][W]) fp32, the three kernels step by step; defect: one of DEFECTS"""
    N, R, C = act.shape
    a, w = act.to(f32), dp.to(f32)
    if defect == "channel tail":                 # every lane makes its first trip only: channels >= 64 are never read
        a = a[:, :, :64]
    if defect == "previous dpooled":
        w = w.roll(1, 0)
    s = torch.einsum("nrc,nc->nr", a, w[:, :a.shape[2]])
    if defect != "no scale":
        s = s * torch.tensor(1.0 / R, dtype=f32)
    if defect != "no relu":
        s = s.clamp_min(0)
    m = s.amax(1).clamp_min(0)
    if defect == "previous maximum":
        m = m.roll(1, 0)
    inv = torch.where(m > 0, 1.0 / m.clamp_min(1e-30), torch.zeros_like(m))
    small = (s * inv[:, None]).view(N, Hs, Ws)
    hs, ws = (Ws, Hs) if defect == "swapped extents" else (Hs, Ws)
    grid = small.reshape(N, hs, ws)
    kw = dict(corners=defect == "align corners", offset=defect != "no offset")
    h0, h1, lh = _axis32(H, hs, H, early=defect == "row clamped early", **kw)
    w0, w1, lw = _axis32(W, ws, W, early=defect == "column clamped early", **kw)
    g = lambda hi, wi: grid[:, hi][:, :, wi]
    lw_, lh_ = lw.view(1, 1, W), lh.view(1, H, 1)
    top = g(h0, w0) * (1 - lw_) + g(h0, w1) * lw_
    bot = g(h1, w0) * (1 - lw_) + g(h1, w1) * lw_
    return small, top * (1 - lh_) + bot * lh_


DEFECTS = ("channel tail", "previous dpooled", "previous maximum", "swapped extents", "align corners", "no offset", "no relu",
           "row clamped early", "column clamped early")
# the cases each defect can show at: a channel tail needs C % 64 != 0, swapped extents Hs != Ws, coordinates an upsample that
# is no identity, a row / column clamp more than one coarse row / column
SHOWS = {
    "channel tail": [c for c in F64.GRADCAM_CASES if c[3] > 64 and c[3] % 64],
    "previous dpooled": list(F64.GRADCAM_CASES),
    "previous maximum": [c for c in F64.GRADCAM_CASES if c[0] > 1 and c[1] * c[2] > 1],
    "swapped extents": [(1, 8, 79, 512, 250, 2500), (2, 9, 11, 33, 4, 6), (5, 2, 3, 8, 7, 7), (2, 17, 19, 16, 40, 40)],
    "align corners": [c for c in F64.GRADCAM_CASES if (c[1], c[2]) != (c[4], c[5]) and c[1] * c[2] > 1],
    "no offset": [c for c in F64.GRADCAM_CASES if (c[1], c[2]) != (c[4], c[5]) and c[1] * c[2] > 1],
    "no relu": [c for c in F64.GRADCAM_CASES if c[1] * c[2] >= 15],
    "row clamped early": [c for c in F64.GRADCAM_CASES if c[1] > 1],
    "column clamped early": [c for c in F64.GRADCAM_CASES if c[2] > 1],
}
SMALL_CASES = [c for c in F64.GRADCAM_CASES if c[0] * c[4] * c[5] <= 200000]


@pytest.fixture(scope="module")
def refs():
    """the float64 reference of every (case, dtype), computed once and left unchanged"""
    out = {}
    for case in F64.GRADCAM_CASES:
        for bf16 in (False, True):
            act, dp = F64.gradcam_inputs(case, bf16)
            out[case, bf16] = (act, dp, F64.gradcam_ref(act, dp, *case[1:3], *case[4:6]))
    return out


def _zero_samples(case):
    neg = F64.GRADCAM_CASES[case]
    return () if neg is None else (neg,)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", list(F64.GRADCAM_CASES))
def test_reference_has_something_to_compare_and_the_checker_accepts_fp32(refs, case, bf16):
    N, Hs, Ws, C, H, W = case
    act, dp, ref = refs[case, bf16]
    assert bool((act >= 0).all()) and bool((dp > 0).any()) and bool((dp < 0).any())
    margin = F64.gradcam_live(ref, _zero_samples(case))
    if Hs * Ws >= 15:                                       # the ReLU clips something in every live sample, and not all of it
        for n in set(range(N)) - set(_zero_samples(case)):
            assert bool((ref.pre[n] < -ref.em[n]).any()) and bool((ref.pre[n] > ref.em[n]).any()), n
    small, out = analogue(act, dp, Hs, Ws, H, W)
    both = F64.gradcam_ratio(out, ref, small, "staged")
    whole = F64.gradcam_ratio(out, ref, None, "operands to map")
    print("%s bf16=%d: m / em >= %.3g; fp32 restatement: coarse %.3g, upsample %.3g, whole %.3g" %
          (case, bf16, margin, both.parts["small"], both.parts["out"], whole.ratio))
    assert both.ok and whole.ok, (str(both), str(whole))
    assert float(ref.out.min()) >= 0 and float(ref.out.max()) <= 1
    for n in _zero_samples(case):
        assert float(small[n].abs().max()) == 0 and float(out[n].abs().max()) == 0
    if (Hs, Ws) == (H, W):
        assert torch.equal(out, small)                      # the identity upsample is exact in the fp32 form as well
    if Hs * Ws == 1:
        assert float((ref.out - ref.small.view(N, 1, 1)).abs().max()) < 2.0 ** -50   # (torch's own float64 lerp rounds)


def test_float64_reference_is_the_textbook_map():
    """gradcam_ref against the textbook computation on autograd: logits = fc(mean over space of A)"""
    torch.manual_seed(0)
    N, C, Hs, Ws, H, W, nc = 3, 10, 4, 5, 13, 17, 2
    A = torch.rand(N, C, Hs, Ws, dtype=torch.float64, requires_grad=True)
    fc = torch.randn(nc, C, dtype=torch.float64)
    logit = (A.mean((2, 3)) @ fc.t())[:, 1].sum()
    g, = torch.autograd.grad(logit, A)
    cam = (g.mean((2, 3), keepdim=True) * A).sum(1).clamp_min(0).detach()
    cam = cam / cam.flatten(1).amax(1)[:, None, None]
    want = torch.nn.functional.interpolate(cam[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    act = A.detach().permute(0, 2, 3, 1).reshape(N, Hs * Ws, C)
    ref = F64.gradcam_ref(act, fc[1].expand(N, C), Hs, Ws, H, W)
    assert float((ref.out - want).abs().max()) < 1e-14


@pytest.mark.parametrize("defect", DEFECTS)
def test_checker_rejects_each_defect(refs, defect):
    shown = 0
    for case in SHOWS[defect]:
        if case not in SMALL_CASES:
            continue
        N, Hs, Ws, C, H, W = case
        for bf16 in (False, True):
            act, dp, ref = refs[case, bf16]
            small, out = analogue(act, dp, Hs, Ws, H, W, defect)
            whole = F64.gradcam_ratio(out, ref, None)
            staged = F64.gradcam_ratio(out, ref, small)
            print("%-22s %s bf16=%d: whole %.3g, staged %s" % (defect, case, bf16, whole.ratio, staged.parts))
            assert not whole.ok and not staged.ok, (defect, case, bf16)
            shown += 1
    assert shown >= 2


def test_dropping_the_scale_is_accepted_because_it_cancels(refs):
    """1 / R multiplies every sum of a sample and its maximum alike: a kernel that leaves it out computes the same map to
    within the same roundings, and the checker must say so -- this is no hole"""
    for case in SMALL_CASES:
        N, Hs, Ws, C, H, W = case
        act, dp, ref = refs[case, False]
        small, out = analogue(act, dp, Hs, Ws, H, W, "no scale")
        assert F64.gradcam_ratio(out, ref, small).ok and F64.gradcam_ratio(out, ref, None).ok, case


def test_a_few_ulps_are_resolved_where_the_derivation_leaves_no_room(refs):
    """4 fp32 ulps on one element.  At a generic element the derived bound is three stages wide (printed below in ulps of the
    element) and cannot resolve them, and nothing is tightened to make it.  It does where the derivation gives exactness: the
    upsample of a stored coarse map at identity size, and a sample that must be zero."""
    case = (2, 3, 5, 70, 3, 5)
    N, Hs, Ws, C, H, W = case
    act, dp, ref = refs[case, False]
    small, out = analogue(act, dp, Hs, Ws, H, W)
    flat = out[1].reshape(-1)
    k = int(torch.argsort(flat)[flat.numel() // 2])
    assert float(flat[k]) > 0
    bad = out.clone()
    bad[1].view(-1).view(torch.int32)[k] += 4
    assert F64.gradcam_ratio(out, ref, small).ok and not F64.gradcam_ratio(bad, ref, small).ok
    ulp = torch.nextafter(flat[k], torch.tensor(2.0)) - flat[k]
    print("bound of the median element from the operands: %.1f ulps" % float(ref.e_out[1].reshape(-1)[k] / ulp))
    # the zero sample: the smallest positive number is already outside
    bad = out.clone()
    bad[0, 1, 2] = 2.0 ** -149
    assert not F64.gradcam_ratio(bad, ref, None).ok and not F64.gradcam_ratio(bad, ref, small).ok
    bad_small = small.clone()
    bad_small[0, 1, 2] = 2.0 ** -149
    assert not F64.gradcam_ratio(out, ref, bad_small).ok


def test_non_finite_and_unwritten_outputs_are_rejected(refs):
    case = (5, 2, 3, 8, 7, 7)
    act, dp, ref = refs[case, False]
    small, out = analogue(act, dp, *case[1:3], *case[4:6])
    for n in (0, 2):                    # a live sample and the zero sample
        bad = out.clone()
        bad[n, 3, 3] = float("nan")
        assert not F64.gradcam_ratio(bad, ref, small).ok and not F64.gradcam_ratio(bad, ref, None).ok
        bad_small = small.clone()
        bad_small[n, 1, 1] = float("nan")
        assert not F64.gradcam_ratio(out, ref, bad_small).ok


def test_dpooled_error_widens_the_first_stage_only_by_what_it_can_cause(refs):
    case = (2, 9, 11, 33, 4, 6)
    N, Hs, Ws, C, H, W = case
    act, dp, ref = refs[case, False]
    dd = 1e-4 * dp.abs().double()
    wide = F64.gradcam_ref(act, dp, Hs, Ws, H, W, dpooled_err=dd)
    assert bool((wide.e_small >= ref.e_small).all()) and float(wide.e_small.max()) < 1e-2
    _s, out = analogue(act, (dp.double() + dd).float(), Hs, Ws, H, W)
    assert not F64.gradcam_ratio(out, ref, None).ok and F64.gradcam_ratio(out, wide, None).ok
