"""Grad-CAM of the two ResNet encoders against float64: the three map kernels of csrc/gradcam.hip through ecgmm_gradcam, op
level, in both compute dtypes, and the two plan entry points (ecgmm_resnet18_gradcam, ecgmm_resnet1d_gradcam) on the tensors
their own workspaces hold.  Reference and bounds: tests/f64check.py, last section (weighted sum, normalise, upsample -- every
bound derived, nothing calibrated); tests/test_gradcam_cpu.py shows on the CPU what those bounds reject and that the
operands used here give the reference something to compare.

Op level: act, dpooled from f64check.gradcam_inputs; the coarse map `small` (exactly N * Hs * Ws floats) and `out` are
NaN-filled views of one arena between sentinel zones.  Every element of both must come back written, no sentinel touched.
`small` is checked against stages 1 and 2, `out` against the float64 upsample of the stored `small` (the consumer-stage
convention of f64check.py) and, again, against the whole chain from the operands.  Beyond the bound: a sample with an
all-negative dpooled is exactly 0 in both buffers and its neighbours are not; an identity upsample returns `small` bit for
bit; 0 <= out <= 1; the coarse maximum of a live sample is 1 or 1 - 2^-24 (the reciprocal form).

Plan level: an eval forward through the C ABI (the harness of tests/test_plan_replay_gpu.py), a dense hash-filled dfeat, then
the plan's Grad-CAM.  The float64 dpooled is the classifier backward of the same dfeat and parameters (ResNet1D_SE: through the
stored ReLU output h1); what the kernel's fp32 dpooled may differ from it by is the dot-product bound of that backward and
enters the first stage (gradcam_ref(dpooled_err=...)).  The map is checked from the last block's stored output; and, dpooled and
the coarse map being named backward views (dpooled, X[0]), ecgmm_gradcam on the plan's own operands must give the same bits.
This pins the tensor and the layout the map is built from, which a whole-model comparison can only suggest.

Measured on the MI355X (worst |err| / bound; 1 is the limit; print with -s, WORST lines).  "coarse": `small` against stages
1 and 2; "upsample": `out` against the float64 upsample of the stored `small`; "whole": `out` against all three stages from
the operands; fp32 / bf16:
  case (N, Hs, Ws, C, H, W)        coarse              upsample         whole
  (2, 7, 7, 512, 224, 224)         0.00059 / 0.00051   0.11 / 0.13      0.00096 / 0.00061
  (1, 8, 79, 512, 250, 2500)       0.00071 / 0.00060   0.51 / 0.52      0.022 / 0.022
  (2, 1, 313, 256, 1, 5000)        0.0014 / 0.0026     0.47 / 0.47      0.13 / 0.13
  (3, 1, 1, 64, 5, 9)              0 / 0               3e-10 / 3e-10    6e-12 / 6e-12
  (2, 3, 5, 70, 3, 5)              0.0050 / 0.0038     0 / 0 (exact)    0.0050 / 0.0032
  (2, 9, 11, 33, 4, 6)             0.025 / 0.024       0.13 / 0.12      0.045 / 0.045
  (5, 2, 3, 8, 7, 7)               0.13 / 0.14         0.12 / 0.093     0.073 / 0.081
  (2, 17, 19, 16, 40, 40)          0.061 / 0.058       0.24 / 0.25      0.11 / 0.11
  (5, 2, 2, 8, 512, 512)           0.053 / 0.096       0.21 / 0.20      0.057 / 0.094
  plans: dpooled against its float64 classifier backward <= 0.099; coarse <= 0.00089; upsample <= 0.37 (ResNet1D_SE (2, 1, 1000));
  whole <= 0.0041; the op on the plan's own operands gave the plan's bits in all eight runs.
The first stage is the standard dot-product bound of C summands, hundreds of times wider than what the wave-strided sum
shows at C = 512; the upsample stage is the tight one (its coordinate term: the worst ratios are at the long axes, W = 2500
and 5000).  The float64 maxima of the live samples stand 1200 (plans) to 7e5 times above the weighted-sum bound.
No kernel broke a bound; no constant is calibrated.  The 27 tests of this module take a few seconds in all (with the
extended tests/test_explain_gpu.py: 46 tests in under 9 s).
"""
import ctypes as C
import functools

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from oracle import fill

from . import f64check as F64
from .lstm_abi import Arena, table
from .test_plan_replay_gpu import OUT_DIM, Plan, ff, same_bits
from .util import DEV, TDT

pytestmark = pytest.mark.gpu
DTYPES = [L.F32, L.BF16]
DTNAME = {L.F32: "fp32", L.BF16: "bf16"}
SUM_WAVES, NORM_THREADS, UP_THREADS, UP_BLOCKS = 4, 256, 256, 4096      # launch geometry of csrc/gradcam.hip

# what each case is here for, and the condition on the launch geometry that makes it so
GRADCAM_REACHES = {
    (2, 7, 7, 512, 224, 224): ("layer4 of a 224 x 224 picture", lambda N, Hs, Ws, C, H, W: (Hs, C) == ((H + 31) // 32, 512)),
    (1, 8, 79, 512, 250, 2500): ("layer4 of a 250 x 2500 picture",
                                 lambda N, Hs, Ws, C, H, W: (Hs, Ws, C) == ((H + 31) // 32, (W + 31) // 32, 512)),
    (2, 1, 313, 256, 1, 5000): ("the 1-D encoder's last block; the normalise loop's second trip",
                                lambda N, Hs, Ws, C, H, W: Hs == H == 1 and Ws == (W + 15) // 16 and Ws > NORM_THREADS),
    (3, 1, 1, 64, 5, 9): ("R == 1", lambda N, Hs, Ws, C, H, W: Hs * Ws == 1 and H * W > 1),
    (2, 3, 5, 70, 3, 5): ("C % 64 != 0 past the first trip; identity size",
                          lambda N, Hs, Ws, C, H, W: C > 64 and C % 64 != 0 and (Hs, Ws) == (H, W)),
    (2, 9, 11, 33, 4, 6): ("C < 64; downsampling", lambda N, Hs, Ws, C, H, W: C < 64 and H < Hs and W < Ws),
    (5, 2, 3, 8, 7, 7): ("partial last workgroup of the sum kernel", lambda N, Hs, Ws, C, H, W: (N * Hs * Ws) % SUM_WAVES != 0),
    (2, 17, 19, 16, 40, 40): ("R no multiple of the normalise block, second trip partial",
                              lambda N, Hs, Ws, C, H, W: Hs * Ws > NORM_THREADS and (Hs * Ws) % NORM_THREADS != 0),
    (5, 2, 2, 8, 512, 512): ("the upsample's grid-stride loop makes a second trip",
                             lambda N, Hs, Ws, C, H, W: N * H * W > UP_BLOCKS * UP_THREADS and C <= 8),
}
assert list(GRADCAM_REACHES) == list(F64.GRADCAM_CASES)


@functools.lru_cache(maxsize=None)
def _case(case, bf16):
    """operands and float64 reference of one (case, dtype), computed once and left unchanged"""
    act, dp = F64.gradcam_inputs(case, bf16)
    ref = F64.gradcam_ref(act, dp, *case[1:3], *case[4:6])
    zero = () if F64.GRADCAM_CASES[case] is None else (F64.GRADCAM_CASES[case],)
    return act, dp, ref, zero, F64.gradcam_live(ref, zero)


def run_op(dt, act, dp, N, Hs, Ws, Cn, H, W):
    """ecgmm_gradcam on device operands -> (small [N][Hs][Ws], out [N][H][W]) on the CPU; both were NaN between sentinels"""
    ar = Arena({"small": (N, Hs, Ws), "out": (N, H, W)})
    L.check(L.lib().ecgmm_gradcam(dt, ptr(act), ptr(dp), ptr(ar.views["small"]), ptr(ar.views["out"]), N, Hs, Ws, Cn, H, W,
                                  stream()), "gradcam")
    torch.cuda.synchronize()
    assert not ar.touched(), "gradcam wrote outside a buffer, next to: %s" % ar.touched()
    return ar.views["small"].cpu(), ar.views["out"].cpu()


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: DTNAME[d])
@pytest.mark.parametrize("case", list(F64.GRADCAM_CASES), ids=lambda c: "x".join(map(str, c)))
def test_gradcam_op_against_float64(case, dt):
    N, Hs, Ws, Cn, H, W = case
    what, reaches = GRADCAM_REACHES[case]
    assert reaches(*case), what
    bf16 = dt == L.BF16
    act, dp, ref, zero, margin = _case(case, bf16)
    small, out = run_op(dt, act.to(DEV).to(TDT[dt]).contiguous(), dp.to(DEV).contiguous(), *case)
    assert bool(torch.isfinite(small).all()), "%d elements of the coarse map not written" % int((~torch.isfinite(small)).sum())
    assert bool(torch.isfinite(out).all()), "%d elements of the map not written" % int((~torch.isfinite(out)).sum())
    staged = F64.check_gradcam(out, ref, small, "gradcam %s %s" % (case, DTNAME[dt]))
    whole = F64.check_gradcam(out, ref, None, "gradcam %s %s from the operands" % (case, DTNAME[dt]))
    print("WORST gradcam %-28s %s (%s): coarse %.3g, upsample %.3g, operands to map %.3g; reference m / em >= %.3g" %
          (case, DTNAME[dt], what, staged.parts["small"], staged.parts["out"], whole.ratio, margin))
    assert float(out.min()) >= 0 and float(out.max()) <= 1
    for n in range(N):
        if n in zero:
            assert float(small[n].abs().max()) == 0 and float(out[n].abs().max()) == 0, "sample %d must be exactly 0" % n
        else:
            assert float(small[n].max()) >= 1 - 2.0 ** -23 and float(out[n].max()) > 0, n
    if (Hs, Ws) == (H, W):
        assert same_bits(out, small), "identity upsample changed %d elements" % int((out != small).sum())
    if Hs * Ws == 1:
        one = small.view(N, 1, 1).double()
        assert bool(((out.double() - one).abs() <= F64.g_k(6) * one).all())


def test_gradcam_op_refuses_bad_calls_and_leaves_the_buffers_alone():
    lib = L.lib()
    ar = Arena({"small": (6,), "out": (2, 4, 4)})
    act, dp = torch.ones(2 * 3 * 8, device=DEV), torch.ones(2 * 8, device=DEV)
    v = ar.views
    call = lambda dt=L.F32, a=act, d=dp, s=v["small"], o=v["out"], shape=(2, 1, 3, 8, 4, 4): lib.ecgmm_gradcam(
        dt, ptr(a), ptr(d), ptr(s), ptr(o), *shape, stream())
    for kw, msg in ((dict(a=None), b"null"), (dict(d=None), b"null"), (dict(s=None), b"null"), (dict(o=None), b"null"),
                    (dict(dt=7), b"dtype"), (dict(shape=(0, 1, 3, 8, 4, 4)), b"bad shape"), (dict(shape=(2, 1, 3, 0, 4, 4)), b"bad shape"),
                    (dict(shape=(2, 1, 3, 8, 4, -1)), b"bad shape"), (dict(shape=(2, 65536, 65536, 8, 4, 4)), b"too large")):
        assert call(**kw) != 0 and msg in lib.ecgmm_last_error(), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(v["small"]).all()) and bool(torch.isnan(v["out"]).all()) and not ar.touched()
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v["out"]).all()) and not ar.touched()


# ----------------------------------------------------------------------------------------------------------------------
# the plan entry points
# ----------------------------------------------------------------------------------------------------------------------
PLAN_SHAPES = [("r18", (2, 3, 64, 64)), ("r18", (1, 3, 65, 97)), ("r1d", (2, 1, 1000)), ("r1d", (2, 12, 999))]
# the dense dfeat [N][out_dim]: salts for which, on the float64 oracle with the harness's parameters and inputs, every sample of
# every shape has positive weighted sums (m / em >= 1300) and negative ones too; about half the salts leave a sample all zero
DFEAT_SALT = {"r18": 821, "r1d": 822}


def dpooled_ref(plan, dfeat):
    """float64 d / d pooled of the classifier for dfeat [N][out_dim], and what an fp32 evaluation may differ by: the
    dot-product bound of each Linear backward (f64check.dot_bound), the first carried through the second"""
    d = dfeat.double()
    if plan.kind == "r18":
        w = plan.P["fc.weight"].double()
        return d @ w, F64.dot_bound(d.abs() @ w.abs(), w.shape[0])
    w4, w1 = plan.P["classifier.4.weight"].double(), plan.P["classifier.1.weight"].double()
    mask = (plan.f32(0, "h1", 0, plan.net.N, 64) > 0).double()          # the stored ReLU output of classifier.1
    dh = (d @ w4) * mask
    e_dh = F64.dot_bound(d.abs() @ w4.abs(), w4.shape[0]) * mask
    return dh @ w1, e_dh @ w1.abs() + F64.dot_bound((dh.abs() + e_dh) @ w1.abs(), w1.shape[0])


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: DTNAME[d])
@pytest.mark.parametrize("kind,shape", PLAN_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_plan_gradcam_against_float64(kind, shape, dt):
    plan = Plan(kind, shape, dt, training=False)
    plan.dfeat = fill.hash_tensor((shape[0], OUT_DIM[kind]), DFEAT_SALT[kind]).to(DEV)
    net, lib = plan.net, plan.lib
    N, last = net.N, net.blocks[-1]
    Hs, Ws, Cn, H, W = last.hout, last.wout, last.cout, net.H, net.W
    R = Hs * Ws
    plan.forward()
    before = plan.wf.clone()
    ff(plan.wb[:plan.nb // 4])
    ar = Arena({"cam": (N, H, W)})
    cam = ar.views["cam"]
    params = table([plan.P[n] for n in plan.names])
    fn = getattr(lib, ("ecgmm_resnet18" if kind == "r18" else "ecgmm_resnet1d") + "_gradcam")
    L.check(fn(C.byref(plan.desc), ptr(plan.dfeat), params, ptr(plan.wf), ptr(plan.wb), plan.nb, ptr(cam), stream()),
            "plan gradcam")
    plan.guards("gradcam")
    assert not ar.touched() and same_bits(plan.wf, before), "the Grad-CAM call wrote outside the map or into the forward workspace"
    assert bool(torch.isfinite(cam).all())
    # the tensors the map has to be built from, as the plan's workspaces hold them
    act = plan.raw(0, "out", len(net.blocks) - 1).view(TDT[dt]).view(N, R, Cn).clone()
    dp_dev = plan.f32(1, "dpooled", 0, N, Cn)
    small_dev = plan.raw(1, "X", 0).view(torch.float32)[:N * R].clone()
    dp64, e_dp = dpooled_ref(plan, plan.dfeat)
    r_dp = F64._ratio((dp_dev.double() - dp64).abs(), e_dp)
    ref = F64.gradcam_ref(act.cpu(), dp64.cpu(), Hs, Ws, H, W, dpooled_err=e_dp.cpu())
    margin = F64.gradcam_live(ref)
    name = "%s %s %s" % (kind, shape, DTNAME[dt])
    staged = F64.check_gradcam(cam.cpu(), ref, small_dev.cpu(), "plan gradcam " + name)
    whole = F64.check_gradcam(cam.cpu(), ref, None, "plan gradcam %s from the operands" % name)
    print("WORST plan gradcam %-26s coarse %dx%d: dpooled %.3g, coarse %.3g, upsample %.3g, operands to map %.3g; "
          "reference m / em >= %.3g" % (name, Hs, Ws, float(r_dp.max()), staged.parts["small"], staged.parts["out"], whole.ratio,
                                        margin))
    assert float(r_dp.max()) <= 1
    assert float(cam.min()) >= 0 and float(cam.max()) <= 1
    # the op on the plan's own operands: the same bits, coarse map and map
    small2, out2 = run_op(dt, act, dp_dev, N, Hs, Ws, Cn, H, W)
    assert same_bits(small2.reshape(-1), small_dev.cpu()) and same_bits(out2, cam.cpu())
