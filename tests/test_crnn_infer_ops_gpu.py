"""The kernels and the launch plan of the CRNN front end's inference path (csrc/crnn_front.hip, csrc/infer_fold.hip,
csrc/plan_infer.hip), op by op:

  ecgmm_relu_maxpool2          exactly torch.max_pool2d(torch.relu(y), 2) of the stored values, both output layouts
  ecgmm_conv5_in1_relu_pool2   bit for bit ecgmm_conv5_in1_fwd(stats = NULL) -> ecgmm_relu_maxpool2; the chain's conv output is
                               held to float64 by the bounds tests/test_crnn_ops_gpu.py uses for ecgmm_conv5_in1_fwd
  ecgmm_fold_conv5_bn          against tests/infer_ref.fold_ref64 with the bounds of tests/test_infer_gpu.py
  ecgmm_crnn_front_infer       bit for bit the same front end built from the per-op entry points in separate buffers, and
                               (fp32) within the op bar 2e-5 of max|ref| of tests/crnn_ref.front_only in float64 on the CPU

Every output and workspace starts as 0xFF bytes (NaN in fp32 and bf16) between sentinel zones (tests/lstm_abi.Arena).
Run with -s to see every figure."""
import copy
import ctypes as C
import functools

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import crnn_ref as R
from . import f64check as F64
from .infer_chain import ff, same_bits
from .infer_ref import fold_ref64
from .lstm_abi import Arena, table
from .test_crnn_ops_gpu import BAR, relmax
from .test_infer_gpu import FOLD_F32_BIAS_REL, FOLD_F32_REL, _bn_case
from .util import bf16_round, conv_desc, dev, from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [L.BF16, L.F32]
DT_IDS = ["bf16", "fp32"]
ESZ = {L.BF16: 2, L.F32: 4}
EPS = 1e-5
POOL_CASES = [(2, 9, 11, 32), (3, 6, 13, 64), (2, 5, 8, 128), (1, 2, 2, 32)]
FUSED_CASES = [(1, 2, 2), (1, 3, 2), (2, 9, 11), (3, 5, 8), (1, 33, 70), (3, 33, 45)]   # the last: several workgroups, ragged tail
PLAN_CASES = [(1, 9, 9), (1, 8, 11), (2, 8, 8), (3, 33, 45)]
ids = lambda c: "x".join(map(str, c))


def arena(**nbytes):
    """one 0xFF-filled view of `nbytes` bytes (a multiple of 4) per name, between sentinel zones"""
    ar = Arena({k: (n // 4,) for k, n in nbytes.items()})
    for v in ar.views.values():
        ff(v)
    return ar


def as_dt(view, dt):
    return view if dt == L.F32 else view.view(torch.bfloat16)


def untouched(ar):
    torch.cuda.synchronize()
    assert not ar.touched(), "written outside an output, next to: %s" % ar.touched()


# ---------------------------------------------------------------------------------------------------
# relu -> MaxPool2d(2)
# ---------------------------------------------------------------------------------------------------
def relu_pool2(y, dt, seq):
    """y [N, C, H, W] CPU fp32 (bf16-representable under bf16) -> pooled [N, C, H/2, W/2] CPU fp32 as the kernel stored it"""
    N, Cn, H, W = y.shape
    PH, PW = H // 2, W // 2
    yg = to_nhwc(y, dt)
    n = N * PH * PW * Cn
    ar = arena(out=n * (4 if seq else ESZ[dt]))
    out = ar.views["out"] if seq else as_dt(ar.views["out"], dt)
    L.check(L.lib().ecgmm_relu_maxpool2(dt, ptr(yg), ptr(out), N, H, W, Cn, int(seq), stream()), "relu_maxpool2")
    untouched(ar)
    if seq:
        return out.view(N, PW, Cn, PH).permute(0, 2, 3, 1).cpu()
    return from_nhwc(out, dt, (N, Cn, PH, PW))


@pytest.mark.parametrize("seq", [False, True], ids=["nhwc", "seq"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", POOL_CASES, ids=ids)
def test_relu_maxpool2_equals_torch_exactly(case, dt, seq):
    N, H, W, Cn = case
    torch.manual_seed(300 + N * 7 + W)
    y = torch.randn(N, Cn, H, W) * 1.5 + 0.3
    if dt == L.BF16:
        y = bf16_round(y)
    got = relu_pool2(y, dt, seq)
    assert torch.equal(got, torch.max_pool2d(torch.relu(y), 2))


@pytest.mark.parametrize("seq", [False, True], ids=["nhwc", "seq"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_relu_maxpool2_ties_and_negatives(dt, seq):
    """small integers: windows full of ties equal torch's; an input of negatives (and -0) alone gives exact (+)zeros"""
    N, Cn, H, W = 2, 32, 7, 10
    torch.manual_seed(3)
    y = torch.randint(-2, 3, (N, Cn, H, W)).float()
    assert torch.equal(relu_pool2(y, dt, seq), torch.max_pool2d(torch.relu(y), 2))
    neg = -torch.randint(0, 4, (N, Cn, H, W)).float()     # (-0.0 where the draw is 0)
    got = relu_pool2(neg, dt, seq)
    assert bool((got.view(torch.int32) == 0).all()), "negative inputs must pool to +0 bits"


# ---------------------------------------------------------------------------------------------------
# block 1 as one kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", FUSED_CASES, ids=ids)
def test_fused_block1_equals_its_chain_bit_for_bit(case, dt):
    N, H, W = case
    PH, PW = H // 2, W // 2
    torch.manual_seed(400 + N * 31 + W)
    rnd = bf16_round if dt == L.BF16 else (lambda t: t)
    x, w, b = torch.randn(N, 1, H, W), torch.randn(32, 1, 5, 5) * 0.2, torch.randn(32) * 0.1
    xg, wg, bg = dev(x), dev(w), dev(b)
    lib = L.lib()
    ar = arena(y=N * H * W * 32 * ESZ[dt], chain=N * PH * PW * 32 * ESZ[dt], fused=N * PH * PW * 32 * ESZ[dt])
    y, chain, fused = (as_dt(ar.views[k], dt) for k in ("y", "chain", "fused"))
    L.check(lib.ecgmm_conv5_in1_fwd(dt, ptr(xg), ptr(wg), ptr(bg), ptr(y), None, N, H, W, stream()), "conv5_in1_fwd")
    L.check(lib.ecgmm_relu_maxpool2(dt, ptr(y), ptr(chain), N, H, W, 32, 0, stream()), "relu_maxpool2")
    L.check(lib.ecgmm_conv5_in1_relu_pool2(dt, ptr(xg), ptr(wg), ptr(bg), ptr(fused), N, H, W, stream()), "conv5_in1_relu_pool2")
    untouched(ar)
    assert bool(torch.isfinite(fused.float()).all())
    assert torch.equal(fused.view(torch.int16 if dt == L.BF16 else torch.int32), chain.view(torch.int16 if dt == L.BF16 else torch.int32))
    # the chain's conv output against float64 (the kernel rounds x and w itself), bounds of tests/test_crnn_ops_gpu.py
    ref = F64.conv_ref64(rnd(x), rnd(w), None, padding=(2, 2), bias=b)
    yc = from_nhwc(y, dt, (N, 32, H, W))
    if dt == L.BF16:
        F64.check_bf16(yc, ref.y, ref.ay, name="chain y")
    else:
        assert relmax(yc, ref.y, "chain y") <= BAR
    # ... and with it the fused output: exactly the pool of those stored values
    assert torch.equal(from_nhwc(fused, dt, (N, 32, PH, PW)), torch.max_pool2d(torch.relu(yc), 2))


def test_fused_block1_without_bias_equals_its_chain():
    N, H, W = 2, 9, 11
    torch.manual_seed(5)
    xg, wg = dev(torch.randn(N, 1, H, W)), dev(torch.randn(32, 1, 5, 5) * 0.2)
    lib = L.lib()
    n = N * (H // 2) * (W // 2) * 32
    ar = arena(y=N * H * W * 32 * 4, chain=n * 4, fused=n * 4)
    v = ar.views
    L.check(lib.ecgmm_conv5_in1_fwd(L.F32, ptr(xg), ptr(wg), None, ptr(v["y"]), None, N, H, W, stream()))
    L.check(lib.ecgmm_relu_maxpool2(L.F32, ptr(v["y"]), ptr(v["chain"]), N, H, W, 32, 0, stream()))
    L.check(lib.ecgmm_conv5_in1_relu_pool2(L.F32, ptr(xg), ptr(wg), None, ptr(v["fused"]), N, H, W, stream()))
    untouched(ar)
    assert same_bits(v["fused"], v["chain"]) and bool(torch.isfinite(v["fused"]).all())


# ---------------------------------------------------------------------------------------------------
# the fold of a 5x5 convolution
# ---------------------------------------------------------------------------------------------------
def fold5(dt, layout, w, cb, gamma, beta, rm, rv):
    """ecgmm_fold_conv5_bn -> (w' as stored, unpacked to OIHW on the CPU; b'; scale)"""
    cout, cin = w.shape[0], w.shape[1]
    wdt = L.F32 if layout == 1 else dt
    ar = arena(w=w.numel() * ESZ[wdt], b=cout * 4, s=cout * 4)
    wout = as_dt(ar.views["w"], wdt)
    ops = [dev(t) for t in (w, cb, gamma, beta, rm, rv)]
    L.check(L.lib().ecgmm_fold_conv5_bn(dt, layout, *(ptr(t) for t in ops), EPS, ptr(wout), ptr(ar.views["b"]), ptr(ar.views["s"]),
                                        cout, cin, stream()), "fold_conv5_bn")
    untouched(ar)
    wout = wout.cpu()
    unpacked = wout.view(w.shape) if layout == 1 else wout.view(cout, 25, cin).permute(0, 2, 1).reshape(w.shape)
    return unpacked, ar.views["b"].cpu(), ar.views["s"].cpu(), ops


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape, layout", [((32, 1, 5, 5), 1), ((64, 32, 5, 5), 0), ((128, 64, 5, 5), 0), ((40, 24, 5, 5), 1)],
                         ids=["cin1_oihw", "block2_pack", "block3_pack", "odd_oihw"])
def test_fold_conv5_against_float64(shape, layout, dt):
    """_bn_case negates a third of the gammas and sets a zero and two tiny ones, a running variance of 3e4 and one below eps"""
    torch.manual_seed(sum(shape))
    w = torch.randn(*shape) * 0.2
    gamma, beta, rm, rv, cb = _bn_case(shape[0], 11, True)
    gamma[10] = gamma[11] = 0.0
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    got_w, got_b, got_s, _ = fold5(dt, layout, w, cb, gamma, beta, rm, rv)
    ref_w, ref_b, ref_s = fold_ref64(w, cb, gamma, beta, rm, rv, eps)
    assert torch.isfinite(got_w.float()).all() and torch.isfinite(got_b).all()
    mag = beta.double().abs() + (cb.double() - rm.double()).abs() * ref_s.abs()
    berr = float(((got_b.double() - ref_b).abs() / mag.clamp_min(1e-300)).max())
    serr = float(((got_s.double() - ref_s).abs() / ref_s.abs().clamp_min(1e-300))[ref_s != 0].max())
    print("fold5 %s layout %d dtype %d: bias rel err %.3g, scale rel err %.3g" % (shape, layout, dt, berr, serr))
    assert berr <= FOLD_F32_BIAS_REL and serr <= FOLD_F32_REL
    zero = gamma == 0
    assert int(zero.sum()) == 3
    assert (got_s[zero] == 0).all() and (got_w.float()[zero] == 0).all(), "zero gamma must fold to exact zeros"
    assert torch.equal(got_b[zero], beta[zero]), "zero gamma must leave b' = beta"
    if layout == 1 or dt == L.F32:
        assert got_w.dtype == torch.float32      # the OIHW layout stays fp32 whatever the dtype
        nz = ref_w != 0
        werr = float(((got_w.double() - ref_w).abs()[nz] / ref_w.abs()[nz]).max())
        print("fold5 fp32 weight rel err %.3g" % werr)
        assert werr <= FOLD_F32_REL
    else:   # exactly bf16_round of the fp32 product the kernel forms (tests/test_infer_gpu.py), one ulp only on a rounding tie
        prod = w.float() * got_s.view(-1, 1, 1, 1)
        want = prod.to(torch.bfloat16)
        tie = (prod.view(torch.int32) & 0xFFFF) == 0x8000
        diff = (got_w.view(torch.int16).int() - want.view(torch.int16).int()).abs()
        assert (diff[~tie] == 0).all() and (diff[tie] <= 1).all()


# ---------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def front_model(seed=5):
    """the three blocks with torch's default initialisation, then running statistics away from (0, 1), a third of the gammas
    negated and some zero"""
    m = R.front_only(seed)
    g = torch.Generator().manual_seed(50 + seed)
    with torch.no_grad():
        for name in ("conv1", "conv2", "conv3"):
            bn = getattr(m, name).block[1]
            n = bn.num_features
            bn.running_mean.copy_(0.3 * torch.randn(n, generator=g))
            bn.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.25)
            bn.weight.copy_(1.0 + 0.3 * torch.randn(n, generator=g))
            bn.weight[::3] = -bn.weight[::3]
            bn.weight[1] = bn.weight[8] = 0.0
            bn.bias.copy_(0.2 * torch.randn(n, generator=g))
    return m.eval()


@functools.lru_cache(maxsize=None)
def plan_input(case):
    B, Fq, T = case
    torch.manual_seed(7000 + B * 31 + T)
    return torch.randn(B, 1, Fq, T)


def tables(m):
    params, buffers = [], []
    for name in ("conv1", "conv2", "conv3"):
        conv, bn = getattr(m, name).block[0], getattr(m, name).block[1]
        params += [dev(t.detach().float()) for t in (conv.weight, conv.bias, bn.weight, bn.bias)]
        buffers += [dev(bn.running_mean.float()), dev(bn.running_var.float()), dev(bn.num_batches_tracked)]
    return params, buffers


def run_plan(case, dt, params, buffers, x):
    """prepare + infer (twice) from 0xFF-filled blob, workspace and outputs, each exactly the reported size -> seq, seq again"""
    B, Fq, T = case
    lib = L.lib()
    d = L.CRNNFrontDesc(B, Fq, T, dt, 0, 0.1, EPS)
    nblob, nws = lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(d)), lib.ecgmm_crnn_front_infer_workspace(C.byref(d))
    assert nblob > 0 and nws > 0 and nblob % 4 == 0 and nws % 4 == 0, lib.ecgmm_last_error()
    nseq = B * (T // 8) * 128 * (Fq // 8) * 4
    ar = arena(blob=nblob, ws=nws, seq=nseq, seq2=nseq)
    v = ar.views
    L.check(lib.ecgmm_crnn_front_infer_prepare(C.byref(d), table(params), table(buffers), ptr(v["blob"]), nblob, stream()), "prepare")
    torch.cuda.synchronize()
    before = v["blob"].clone()
    L.check(lib.ecgmm_crnn_front_infer(C.byref(d), ptr(x), ptr(v["blob"]), nblob, ptr(v["seq"]), ptr(v["ws"]), nws, stream()), "infer")
    L.check(lib.ecgmm_crnn_front_infer(C.byref(d), ptr(x), ptr(v["blob"]), nblob, ptr(v["seq2"]), ptr(v["ws"]), nws, stream()), "infer")
    untouched(ar)
    assert same_bits(before, v["blob"]), "the forward wrote into its blob"
    shape = (B, T // 8, 128 * (Fq // 8))
    return v["seq"].view(shape), v["seq2"].view(shape)


def run_chain(case, dt, params, buffers, x):
    """the same front end from the per-op entry points alone, every tensor in a buffer of its own"""
    B, Fq, T = case
    lib = L.lib()
    es = ESZ[dt]
    h, w, cin, cur = Fq, T, 1, None
    for i in range(3):
        cout, ph, pw = 32 << i, h // 2, w // 2
        p = params[4 * i:4 * i + 4]
        bf = buffers[3 * i:3 * i + 2]
        last = i == 2
        ar = arena(w=cout * cin * 25 * (4 if i == 0 else es), b=cout * 4, y=B * h * w * cout * es,
                   pool=B * ph * pw * cout * (4 if last else es))
        v = ar.views
        wf = v["w"] if i == 0 else as_dt(v["w"], dt)
        L.check(lib.ecgmm_fold_conv5_bn(dt, 1 if i == 0 else 0, ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(bf[0]), ptr(bf[1]),
                                        EPS, ptr(wf), ptr(v["b"]), None, cout, cin, stream()), "fold block %d" % (i + 1))
        pool = v["pool"] if last else as_dt(v["pool"], dt)
        if i == 0:
            L.check(lib.ecgmm_conv5_in1_relu_pool2(dt, ptr(x), ptr(wf), ptr(v["b"]), ptr(pool), B, h, w, stream()), "block 1")
        else:
            y = as_dt(v["y"], dt)
            cd = conv_desc(B, h, w, cin, cout, 5, 5, 1, 2, 2)
            L.check(lib.ecgmm_conv_fwd_fused(dt, C.byref(cd), ptr(cur), ptr(wf), ptr(v["b"]), None, ptr(y), L.ACT_NONE, stream()),
                    "conv block %d" % (i + 1))
            L.check(lib.ecgmm_relu_maxpool2(dt, ptr(y), ptr(pool), B, h, w, cout, int(last), stream()), "pool block %d" % (i + 1))
        untouched(ar)
        cur, h, w, cin = pool, ph, pw, cout
    return cur.view(B, T // 8, 128 * (Fq // 8))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", PLAN_CASES, ids=ids)
def test_plan_equals_the_per_op_chain_bit_for_bit(case, dt):
    params, buffers = tables(front_model())
    x = dev(plan_input(case))
    seq, again = run_plan(case, dt, params, buffers, x)
    chain = run_chain(case, dt, params, buffers, x)
    assert bool(torch.isfinite(seq).all()), "NaN / inf left in seq"
    assert same_bits(seq, again), "two calls differ"
    assert same_bits(seq, chain), "the plan's seq is not the per-op chain's"


@pytest.mark.parametrize("case", PLAN_CASES, ids=ids)
def test_plan_fp32_against_float64(case):
    """the op bar of tests/test_crnn_ops_gpu.py (2e-5 of max|ref|) times one, over three blocks, as its
    test_front_end_fp32_* do.  ReLU and max are continuous, so the forward needs no margins."""
    m = front_model()
    params, buffers = tables(m)
    x = plan_input(case)
    seq, _ = run_plan(case, L.F32, params, buffers, dev(x))
    with torch.no_grad():
        ref = copy.deepcopy(m).double().front(x.double())
    assert relmax(seq, ref, "front end seq %s" % (case,)) <= BAR
