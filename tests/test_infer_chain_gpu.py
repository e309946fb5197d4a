"""The inference plans (csrc/plan_infer.hip, csrc/infer_fold.hip) op by op against float64 and as a whole.

1. ecgmm_relu_maxpool and ecgmm_gate_res_relu, the two passes only the inference plans run, on their own: every 1-D / 2-D
   edge of the 3x3 / stride 2 / pad 1 window (one row, one column, one pixel, odd and even extents), the plans' channel
   counts, one that is no power of two and the narrowest a 16-byte chunk allows; the gate at every rows_per_sample boundary,
   in place and out of place, with zero and negative gates; and one case each that passes the block cap of its launch, so that
   the grid-stride loop takes another trip.  Bars: tests/f64check.py check_relu_maxpool (exact) and check_gate_res_relu.
2. Either encoder's inference forward rebuilt as a chain of per-op entry points in separate buffers (tests/infer_chain.py):
   (a) every tensor of the chain against float64 of the one op that wrote it, on that op's stored inputs;
   (b) ecgmm_resnet18_infer / ecgmm_resnet1d_infer give features equal to the chain's BIT FOR BIT -- plan and chain run the
       same kernel instantiations on the same operand values, and no forward kernel uses atomics or a split reduction -- with
       blob, workspace and features views of one Arena between sentinels, 0xFF-filled before the calls; ResNet18 under both
       ECGMM_INFER_DOWN_SIDE settings.  What (b) adds to (a) is the plan's own logic: the blob layout, the rotating block
       buffers that alias the dead stem output, which tensor is handed on as addend or next input, the in-place gate pass;
   (c) liveness: one changed element of one folded bias in the chain changes the features;
   (d) one blob at two batch sizes: the features of the first sample alone equal row 0 of the batch bit for bit.
   Shapes: the replay shapes of tests/test_plan_replay_gpu.py (odd extents into the stride-2 blocks, 999-sample records,
   N = 3 and 2) and the smallest input each encoder accepts at N = 1.

Found by this file: ecgmm_relu_maxpool refused every channel count whose 16-byte chunks do not divide its 256 threads (C = 72
among them), a condition only ecgmm_gate_res_relu's kernel needs; relu_maxpool now asks for whole 16-byte chunks alone.

Also found: the rounding term of the bf16 bounds took half an ulp from the binade of the value, which is too small below 2^-126,
where bf16 is evenly spaced.  At ResNet1D_SE (2, 12, 1000) bf16 one squeeze-excite gate saturates to a subnormal fp32 value
(0x1.d1022p-128); y2 * gate + 0 = 0x1.ee124p-127 is stored as the nearest bf16 subnormal 0x1.f0p-127 -- torch's own conversion
gives the same bits -- at 1.93 times the old bound.  The kernel is right; tests/f64check.py half_ulp_bf16 now keeps the half
ulp at 2^-134 in that range, a property of the format (tests/test_f64check.py test_half_ulp).  KAPPA is unchanged.

No op reaches another instantiation through its entry point than through the plan: (b) holds bit for bit in every case, under
both ECGMM_INFER_DOWN_SIDE settings, and so does (d).

Measured on the MI355X, worst |err| / bound per op class over every case of the chain (1 is a bf16 rounding tie: the stored
rounding term alone; 0 is an exact comparison; print them with -s, CHAIN lines):

  op class                         ResNet18 bf16   ResNet18 fp32   ResNet1D_SE bf16   ResNet1D_SE fp32
  stem (y0)                        1               0.21            1                  0.32
  relu_maxpool (p0)                0               0               0                  0
  conv (a1 y2 yd out)              1               0.87            1                  0.84
  avgpool (m, pooled)              0.058           0.20            0.026              0.32
  se_mlp (h g)                     -               -               0.050              0.046
  gate_res_relu (out)              -               -               1                  0.27
  linear (fc / classifier)         0.0021          0.0022          0.011              0.012

(the fp32 convolutions against min(g_k(K + 2), KAPPA_F32) * A, the bound of tests/test_conv_edges_f64_gpu.py.)  The op-level
cases of part 1: relu_maxpool exact everywhere; gate_res_relu worst 1 (bf16: a rounding tie) and 0.25 of the two-rounding
bound (fp32), the case past the block cap included.

Run time on the MI355X: the 123 tests of this module take 6.4 s run alone, 2.4 s of that the start-up inside the first test
(the slowest after it 0.30 s, the first chain of ResNet18), beside about 130 s for the suite.  The two cases past a block
cap: relu_maxpool (kernel + float64 check) under 0.01 s, gate_res_relu (operands, both kernels, float64 check) 0.01 s.
"""
import functools
import time

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from .infer_chain import Chain, check_chain, same_bits
from .test_conv_edges_f64_gpu import _op
from .test_conv_layers_f64_gpu import TDT, _nhwc, poisoned, unguard
from .test_plan_replay_gpu import SHAPES
from .util import switches

pytestmark = pytest.mark.gpu
DTS = [L.BF16, L.F32]
NAME = {L.BF16: "bf16", L.F32: "fp32"}
dt_ids = lambda dt: NAME[dt]


def _width(C, dt):
    """"narrow": the narrowest row of whole 16-byte chunks"""
    return (8 if dt == L.BF16 else 4) if C == "narrow" else C


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ relu_maxpool
def _pool(dt, x, N, H, W, C):
    """x [N][H][W][C] in the stored type -> out [N][OH][OW][C], NaN-prefilled with guard elements"""
    n = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * C
    out = poisoned(n, TDT[dt])
    L.check(L.lib().ecgmm_relu_maxpool(dt, ptr(x), ptr(out), N, H, W, C, stream()), "relu_maxpool")
    return unguard(out, n, "relu_maxpool out")


POOL_SHAPES = [(2, 7, 9), (1, 8, 8), (1, 1, 37), (3, 1, 2), (1, 1, 1), (2, 2, 1)]


@pytest.mark.parametrize("dt", DTS, ids=dt_ids)
@pytest.mark.parametrize("C", [64, 72, "narrow"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_relu_maxpool_equals_the_float64_window_maximum(shape, C, dt):
    N, H, W = shape
    C = _width(C, dt)
    x = _nhwc(_op((N, C, H, W), 301 + H * W, "grad", dt), dt)
    if shape == (2, 7, 9) and C == 64:
        x[1, 3, 4, 5] = float("nan")             # a NaN tap never wins: it is skipped like a tap outside the image
    out = _pool(dt, x, N, H, W, C)
    assert not bool(torch.isnan(out.float()).any()), "a NaN tap won, or an element was left unwritten"
    F64.check_relu_maxpool(out, x, N, H, W, C, dt == L.BF16, "relu_maxpool %s C=%d %s" % (shape, C, NAME[dt]))


@pytest.mark.parametrize("dt", DTS, ids=dt_ids)
def test_relu_maxpool_of_an_all_negative_input_is_plus_zero(dt):
    N, H, W, C = 2, 7, 9, 64
    x = _nhwc(-_op((N, C, H, W), 331, "act", dt), dt)        # negative values and -0.0
    assert bool((x.float() <= 0).all()) and bool(torch.signbit(x.float()).all()) and bool((x.float() == 0).any())
    out = _pool(dt, x, N, H, W, C)
    assert bool((_bits(out) == 0).all()), "an all-negative window must give +0"
    F64.check_relu_maxpool(out, x, N, H, W, C, dt == L.BF16, "relu_maxpool all negative")


def test_relu_maxpool_second_trip_of_the_grid_stride_loop():
    """bf16 (1, 1, 262207) at C = 64: 131104 output pixels x 8 chunks = 4097 blocks of 256 threads, one more than the cap"""
    N, H, W, C = 1, 1, 262207, 64
    assert -(-(((W - 1) // 2 + 1) * (C // 8)) // 256) == 4097
    x = _nhwc(_op((N, C, H, W), 341, "grad", L.BF16), L.BF16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _pool(L.BF16, x, N, H, W, C)
    F64.check_relu_maxpool(out, x, N, H, W, C, True, "relu_maxpool 262207")
    print("relu_maxpool grid-stride case: kernel + float64 check %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ gate_res_relu
def _gate_operands(dt, N, rps, C, seed):
    """y, res [M][C] in the stored type (signed, an offset per sample and channel), gate [N][C] fp32 with negative values
    and exact zeros"""
    y = _nhwc(_op((N, C, 1, rps), seed, "grad", dt), dt).view(N * rps, C)
    res = _nhwc(_op((N, C, 1, rps), seed + 1, "grad", dt), dt).view(N * rps, C)
    gate = (_op((N, C), seed + 2, "grad", L.F32) * 0.4).contiguous()
    gate[0, 0], gate[N - 1, 2] = 0.0, 0.0
    gate[0, 1], gate[N - 1, 3] = -gate[0, 1].abs() - 0.25, gate[N - 1, 3].abs() + 0.25
    return y, gate, res


def _gate(dt, y, gate, res, rps, in_place):
    M, C = y.shape
    out = poisoned(M * C, TDT[dt])
    src = y
    if in_place:
        out[:M * C] = y.reshape(-1)
        src = out
    L.check(L.lib().ecgmm_gate_res_relu(dt, ptr(src), ptr(gate), ptr(res), ptr(out), M, C, rps, stream()), "gate_res_relu")
    return unguard(out, M * C, "gate_res_relu out").view(M, C)


def _gate_case(dt, N, rps, C, seed):
    y, gate, res = _gate_operands(dt, N, rps, C, seed)
    out = _gate(dt, y, gate, res, rps, False)
    r = F64.check_gate_res_relu(out, y, gate, res, rps, dt == L.BF16, "gate_res_relu N=%d rps=%d C=%d %s" % (N, rps, C, NAME[dt]))
    inp = _gate(dt, y, gate, res, rps, True)
    assert torch.equal(_bits(out), _bits(inp)), "in place (out == y) and out of place differ"
    return r


@pytest.mark.parametrize("dt", DTS, ids=dt_ids)
@pytest.mark.parametrize("C", [64, 128, 256, "narrow", 512])
@pytest.mark.parametrize("N,rps", [(3, 313), (5, 1), (1, 1), (2, 125)])
def test_gate_res_relu_against_float64_in_and_out_of_place(N, rps, C, dt):
    _gate_case(dt, N, rps, _width(C, dt), 401 + rps)


def test_gate_res_relu_past_the_block_cap():
    """fp32, C = 512 (8 rows per workgroup trip), N = 8, rows_per_sample = 8197: 65576 rows ask for 2050 blocks of 4 trips,
    the cap is 2048, so the grid-stride loop goes on past row 65536 into a fifth trip"""
    N, rps, C = 8, 8197, 512
    assert -(-(N * rps) // (8 * 4)) == 2050
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _gate_case(L.F32, N, rps, C, 451)
    print("gate_res_relu block-cap case: operands + 2 kernels + float64 check %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ the chain and the plan
MIN_SHAPE = {"r18": (1, 3, 32, 32), "r1d": (1, 1, 64)}
CASES = [(k, s, dt) for k in ("r18", "r1d") for s in SHAPES[k] + [MIN_SHAPE[k]] for dt in DTS]
BATCH_CASES = [c for c in CASES if c[1][0] > 1]
ids = lambda cases: ["%s-%s-%s" % (k, "x".join(map(str, s)), NAME[dt]) for k, s, dt in cases]


@functools.lru_cache(maxsize=None)
def chain(kind, shape, dt):
    """(built once per case and shared by the tests below, which leave it unchanged)"""
    return Chain(kind, shape, dt)


def test_the_smallest_shapes_are_the_smallest_the_plans_accept():
    import ctypes as C
    lib = L.lib()
    for H, W, ok in ((32, 32, True), (31, 32, False), (32, 31, False)):
        assert (lib.ecgmm_resnet18_infer_workspace(C.byref(L.ResNet18Desc(1, H, W, 16, L.F32, 0, 0.1, 1e-5))) > 0) == ok
    for Ln, ok in ((64, True), (63, False)):
        assert (lib.ecgmm_resnet1d_infer_workspace(C.byref(L.ResNet1DDesc(1, 1, Ln, 5, L.F32, 0, 0.1, 1e-5, 0.0, 0, 0))) > 0) == ok


@pytest.mark.parametrize("kind,shape,dt", CASES, ids=ids(CASES))
def test_every_chain_tensor_against_float64(kind, shape, dt):
    """(a)"""
    ch = chain(kind, shape, dt)
    assert bool(torch.isfinite(ch.feat).all())
    rep = check_chain(ch)
    print("CHAIN %s %s %s: " % (kind, shape, NAME[dt]) + ", ".join("%s %.3g" % kv for kv in sorted(rep.worst.items())))
    want = {"stem", "relu_maxpool", "conv", "avgpool", "linear"} | ({"se_mlp", "gate_res_relu"} if kind == "r1d" else set())
    assert set(rep.worst) == want


PLAN_CASES = [(k, s, dt, side) for k, s, dt in CASES for side in ((0, 1) if k == "r18" else (None,))]


PLAN_IDS = [i + ("" if c[3] is None else "-side%d" % c[3]) for i, c in zip(ids([c[:3] for c in PLAN_CASES]), PLAN_CASES)]


@pytest.mark.parametrize("kind,shape,dt,side", PLAN_CASES, ids=PLAN_IDS)
def test_plan_features_equal_the_chain_bit_for_bit(kind, shape, dt, side):
    """(b)"""
    ch = chain(kind, shape, dt)
    sw = {} if side is None else {"ECGMM_INFER_DOWN_SIDE": side}
    with switches(L.lib(), **sw):
        feat = ch.plan()
    assert bool(torch.isfinite(feat).all()), "the plan left NaN in its features"
    diff = (feat.double() - ch.feat.double()).abs().max()
    assert same_bits(feat, ch.feat), "plan and chain differ: max |difference| %.3g of max |feature| %.3g" % (
        float(diff), float(ch.feat.abs().max()))


LIVE_CASES = [c for c in CASES if c[1] == SHAPES[c[0]][0]]


@pytest.mark.parametrize("kind,shape,dt", LIVE_CASES, ids=ids(LIVE_CASES))
def test_one_folded_bias_element_changes_the_features(kind, shape, dt):
    """(c) the comparison of (b) is not vacuous: block 1's folded conv2 bias, one channel moved by 1"""
    ch = chain(kind, shape, dt)
    b = ch.W[("b2", 1)]
    old = b[3].clone()
    try:
        b[3] = old.abs() + 1.0
        T, feat = ch.run()
    finally:
        b[3] = old
    assert bool(torch.isfinite(feat).all())
    assert not same_bits(T[("out", 1)], ch.T[("out", 1)]) and not same_bits(feat, ch.feat)
    assert same_bits(T[("a1", 1)], ch.T[("a1", 1)])          # (nothing before that bias moved)


@pytest.mark.parametrize("kind,shape,dt", BATCH_CASES, ids=ids(BATCH_CASES))
def test_one_blob_serves_two_batch_sizes_with_the_same_bits(kind, shape, dt):
    """(d)"""
    ch = chain(kind, shape, dt)
    full = ch.plan()
    one = ch.plan(1, blob=ch.blob)
    assert same_bits(one[0], full[0]), "sample 0 alone and in the batch differ by %.3g" % float((one[0] - full[0]).abs().max())
