"""The element-wise passes that issue every load of a trip before the first wait (csrc/elementwise.hip): the fused
BatchNorm + ReLU + max-pool forward (two outputs per thread from a 3 x 5 window) and the merged SE / BatchNorm backward's
first pass (four rows in flight per thread); and the masked BatchNorm backward (single and dual), whose form with the mask
operand loaded early was measured and not kept -- its cases test the kernels as they are.  What batching
the loads can get wrong is tested here, on shapes small enough for well under a second per case; the step's shapes, the
float64 element-by-element checks and the plan replays are in the files that were there before.

Max-pool (ecgmm_bnrelu_maxpool, C = 64, bf16 and fp32, [N, H, W] = (2, 7, 9), (1, 8, 8), (1, 1, 37) -- the 1-D form -- and
(1, 2, 3)).  A tap outside the image is now LOADED, from coordinates clamped into the image, and taken out of the running
afterwards; a clamped duplicate carries an earlier tap code and would steal ties.  So:
(a) every element equal, positive scale: every tap ties, and the argmax byte must be exactly the earliest tap inside the image
    -- 4 at the top-left output, 3 along the top edge, 1 along the left edge, 0 in the interior; for H == 1: 4 at the left
    end, 3 elsewhere -- and the pooled value the library's own BN + ReLU of the element;
(b) the same with every input negative after BN: the ReLU gives 0 everywhere, pooled value 0, same argmax rule;
(c) equal input, gamma negative in every other channel: both kinds of channel in one 16-byte chunk, same rule;
(d) random input (a negative gamma in every fourth channel): the pooled value has the bits of the BN + ReLU value AS STORED
    (ecgmm_bn_act, ReLU on, of the same tensor) of the tap the argmax byte names; that tap lies inside the image and holds the
    window's maximum; no earlier in-image tap holds an equal value.  All exact, no tolerance.
(e) two outputs per thread: OW is odd at (2, 7, 9) (OW = 5) and (1, 1, 37) (OW = 19), where the last thread of a row has one
    output, and even at the other two; every case above runs at all four shapes.

Masked BatchNorm backward, (M, C) = (98, 512), (300, 64), (1, 128): ragged against the rows per iteration, a last partial
trip, a single row; with the finalize folded into the apply pass and as a launch of its own (ECGMM_BN_FOLD):
  * ecgmm_bn_bwd_bits and ecgmm_bn_bwd with the same mask as a tensor give identical dy, dz, dgamma, dbeta and partial rows
    -- with dz_out (the reduce pass stores dz, the apply pass reads it back) and without (the apply pass masks, too);
  * ecgmm_bn_bwd_dual gives the bits of the two separate calls, with the bit mask, with the mask tensor and in fp32;
  * one float64 comparison per shape (tests/f64check.py: check_bn_bwd, its bounds unchanged).
The bits buffer holds exactly M * C / 8 bytes.

SE gate (ecgmm_se_gate_bn), N = 3, C in {64, 256}, R in {1, 5, 37} (row slices with no row, groups shorter than the four rows
kept in flight; C = 256 at R = 37 runs a full group and a remainder) and (C, R) = (64, 133), where the 64-channel form runs
a full group: dg has the bits of ecgmm_se_gate_grad's, dz is exactly the masked gradient, and the per-sample sums against
float64 within the bound of an fp32 sum taken in any order (f64check.check_plain: |got - ref| <= g_k(K) * A):
  a1 = sum_r dz              K = R             A = sum_r |dz|
  a2 = sum_r dz * (y - mu)   K = R + 2         A = sum_r |dz| (|y| + |mu|)     (the difference, the product, R in the sum)
  a3 = sum_r (y - mu)        K = R + 1         A = sum_r (|y| + |mu|)
"""
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from oracle import fill

from . import f64check as F64
from .util import DEV, TDT, dev, switches

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64


def nanbuf(n, dtype=torch.float32):
    return torch.full((n,) if isinstance(n, int) else n, NAN, device=DEV, dtype=dtype)


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits_of(a) == bits_of(b)).all())


# ---------------------------------------------------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 7, 9), (1, 8, 8), (1, 1, 37), (1, 2, 3)]
POOL_C = 64


def earliest_tap(N, H, W):
    """[N][OH][OW]: the first tap (kh * 3 + kw) of each 3x3 / stride 2 / pad 1 window that lies inside the image"""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    kh = (torch.arange(OH) == 0).long()          # row -1 is outside: the window of output row 0 starts at kh = 1
    kw = (torch.arange(OW) == 0).long()
    return (kh[:, None] * 3 + kw[None, :]).expand(N, OH, OW)


def run_pool(lib, dt, y, coef, N, H, W):
    """y [N][H][W][C] fp32 on the CPU (bf16-rounded for bf16) -> pooled, idx [N][OH][OW][C] and the library's own
    BN + ReLU of y as stored [N][H][W][C], all on the GPU, outputs NaN- / 0xFF-filled first"""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    yt = dev(y).to(TDT[dt]).contiguous()
    cg = dev(coef)
    pooled = nanbuf((N, OH, OW, POOL_C), TDT[dt])
    idx = torch.full((N, OH, OW, POOL_C), 255, device=DEV, dtype=torch.uint8)
    act = nanbuf((N, H, W, POOL_C), TDT[dt])
    L.check(lib.ecgmm_bnrelu_maxpool(dt, ptr(yt), ptr(cg), ptr(pooled), ptr(idx), N, H, W, POOL_C, stream()))
    L.check(lib.ecgmm_bn_act(dt, ptr(yt), ptr(cg), None, None, None, 1, 1, ptr(act), N * H * W, POOL_C, stream()))
    torch.cuda.synchronize()
    return pooled, idx, act


def pool_coef(scale, shift):
    coef = torch.zeros(4, POOL_C)
    coef[0], coef[1], coef[3] = scale, shift, 1.0
    return coef


@pytest.mark.parametrize("case", ["equal-positive", "equal-negative", "negative-gamma"])
@pytest.mark.parametrize("N,H,W", POOL_SHAPES)
@pytest.mark.parametrize("dt", [L.BF16, L.F32], ids=["bf16", "fp32"])
def test_maxpool_all_taps_tie_earliest_in_image_tap_wins(dt, N, H, W, case):
    lib = L.lib()
    y = torch.full((N, H, W, POOL_C), 1.5)
    scale = 1 + 0.25 * fill.hash_tensor((POOL_C,), 71).abs()
    shift = torch.full((POOL_C,), 0.125)
    if case == "equal-negative":
        shift = -4 * scale                                   # 1.5 * scale - 4 * scale < 0 in every channel
    elif case == "negative-gamma":
        scale = scale * (1 - 2 * (torch.arange(POOL_C) % 2).float())     # odd channels: 0.125 - 1.5 |scale| < 0
    pooled, idx, act = run_pool(lib, dt, y, pool_coef(scale, shift), N, H, W)
    want = earliest_tap(N, H, W).to(DEV)[..., None].expand_as(idx)
    assert bool((idx.long() == want).all()), "argmax bytes: %s" % idx[0, :, :, 0].tolist()
    val = act[0, 0, 0]                                       # [C]: the BN + ReLU value of the one element, as stored
    dead = {"equal-positive": torch.zeros(POOL_C, dtype=torch.bool), "equal-negative": torch.ones(POOL_C, dtype=torch.bool),
            "negative-gamma": torch.arange(POOL_C) % 2 == 1}[case].to(DEV)
    assert bool(((val.float() == 0) == dead).all())
    assert bool((val.float()[~dead] > 0).all())
    assert bool((pooled.float() == val.float().expand_as(pooled)).all())
    assert same_bits(pooled[..., ~dead], val[~dead].expand_as(pooled[..., ~dead]).contiguous())


@pytest.mark.parametrize("N,H,W", POOL_SHAPES)
@pytest.mark.parametrize("dt", [L.BF16, L.F32], ids=["bf16", "fp32"])
def test_maxpool_random_value_is_the_named_taps_and_no_earlier_tap_ties(dt, N, H, W):
    lib = L.lib()
    bf16 = dt == L.BF16
    y = fill.hash_tensor((N, H, W, POOL_C), 72, 2.0)
    if bf16:
        # a coarse grid: many exact ties between the taps of a window, in bf16 and after the affine map
        y = (y * 4).round() / 4
    scale = 1 + 0.25 * fill.hash_tensor((POOL_C,), 73)
    scale = scale * (1 - 2 * (torch.arange(POOL_C) % 4 == 3).float())    # a negative gamma in every fourth channel
    shift = 0.1 * fill.hash_tensor((POOL_C,), 74) - 0.3
    pooled, idx, act = run_pool(lib, dt, y, pool_coef(scale, shift), N, H, W)
    a = act.double()
    T = F64.pool_taps(a, float("-inf"))                      # [N][OH][OW][9][C], -inf outside the image
    ix = idx.long()
    assert bool((ix < (6 if H == 1 else 9)).all()) and (H > 1 or bool((ix >= 3).all()))
    sel = T.gather(3, ix.unsqueeze(3)).squeeze(3)
    assert bool(torch.isfinite(sel).all()), "an argmax byte names a tap outside the image"
    mx = T.amax(3)
    assert bool((sel == mx).all()), "the named tap does not hold the window's maximum"
    first = (T == mx.unsqueeze(3)).double().argmax(3)
    assert bool((ix == first).all()), "%d windows: an earlier in-image tap holds an equal value" % int((ix != first).sum())
    assert bool((pooled.double() == sel).all())
    nz = sel != 0                                            # (+0 and -0 are the same stored activation for the ReLU)
    assert bool((bits_of(pooled)[nz] == bits_of(sel.to(TDT[dt]))[nz]).all())
    ties = int(((T == mx.unsqueeze(3)).sum(3) > 1).sum())
    assert ties > 0, "the input has no window with two equal maxima"
    print("windows x channels with tied maxima: %d of %d" % (ties, mx.numel()))


# ---------------------------------------------------------------------------------------------------------------------
# masked BatchNorm backward
# ---------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(98, 512), (300, 64), (1, 128)]
FOLDS = {"fold": dict(ECGMM_BN_FOLD=1), "finalize": dict(ECGMM_BN_FOLD=0)}


def stat_rows(y64, rows=7):
    """[M][C] float64 -> fp32 statistics rows [rows + TAIL][2][C] of (sum y, sum y^2), as a producer writes them"""
    M, Cn = y64.shape
    k = torch.arange(M, device=y64.device) % rows
    part = torch.zeros(rows, 2, Cn, dtype=torch.float64, device=y64.device)
    part[:, 0].index_add_(0, k, y64)
    part[:, 1].index_add_(0, k, y64 * y64)
    return torch.cat([part.float(), nanbuf((TAIL, 2, Cn))]).contiguous()


def forward_coef(lib, y, gamma, beta, M, Cn):
    coef = nanbuf((4, Cn))
    L.check(lib.ecgmm_bn_finalize(ptr(stat_rows(y.double())), 7, Cn, float(M), ptr(gamma), ptr(beta), None, None, None, 0.1, 1e-5,
                                  ptr(coef), stream()))
    return coef


class BwdCase:
    """operands of one masked BatchNorm backward (and of the dual form: a second BatchNorm on yb), mask as tensor and bits"""

    def __init__(self, lib, M, Cn, bf16):
        self.M, self.Cn, self.bf16 = M, Cn, bf16
        self.dt = dt = L.BF16 if bf16 else L.F32
        d = F64.bn_inputs(M, Cn, bf16)
        g = {k: dev(v) for k, v in d.items() if torch.is_tensor(v)}
        self.ya, self.yb, self.dout = g["y"], g["res"], g["dout"]
        self.gam = [g["gamma"].clone(), g["rscale"].clone()]
        self.gam[0][3] = -self.gam[0][3]                     # a negative gamma
        bet = [g["beta"], g["rshift"]]
        self.coef = [forward_coef(lib, y, self.gam[b], bet[b], M, Cn) for b, y in enumerate((self.ya, self.yb))]
        self.ya_t, self.yb_t, self.dout_t = (t.to(TDT[dt]).contiguous() for t in (self.ya, self.yb, self.dout))
        # the ReLU'd block output as the mask reference (with one row the BatchNorm output is beta: the hash tensor instead)
        self.maskt = nanbuf(M * Cn, TDT[dt])
        if M > 1:
            L.check(lib.ecgmm_bn_act(dt, ptr(self.ya_t), ptr(self.coef[0]), ptr(self.yb_t), None, None, 1, 1, ptr(self.maskt), M, Cn,
                                     stream()))
            torch.cuda.synchronize()
        else:
            self.maskt = dev(fill.hash_tensor((M * Cn,), 75)).clamp_min(0).to(TDT[dt]).contiguous()
        self.maskt.view(M, Cn)[:, 5] = 0                     # channel 5 is masked everywhere
        share = float((self.maskt.float() > 0).double().mean())
        assert 0.2 < share < 0.8, share                      # the mask really masks
        self.mbits = None
        if bf16:
            w = 1 << torch.arange(8, device=DEV, dtype=torch.int32)
            self.mbits = ((self.maskt.view(M, Cn // 8, 8).float() > 0).int() * w).sum(2).to(torch.uint8).view(-1).contiguous()
            assert self.mbits.numel() * 8 == M * Cn          # exactly M * C / 8 bytes: no slack behind the last row's byte
        self.n1 = lib.ecgmm_bn_bwd_scratch(dt, M, Cn) // 4
        self.brows = (self.n1 - 3 * Cn) // (2 * Cn) - TAIL   # the grid of the reduce pass = its partial rows
        self.K = F64.chain_len(M, self.brows, Cn, 8 if bf16 else 4, 1024)

    def single(self, lib, bits, want_dz):
        """ecgmm_bn_bwd_bits / ecgmm_bn_bwd (mask tensor) of the first BatchNorm; every output NaN-filled first"""
        M, Cn, dt = self.M, self.Cn, self.dt
        o = dict(dy=nanbuf(M * Cn, TDT[dt]), dz=nanbuf(M * Cn, TDT[dt]) if want_dz else None, dgamma=nanbuf(Cn), dbeta=nanbuf(Cn))
        sc = nanbuf(self.n1)
        fn = lib.ecgmm_bn_bwd_bits if bits else lib.ecgmm_bn_bwd
        L.check(fn(dt, ptr(self.dout_t), ptr(self.mbits if bits else self.maskt), None, None, 1, ptr(self.ya_t), ptr(self.coef[0]),
                   ptr(self.gam[0]), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o["dy"]), ptr(o["dz"]) if want_dz else None, None, M, Cn,
                   ptr(sc), stream()))
        torch.cuda.synchronize()
        o["rows"] = sc[:self.brows * 2 * Cn]
        return o

    def separate(self, lib, bits):
        o = self.single(lib, bits, True)
        M, Cn, dt = self.M, self.Cn, self.dt
        o2 = dict(dy=nanbuf(M * Cn, TDT[dt]), dgamma=nanbuf(Cn), dbeta=nanbuf(Cn))
        sc = nanbuf(self.n1)
        L.check(lib.ecgmm_bn_bwd(dt, ptr(o["dz"]), None, None, None, 1, ptr(self.yb_t), ptr(self.coef[1]), ptr(self.gam[1]),
                                 ptr(o2["dgamma"]), ptr(o2["dbeta"]), ptr(o2["dy"]), None, None, M, Cn, ptr(sc), stream()))
        torch.cuda.synchronize()
        o2["rows"] = sc[:self.brows * 2 * Cn]
        return o, o2

    def dual(self, lib, bits):
        M, Cn, dt = self.M, self.Cn, self.dt
        o = [dict(dy=nanbuf(M * Cn, TDT[dt]), dgamma=nanbuf(Cn), dbeta=nanbuf(Cn)) for _ in range(2)]
        o[0]["dz"] = nanbuf(M * Cn, TDT[dt])
        sc = [nanbuf(self.n1), nanbuf(self.n1)]
        L.check(lib.ecgmm_bn_bwd_dual(dt, ptr(self.dout_t), None if bits else ptr(self.maskt), ptr(self.mbits) if bits else None, None,
                                      None, ptr(self.ya_t), ptr(self.coef[0]), ptr(self.gam[0]), ptr(o[0]["dgamma"]), ptr(o[0]["dbeta"]),
                                      ptr(o[0]["dy"]), ptr(self.yb_t), ptr(self.coef[1]), ptr(self.gam[1]), ptr(o[1]["dgamma"]),
                                      ptr(o[1]["dbeta"]), ptr(o[1]["dy"]), ptr(o[0]["dz"]), None, M, Cn, ptr(sc[0]), ptr(sc[1]), stream()),
                "bn_bwd_dual")
        torch.cuda.synchronize()
        for b in range(2):
            o[b]["rows"] = sc[b][:self.brows * 2 * Cn]
        return o


def assert_same(got, ref, what):
    for k, v in ref.items():
        if v is None:
            continue
        assert torch.isfinite(got[k].float()).all(), "%s: %s not written everywhere" % (what, k)
        assert same_bits(got[k], v), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("fold", list(FOLDS))
@pytest.mark.parametrize("M,Cn", BWD_SHAPES)
def test_bn_bwd_bit_mask_and_mask_tensor_give_the_same_bits(M, Cn, fold):
    lib = L.lib()
    c = BwdCase(lib, M, Cn, True)
    with switches(lib, **FOLDS[fold]):
        for want_dz in (True, False):
            ref = c.single(lib, False, want_dz)
            got = c.single(lib, True, want_dz)
            assert_same(got, ref, "%s, dz_out %s" % (fold, want_dz))
            if want_dz:
                assert bool((got["dz"].view(M, Cn)[:, 5].float() == 0).all())
            else:
                with_dz = c.single(lib, True, True)                      # the apply pass masking itself: the same dy
                assert same_bits(got["dy"], with_dz["dy"]), "%s: dy differs between the masking and the dz-reading apply pass" % fold
    if fold == "fold":
        F64.check_bn_bwd(c.dout, c.ya, c.coef[0], c.gam[0], True, c.K, got["dgamma"], got["dbeta"], got["dy"].view(M, Cn),
                         with_dz["dz"].view(M, Cn), maskref=c.maskt.view(M, Cn), name="bn_bwd bits (%d, %d)" % (M, Cn))


@pytest.mark.parametrize("fold", list(FOLDS))
@pytest.mark.parametrize("mode", ["bf16-bits", "bf16-maskref", "fp32"])
@pytest.mark.parametrize("M,Cn", BWD_SHAPES)
def test_bn_bwd_dual_gives_the_bits_of_the_separate_calls(M, Cn, mode, fold):
    lib = L.lib()
    c = BwdCase(lib, M, Cn, mode != "fp32")
    bits = mode == "bf16-bits"
    with switches(lib, **FOLDS[fold]):
        ref = c.separate(lib, bits)
        got = c.dual(lib, bits)
    for b in range(2):
        assert_same(got[b], ref[b], "%s %s BatchNorm %d" % (mode, fold, b))
    if fold == "fold" and mode != "bf16-bits":               # (the bit-mask form has its float64 comparison above)
        F64.check_bn_bwd(c.dout, c.ya, c.coef[0], c.gam[0], c.bf16, c.K, got[0]["dgamma"], got[0]["dbeta"], got[0]["dy"].view(M, Cn),
                         got[0]["dz"].view(M, Cn), maskref=c.maskt.view(M, Cn), name="dual a %s (%d, %d)" % (mode, M, Cn))
        F64.check_bn_bwd(got[0]["dz"].view(M, Cn).float(), c.yb, c.coef[1], c.gam[1], c.bf16, c.K, got[1]["dgamma"], got[1]["dbeta"],
                         got[1]["dy"].view(M, Cn), name="dual b %s (%d, %d)" % (mode, M, Cn))


# ---------------------------------------------------------------------------------------------------------------------
# SE gate
# ---------------------------------------------------------------------------------------------------------------------
SE_CASES = [(Cn, R) for Cn in (64, 256) for R in (1, 5, 37)] + [(64, 133)]


@pytest.mark.parametrize("Cn,R", SE_CASES)
@pytest.mark.parametrize("dt", [L.BF16, L.F32], ids=["bf16", "fp32"])
def test_se_gate_bn_matches_se_gate_grad_and_float64(dt, Cn, R):
    lib = L.lib()
    N = 3
    bf16 = dt == L.BF16
    h = fill.hash_tensor
    dout, mref, y = h((N, R, Cn), 81), h((N, R, Cn), 82), h((N, R, Cn), 83, 2.0) + 0.5
    if bf16:
        dout, mref, y = (t.to(torch.bfloat16).float() for t in (dout, mref, y))
    mref[:, :, 5] = -1.0                                     # channel 5 is masked everywhere
    coef = torch.zeros(4, Cn)
    coef[0], coef[1], coef[2], coef[3] = 1 + 0.1 * h((Cn,), 84), 0.1 * h((Cn,), 85), 0.5 + 0.2 * h((Cn,), 86), 1.0
    dg_, mg_, yg_, cg = (dev(t) for t in (dout, mref, y, coef))
    dout_t, mref_t, y_t = (t.to(TDT[dt]).contiguous() for t in (dg_, mg_, yg_))
    dg_ref, dg, a1, a2, a3 = (nanbuf((N, Cn)) for _ in range(5))
    dz = nanbuf((N, R, Cn), TDT[dt])
    L.check(lib.ecgmm_se_gate_grad(dt, ptr(dout_t), ptr(mref_t), ptr(y_t), ptr(cg), ptr(dg_ref), N, R, Cn, stream()))
    L.check(lib.ecgmm_se_gate_bn(dt, ptr(dout_t), ptr(mref_t), ptr(y_t), ptr(cg), ptr(dz), ptr(dg), ptr(a1), ptr(a2), ptr(a3), N, R, Cn,
                                 stream()))
    torch.cuda.synchronize()
    for n, t in (("dg", dg), ("a1", a1), ("a2", a2), ("a3", a3), ("dz", dz)):
        assert torch.isfinite(t.float()).all(), n + " not written everywhere"
    assert same_bits(dg, dg_ref), "dg differs from ecgmm_se_gate_grad's"
    mask = mg_ > 0
    d64, y64, mu = dg_.double(), yg_.double(), cg[2].double()
    z64 = torch.where(mask, d64, torch.zeros_like(d64))
    assert bool((dz.double() == z64).all()), "dz is not the masked gradient"
    assert bool((dz[:, :, 5].float() == 0).all())
    F64.check_se_gate_grad(dg, dg_, mask, yg_, cg[0], cg[1], "se_gate_bn dg")
    yc, Ayc = y64 - mu, y64.abs() + mu.abs()
    F64.check_plain(a1, z64.sum(1), z64.abs().sum(1), R, "se_gate_bn a1")
    F64.check_plain(a2, (z64 * yc).sum(1), (z64.abs() * Ayc).sum(1), R + 2, "se_gate_bn a2")
    F64.check_plain(a3, yc.sum(1), Ayc.sum(1), R + 1, "se_gate_bn a3")
