"""The dual BatchNorm backward (csrc/elementwise.hip: bn_bwd_dual_kernel, ecg_bn_bwd_dual): bn2 and the shortcut BatchNorm of a
ResNet18 downsample block differentiate the same masked gradient dz = [out > 0] * dcur, and one reduce + one apply pass serve
both instead of a pass pair each.

Per op, through ecgmm_bn_bwd_dual, against the two separate calls it replaces (ecgmm_bn_bwd_bits / ecgmm_bn_bwd with dz_out,
then ecgmm_bn_bwd of that dz with the second BatchNorm's operands), every output NaN-filled before each call:
(a) dz, dy_a, dy_b, both (dgamma, dbeta) pairs and both sets of partial rows are bit-identical -- with the finalize folded
    into the apply pass (sliced at C >= 256), folded unsliced, and as separate finalize launches;
(b) dy_a, dy_b, dz and the four parameter gradients are checked element by element against float64 with the checkers and
    constants of tests/f64check.py, as tests/test_bn_fold_slice_gpu.py uses them.
Shapes (M, C): (4099, 64) -- M prime, a ragged last iteration, the unsliced fold; (1030, 128); (777, 256) and (197, 512) --
the sliced fold, fewer rows than the grid.  Each in bf16 with the bit mask, in bf16 with a mask tensor and in fp32.  In each
BatchNorm one channel has a negative gamma, and one channel is masked everywhere.

Through the plan: ecgmm_resnet18_backward at N = 2, 64 x 64 (the smallest geometry with the three downsample blocks), one
stage per call and as one call, with ecgmm_bn_dual(0) and (1): every gradient, the input gradient and dz / dy / dyd after
every stage have the same bits.
"""
import ctypes as C

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from .test_plan_replay_gpu import Plan
from .util import DEV, TDT, dev, switches

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64
SHAPES = [(4099, 64), (1030, 128), (777, 256), (197, 512)]
MODES = ["bf16-bits", "bf16-maskref", "fp32"]
FOLDS = {"sliced": dict(ECGMM_BN_FOLD=1, ECGMM_BN_FOLD_SLICE=1), "unsliced": dict(ECGMM_BN_FOLD=1, ECGMM_BN_FOLD_SLICE=0),
         "finalize": dict(ECGMM_BN_FOLD=0)}


def nanbuf(n, dtype=torch.float32):
    return torch.full((n,) if isinstance(n, int) else n, NAN, device=DEV, dtype=dtype)


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits_of(a) == bits_of(b)).all())


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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,Cn", SHAPES)
def test_dual_op_matches_the_two_separate_calls_and_float64(M, Cn, mode):
    lib = L.lib()
    bf16 = mode != "fp32"
    dt = L.BF16 if bf16 else L.F32
    vec = 8 if bf16 else 4
    d = F64.bn_inputs(M, Cn, bf16)
    g = {k: dev(v) for k, v in d.items() if torch.is_tensor(v)}
    ya, yb, dout = g["y"], g["res"], g["dout"]             # two conv outputs, one incoming gradient (bf16-rounded for bf16)
    gam = [g["gamma"].clone(), g["rscale"].clone()]
    bet = [g["beta"], g["rshift"]]
    gam[0][3], gam[1][Cn - 2] = -gam[0][3], -gam[1][Cn - 2]          # a negative gamma in each BatchNorm
    coef = [forward_coef(lib, y, gam[b], bet[b], M, Cn) for b, y in enumerate((ya, yb))]
    ya_t, yb_t, dout_t = (t.to(TDT[dt]).contiguous() for t in (ya, yb, dout))
    # the ReLU'd block output as the mask reference; channel 5 is masked everywhere
    maskt = nanbuf(M * Cn, TDT[dt])
    L.check(lib.ecgmm_bn_act(dt, ptr(ya_t), ptr(coef[0]), ptr(yb_t), None, None, 1, 1, ptr(maskt), M, Cn, stream()))
    torch.cuda.synchronize()
    maskt.view(M, Cn)[:, 5] = 0
    mbits = None
    if mode == "bf16-bits":
        w = 1 << torch.arange(8, device=DEV, dtype=torch.int32)
        mbits = ((maskt.view(M, Cn // 8, 8).float() > 0).int() * w).sum(2).to(torch.uint8).view(-1).contiguous()
    share = float((maskt.float() > 0).double().mean())
    assert 0.2 < share < 0.8, share                                    # the mask really masks
    n1 = lib.ecgmm_bn_bwd_scratch(dt, M, Cn) // 4
    brows = (n1 - 3 * Cn) // (2 * Cn) - TAIL                           # the grid of the reduce pass = its partial rows
    K = F64.chain_len(M, brows, Cn, vec, 1024)

    def outputs():
        return dict(dz=nanbuf(M * Cn, TDT[dt]), dy=[nanbuf(M * Cn, TDT[dt]) for _ in range(2)], dgamma=[nanbuf(Cn), nanbuf(Cn)],
                    dbeta=[nanbuf(Cn), nanbuf(Cn)])

    def separate():
        o = outputs()
        sc = [nanbuf(n1), nanbuf(n1)]
        if mbits is not None:
            L.check(lib.ecgmm_bn_bwd_bits(dt, ptr(dout_t), ptr(mbits), None, None, 1, ptr(ya_t), ptr(coef[0]), ptr(gam[0]),
                                          ptr(o["dgamma"][0]), ptr(o["dbeta"][0]), ptr(o["dy"][0]), ptr(o["dz"]), None, M, Cn,
                                          ptr(sc[0]), stream()))
        else:
            L.check(lib.ecgmm_bn_bwd(dt, ptr(dout_t), ptr(maskt), None, None, 1, ptr(ya_t), ptr(coef[0]), ptr(gam[0]),
                                     ptr(o["dgamma"][0]), ptr(o["dbeta"][0]), ptr(o["dy"][0]), ptr(o["dz"]), None, M, Cn,
                                     ptr(sc[0]), stream()))
        L.check(lib.ecgmm_bn_bwd(dt, ptr(o["dz"]), None, None, None, 1, ptr(yb_t), ptr(coef[1]), ptr(gam[1]), ptr(o["dgamma"][1]),
                                 ptr(o["dbeta"][1]), ptr(o["dy"][1]), None, None, M, Cn, ptr(sc[1]), stream()))
        torch.cuda.synchronize()
        o["rows"] = [s[:brows * 2 * Cn] for s in sc]
        return o

    def dual(**extra):
        o = outputs()
        sc = [nanbuf(n1), nanbuf(n1)]                                   # one scratch per BatchNorm, each the single form's size
        a = dict(gate=None, addc=None, dbias=None)
        a.update(extra)
        rc = lib.ecgmm_bn_bwd_dual(dt, ptr(dout_t), None if mbits is not None else ptr(maskt), None if mbits is None else ptr(mbits),
                                   a["gate"], a["addc"], ptr(ya_t), ptr(coef[0]), ptr(gam[0]), ptr(o["dgamma"][0]), ptr(o["dbeta"][0]),
                                   ptr(o["dy"][0]), ptr(yb_t), ptr(coef[1]), ptr(gam[1]), ptr(o["dgamma"][1]), ptr(o["dbeta"][1]),
                                   ptr(o["dy"][1]), ptr(o["dz"]), a["dbias"], M, Cn, ptr(sc[0]), ptr(sc[1]), stream())
        torch.cuda.synchronize()
        o["rows"] = [s[:brows * 2 * Cn] for s in sc]
        return rc, o

    for fold, sw in FOLDS.items():
        if fold == "unsliced" and Cn < 256:
            continue                                                    # (slicing applies from C = 256)
        with switches(lib, **sw):
            ref = separate()
            rc, got = dual()
        L.check(rc, "bn_bwd_dual")
        assert same_bits(got["dz"], ref["dz"]), "%s: dz differs" % fold                                                  # (a)
        for b in range(2):
            for k in ("dy", "dgamma", "dbeta", "rows"):
                assert torch.isfinite(got[k][b].float()).all(), "%s: %s[%d] not written everywhere" % (fold, k, b)
                assert same_bits(got[k][b], ref[k][b]), "%s: %s[%d] differs from the separate calls" % (fold, k, b)
        if fold != "sliced":
            continue
        F64.check_bn_bwd(dout, ya, coef[0], gam[0], bf16, K, got["dgamma"][0], got["dbeta"][0], got["dy"][0].view(M, Cn),          # (b)
                         got["dz"].view(M, Cn), maskref=maskt.view(M, Cn), name="dual bn_bwd a " + mode)
        F64.check_bn_bwd(got["dz"].view(M, Cn).float(), yb, coef[1], gam[1], bf16, K, got["dgamma"][1], got["dbeta"][1],
                         got["dy"][1].view(M, Cn), name="dual bn_bwd b " + mode)
        assert bool((got["dz"].view(M, Cn)[:, 5].float() == 0).all())
    # what the dual form does not take
    one = torch.ones(Cn, device=DEV)
    for kw in ("gate", "addc", "dbias"):
        rc, _ = dual(**{kw: ptr(one)})
        assert rc == 1 and b"bn_bwd_dual" in lib.ecgmm_last_error(), kw


def run_plan(lib, dt, on):
    """the staged backward and the one-call backward with the switch as given: {name: bits} of everything compared"""
    L.check(lib.ecgmm_bn_dual(on))
    try:
        plan = Plan("r18", (2, 3, 64, 64), dt)
        plan.forward()
        out = {}
        plan.fill_backward()
        for st in range(plan.net.n_stages):
            plan.backward(st, st + 1)
            for n, idx in (("dz", (0,)), ("dy", (0, 1)), ("dyd", (0, 1))):
                for i in idx:
                    out["stage %d %s[%d]" % (st, n, i)] = plan.raw(1, n, i).clone()
            for n, gr in plan.grads().items():
                if bool(torch.isfinite(gr).all()):
                    out["staged g:" + n] = gr.view(torch.int32).clone()
            if st == plan.net.n_stages - 1:
                out["staged dx"] = plan.arena.views["dx"].view(torch.int32).clone()
            plan.fill_backward(keep=st & 1)      # 0xFF over every named tensor but the X buffer the next stage reads
        plan.fill_backward()
        plan.backward(0, plan.net.n_stages)
        for n, gr in plan.grads().items():
            assert bool(torch.isfinite(gr).all()), n
            out["whole g:" + n] = gr.view(torch.int32).clone()
        out["whole dx"] = plan.arena.views["dx"].view(torch.int32).clone()
        down = [k.i for k in plan.net.blocks if k.down]
        return out, down
    finally:
        L.check(lib.ecgmm_bn_dual(1))


@pytest.mark.parametrize("dt", [L.BF16, L.F32], ids=["bf16", "fp32"])
def test_resnet18_backward_has_the_same_bits_with_the_dual_pass_off_and_on(dt):
    lib = L.lib()
    off, down = run_plan(lib, dt, 0)
    on, _ = run_plan(lib, dt, 1)
    assert down == [2, 4, 6]
    assert sorted(on) == sorted(off) and len([k for k in on if k.startswith("staged g:")]) == L.RESNET18_NPARAMS
    for k in sorted(on):
        assert torch.equal(on[k], off[k]), "%s differs between ecgmm_bn_dual(0) and (1)" % k
    # the downsample blocks wrote dz, dy and dyd in their stage (blocks 6, 4, 2 = stages 2, 4, 6; buffer st & 1)
    for st in (2, 4, 6):
        for n in ("dz[0]", "dy[%d]" % (st & 1), "dyd[%d]" % (st & 1)):
            t = on["stage %d %s" % (st, n)]
            assert not bool((t == 0xFF).all()), "stage %d left %s unwritten" % (st, n)
