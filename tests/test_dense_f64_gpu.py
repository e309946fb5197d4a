"""The fp32 dense tails against float64: Linear on its three routes (dense16 MFMA tiles, implicit GEMM, VALU), the
squeeze-excite MLP kernels, the fused head and its per-op fallback, LayerNorm, attention fusion, var_loss, cross-entropy /
focal loss and Adam, at the smallest shapes that reach each edge of their launch geometry: K % 64 != 0 on dense16, the
8192-wave / 524288-element grid caps of the VALU Linear kernels, fewer rows than batch slices and the 4x-unrolled trip of
the SE weight-gradient kernel, a wave's second row in head_rows_bwd_kernel (B = 272) and layernorm_bwd_kernel (B = 1028),
partial 64-lane chunks, NC = 1 and 4, the 49 KB LDS limit of the head, the block-strided loop of ce_loss_kernel and the
scalar path of the Adam kernel.

Bounds and references: tests/f64check.py, "The fp32 dense tails" (the dot-product bound per element; the chain bar of
8 x torch's own CPU fp32 figure).  The C entry points are called through ctypes with every output, workspace and scratch
buffer NaN-filled first; LayerNorm, fusion and the losses go through hip/functional.py, the product path.  Each test prints
its figures (run with -s).

Measured on the MI355X (worst ratio to the bound / to the bar per test over its cases; 1 is the limit):
  Linear (dot-product bound): y 0.31 ((6, 4, 64)), dx 0.48 ((1040, 768, 2), K = 2), dw 0.31 ((1, 16, 16)), db 0.10; the dense16
    cases stay under 0.14; dz of the sigmoid from ecgmm_act_bwd 0.71 (of g_k(4) |ref|)
  SE MLP: h 0.014, g 0.26, ds 0.73 ((67, 1024, 64), of g_k(4) |ref|), dh 0.011, dm 0.45, dw1 0.30, dw2 0.32, db1 0.06, db2 0.14
  fused head (chain bar): 0.55 (d fc3.bias, (16, 3x256, 128, 2)), outputs <= 0.27, d raw <= 0.20, B = 272 cases <= 0.35,
    the 3x512 / NC = 4 limit 0.32, width 2 / NC = 1 0.17
  per-op fallback of the head: 0.47 at B = 24, 0.64 at B = 1028 (d signal_norm.weight: 4.0e-7 against torch fp32's 7.8e-8)
  LayerNorm 0.26 (dbeta, (1028, 100)); at (1, 2) dx is cancellation residue on both sides (4.5e-4 against 3.3e-4): 0.17
    (rows wider than 1024 run on the kernels' 24-values-per-lane instantiation: (2, 1025) 0.17, (5, 1536) 0.15, both dgamma)
  attention fusion + var_loss 0.36 (d weights, B = 1028);  cross-entropy 0.13, focal 0.20, cross_entropy_plus 0.13
  Adam 0.13 (vector path and scalar path alike)
No kernel broke a bound or the bar.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from oracle import fill, ref_models as O

from . import f64check as F64
from .util import DEV, dev, switch_get

pytestmark = pytest.mark.gpu
NAN = float("nan")
vp = C.c_void_p
ACT = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "sigmoid": L.ACT_SIGMOID}


def nanbuf(shape):
    return torch.full((shape,) if isinstance(shape, int) else tuple(shape), NAN, device=DEV, dtype=torch.float32)


def nanbytes(nbytes):
    """a NaN-filled fp32 buffer of at least nbytes"""
    return nanbuf(int(nbytes) // 4 + 64)


def table(ts):
    return (vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class Worst:
    def __init__(self, what):
        self.what, self.ratio, self.name = what, 0.0, "-"

    def __call__(self, r):
        if r.ratio >= self.ratio:
            self.ratio, self.name = r.ratio, r.name
        return r

    def show(self):
        print("WORST %-44s ratio %.3g  (%s)" % (self.what, self.ratio, self.name))


# ----------------------------------------------------------------------------------------------------------------------
# Linear
# ----------------------------------------------------------------------------------------------------------------------
def mfma_reduce_ok(k):
    """mirrors mfma_reduce_ok (csrc/linear.hip)"""
    return k % 4 == 0 and k >= 16


def dense16_ok(B, In, Out):
    """mirrors dense16_route (csrc/linear.hip) for 16-byte aligned buffers"""
    return B % 16 == 0 and In % 16 == 0 and Out % 16 == 0 and B * In * Out <= 134217728


def linear_routes(B, In, Out, act, dense16):
    """(forward, dgrad, wgrad) routes, as ecg_linear_fwd / ecg_linear_bwd decide them from the shape"""
    d16 = dense16 and dense16_ok(B, In, Out)
    fwd = "dense16" if d16 and act != "sigmoid" else ("igemm" if mfma_reduce_ok(In) and Out >= 16 and act != "sigmoid" else "valu")
    dgrad = "dense16" if d16 else ("igemm" if mfma_reduce_ok(Out) and In >= 16 else "valu")
    wgrad = "dense16" if d16 else ("igemm" if mfma_reduce_ok(In) and mfma_reduce_ok(Out) else "valu")
    return fwd, dgrad, wgrad


# what each case is here for: the routes (with ECGMM_DENSE16 on, act none) and a launch-geometry condition
LINEAR_REACHES = {
    (16, 16, 16): (("dense16",) * 3, lambda B, In, Out: In == Out == B == 16),
    (48, 80, 16): (("dense16",) * 3, lambda B, In, Out: (In % 64, B % 64, Out % 64) == (16, 48, 16)),
    (272, 672, 128): (("dense16",) * 3, lambda B, In, Out: In % 64 == 32),
    (17, 672, 128): (("igemm",) * 3, lambda B, In, Out: B % 16 != 0),
    (7, 96, 40): (("igemm",) * 3, lambda B, In, Out: Out % 16 != 0),
    (300, 10, 30): (("valu",) * 3, lambda B, In, Out: In % 4 != 0 and B * Out > 8192),
    (70, 300, 30): (("igemm", "valu", "valu"), lambda B, In, Out: Out * In + Out > 8192),
    (1040, 768, 2): (("valu", "valu", "valu"), lambda B, In, Out: B * In > 524288),
    (6, 4, 64): (("valu", "valu", "valu"), lambda B, In, Out: In < 16),
    (6, 64, 4): (("valu", "valu", "valu"), lambda B, In, Out: Out < 16),
    (1, 16, 16): (("igemm",) * 3, lambda B, In, Out: B == 1),
}
assert sorted(LINEAR_REACHES) == sorted(F64.LINEAR_CASES)


@pytest.mark.parametrize("act", list(ACT))
@pytest.mark.parametrize("shape", F64.LINEAR_CASES)
def test_linear_against_float64(shape, act):
    """ecgmm_linear_fwd (bias given and null) and ecgmm_linear_bwd (db given and null) on the pre-activation gradient
    ecgmm_act_bwd stored: y, dz, dx, dw, db element by element"""
    B, In, Out = shape
    lib = L.lib()
    worst = Worst("linear %s %s" % (shape, act))
    d16 = bool(switch_get(lib, "ECGMM_DENSE16"))
    routes, reaches = LINEAR_REACHES[shape]
    assert reaches(B, In, Out)
    if d16:
        assert linear_routes(B, In, Out, "none", True) == routes
    print("\n[linear %s %s] routes %s" % (shape, act, linear_routes(B, In, Out, act, d16)))
    x, w, b, dy = F64.linear_inputs(B, In, Out)
    xg, wg, bg, dyg = dev(x), dev(w), dev(b), dev(dy)
    y, y0 = nanbuf((B, Out)), nanbuf((B, Out))
    L.check(lib.ecgmm_linear_fwd(ptr(xg), ptr(wg), ptr(bg), ptr(y), B, In, Out, ACT[act], stream()), "linear_fwd")
    L.check(lib.ecgmm_linear_fwd(ptr(xg), ptr(wg), None, ptr(y0), B, In, Out, ACT[act], stream()), "linear_fwd")
    # the gradient of the pre-activation from the stored activation output (exact for ReLU, three roundings for the sigmoid)
    if act == "none":
        dz = dyg
    else:
        dz = nanbuf((B, Out))
        L.check(lib.ecgmm_act_bwd(ptr(dyg), ptr(y), ptr(dz), B * Out, ACT[act], stream()), "act_bwd")
    nb = lib.ecgmm_linear_bwd_scratch(B, In, Out)
    outs = []
    for with_db in (True, False):
        scratch = nanbytes(nb)
        dx, dw, db = nanbuf((B, In)), nanbuf((Out, In)), nanbuf(Out)
        L.check(lib.ecgmm_linear_bwd(ptr(dz), ptr(xg), ptr(wg), ptr(dx), ptr(dw), ptr(db) if with_db else None, B, In, Out,
                                     ptr(scratch), scratch.numel() * 4, stream()), "linear_bwd")
        outs.append((dx, dw, db))
    torch.cuda.synchronize()
    y, y0, dzc = y.cpu(), y0.cpu(), dz.cpu()
    if act == "relu":
        assert torch.equal(dzc, torch.where(y > 0, dy, torch.zeros_like(dy)))
    elif act == "sigmoid":
        ref = dy.double() * y.double() * (1 - y.double())
        worst(F64.check_se_mlp({"dz": (ref, ref.abs(), 0, "ds")}, {"dz": dzc}, "act_bwd")["dz"])
    ref = F64.linear_ref(x, w, b, dzc, act)
    r, A, K, sig = ref["y"]
    worst(F64.check_dot(y, r, A, K, "y", sigmoid=sig))
    r, A, K, sig = F64.linear_ref(x, w, None, None, act)["y"]
    worst(F64.check_dot(y0, r, A, K, "y (no bias)", sigmoid=sig))
    (dx, dw, db), (dx2, dw2, db2) = [[t.cpu() for t in o] for o in outs]
    for k, got in (("dx", dx), ("dw", dw), ("db", db)):
        r, A, K, _ = ref[k]
        worst(F64.check_dot(got, r, A, K, k))
    # db null: the same dx and dw, db untouched
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and torch.isnan(db2).all()
    worst.show()


# ----------------------------------------------------------------------------------------------------------------------
# Squeeze-excite MLP
# ----------------------------------------------------------------------------------------------------------------------
def _se_run(lib, d, N, C, CR, want=("dw1", "db1", "dw2", "db2")):
    g = {k: dev(v) for k, v in d.items()}
    o = dict(h=nanbuf((N, CR)), g=nanbuf((N, C)), ds=nanbuf((N, C)), dh=nanbuf((N, CR)), dm=nanbuf((N, C)),
             dw1=nanbuf((CR, C)), db1=nanbuf(CR), dw2=nanbuf((C, CR)), db2=nanbuf(C))
    L.check(lib.ecgmm_se_mlp_fwd(ptr(g["m"]), ptr(g["w1"]), ptr(g["b1"]), ptr(g["w2"]), ptr(g["b2"]), ptr(o["h"]), ptr(o["g"]),
                                 N, C, CR, stream()), "se_mlp_fwd")
    p = {k: (ptr(o[k]) if k in want else None) for k in ("dw1", "db1", "dw2", "db2")}
    L.check(lib.ecgmm_se_mlp_bwd(ptr(g["dg"]), ptr(o["g"]), ptr(o["h"]), ptr(g["m"]), ptr(g["w1"]), ptr(g["w2"]), ptr(o["ds"]),
                                 ptr(o["dh"]), ptr(o["dm"]), p["dw1"], p["db1"], p["dw2"], p["db2"], N, C, CR, F64.SE_SCALE,
                                 stream()), "se_mlp_bwd")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("shape", F64.SE_CASES)
def test_se_mlp_against_float64(shape):
    """ecgmm_se_mlp_fwd / ecgmm_se_mlp_bwd stage by stage, each stage from the stored output of the one before"""
    N, C, CR = shape
    lib = L.lib()
    worst = Worst("se_mlp %s" % (shape,))
    # the weight kernel: 16 batch slices; slice s makes an unrolled trip iff s + 48 < N
    unrolled = sum(1 for s in range(16) if s + 48 < N)
    idle = max(0, 16 - N)
    print("\n[se_mlp %s] slices without a row %d, slices with an unrolled trip %d" % (shape, idle, unrolled))
    assert {1: idle == 15, 5: idle == 11, 16: idle == 0 and unrolled == 0, 17: unrolled == 0, 49: unrolled == 1,
            67: unrolled == 16, 130: unrolled == 16}[N]
    d = F64.se_inputs(N, C, CR)
    o = _se_run(lib, d, N, C, CR)
    st = F64.se_mlp_stages(d["m"], d["w1"], d["b1"], d["w2"], d["b2"], o["h"], o["g"], d["dg"], o["ds"], o["dh"], F64.SE_SCALE)
    for r in F64.check_se_mlp(st, o, "se_mlp").values():
        worst(r)
    assert len(st) == 9
    worst.show()


def test_se_mlp_frozen_outputs_and_refusals():
    """null parameter outputs leave dm / ds / dh bit-identical and write nothing else; shapes beyond the kernels' LDS
    arrays are refused by return code"""
    N, C, CR = 17, 128, 8
    lib = L.lib()
    d = F64.se_inputs(N, C, CR)
    full = _se_run(lib, d, N, C, CR)
    none = _se_run(lib, d, N, C, CR, want=())
    only = _se_run(lib, d, N, C, CR, want=("dw1",))
    for o in (none, only):
        for k in ("h", "g", "dm", "ds", "dh"):
            assert torch.equal(o[k], full[k]), k
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.isnan(none[k]).all(), k
    assert torch.equal(only["dw1"], full["dw1"])
    for k in ("db1", "dw2", "db2"):
        assert torch.isnan(only[k]).all(), k
    st = F64.se_mlp_stages(d["m"], d["w1"], d["b1"], d["w2"], d["b2"], only["h"], only["g"], d["dg"], only["ds"], only["dh"],
                           F64.SE_SCALE)
    F64.check_se_mlp(st, {k: only[k] for k in ("h", "g", "ds", "dh", "dm", "dw1")}, "se_mlp frozen")
    big = nanbuf(4096)
    for n, c, cr in ((4, 1025, 8), (4, 128, 65), (0, 128, 8)):
        a = [ptr(big)] * 7
        assert lib.ecgmm_se_mlp_fwd(*a, n, c, cr, stream()) == 1          # ECGMM_ERR_SHAPE
        assert lib.ecgmm_se_mlp_bwd(*([ptr(big)] * 13), n, c, cr, 0.5, stream()) == 1
    torch.cuda.synchronize()
    assert torch.isnan(big).all()


# ----------------------------------------------------------------------------------------------------------------------
# The head: fused row kernels and the per-op fallback of the same plan
# ----------------------------------------------------------------------------------------------------------------------
def head_fused_ok(B, dims, hidden, nc):
    """mirrors ecg_head_fused_ok (csrc/head_fused.hip) with the switch on"""
    return all(2 <= d <= 512 for d in dims) and 1 <= nc <= 4 and B % 16 == 0 and sum(dims) % 16 == 0 and hidden % 16 == 0


def head_partial_floats(dims, nc):
    """mirrors head_part_base(.., 3)"""
    return 2 * sum(dims) + 4 + sum(2 * d + nc * d + 4 for d in dims)


def _head_gpu(head, raws, lab, kind, hidden, nc):
    """ecgmm_head_forward / ecgmm_head_backward with every buffer NaN-filled; the loss between them on the GPU.
    Returns outputs (6), d raw (3), the 19 gradient buffers and the upstream gradients given"""
    lib = L.lib()
    B, dims = raws[0].shape[0], [r.shape[1] for r in raws]
    desc = L.HeadDesc(B, (C.c_int * 3)(*dims), hidden, nc, 1, 1e-5, 0.0, 0, 0)
    nf, nb = lib.ecgmm_head_fwd_workspace(C.byref(desc)), lib.ecgmm_head_bwd_workspace(C.byref(desc))
    assert nf > 0 and nb > 0
    ws, bws = nanbytes(nf), nanbytes(nb)
    params = [dev(p.detach().float()) for p in head.table()]
    rg = [dev(r) for r in raws]
    logits = [nanbuf((B, nc)) for _ in range(4)]
    var, soft = nanbuf(()), nanbuf(3)
    L.check(lib.ecgmm_head_forward(C.byref(desc), table(rg), table(params), table(logits), ptr(var), ptr(soft), ptr(ws),
                                   ws.numel() * 4, stream()), "head forward")
    torch.cuda.synchronize()
    leaves = [t.clone().requires_grad_(True) for t in logits + [var]]
    F64.head_loss(leaves, dev(lab), kind, HF.cross_entropy).backward()
    up = [t.grad for t in leaves]
    dvar = None if up[4] is None else up[4].reshape(1).contiguous()
    grads = [nanbuf(p.shape) for p in params]
    draw = [nanbuf(r.shape) for r in rg]
    L.check(lib.ecgmm_head_backward(C.byref(desc), table(rg), table(params), table(grads), table(up[:4]), ptr(dvar),
                                    table(draw), ptr(ws), ptr(bws), bws.numel() * 4, stream()), "head backward")
    torch.cuda.synchronize()
    return [t.cpu() for t in logits + [var, soft]], [t.cpu() for t in draw], [t.cpu() for t in grads], up


def _check_head(B, dims, hidden, nc, kind, fused):
    lib = L.lib()
    worst = Worst("head %s %s" % ((B, dims, hidden, nc), kind))
    assert head_fused_ok(B, dims, hidden, nc) == fused
    rows_on = bool(switch_get(lib, "ECGMM_HEAD_FUSED"))     # (off in an A/B environment: the same checks on the per-op plan)
    head = F64.head_fill(F64.HeadRef(dims, hidden, nc), salt=len(dims) + nc)
    raws, lab = F64.head_inputs(B, dims, nc)
    out, draw, grads, up = _head_gpu(head, raws, lab, kind, hidden, nc)
    out64, draw64, g64 = F64.head_run(head, raws, lab, kind, torch.float64)
    out32, draw32, g32 = F64.head_run(head, raws, lab, kind, torch.float32)
    print("\n[head %s %s %s]" % ((B, dims, hidden, nc), kind, "fused" if fused and rows_on else "per-op"))
    names = ("image logits", "signal logits", "clinical logits", "fusion logits", "var_loss", "softmax weights")
    for n, a, r, o in zip(names, out, out64, out32):
        worst(F64.check_chain(a, r, o, n))
    for m in range(3):
        if draw64[m] is None:       # nothing upstream reaches the branch: the plan writes zeros
            assert torch.equal(draw[m], torch.zeros_like(draw[m])), "d raw %d of a branch outside the loss" % m
        else:
            worst(F64.check_chain(draw[m], draw64[m], draw32[m], "d raw %d" % m))
    for i, n in enumerate(F64.HeadRef.TABLE_NAMES):
        if g64[i] is None:          # its branch is not in the loss: left untouched
            assert torch.isnan(grads[i]).all(), n
        else:
            worst(F64.check_chain(grads[i], g64[i], g32[i], "d " + n))
    worst.show()
    return worst


# (B, dims, hidden, NC): what each reaches is asserted in the test
HEAD_CASES = [(16, (256, 256, 256), 128, 2), (272, (256, 256, 256), 128, 2), (272, (512, 128, 32), 128, 2),
              (32, (72, 40, 48), 16, 3), (16, (512, 512, 512), 64, 4), (32, (2, 6, 8), 16, 1)]
HEAD_PARAMS = [(c, k) for i, c in enumerate(HEAD_CASES) for k in (F64.HEAD_LOSSES if i < 2 else F64.HEAD_LOSSES[:1])]


@pytest.mark.parametrize("case,kind", HEAD_PARAMS)
def test_fused_head_against_float64(case, kind):
    B, dims, hidden, nc = case
    blocks = min(64, -(-B // 4))                       # mirrors ecg_head_bwd_blocks
    pmb, tab = all(d <= 256 for d in dims), dims[0] <= 512 and dims[1] <= 128 and dims[2] <= 64
    inst = "<4,4,4,2>" if pmb and nc <= 2 else "<8,2,1,2>" if tab and nc <= 2 else "<8,8,8,4>"
    i = HEAD_CASES.index(case)
    assert [B <= 4 * blocks and inst == "<4,4,4,2>",
            B > 4 * blocks and inst == "<4,4,4,2>",                                       # waves of blocks 0..3 take a second row
            B > 4 * blocks and inst == "<8,2,1,2>" and dims[2] < 64,
            inst == "<8,8,8,4>" and all(d % 64 for d in dims) and sum(dims) % 64 and hidden == 16,
            inst == "<8,8,8,4>" and nc == 4 and 4 * head_partial_floats(dims, nc) > 49000,   # the dynamic LDS at its largest
            dims[0] == 2 and nc == 1][i]
    _check_head(B, dims, hidden, nc, kind, fused=True)


@pytest.mark.parametrize("case", [(24, (256, 256, 256), 128, 2), (1028, (72, 40, 48), 16, 3)])
def test_head_per_op_fallback_against_float64(case):
    B, dims, hidden, nc = case
    if B > 1024:
        assert -(-B // 4) > 256                        # ln_bwd_grid caps at 256 blocks: block 0's waves take a second row
    _check_head(B, dims, hidden, nc, "all_heads", fused=False)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm, attention fusion + var_loss, cross-entropy / focal: through hip/functional.py
# ----------------------------------------------------------------------------------------------------------------------
def _param(t):
    """a device parameter whose gradient sink is NaN-filled: the backward has to write all of it"""
    p = torch.nn.Parameter(dev(t.clone()))
    p.grad = torch.full_like(p, NAN)
    return p


def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


# (1025 and 1536: the first and the last width on the kernels' 24-values-per-lane instantiation)
@pytest.mark.parametrize("B,D", [(1, 2), (3, 100), (33, 1024), (1028, 100), (2, 1025), (5, 1536)])
def test_layernorm_against_float64(B, D):
    worst = Worst("layernorm (%d, %d)" % (B, D))
    x = fill.hash_tensor((B, D), 5, 2.0) + 0.3
    g, b, dy = 1 + 0.2 * fill.hash_tensor((D,), 6), 0.1 * fill.hash_tensor((D,), 7), fill.hash_tensor((B, D), 8)
    res = {}
    for dt in (torch.float64, torch.float32):
        xr, gr, br = _leaf(x, dt), _leaf(g, dt), _leaf(b, dt)
        y = F.layer_norm(xr, (D,), gr, br, 1e-5)
        y.backward(dy.to(dt))
        res[dt] = (y.detach(), xr.grad, gr.grad, br.grad)
    xg = dev(x).requires_grad_(True)
    gg, bg = _param(g), _param(b)
    y = HF.layer_norm(xg, gg, bg)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    print("\n[layernorm (%d, %d)]" % (B, D))
    got = (y.detach().cpu(), xg.grad.cpu(), gg.grad.cpu(), bg.grad.cpu())
    for n, a, r, o in zip(("y", "dx", "dgamma", "dbeta"), got, res[torch.float64], res[torch.float32]):
        worst(F64.check_chain(a, r, o, n))
    worst.show()


def test_layernorm_refuses_a_row_wider_than_1536():
    """(1536 = three 512-wide branches, the widest concatenation the head admits: its per-op form normalises it here)"""
    x = dev(torch.zeros(2, 1537))
    with pytest.raises(RuntimeError, match="layernorm: D=1537 > 1536"):
        HF.layer_norm(x, dev(torch.ones(1537)), dev(torch.zeros(1537)))


@pytest.mark.parametrize("B,dims", [(5, (72, 40, 48)), (1028, (256, 256, 256))])
def test_attention_fusion_and_var_loss_against_float64(B, dims):
    worst = Worst("fusion + var_loss (%d, %s)" % (B, dims))
    D = sum(dims)
    feats = [fill.hash_tensor((B, d), 10 + i, 1.0 + 0.5 * i) for i, d in enumerate(dims)]
    w0 = torch.tensor([4.0, -3.0, 0.0])          # far apart: the softmax is not near uniform
    g, b, dy = 1 + 0.1 * fill.hash_tensor((D,), 20), 0.1 * fill.hash_tensor((D,), 21), fill.hash_tensor((B, D), 22)
    res = {}
    for dt in (torch.float64, torch.float32):
        ref = O.AttentionFusion(list(dims)).to(dt)
        with torch.no_grad():
            ref.weights.copy_(w0); ref.norm.weight.copy_(g); ref.norm.bias.copy_(b)
        fr = [_leaf(f, dt) for f in feats]
        fused, w = ref(*fr)
        v = [torch.var(f, dim=1).mean() for f in fr]
        vl = (v[0] - v[1]).abs() + (v[0] - v[2]).abs() + (v[1] - v[2]).abs()
        ((fused * dy.to(dt)).sum() + 0.1 * vl).backward()
        res[dt] = [fused.detach(), w.detach(), vl.detach()] + [f.grad for f in fr] + [ref.weights.grad, ref.norm.weight.grad,
                                                                                      ref.norm.bias.grad]
    fg = [dev(f).requires_grad_(True) for f in feats]
    wg, gg, bg = _param(w0), _param(g), _param(b)
    fused, soft = HF.attention_fusion(fg[0], fg[1], fg[2], wg, gg, bg)
    vl = HF.var_loss(*fg)
    ((fused * dev(dy)).sum() + 0.1 * vl).backward()
    torch.cuda.synchronize()
    got = [fused.detach(), soft, vl.detach()] + [f.grad for f in fg] + [wg.grad, gg.grad, bg.grad]
    names = ("fused", "softmax weights", "var_loss", "d feat 0", "d feat 1", "d feat 2", "d weights", "dgamma", "dbeta")
    print("\n[fusion + var_loss (%d, %s)]" % (B, dims))
    for n, a, r, o in zip(names, got, res[torch.float64], res[torch.float32]):
        worst(F64.check_chain(a.cpu(), r, o, n))
    worst.show()


LOSSES = {"ce": None, "focal(1,2)": (1.0, 2.0), "focal(0.25,2)": (0.25, 2.0), "focal(1,0)": (1.0, 0.0)}


def _loss_inputs(B, Cn):
    logits = fill.hash_tensor((B, Cn), 61, 2.0)
    lab = (torch.arange(B) * 7 + 1) % Cn
    if B > 7:                       # one row whose logit gap is 30: pt rounds to 1 in fp32
        logits[7] = -15.0
        logits[7, lab[7]] = 15.0
    return logits, lab


@pytest.mark.parametrize("Cn", [2, 3, 5])
@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("kind", list(LOSSES))
def test_cross_entropy_and_focal_against_float64(kind, B, Cn):
    worst = Worst("%s (%d, %d)" % (kind, B, Cn))
    logits, lab = _loss_inputs(B, Cn)
    res = {}
    for dt in (torch.float64, torch.float32):
        lr = _leaf(logits, dt)
        loss = F.cross_entropy(lr, lab) if LOSSES[kind] is None else O.FocalLoss(*LOSSES[kind])(lr, lab)
        (loss * 1.7).backward()
        res[dt] = (loss.detach(), lr.grad)
    lg = dev(logits).requires_grad_(True)
    loss = HF.cross_entropy(lg, dev(lab)) if LOSSES[kind] is None else HF.focal_loss(lg, dev(lab), *LOSSES[kind])
    (loss * 1.7).backward()
    torch.cuda.synchronize()
    print("\n[%s (%d, %d)]" % (kind, B, Cn))
    for n, a, r, o in zip(("loss", "dlogits"), (loss.detach().cpu(), lg.grad.cpu()), res[torch.float64], res[torch.float32]):
        worst(F64.check_chain(a, r, o, n))
    worst.show()


def test_cross_entropy_plus_against_float64():
    B, Cn = 300, 2
    worst = Worst("cross_entropy_plus (%d, %d)" % (B, Cn))
    logits, lab = _loss_inputs(B, Cn)
    res = {}
    for dt in (torch.float64, torch.float32):
        lr, er = _leaf(logits, dt), _leaf(torch.tensor(0.37), dt)
        loss = F.cross_entropy(lr, lab) + torch.tensor(0.1, dtype=torch.float32).to(dt) * er
        (loss * 1.7).backward()
        res[dt] = (loss.detach(), lr.grad, er.grad)
    lg, eg = dev(logits).requires_grad_(True), dev(torch.tensor(0.37)).requires_grad_(True)
    loss = HF.cross_entropy_plus(lg, dev(lab), eg, 0.1)
    (loss * 1.7).backward()
    torch.cuda.synchronize()
    print("\n[cross_entropy_plus (%d, %d)]" % (B, Cn))
    got = (loss.detach().cpu(), lg.grad.cpu(), eg.grad.cpu())
    for n, a, r, o in zip(("loss", "dlogits", "dextra"), got, res[torch.float64], res[torch.float32]):
        worst(F64.check_chain(a, r, o, n))
    worst.show()


# ----------------------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------------------
ADAM_CASES = [(n, wd, 4) for n in (1, 3, 4099) for wd in (0.0, 1e-2)] + [(4099, 1e-2, 1)]


@pytest.mark.parametrize("n,wd,offset", ADAM_CASES)
def test_adam_against_float64(n, wd, offset):
    """three steps of ecgmm_adam against torch.optim.Adam in float64; offset 4: 16-byte aligned views (float4 path + tail),
    offset 1: views one float into their allocations (vec = 0: the scalar path)"""
    lib = L.lib()
    worst = Worst("adam n=%d wd=%g offset=%d" % (n, wd, offset))
    lr, b1, b2, eps, wdf, gscale = (F64.f32(v) for v in (1e-3, 0.95, 0.999, 1e-8, wd, 0.5))
    p0 = fill.hash_tensor((n,), 81)
    gs = [fill.hash_tensor((n,), 82 + s, 0.3) for s in range(3)]
    res = {}
    for dt in (torch.float64, torch.float32):
        p = torch.nn.Parameter(p0.to(dt).clone())
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
        for g in gs:
            p.grad = (g.to(dt) * gscale).clone()
            opt.step()
        st = opt.state[p]
        res[dt] = (p.detach(), st["exp_avg"], st["exp_avg_sq"])
    bufs = [nanbuf(n + 8) for _ in range(4)]
    pv, gv, mv, vv = (t[offset:offset + n] for t in bufs)
    assert all((t.data_ptr() % 16 == 0) == (offset == 4) for t in (pv, gv, mv, vv))
    pv.copy_(dev(p0)); mv.zero_(); vv.zero_()
    for s, g in enumerate(gs):
        gv.copy_(dev(g))
        L.check(lib.ecgmm_adam(ptr(pv), ptr(gv), ptr(mv), ptr(vv), n, lr, b1, b2, eps, wdf, s + 1, gscale, stream()), "adam")
    torch.cuda.synchronize()
    for t in bufs:      # nothing written outside the run
        assert torch.isnan(t[:offset]).all() and torch.isnan(t[offset + n:]).all()
    print("\n[adam n=%d wd=%g offset=%d]" % (n, wd, offset))
    for name, a, r, o in zip(("p", "m", "v"), (pv.cpu(), mv.cpu(), vv.cpu()), res[torch.float64], res[torch.float32]):
        worst(F64.check_chain(a, r, o, name))
    worst.show()
