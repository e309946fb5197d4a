"""The BatchNorm and pooling passes of csrc/elementwise.hip (and csrc/bn_eval_bwd.hip) against float64, element by element,
at the smallest shapes that reach each path of their launch arithmetic: the 1024-row cap of the statistics launch and the
row folding behind it, the 256-row cap of the backward, the grid-stride loops of col_stats / bn_act / bn_bwd and of both
pooling kernels, the four-rows-per-trip finalize loops, the two-rows-per-trip tail of bn_act, C < 16 and C > 512, the
consumer-side fold with G = C = 16, and the row -> sample division with rows_per_sample = 313 and 625.

Bounds and references: tests/f64check.py (derived worst-case constants; the CPU mutation tests are in tests/test_f64check.py).
Every output and scratch buffer is NaN-filled first; each test prints its worst ratio (run with -s).

Measured on the MI355X (worst |err| / bound per kernel over the cases of this file; 1 is a bf16 rounding tie, the stored
rounding term alone): col_stats 0.06, bn_finalize 0.99 (fp32 mean, (626, 64)), bn_act fp32 0.97 / bf16 1, bn_act_from_rows
coef 0.99 / out 1, bn_bwd dy fp32 0.84 ((20000, 512) gated) / bf16 1, dgamma / dbeta / dbias < 0.1, bn_eval_bwd dy 0.65 / 1,
bnrelu_maxpool 1 (bf16) / < 0.4 (fp32), maxpool_relu_bwd 1 (bf16) / 0 (fp32: exact), pool_bn_bwd dy 0.99 (bf16),
large-mean coef 0.046.  No kernel broke a bound.
"""
import math

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from .util import DEV, TDT, dev, switches

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64                       # spare rows every partial-row buffer carries


class Worst:
    def __init__(self):
        self.ratio, self.name = 0.0, "-"

    def __call__(self, r, name=None):
        ratio = r.ratio if hasattr(r, "ratio") else float(r)
        if ratio >= self.ratio:
            self.ratio, self.name = ratio, (name or getattr(r, "name", "?")) + (" at %s" % (r.where,) if hasattr(r, "where") else "")
        return r

    def show(self, what):
        print("WORST %-40s ratio %.3g  (%s)" % (what, self.ratio, self.name))


def nanbuf(n, dtype=torch.float32):
    return torch.full((n,) if isinstance(n, int) else n, NAN, device=DEV, dtype=dtype)


# The library reports the statistics rows (ecgmm_col_stats_rows) and, through the scratch size, the backward rows; the other
# launch shapes below are copies of its host code, each naming the function it mirrors.  A NaN-tail assert pins the ones that
# size a buffer (backward rows, eval-backward grid); the rest only size a summation chain or prove a path.
def fold_ok(C, rows):
    """mirrors ecg_bn_fold_ok (csrc/elementwise.hip) with the switch on"""
    return 1 <= rows <= 512 and C <= 512 and (C % 128 == 0 if C >= 128 else (C >= 16 and 1024 % C == 0))


def bwd_rows(lib, dt, M, C):
    """bn_bwd_rows, recovered from ecg_bn_bwd_scratch = ((rows + ECG_TAIL_ROWS) * 2 C + 3 C) floats (csrc/elementwise.hip)"""
    return (lib.ecgmm_bn_bwd_scratch(dt, M, C) // 4 - 3 * C) // (2 * C) - TAIL


# (M, C, dtypes, rows_per_sample, statistics rows, backward rows): the row counts are asserted against the library's
BN_CASES = {
    "M1": (1, 64, (L.F32, L.BF16), None),
    "cpr1_f32": (7, 4, (L.F32,), None),
    "cpr1_bf16": (7, 8, (L.BF16,), None),
    "foldG16": (777, 16, (L.F32, L.BF16), None),
    "rps313": (626, 64, (L.F32, L.BF16), 313),
    "tail": (4099, 128, (L.F32, L.BF16), None),
    "caps_f32": (20000, 512, (L.F32,), 625),
    "caps_bf16": (40000, 512, (L.BF16,), 625),
    "wide": (300, 1024, (L.BF16,), None),
}
BN_PARAMS = [(k, dt) for k, v in BN_CASES.items() for dt in v[2]]


def _upload(d, dt):
    g = {k: dev(v) for k, v in d.items() if torch.is_tensor(v)}
    for k in ("y", "res", "dout"):
        g[k + "_t"] = g[k].to(TDT[dt]).contiguous()
    return g


def _forward(lib, g, M, C, dt, worst):
    """col_stats + bn_finalize, both checked; returns the kernel's rows and coef"""
    bf16 = dt == L.BF16
    vec = 8 if bf16 else 4
    rows = lib.ecgmm_col_stats_rows(dt, M, C)
    partial = nanbuf((rows + TAIL, 2, C))
    L.check(lib.ecgmm_col_stats(dt, ptr(g["y_t"]), M, C, ptr(partial), stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(partial[:rows]).all() and torch.isnan(partial[rows:]).all()
    K = F64.chain_len(M, rows, C, vec, 256)
    worst(F64.check_colstats(partial[:rows], g["y"], K), "col_stats")
    stat_rows = partial[:rows].clone()
    coef, rm, rv = nanbuf((4, C)), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.full((), 6, dtype=torch.int64, device=DEV)
    L.check(lib.ecgmm_bn_finalize(ptr(partial), rows, C, float(M), ptr(g["gamma"]), ptr(g["beta"]), ptr(rm), ptr(rv), ptr(nbt),
                                  0.1, 1e-5, ptr(coef), stream()))
    torch.cuda.synchronize()
    assert int(nbt) == 7 and torch.isfinite(coef).all()
    # rows > 512 are first folded to <= 64 tail rows, each a double sum rounded to fp32: one rounding of the magnitudes
    folded = rows > 512
    assert torch.isfinite(partial[rows:]).all() if folded else torch.isnan(partial[rows:]).all()
    r64 = stat_rows.double()
    ds = [F64.U * r64[:, i].abs().sum(0) for i in range(2)] if folded else [None, None]
    ref = F64.coef_ref(r64[:, 0].sum(0), r64[:, 1].sum(0), M, g["gamma"], g["beta"], 1e-5, torch.zeros_like(rm), torch.ones_like(rv), 0.1,
                       ds[0], ds[1])
    worst(F64.check_coef(coef, ref, rm, rv, name="bn_finalize"))
    return rows, stat_rows, coef, ref, (rm, rv)


@pytest.mark.parametrize("case,dt", BN_PARAMS)
def test_batchnorm_forward_against_float64(case, dt):
    M, C, _, rps = BN_CASES[case]
    lib = L.lib()
    bf16 = dt == L.BF16
    vec = 8 if bf16 else 4
    worst = Worst()
    d = F64.bn_inputs(M, C, bf16, rps)
    g = _upload(d, dt)
    rows, stat_rows, coef, cref, (rm, rv) = _forward(lib, g, M, C, dt, worst)
    # the launch arithmetic this case is here for
    # (mirrors the grid of ecg_bn_act / ecg_bn_act_fold, csrc/elementwise.hip: ew_grid(M, rpi * 4) capped at 256, rpi = 1024 / cpr)
    act_grid = min(256, max(1, -(-M // ((1024 // (C // vec)) * 4))))
    if case.startswith("caps"):
        assert rows == 1024 and M > 1024 * (256 // (C // vec)) and act_grid == 256        # cap, fold_rows, grid-stride loops
    if case == "tail":
        per = M / (act_grid * (1024 // (C // vec)))
        assert M % 2 == 1 and 3 < per < 4                                                    # threads with 3 rows: `two` false on the second trip
    if case.startswith("cpr1"):
        assert C // vec == 1 and not fold_ok(C, rows)
    if case == "foldG16":
        assert fold_ok(C, rows) and 1024 // C == 64
    if case == "wide":
        assert C > 512 and not fold_ok(C, rows)
    if case == "M1":
        # by hand (torch refuses one value per channel): mean = y, var = 0, invstd = 1 / sqrt(eps), count - 1 = 0 so the running
        # variance takes var itself.  bf16 squares are exact in fp32, so var is exactly 0; an fp32 y * y carries one rounding,
        # u y^2, which the bound carries through var + eps
        assert rows == 1
        y1 = g["y"][0].double()
        hand = F64.coef_ref(y1, y1 * y1, 1, g["gamma"], g["beta"], 1e-5, torch.zeros_like(rm), torch.ones_like(rv), 0.1,
                            None, None if bf16 else F64.g_k(1) * y1 * y1)
        assert bool((hand.val["invstd"] - 1 / math.sqrt(F64.f32(1e-5))).abs().max() < 1e-9) and bool((hand.val["rv"] - 0.9).abs().max() < 1e-7)
        worst(F64.check_coef(coef, hand, rm, rv, name="bn_finalize M == 1, by hand"))
    gate = F64.per_row(g["gate"], rps, M) if rps else None
    forms = [("plain", None, None, None, 0), ("relu", None, None, None, 1), ("res+rcoef", g["res"], g["rscale"], g["rshift"], 1)]
    if rps:
        forms.append(("gate+res", g["res"], None, None, 1))
    rcoef = torch.stack([g["rscale"], g["rshift"]]).contiguous()
    for name, res, rs, rb, relu in forms:
        out = nanbuf(M * C, TDT[dt])
        gated = name.startswith("gate")
        L.check(lib.ecgmm_bn_act(dt, ptr(g["y_t"]), ptr(coef), ptr(g["res_t"]) if res is not None else None,
                                 ptr(rcoef) if rs is not None else None, ptr(g["gate"]) if gated else None, rps or 1, relu,
                                 ptr(out), M, C, stream()))
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        want, A = F64.bn_act_ref(g["y"], coef[0], coef[1], res, rs, rb, gate if gated else None, bool(relu))
        worst(F64.check_stored(out.view(M, C), want, A, F64.K_ACT, bf16, "bn_act " + name))
    # finalize folded into the consumer, from the real statistics rows: against coefficients derived from the same rows in
    # float64, their bound carried through (rows > 512 or an unfoldable C: the two-launch route, same contract)
    with switches(lib, ECGMM_BN_FOLD=1):
        partial = torch.cat([stat_rows, nanbuf((TAIL, 2, C))]).contiguous()
        coef2, rm2, rv2 = nanbuf((4, C)), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        out = nanbuf(M * C, TDT[dt])
        L.check(lib.ecgmm_bn_act_from_rows(dt, ptr(g["y_t"]), ptr(partial), rows, float(M), ptr(g["gamma"]), ptr(g["beta"]), ptr(rm2),
                                           ptr(rv2), ptr(nbt), 0.1, 1e-5, ptr(coef2), ptr(g["res_t"]), None,
                                           ptr(g["gate"]) if rps else None, rps or 1, 1, ptr(out), M, C, stream()))
        torch.cuda.synchronize()
    assert int(nbt) == 1 and torch.isfinite(out.float()).all()
    worst(F64.check_coef(coef2, cref, rm2, rv2, name="bn_act_from_rows coef"))
    want, A = F64.bn_act_ref(g["y"], cref.val["scale"], cref.val["shift"], g["res"], None, None, gate, True)
    extra = g["y"].double().abs() * cref.bound["scale"] + cref.bound["shift"]
    if gate is not None:
        extra = extra * gate.abs()
    worst(F64.check_stored(out.view(M, C), want, A + extra / F64.g_k(F64.K_ACT), F64.K_ACT, bf16, "bn_act_from_rows out"))
    worst.show("forward %s %s" % (case, "bf16" if bf16 else "fp32"))


@pytest.mark.parametrize("case,dt", BN_PARAMS)
def test_batchnorm_backward_against_float64(case, dt):
    M, C, _, rps = BN_CASES[case]
    lib = L.lib()
    bf16 = dt == L.BF16
    vec = 8 if bf16 else 4
    worst = Worst()
    d = F64.bn_inputs(M, C, bf16, rps)
    g = _upload(d, dt)
    rows, _, coef, _, _ = _forward(lib, g, M, C, dt, Worst())
    brows = bwd_rows(lib, dt, M, C)
    assert brows == min(256, max(1, -(-M // ((1024 // (C // vec)) * 8))))
    if case.startswith("caps"):
        assert brows == 256 and M > 256 * (1024 // (C // vec))                       # cap, grid-stride, four-per-trip finalize loops
        assert brows > 3 * (1024 // 128) and brows > 48
    K = F64.chain_len(M, brows, C, vec, 1024)
    nscratch = lib.ecgmm_bn_bwd_scratch(dt, M, C) // 4
    # a ReLU'd tensor as the separate mask reference
    maskt = nanbuf(M * C, TDT[dt])
    L.check(lib.ecgmm_bn_act(dt, ptr(g["y_t"]), ptr(coef), ptr(g["res_t"]), None, None, 1, 1, ptr(maskt), M, C, stream()))
    gate = F64.per_row(g["gate"], rps or M, M)
    addc = F64.per_row(g["addc"], rps or M, M)

    def run(form, fold):
        scratch = nanbuf(nscratch)
        dgam, dbet, dbias = nanbuf(C), nanbuf(C), nanbuf(C)
        dy, dz = nanbuf(M * C, TDT[dt]), nanbuf(M * C, TDT[dt])
        a = dict(mask=None, gate=None, addc=None, dy=ptr(dy), dz=None, dbias=None)
        if form == "mask=y":
            a["mask"] = ptr(g["y_t"])
        elif form == "mask+dz_out":
            a.update(mask=ptr(maskt), dz=ptr(dz))
        elif form == "gate+addc+dbias":
            a.update(mask=ptr(maskt), dz=ptr(dz), gate=ptr(g["gate"]), addc=ptr(g["addc"]), dbias=ptr(dbias))
        else:
            a.update(mask=ptr(g["y_t"]), dy=None)
        with switches(lib, ECGMM_BN_FOLD=fold):
            L.check(lib.ecgmm_bn_bwd(dt, ptr(g["dout_t"]), a["mask"], a["gate"], a["addc"], rps or M, ptr(g["y_t"]), ptr(coef),
                                     ptr(g["gamma"]), ptr(dgam), ptr(dbet), a["dy"], a["dz"], a["dbias"], M, C, ptr(scratch), stream()))
            torch.cuda.synchronize()
        rowsbuf = scratch[:(brows + TAIL) * 2 * C].view(brows + TAIL, -1)
        assert torch.isnan(rowsbuf[brows:]).all()                                        # nothing beyond the rows the library reports
        assert torch.isfinite(dgam).all() and torch.isfinite(dbet).all()
        name = "%s fold=%d" % (form, fold)
        gated = form == "gate+addc+dbias"
        res = F64.check_bn_bwd(g["dout"], g["y"], coef, g["gamma"], bf16, K, dgam, dbet,
                               dy.view(M, C) if a["dy"] else None, dz.view(M, C) if a["dz"] else None,
                               dbias if a["dbias"] else None, K, maskref="y" if form in ("mask=y", "reduce only") else maskt.view(M, C),
                               gate=gate if gated else None, addc=addc if gated else None, name=name)
        if a["dy"]:
            assert torch.isfinite(dy.float()).all()
        else:
            assert torch.isnan(dy.float()).all()
        for k, v in res.items():
            worst(v, name + " " + k)

    for form in ("mask=y", "mask+dz_out", "gate+addc+dbias", "reduce only"):
        for fold in ((1, 0) if fold_ok(C, brows) and form in ("mask=y", "mask+dz_out") else (0,)):
            run(form, fold)
    worst.show("backward %s %s" % (case, "bf16" if bf16 else "fp32"))


@pytest.mark.parametrize("dt", [L.F32, L.BF16])
def test_batchnorm_eval_backward_against_float64(dt):
    """ecgmm_bn_eval_bwd, gated with rows_per_sample = 313: dy = dz * scale (K_EVAL_DY), dbeta, dgamma, dbias, dz_out"""
    M, C, rps = 626, 64, 313
    lib = L.lib()
    bf16 = dt == L.BF16
    vec = 8 if bf16 else 4
    worst = Worst()
    g = _upload(F64.bn_inputs(M, C, bf16, rps), dt)
    _, _, coef, _, _ = _forward(lib, g, M, C, dt, Worst())
    nscratch = lib.ecgmm_bn_bwd_scratch(dt, M, C) // 4
    # (mirrors the grid of ecg_bn_eval_bwd, csrc/bn_eval_bwd.hip: ceil(M / (rpi * 8)) capped at 1024 and at scratch / 3 C rows)
    rpi = 256 // (C // vec)
    grid = max(1, min(-(-M // (rpi * 8)), 1024, nscratch // (3 * C)))
    assert grid == -(-M // (rpi * 8))
    K = F64.chain_len(M, grid, C, vec, 256)
    scratch = nanbuf(nscratch)
    dgam, dbet, dbias = nanbuf(C), nanbuf(C), nanbuf(C)
    dy, dz = nanbuf(M * C, TDT[dt]), nanbuf(M * C, TDT[dt])
    L.check(lib.ecgmm_bn_eval_bwd(dt, ptr(g["dout_t"]), ptr(g["y_t"]), ptr(g["gate"]), ptr(g["addc"]), rps, ptr(g["y_t"]), ptr(coef),
                                  ptr(dgam), ptr(dbet), ptr(dy), ptr(dz), ptr(dbias), M, C, ptr(scratch), stream()))
    torch.cuda.synchronize()
    assert torch.isnan(scratch[grid * 3 * C:]).all()
    for t in (dgam, dbet, dbias, dy.float(), dz.float()):
        assert torch.isfinite(t).all()
    mask, unsure = F64.affine_mask(g["y"], coef[0], coef[1])
    F64.check_unsure(unsure, "eval bwd")
    gate, addc = F64.per_row(g["gate"], rps, M), F64.per_row(g["addc"], rps, M)
    dzr, A, masked = F64.bn_dz_ref(g["dout"], mask, gate, addc)
    xh = F64.xhat_ref(g["y"], coef)
    sums, slack, mags = F64.bn_bwd_sums_ref(dzr, A, xh, unsure, g["dout"].double() * gate)
    worst(F64.check_sum(dbet, sums[0], mags[0], F64.K_DZ + K + 1, "eval dbeta", slack[0]))
    worst(F64.check_sum(dgam, sums[1], mags[1], F64.K_DZXHAT + K + 1, "eval dgamma", slack[1]))
    assert not bool(((dz.view(M, C).double() != masked) & ~unsure).any())
    want, Ady = F64.bn_eval_dy_ref(dzr, A, coef[0])
    worst(F64.check_stored(dy.view(M, C), want, Ady, F64.K_EVAL_DY, bf16, "eval dy", skip=unsure))
    s = dy.view(M, C).double()
    worst(F64.check_sum(dbias, s.sum(0), s.abs().sum(0), K + 1, "eval dbias"))
    worst.show("eval backward %s" % ("bf16" if bf16 else "fp32"))


def test_large_mean_variance_cancellation():
    """var = s2 / count - mean^2 from fp32 partial rows, channel families with |mean| / std of 0, 4, 32, 256 at (4099, 64) fp32.
    The assertion is the derived coef bound (it loosens with mean^2 / var by construction); the measured relative error of
    invstd is printed per family next to that of torch's CPU fp32 batch norm, and for a sweep of ratios 1 .. 32768 (DESIGN.md
    records where it passes 2^-9)."""
    M, C, dt = 4099, 64, L.F32
    lib = L.lib()
    worst = Worst()
    rows = lib.ecgmm_col_stats_rows(dt, M, C)
    K = F64.chain_len(M, rows, C, 4, 256)
    for label, ratios in (("families", (0, 4, 32, 256)), ("sweep", tuple(2 ** k for k in range(16)))):
        d = F64.bn_inputs(M, C, False, None, ratios)
        g = _upload(d, dt)
        partial, coef = nanbuf((rows + TAIL, 2, C)), nanbuf((4, C))
        L.check(lib.ecgmm_col_stats(dt, ptr(g["y_t"]), M, C, ptr(partial), stream()))
        L.check(lib.ecgmm_bn_finalize(ptr(partial), rows, C, float(M), ptr(g["gamma"]), ptr(g["beta"]), None, None, None, 0.1, 1e-5,
                                      ptr(coef), stream()))
        torch.cuda.synchronize()
        (s1, s2), (m1, m2) = F64.colstats_ref(g["y"])
        ref = F64.coef_ref(s1, s2, M, g["gamma"], g["beta"], 1e-5, ds1=F64.g_k(K) * m1, ds2=F64.g_k(K + 1) * m2)
        _, _, tinv = torch.native_batch_norm(d["y"].t().reshape(1, C, M, 1).contiguous(), d["gamma"], d["beta"], None, None, True, 0.1, 1e-5)
        rel = ((coef[3].double() - ref.val["invstd"]).abs() / ref.val["invstd"]).cpu()
        trel = ((tinv.double() - ref.val["invstd"].cpu()).abs() / ref.val["invstd"].cpu())
        allowed = (ref.bound["invstd"] / ref.val["invstd"]).cpu()
        for i, r in enumerate(ratios):
            ch = torch.arange(C) % len(ratios) == i
            print("LARGE-MEAN %-8s |mean|/std %6d: invstd rel err kernel %.3g  torch-cpu-fp32 %.3g  allowed %.3g"
                  % (label, r, float(rel[ch].max()), float(trel[ch].max()), float(allowed[ch].max())))
        if label == "families":
            worst(F64.check_coef(coef, ref, name="large-mean coef"))
    worst.show("large mean")


# ---------------------------------------------------------------- pooling ----------------------------------------------------------------
POOL_SHAPES = [(2, 64, 1, 1), (1, 64, 2, 2), (3, 64, 1, 41), (2, 64, 7, 1), (2, 64, 9, 7), (1, 128, 12, 10)]
POOL_PARAMS = [(s, dt) for s in POOL_SHAPES for dt in (L.F32, L.BF16)] + [((2, 64, 364, 364), L.F32)]


@pytest.mark.parametrize("shape,dt", POOL_PARAMS)
def test_pooling_against_float64(shape, dt):
    """bnrelu_maxpool, maxpool_relu_bwd and pool_bn_bwd: the forward against the float64 window maximum (ties: earliest tap),
    the backward as the exact float64 scatter of dp through the kernel's own pooled / idx, the fused stem backward stage by
    stage through its own stored dbeta / dgamma, and fused == two-pass as tests/test_ops_gpu.py requires."""
    N, C, H, W = shape
    lib = L.lib()
    bf16 = dt == L.BF16
    vec = 8 if bf16 else 4
    worst = Worst()
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M, MP = N * H * W, N * OH * OW
    if H > 300:
        assert MP * (C // vec) > 4096 * 256 and N * ((H + 1) // 2) * ((W + 1) // 2) * (C // vec) > 4096 * 256   # grid-stride loops
    p = F64.pool_inputs(N, C, H, W, bf16)
    g = {k: dev(v) for k, v in p.items()}
    mean, inv = g["mean"], g["invstd"]
    coef = torch.stack([g["scale"], g["shift"], mean, inv]).contiguous()
    gamma = g["gamma"]
    yt, dpt = g["y"].to(TDT[dt]).contiguous(), g["dp"].to(TDT[dt]).contiguous()
    pooled = nanbuf((N, OH, OW, C), TDT[dt])
    idx = torch.full((N, OH, OW, C), 255, device=DEV, dtype=torch.uint8)
    L.check(lib.ecgmm_bnrelu_maxpool(dt, ptr(yt), ptr(coef), ptr(pooled), ptr(idx), N, H, W, C, stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(pooled.float()).all() and int(idx.max()) < 9
    r = worst(F64.check_pool_fwd(pooled, idx, g["y"], coef[0], coef[1], bf16))
    assert r.ties > 0 or H * W == 1
    dz = nanbuf((N, H, W, C), TDT[dt])
    L.check(lib.ecgmm_maxpool_relu_bwd(dt, ptr(dpt), ptr(pooled), ptr(idx), ptr(dz), N, H, W, C, stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(dz.float()).all()
    worst(F64.check_pool_bwd(dz, g["dp"], pooled, idx, bf16))
    # fused stem backward
    nscratch = lib.ecgmm_bn_bwd_scratch(dt, M, C) // 4
    brows = bwd_rows(lib, dt, M, C)
    scratch = nanbuf(nscratch)
    dgam, dbet, dbias = nanbuf(C), nanbuf(C), nanbuf(C)
    dy = nanbuf((N, H, W, C), TDT[dt])
    L.check(lib.ecgmm_pool_bn_bwd(dt, ptr(dpt), ptr(pooled), ptr(idx), ptr(yt), ptr(coef), ptr(gamma), ptr(dgam), ptr(dbet), ptr(dy),
                                  ptr(dbias), N, H, W, C, ptr(scratch), stream()))
    torch.cuda.synchronize()
    for t in (dgam, dbet, dbias, dy.float()):
        assert torch.isfinite(t).all()
    assert torch.isnan(scratch[brows * 2 * C:(brows + TAIL) * 2 * C]).all()
    # (mirrors pool_bwd_launch, csrc/elementwise.hip: reduce grid g1 = min(ew_grid(MP, rpi * 8), rows), rpi = BWD_THREADS / cpr;
    #  apply grid g2 = min(ew_grid(nblk, bpi), rows) when dbias is asked for, bpi = POOL_THREADS / cpr, four adds per 2x2 block)
    rpi = 1024 // (C // vec)
    g1 = min(brows, max(1, min(4096, -(-MP // (rpi * 8)))))
    Kr = F64.chain_len(MP, g1, C, vec, 1024)
    (s1, s2), (m1, m2) = F64.pool_red_ref(g["dp"], pooled, coef)
    worst(F64.check_sum(dbet, s1, m1, Kr + 1, "pool_bn_bwd dbeta"))
    worst(F64.check_sum(dgam, s2, m2, F64.K_POOL_RED + Kr + 1, "pool_bn_bwd dgamma"))
    dz64, mag = F64.pool_bwd_ref(g["dp"], pooled, idx, H, W)
    k1 = gamma.double() * inv.double()
    want, A = F64.pool_dy_ref(dz64, mag, g["y"], coef, k1, dbet.double() / M, dgam.double() / M)
    worst(F64.check_stored(dy, want, A, F64.K_POOL_DY, bf16, "pool_bn_bwd dy"))
    nblk, bpi = N * ((H + 1) // 2) * ((W + 1) // 2), 512 // (C // vec)
    g2 = min(brows, max(1, min(4096, -(-nblk // bpi))))
    Kb = 4 * -(-nblk // (g2 * bpi)) + bpi
    s = dy.double().reshape(-1, C)
    worst(F64.check_sum(dbias, s.sum(0), s.abs().sum(0), Kb + 1, "pool_bn_bwd dbias"))
    # == max-pool backward + BatchNorm backward as two passes
    dy2 = nanbuf((N, H, W, C), TDT[dt])
    dgam2, dbet2, dbias2 = nanbuf(C), nanbuf(C), nanbuf(C)
    L.check(lib.ecgmm_bn_bwd(dt, ptr(dz), None, None, None, 1, ptr(yt), ptr(coef), ptr(gamma), ptr(dgam2), ptr(dbet2), ptr(dy2), None,
                             ptr(dbias2), M, C, ptr(scratch), stream()))
    torch.cuda.synchronize()
    res = F64.check_bn_bwd(dz.view(M, C).float(), g["y"].view(M, C), coef, gamma, bf16, F64.chain_len(M, brows, C, vec, 1024), dgam2, dbet2,
                           dy2.view(M, C), None, dbias2, F64.chain_len(M, brows, C, vec, 1024), name="two-pass bn_bwd")
    for k, v in res.items():
        worst(v, "two-pass " + k)
    tol = 2e-5 if dt == L.F32 else 1.5e-2

    def rel(a, b):
        return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    assert rel(dy.float(), dy2.float()) < tol and rel(dgam, dgam2) < tol and rel(dbet, dbet2) < tol
    worst.show("pooling %s %s" % (shape, "bf16" if bf16 else "fp32"))
