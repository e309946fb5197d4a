"""The channel-sliced launch of the folded BatchNorm passes (csrc/elementwise.hip: ChanSlice, bn_fold_slices) through the
per-op C ABI: ecgmm_bn_act_from_rows(_bits), ecgmm_bn_bwd(_bits) and ecgmm_bn_bwd_from_rows, bf16 and fp32.

C = 256 and 512 are sliced (NS = 2, 4), C = 128 keeps the unsliced launch.  A sliced workgroup walks 64 rows (bf16; 32 in
fp32) of 128 channels per iteration: M = 1 and 63 are fewer rows than one iteration, 64 / 65 one iteration and a ragged
second, 1000 several pixel chunks next to the NS slices.  The partial rows (1, 7, 256, 512 of them: a single row, fewer
than the 8 row slices of the fold, its four-rows-per-trip loop, the longest buffer it accepts) are built on the host from
float64 column sums, so that their number does not depend on M.  gamma has negative entries, the gate runs with
rows_per_sample = 7, the residual carries rcoef, bf16 writes and reads the ReLU bit mask.

(a) every output is bit-identical between ecgmm_bn_fold_slice(1) and (0);
(b) the switch-on results are checked element by element against float64 with the checkers and constants of
    tests/f64check.py, exactly as tests/test_bn_pool_f64_gpu.py uses them for the same passes;
(c) num_batches_tracked advances by exactly 1 per call.
Every output buffer is NaN-filled (0xAA for the bit mask) before each call.
"""
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import f64check as F64
from .util import DEV, TDT, dev, switches

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64
RPS = 7

# (M, partial rows): every M and every row count of the issue, each row count with a small and a large M
CASES = [(1, 7), (63, 1), (64, 512), (65, 256), (1000, 512), (1000, 7), (1000, 1), (63, 256)]
PARAMS = [(C, M, rows, dt) for C in (128, 256, 512) for (M, rows) in CASES for dt in (L.BF16, L.F32)]
_inputs = {}


def nanbuf(n, dtype=torch.float32):
    return torch.full((n,) if isinstance(n, int) else n, NAN, device=DEV, dtype=dtype)


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits_of(a) == bits_of(b)).all())


def inputs(M, C, dt):
    """uploaded once per (M, C, dtype) and left unchanged; gamma negative in the first and the last slice"""
    key = (M, C, dt)
    if key not in _inputs:
        bf16 = dt == L.BF16
        rps = RPS if M > 1 else None
        d = F64.bn_inputs(M, C, bf16, rps)
        d["gamma"][3] = -d["gamma"][3]
        d["gamma"][C - 2] = -d["gamma"][C - 2]
        g = {k: dev(v) for k, v in d.items() if torch.is_tensor(v)}
        for k in ("y", "res", "dout"):
            g[k + "_t"] = g[k].to(TDT[dt]).contiguous()
        g["rcoef"] = torch.stack([g["rscale"], g["rshift"]]).contiguous()
        g["rps"] = rps or 1
        g["gate_rows"] = F64.per_row(g["gate"], g["rps"], M)
        g["addc_rows"] = F64.per_row(g["addc"], g["rps"], M)
        _inputs[key] = g
    return _inputs[key]


def split_rows(a, b, rows):
    """[M][C] float64 terms a, b -> fp32 partial rows [rows + TAIL][2][C] (NaN tail): row k sums the pixels i = k mod rows"""
    M, C = a.shape
    k = torch.arange(M, device=a.device) % rows
    part = torch.zeros(rows, 2, C, dtype=torch.float64, device=a.device)
    part[:, 0].index_add_(0, k, a)
    part[:, 1].index_add_(0, k, b)
    return torch.cat([part.float(), nanbuf((TAIL, 2, C))]).contiguous()


def fold_sliced(lib, sliced):
    """fold on, slicing as asked; both back to what ecgmm_switch_get returned before"""
    return switches(lib, ECGMM_BN_FOLD=1, ECGMM_BN_FOLD_SLICE=sliced)


@pytest.mark.parametrize("C,M,rows,dt", PARAMS)
def test_folded_bn_act_sliced(C, M, rows, dt):
    lib = L.lib()
    bf16 = dt == L.BF16
    g = inputs(M, C, dt)
    y64 = g["y"].double()
    partial = split_rows(y64, y64 * y64, rows)

    def run(sliced):
        coef, rm, rv = nanbuf((4, C)), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        nbt = torch.full((), 6, dtype=torch.int64, device=DEV)
        out = nanbuf(M * C, TDT[dt])
        bits = torch.full((M * C // 8,), 0xAA, dtype=torch.uint8, device=DEV) if bf16 else None
        with fold_sliced(lib, sliced):
            for n in (7, 8):
                if n == 8:                      # (the second call starts from the first call's running statistics)
                    rm1, rv1 = rm.clone(), rv.clone()
                L.check(lib.ecgmm_bn_act_from_rows_bits(dt, ptr(g["y_t"]), ptr(partial), rows, float(M), ptr(g["gamma"]), ptr(g["beta"]),
                                                        ptr(rm), ptr(rv), ptr(nbt), 0.1, 1e-5, ptr(coef), ptr(g["res_t"]), ptr(g["rcoef"]),
                                                        ptr(g["gate"]), g["rps"], 1, ptr(out), ptr(bits) if bf16 else None, M, C, stream()))
                torch.cuda.synchronize()
                assert int(nbt) == n                                                             # (c)
        assert torch.isnan(partial[rows:]).all()
        return dict(out=out, coef=coef, rm=rm, rv=rv, rm1=rm1, rv1=rv1, bits=bits)

    on, off = run(1), run(0)
    for k in ("out", "coef", "rm", "rv", "rm1", "rv1"):
        assert same_bits(on[k], off[k]), "%s differs between the sliced and the unsliced launch" % k                    # (a)
    r64 = partial[:rows].double()
    cref = F64.coef_ref(r64[:, 0].sum(0), r64[:, 1].sum(0), M, g["gamma"], g["beta"], 1e-5, torch.zeros(C, device=DEV),
                        torch.ones(C, device=DEV), 0.1)
    assert torch.isfinite(on["coef"]).all() and torch.isfinite(on["out"].float()).all()
    F64.check_coef(on["coef"], cref, on["rm1"], on["rv1"], name="sliced bn_act_from_rows coef")                        # (b)
    want, A = F64.bn_act_ref(g["y"], cref.val["scale"], cref.val["shift"], g["res"], g["rscale"], g["rshift"], g["gate_rows"], True)
    extra = (g["y"].double().abs() * cref.bound["scale"] + cref.bound["shift"]) * g["gate_rows"].abs()
    F64.check_stored(on["out"].view(M, C), want, A + extra / F64.g_k(F64.K_ACT), F64.K_ACT, bf16, "sliced bn_act_from_rows out")
    if bf16:
        assert bool((on["bits"] == off["bits"]).all())
        w = 1 << torch.arange(8, device=DEV, dtype=torch.int32)
        expect = ((on["out"].view(M, C // 8, 8).float() > 0).int() * w).sum(2).to(torch.uint8).view(-1)
        assert bool((on["bits"] == expect).all()), "relu_bits is not the sign mask of the stored output"


@pytest.mark.parametrize("C,M,rows,dt", PARAMS)
def test_folded_bn_bwd_sliced(C, M, rows, dt):
    lib = L.lib()
    bf16 = dt == L.BF16
    vec = 8 if bf16 else 4
    g = inputs(M, C, dt)
    y64 = g["y"].double()
    # forward coefficients and a ReLU'd tensor / its bit mask as the separate mask reference (unsliced, fold off: not under test)
    stat = split_rows(y64, y64 * y64, 7)
    coef = nanbuf((4, C))
    maskt = nanbuf(M * C, TDT[dt])
    mbits = torch.zeros(M * C // 8, dtype=torch.uint8, device=DEV)
    L.check(lib.ecgmm_bn_finalize(ptr(stat), 7, C, float(M), ptr(g["gamma"]), ptr(g["beta"]), None, None, None, 0.1, 1e-5, ptr(coef), stream()))
    L.check(lib.ecgmm_bn_act(dt, ptr(g["y_t"]), ptr(coef), ptr(g["res_t"]), None, None, 1, 1, ptr(maskt), M, C, stream()))
    torch.cuda.synchronize()
    if bf16:
        w = 1 << torch.arange(8, device=DEV, dtype=torch.int32)
        mbits = ((maskt.view(M, C // 8, 8).float() > 0).int() * w).sum(2).to(torch.uint8).view(-1).contiguous()
    nscratch = lib.ecgmm_bn_bwd_scratch(dt, M, C) // 4
    brows = (nscratch - 3 * C) // (2 * C) - TAIL
    K = F64.chain_len(M, brows, C, vec, 1024)
    # reduction rows of (sum g, sum g * (y - mean)), g = [bn(y) > 0] * dout, as the producing dgrad's epilogue writes them
    mask, _ = F64.affine_mask(g["y"], coef[0], coef[1])
    gm = torch.where(mask, g["dout"].double(), torch.zeros_like(y64))
    red = split_rows(gm, gm * (y64 - coef[2].double()), rows)

    def run(form, sliced):
        scratch = nanbuf(nscratch)
        dgam, dbet = nanbuf(C), nanbuf(C)
        dy, dz = nanbuf(M * C, TDT[dt]), nanbuf(M * C, TDT[dt])
        with fold_sliced(lib, sliced):
            if form == "gated":       # mask tensor + dz_out, gate and addc with rows_per_sample = 7
                L.check(lib.ecgmm_bn_bwd(dt, ptr(g["dout_t"]), ptr(maskt), ptr(g["gate"]), ptr(g["addc"]), g["rps"], ptr(g["y_t"]),
                                         ptr(coef), ptr(g["gamma"]), ptr(dgam), ptr(dbet), ptr(dy), ptr(dz), None, M, C, ptr(scratch), stream()))
            elif form == "bits":      # the bit mask, read by the apply pass itself (no dz_out)
                L.check(lib.ecgmm_bn_bwd_bits(dt, ptr(g["dout_t"]), ptr(mbits), None, None, 1, ptr(g["y_t"]), ptr(coef), ptr(g["gamma"]),
                                              ptr(dgam), ptr(dbet), ptr(dy), None, None, M, C, ptr(scratch), stream()))
            else:                     # finalize + apply from `rows` given rows, mask recomputed from y
                L.check(lib.ecgmm_bn_bwd_from_rows(dt, ptr(g["dout_t"]), ptr(g["y_t"]), ptr(g["y_t"]), ptr(coef), ptr(g["gamma"]), ptr(dgam),
                                                   ptr(dbet), ptr(dy), ptr(red), rows, M, C, ptr(scratch), stream()))
            torch.cuda.synchronize()
        return dict(dy=dy, dz=dz, dgamma=dgam, dbeta=dbet)

    # (the row count only reaches the from_rows form: the other two run once per M)
    once = rows == next(r for (m, r) in CASES if m == M)
    for form in ("from_rows",) + (("gated",) + (("bits",) if bf16 else ()) if once else ()):
        on, off = run(form, 1), run(form, 0)
        for k in ("dy", "dgamma", "dbeta") + (("dz",) if form == "gated" else ()):
            assert same_bits(on[k], off[k]), "%s: %s differs between the sliced and the unsliced launch" % (form, k)     # (a)
        for k in ("dy", "dgamma", "dbeta"):
            assert torch.isfinite(on[k].float()).all()
        gated = form == "gated"
        F64.check_bn_bwd(g["dout"], g["y"], coef, g["gamma"], bf16, 1 if form == "from_rows" else K, on["dgamma"], on["dbeta"],        # (b)
                         on["dy"].view(M, C), on["dz"].view(M, C) if gated else None,
                         maskref="y" if form == "from_rows" else maskt.view(M, C),
                         gate=g["gate_rows"] if gated else None, addc=g["addc_rows"] if gated else None, name="sliced bn_bwd " + form)
    assert torch.isnan(red[rows:]).all()
