"""The LSTM recurrence (csrc/lstm.hip) against float64, element by element, at every tiling of the hidden size, and
HF.seq_mean, which feeds its output to the classifier.

Bounds and references: tests/f64check.py, "The LSTM recurrence": (a) the per-slice chain bar -- every time step of y / dx, every
(layer, direction) of the states and every parameter gradient within 8 x the worst slice of torch's own CPU fp32 run, no slice
skipped -- and (b) the derived bound of one step (T = 1), whose only measured constant is K_FN.  tests/test_lstm_gpu.py keeps
the whole-tensor 2e-5 bar and the module path.  Everything here goes through the C entry points (tests/lstm_abi.py): outputs
are NaN-filled views into one arena between sentinel zones, the workspace and the scratch are NaN-filled and followed by a
sentinel KiB, and every run checks every sentinel and that no NaN is left.  Each test prints its figures (run with -s).

What each group reaches in the kernels: the tile loop `ht = wave; ht * 16 < Hp; ht += 8` with H < 4, partial tiles, exactly
one (H = 128) and two (H = 256) tiles per wave, wave 0 alone taking a second one (H = 132), the cap H = 384 (148 224 B of LDS
in the backward); the scalar W_hh load for an aligned H behind a misaligned pointer; the two alternating layer-output buffers
of the save_for_backward = 0 forward (3 and 4 layers); 8 layers; T = 1 through the backward's `first` branch; every optional
pointer of the ABI null; stores of masked rows (the sentinels); causality and row independence bit for bit.

Measured on the MI355X (1 is the limit; the module runs in under 5 s, no test above 0.8 s):
  single step, worst |err| / bound per H over B in {1, 16, 17}, In in {3, 24}, one and two directions: H = 1 0.085, 4 0.143,
    16 0.097, 37 0.032, 128 0.013, 132 0.017, 200 0.012, 256 0.0084, 380 0.0056, 384 0.0066; saturated 0.0063.  Function error
    seen beyond the bound's other terms: 0.00 u at every case, hence K_FN = 0 (f64check.py); hn == y bit for bit everywhere
  per-slice chain bar, worst slice of the worst tensor (ours / torch fp32's own worst slice of the case, in u = 2^-24):
    t70_hn_only 0.154 (cn; 5.7 / 22.1), h132_cn_only 0.206 (dweight_hh; 24.1 / 19.6), h384_cap 0.346 (dx; 40.6 / 27.4),
    h128 0.144, h256 0.242 (dx; 24.7 / 23.7), layers8 0.196 (32.1 / 45.6), t1x2 0.25, h1 0.562 (dc0; 10.1 / 13.9)
  misaligned W_hh: 0.145 (H = 8), 0.185 (H = 200), every tensor bit-identical to the aligned run
  no-save forward: 0.127 (3 layers), 0.154 (4 layers), bit-identical to the saving forward
  dy null: 0.183;  dx of 5 rows alone and among 33: 0.114 both;  no sentinel touched, no NaN left in any run
  seq_mean, forward / backward: (8, 9, 400) 0.27 / 0.55, (3, 70, 64) 0.02 / 0.47, (5, 1, 6) 0 / 0, (2, 8, 1024) 0.23 / 0,
    (17, 5, 400) 0.38 / 0.60
One defect found: with dweight_ih null, dbias_ih came from another kernel than with it (ecg_linear_bwd's VALU route sums db
beside dw) and differed in the last bits; ecg_lstm_backward now sums both bias gradients with ecg_rows_sum whatever else is
requested (test_null_pointers_leave_the_rest_bit_identical[w_ih]), so dbias_ih == dbias_hh bit for bit.
"""
import pytest
import torch

from ecgmm.hip import functional as HF

from . import f64check as F64
from . import lstm_abi
from .test_lstm_gpu import SMALL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = F64.U
ALL = ("y", "h", "c")


def cpu(out):
    return {k: v.detach().cpu() for k, v in out.items()}


# ----------------------------------------------------------------------------------------------------------------------
# (b) one step against the float64 cell
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", F64.LSTM_STEP_H)
def test_single_step_forward_bound(H):
    worst, seen = 0.0, 0.0
    for B in F64.LSTM_STEP_B:
        for In in F64.LSTM_STEP_IN:
            for bi in (False, True):
                case = F64.lstm_step_case(B, In, H, bi)
                ins = F64.lstm_inputs(case)
                out = cpu(lstm_abi.run(case, ins, backward=False))
                r = F64.lstm_step_check(out, ins, "H=%d B=%d In=%d D=%d" % (H, B, In, 1 + bi))
                worst, seen = max(worst, r.ratio), max(seen, r.fn_seen)
    print("[lstm step] H = %d: worst ratio to the bound %.3g, function error seen %.2f u (K_FN = %g)" % (H, worst, seen, F64.K_FN))


def test_single_step_forward_bound_saturated():
    case = F64.lstm_step_case(17, 24, 132, True)
    ins = F64.lstm_inputs(case, 3.0, 4.0)
    out = cpu(lstm_abi.run(case, ins, backward=False))
    F64.lstm_step_check(out, ins, "saturated (weights x3, inputs x4) H=132")


# ----------------------------------------------------------------------------------------------------------------------
# (a) the per-slice chain bar
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,use", F64.LSTM_CHAIN_CASES, ids=F64.LSTM_CHAIN_IDS)
def test_every_slice_against_float64(case, use):
    r64, r32 = F64.lstm_refs(case, use)
    out = cpu(lstm_abi.run(case, F64.lstm_inputs(case), use=use))
    assert set(out) == set(r64)
    for k in out:       # both bias gradients are the column sums of the same gate gradients, summed by the same kernel
        if k.startswith("dbias_ih"):
            assert torch.equal(out[k], out[k.replace("dbias_ih", "dbias_hh")]), k
    F64.lstm_chain_check(out, r64, r32, case[6], "chain " + F64.LSTM_CHAIN_IDS[F64.LSTM_CHAIN_CASES.index((case, use))], quiet=False)


@pytest.mark.parametrize("case", [(5, 6, 16, 8, 1, True, True, True), (17, 4, 24, 200, 1, True, True, True)], ids=["h8", "h200"])
def test_misaligned_w_hh_takes_the_scalar_load(case):
    r64, r32 = F64.lstm_refs(case, ALL)
    ins = F64.lstm_inputs(case)
    mis = cpu(lstm_abi.run(case, ins, misalign_whh=True))
    F64.lstm_chain_check(mis, r64, r32, case[6], "misaligned W_hh H=%d" % case[3])
    ali = cpu(lstm_abi.run(case, ins))
    same = [k for k in ali if torch.equal(ali[k], mis[k])]
    print("[lstm f64] misaligned W_hh H=%d: bit-identical to the aligned run in %d of %d tensors%s" %
          (case[3], len(same), len(ali), "" if len(same) == len(ali) else " (differ: %s)" % sorted(set(ali) - set(same))))


@pytest.mark.parametrize("layers", [3, 4])
def test_no_save_forward_alternates_its_two_buffers(layers):
    case = (5, 4, 12, 37, layers, True, True, True)
    r64, r32 = F64.lstm_refs(case, ALL)
    ins = F64.lstm_inputs(case)
    lean = cpu(lstm_abi.run(case, ins, save=0, backward=False))
    F64.lstm_chain_check(lean, r64, r32, case[6], "no-save forward, %d layers" % layers, keys=("y", "hn", "cn"))
    full = cpu(lstm_abi.run(case, ins, save=1, backward=False))
    for k in ("y", "hn", "cn"):
        assert torch.equal(lean[k], full[k]), k


# ----------------------------------------------------------------------------------------------------------------------
# the optional pointers of the ABI
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_full():
    return cpu(lstm_abi.run(SMALL, F64.lstm_inputs(SMALL)))


def same_as(full, part, gone):
    assert set(part) == set(full) - set(gone), (sorted(part), gone)
    for k in part:
        assert torch.equal(part[k], full[k]), k


NAMES = [n for n, _ in F64.lstm_inputs(SMALL)[0].named_parameters()]
ENTRY = 12      # layer 1, reverse direction: entries 12 .. 15 of the parameter table


@pytest.mark.parametrize("null,gone", [
    (("hn", "cn"), ("hn", "cn")),
    (("grads",), tuple("d" + n for n in NAMES)),
    ((("grad", ENTRY),), ("d" + NAMES[ENTRY],)),
    ((("grad", ENTRY + 1),), ("d" + NAMES[ENTRY + 1],)),
    ((("grad", ENTRY + 2),), ("d" + NAMES[ENTRY + 2],)),
    ((("grad", ENTRY + 3),), ("d" + NAMES[ENTRY + 3],)),
    (("dx",), ("dx",)),
    (("dh0", "dc0"), ("dh0", "dc0")),
], ids=["hn_cn", "grads", "w_ih", "w_hh", "b_ih", "b_hh", "dx", "dh0_dc0"])
def test_null_pointers_leave_the_rest_bit_identical(small_full, null, gone):
    same_as(small_full, cpu(lstm_abi.run(SMALL, F64.lstm_inputs(SMALL), null=null)), gone)


def test_null_dy_is_a_zero_dy():
    ins = F64.lstm_inputs(SMALL)
    r64, r32 = F64.lstm_refs(SMALL, ("h",))
    out = cpu(lstm_abi.run(SMALL, ins, use=("h",)))
    F64.lstm_chain_check(out, r64, r32, SMALL[6], "dy null, dhn only")
    zero = ins[:4] + (torch.zeros_like(ins[4]),) + ins[5:]
    same_as(cpu(lstm_abi.run(SMALL, zero, use=("y", "h"))), out, ())


def test_the_sentinels_see_a_stray_store():
    ar = lstm_abi.Arena({"a": (5, 3), "b": (7,)})
    assert not ar.touched()
    ar.views["a"].fill_(1.0)
    assert not ar.touched()
    ar.buf[lstm_abi.GUARD + 15] = 0.0          # the float right behind "a"
    assert ar.touched() == ["a+15"]
    t = lstm_abi.guarded_bytes(64)
    assert not lstm_abi.tail_touched(t)
    t[16] = 0.0
    assert lstm_abi.tail_touched(t)


@pytest.mark.parametrize("case", [(17, 3, 8, 37, 2, True, True, True), (1, 3, 8, 384, 1, False, True, True)], ids=["b17h37", "b1h384"])
def test_nothing_is_written_outside_the_outputs(case):
    """lstm_abi.run checks every sentinel zone around every output, the KiB behind the workspace and the scratch, and that
    every element of every output is finite"""
    out = lstm_abi.run(case, F64.lstm_inputs(case))
    assert len(out) == 6 + 4 * case[4] * (2 if case[5] else 1)


# ----------------------------------------------------------------------------------------------------------------------
# causality and row independence, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def test_causality_of_both_directions():
    case = (5, 9, 12, 37, 1, True, True, False)
    H = case[3]
    ins = F64.lstm_inputs(case)
    base = cpu(lstm_abi.run(case, ins, backward=False))["y"]
    noise = torch.randn(ins[1].shape, generator=torch.Generator().manual_seed(3))
    late, early = ins[1].clone(), ins[1].clone()
    late[:, 5:] += noise[:, 5:]
    early[:, :5] += noise[:, :5]
    y_late = cpu(lstm_abi.run(case, (ins[0], late) + ins[2:], backward=False))["y"]
    y_early = cpu(lstm_abi.run(case, (ins[0], early) + ins[2:], backward=False))["y"]
    assert torch.equal(y_late[:, :5, :H], base[:, :5, :H]) and not torch.equal(y_late[:, 5:, :H], base[:, 5:, :H])
    assert torch.equal(y_early[:, 5:, H:], base[:, 5:, H:]) and not torch.equal(y_early[:, :5, H:], base[:, :5, H:])


def test_causality_of_the_backward():
    case = (5, 9, 12, 37, 1, False, True, False)
    ins = F64.lstm_inputs(case)
    base = cpu(lstm_abi.run(case, ins, use=("y",)))["dx"]
    gy = ins[4].clone()
    gy[:, :5] += torch.randn(gy[:, :5].shape, generator=torch.Generator().manual_seed(4))
    dx = cpu(lstm_abi.run(case, ins[:4] + (gy,) + ins[5:], use=("y",)))["dx"]
    assert torch.equal(dx[:, 5:], base[:, 5:]) and not torch.equal(dx[:, :5], base[:, :5])


def test_backward_rows_do_not_depend_on_the_rest_of_the_batch():
    """dh0 / dc0 come straight from the recurrence kernel: bit for bit.  dx goes through a GEMM whose route may depend on the
    row count: within the chain bar of the 5-row problem."""
    big, small = (33, 6, 16, 37, 1, True, True, True), (5, 6, 16, 37, 1, True, True, True)
    mod, x, h0, c0, gy, gh, gc = F64.lstm_inputs(big)
    ins5 = (mod, x[:5].contiguous(), h0[:, :5].contiguous(), c0[:, :5].contiguous(), gy[:5].contiguous(), gh[:, :5].contiguous(),
            gc[:, :5].contiguous())
    o33 = cpu(lstm_abi.run(big, F64.lstm_inputs(big)))
    o5 = cpu(lstm_abi.run(small, ins5))
    for k in ("y", "hn", "cn", "dh0", "dc0"):
        a = o33[k][:5] if k == "y" else o33[k][:, :5]
        assert torch.equal(a, o5[k]), k
    r64, r32 = F64.lstm_run(ins5, torch.float64), F64.lstm_run(ins5, torch.float32)
    F64.seq_chain_check(o5["dx"], r64["dx"], r32["dx"], 1, "dx at B = 5")
    F64.seq_chain_check(o33["dx"][:5], r64["dx"], r32["dx"], 1, "dx[:5] at B = 33")


# ----------------------------------------------------------------------------------------------------------------------
# HF.seq_mean
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 9, 400), (3, 70, 64), (5, 1, 6), (2, 8, 1024), (17, 5, 400)], ids=str)
def test_seq_mean_against_float64(shape):
    """forward: |out - ref| <= g_k(T + 1) * mean_t |x| (T - 1 additions in any order, the scale, one spare);
    backward: |dx - ref| <= g_k(2) * |dy| / T (the fp32 value of 1 / T and the product)"""
    B, T, Cn = shape
    g = torch.Generator().manual_seed(B * 1000 + T)
    x, dy = torch.randn(shape, generator=g) + 0.3, torch.randn(B, Cn, generator=g)
    xd = x.to(DEV).requires_grad_()
    out = HF.seq_mean(xd)
    assert tuple(out.shape) == (B, Cn) and out.is_contiguous()
    filler = torch.full(shape, float("nan"), device=DEV)      # what the backward's torch.empty most likely gets
    del filler
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    dx = xd.grad.cpu()
    assert tuple(dx.shape) == shape and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(out).all())
    x64 = x.double()
    rf = F64._ratio((out.detach().cpu().double() - x64.mean(1)).abs(), F64.g_k(T + 1) * x64.abs().mean(1))
    ref_dx = (dy.double() / T)[:, None, :].expand(shape)
    rb = F64._ratio((dx.double() - ref_dx).abs(), F64.g_k(2) * ref_dx.abs())
    print("[seq_mean] %s: worst ratio to the bound: forward %.3g, backward %.3g" % (shape, float(rf.max()), float(rb.max())))
    assert float(rf.max()) <= 1.0 and float(rb.max()) <= 1.0


def test_seq_mean_refuses_more_than_1024_columns():
    with pytest.raises(RuntimeError, match="above 1024 is not supported"):
        HF.seq_mean(torch.zeros(2, 3, 1028, device=DEV))
