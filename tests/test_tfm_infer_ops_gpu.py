"""The two fused layer tails of csrc/transformer_infer.hip and the plan built on them, through the C ABI between sentinel
zones (tests/tfm_infer_abi.py): every element within its float64 bound (tests/tfm_infer_bounds.py, nothing tuned), nothing
written outside an output, two calls the same bits, a row's bits independent of R and of its place in a tile, and the plan
equal bit for bit to the same forward from the per-op entry points in separate buffers (the check on its workspace rotation).

The row tile of a workgroup is 64 rows, four waves of 16.  R runs over 1, the rows below, at and above 16, 32 and 64, and
130 (three workgroups, the last one ragged)."""
import pytest
import torch

from . import tfm_infer_abi as A
from . import tfm_infer_bounds as TB
from . import tfm_infer_ref as TR

pytestmark = pytest.mark.gpu
ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
RMAX = max(ROWS)
ALONE = [0, 15, 16, 31, 32, 47, 63, 64, 129]   # rows re-run alone (R = 1): first / last of a wave's 16-row tile, of a workgroup, of the call
EPS = 1e-5


def _judge(name, got, f, bound_fn):
    bound, r = bound_fn(f)
    ratio = TB.ratio((got.cpu().double() - f.n.y).abs(), bound)
    print("%-46s worst error / bound %.3g   (r = %.3g)" % (name, ratio, r))
    assert r < TB.R_MAX, "%s: the case leaves the bound's first-order range (r = %.3g)" % (name, r)
    assert ratio <= 1.0, "%s: error %.3g x its bound" % (name, ratio)
    return ratio


def _rows_and_repeats(name, run, full):
    """full = run(R = RMAX): every smaller R gives the first R rows of it, a row alone gives that row, a repeat the same bits"""
    assert torch.equal(run(R=RMAX), full), name + ": two identical calls differ"
    for R in ROWS[:-1]:
        assert torch.equal(run(R=R), full[:R]), "%s: the rows of an R = %d call are not those of the R = %d call" % (name, R, RMAX)
    for r in ALONE:
        assert torch.equal(run(rows=slice(r, r + 1)), full[r:r + 1]), "%s: row %d alone differs from row %d of %d" % (name, r, r, RMAX)


@pytest.mark.parametrize("K", [16, 128, 256])
@pytest.mark.parametrize("E", [16, 64, 128, 256])
def test_linear_res_ln(E, K):
    c = TR.linear_case(RMAX, K, E, seed=E + K)
    f = TR.linear_res_ln(c["a"], c["w"], c["b"], c["res"], c["gamma"], c["beta"], EPS)
    d = A.to_dev(c)
    run = lambda **kw: A.linear_res_ln(d, eps=EPS, **kw)
    full = run(R=RMAX)
    _judge("linear_res_ln E%d K%d" % (E, K), full, f, TB.linear_res_ln)
    _rows_and_repeats("linear_res_ln E%d K%d" % (E, K), run, full)


@pytest.mark.parametrize("ff", [16, 128, 256])
@pytest.mark.parametrize("E", [16, 64, 128, 256])
def test_ffn_res_ln(E, ff):
    c = TR.ffn_case(RMAX, E, ff, seed=E + ff)
    f = TR.ffn_res_ln(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["gamma"], c["beta"], EPS)
    d = A.to_dev(c)
    run = lambda **kw: A.ffn_res_ln(d, eps=EPS, **kw)
    full = run(R=RMAX)
    _judge("ffn_res_ln E%d ff%d" % (E, ff), full, f, TB.ffn_res_ln)
    _rows_and_repeats("ffn_res_ln E%d ff%d" % (E, ff), run, full)


@pytest.mark.parametrize("what,kw", [("ff 2048", dict(R=65, E=128, ff=2048)), ("odd chunk count, guarded tiles", dict(R=33, E=48, ff=48)),
                                     ("small variance", dict(R=65, E=128, ff=256, small_var=True)),
                                     ("input scale 30", dict(R=65, E=128, ff=256, scale=30.0))])
def test_ffn_res_ln_special_cases(what, kw):
    c = TR.ffn_case(kw.pop("R"), kw.pop("E"), kw.pop("ff"), seed=7, **kw)
    f = TR.ffn_res_ln(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["gamma"], c["beta"], EPS)
    d = A.to_dev(c)
    got = A.ffn_res_ln(d, eps=EPS)
    _judge("ffn_res_ln " + what, got, f, TB.ffn_res_ln)
    assert torch.equal(A.ffn_res_ln(d, eps=EPS), got)
    assert torch.equal(A.ffn_res_ln(d, rows=slice(20, 21), eps=EPS), got[20:21])


@pytest.mark.parametrize("what,kw", [("K 2048", dict(R=65, K=2048, E=128)), ("guarded tiles", dict(R=33, K=48, E=80)),
                                     ("small variance", dict(R=65, K=128, E=128, small_var=True)),
                                     ("input scale 30", dict(R=65, K=128, E=128, scale=30.0))])
def test_linear_res_ln_special_cases(what, kw):
    c = TR.linear_case(kw.pop("R"), kw.pop("K"), kw.pop("E"), seed=7, **kw)
    f = TR.linear_res_ln(c["a"], c["w"], c["b"], c["res"], c["gamma"], c["beta"], EPS)
    d = A.to_dev(c)
    got = A.linear_res_ln(d, eps=EPS)
    _judge("linear_res_ln " + what, got, f, TB.linear_res_ln)
    assert torch.equal(A.linear_res_ln(d, eps=EPS), got)
    assert torch.equal(A.linear_res_ln(d, rows=slice(20, 21), eps=EPS), got[20:21])


def test_the_python_wrappers_give_the_abi_bits():
    from ecgmm.hip import functional as HF
    c, f = A.to_dev(TR.linear_case(37, 64, 64, seed=1)), A.to_dev(TR.ffn_case(37, 64, 128, seed=1))
    with torch.no_grad():
        assert torch.equal(HF.linear_res_ln(c["a"], c["w"], c["b"], c["res"], c["gamma"], c["beta"], EPS), A.linear_res_ln(c, eps=EPS))
        assert torch.equal(HF.ffn_res_ln(f["x"], f["w1"], f["b1"], f["w2"], f["b2"], f["gamma"], f["beta"], EPS), A.ffn_res_ln(f, eps=EPS))


@pytest.mark.parametrize("batch_first,lengths", [(1, None), (1, "lengths"), (0, None)], ids=["time", "time-lengths", "across"])
@pytest.mark.parametrize("B,Ln,E,heads,ff,layers", [(3, 40, 64, 4, 128, 2), (5, 17, 128, 4, 256, 1)])
def test_plan_equals_the_per_op_forward_bit_for_bit(B, Ln, E, heads, ff, layers, batch_first, lengths):
    p = A.plan_params(B, Ln, 1, E, heads, ff, layers, 2, seed=B)
    x = torch.randn(B, 1, Ln, generator=torch.Generator().manual_seed(B + Ln)).to(A.DEV)
    if lengths is not None:
        lengths = torch.tensor([Ln, 1, Ln // 2, 9, Ln - 1][:B], dtype=torch.int32, device=A.DEV)
    want, calls = A.per_op_forward(p, x, lengths, heads, batch_first, EPS)
    got = A.plan_forward(p, x, lengths, heads, batch_first, EPS)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want), "the plan's logits are not those of the per-op forward: max |d| %.3g" % float((got - want).abs().max())
    assert torch.equal(A.plan_forward(p, x, lengths, heads, batch_first, EPS), got), "two identical plan calls differ"
    # four launches per layer: that is the sequence the plan runs
    assert calls.per_layer == [4] * layers
    assert calls.total == 1 + 4 * layers + 3
    if lengths is not None:   # the plan zeroes the raw padding itself: NaN there changes nothing
        xn = x.clone()
        for b in range(B):
            xn[b, :, int(lengths[b]):] = float("nan")
        assert torch.equal(A.plan_forward(p, xn, lengths, heads, batch_first, EPS), got)


def test_plan_takes_a_width_the_pooling_kernel_does_not():
    """E = 48 without lengths: the mean runs as the masked mean over full lengths; against float64 torch within the chain bar
    of tests/f64check.py would need a model -- here: equal to the plan with explicit full lengths, whose mean is that kernel"""
    B, Ln, E, heads, ff = 3, 21, 48, 3, 80
    p = A.plan_params(B, Ln, 2, E, heads, ff, 1, 3, seed=9)
    x = torch.randn(B, 2, Ln, generator=torch.Generator().manual_seed(4)).to(A.DEV)
    full = torch.full((B,), Ln, dtype=torch.int32, device=A.DEV)
    a, b = A.plan_forward(p, x, None, heads, 1, EPS), A.plan_forward(p, x, full, heads, 1, EPS)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
