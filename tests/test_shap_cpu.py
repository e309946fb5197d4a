"""tests/shap_ref.py against independent float64 statements in torch, the host-side draws of ecgmm.shap_explainers, the
workspace query and every refusal (none of which needs a GPU), and the cap on undecided gates that the end-to-end GPU test
relies on."""
import numpy as np
import pytest
import torch

from ecgmm import shap_explainers as SE
from ecgmm import shap_fusion_modal_balance as X
from ecgmm.hip import lib as L
from ecgmm.hip import nn as hnn

from . import shap_bounds as Bd
from . import shap_ref as R


def _torch_mlp(w1, b1, w2, b2, relu=None, dtype=torch.float64):
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype)
    relu = relu or torch.relu
    return lambda p: relu(p @ t(w1).T + t(b1)) @ t(w2).T + t(b2)


def test_expected_gradients_equal_torch_float64_autograd():
    B, N, K, D, H, C = 3, 6, 9, 37, 11, 3
    x, bg, w1, b1, w2, b2 = R.make_inputs(B, N, D, H, C, seed=1)
    ridx, t = R.make_draws(B, N, K, seed=2)
    phi, var = R.expected_gradients(x, bg, ridx, t, w1, b1, w2)
    f = _torch_mlp(w1, b1, w2, b2)
    x64, bg64, t64 = (torch.from_numpy(a.astype(np.float64)) for a in (x, bg, t))
    prods = torch.zeros(B, K, C, D, dtype=torch.float64)
    for k in range(K):
        base = bg64[torch.from_numpy(ridx[:, k].astype(np.int64))]
        p = (t64[:, k:k + 1] * x64 + (1 - t64[:, k:k + 1]) * base).requires_grad_(True)
        out = f(p)
        for c in range(C):
            g, = torch.autograd.grad(out[:, c].sum(), p, retain_graph=True)
            prods[:, k, c] = g * (x64 - base)
    want = prods.mean(1).permute(0, 2, 1).numpy()
    want_var = (prods.var(1, unbiased=False) / np.sqrt(K)).permute(0, 2, 1).numpy()
    assert phi.shape == (B, D, C) and np.abs(phi - want).max() < 1e-12
    assert np.abs(var - want_var).max() < 1e-12 and want_var.max() > 0


class _RescaleReLU(torch.autograd.Function):
    """the hook shap's PyTorch DeepExplainer puts on a ReLU (nonlinear_1d): the batch is [x tiled; background]"""

    @staticmethod
    def forward(ctx, inp):
        out = inp.clamp(min=0)
        ctx.save_for_backward(inp, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        inp, out = ctx.saved_tensors
        half = inp.shape[0] // 2
        d_in, d_out = inp[:half] - inp[half:], out[:half] - out[half:]
        small = (d_in.abs() < 1e-6).repeat(2, 1)
        ratio = (d_out / torch.where(d_in.abs() < 1e-6, torch.ones_like(d_in), d_in)).repeat(2, 1)
        return torch.where(small, grad_out * (inp > 0), grad_out * ratio)


def test_deeplift_equals_the_rescale_hook_on_the_joint_batch_and_sums_to_delta():
    B, N, D, H, C = 3, 5, 29, 13, 2
    x, bg, w1, b1, w2, b2 = R.make_inputs(B, N, D, H, C, seed=3)
    bg[2] = x[1]                                   # zx - zb = 0 exactly: the < 1e-6 branch
    phi = R.deeplift(x, bg, w1, b1, w2)
    f = _torch_mlp(w1, b1, w2, b2, relu=_RescaleReLU.apply)
    x64, bg64 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(bg.astype(np.float64))
    want = np.zeros((B, D, C))
    for b in range(B):
        joint = torch.cat([x64[b:b + 1].repeat(N, 1), bg64]).requires_grad_(True)
        out = f(joint)
        for c in range(C):
            g, = torch.autograd.grad(out[:, c].sum(), joint, retain_graph=True)
            want[b, :, c] = (g[N:] * (x64[b:b + 1] - bg64)).mean(0).numpy()
    assert R.rescale_branch(R.preact(x, w1, b1), R.preact(bg, w1, b1))[1, 2].all()
    assert np.abs(phi - want).max() < 1e-12
    # summation to delta, pair by pair
    gates = R.gate_rescale(R.preact(x, w1, b1), R.preact(bg, w1, b1))
    rows = np.broadcast_to(R.f64(bg)[None], (B, N, D))
    prod = R.products(x, rows, gates, w1, w2)[0]                     # [B, N, C, D]
    fx, fb = R.forward(x, w1, b1, w2, b2), R.forward(bg, w1, b1, w2, b2)
    delta = fx[:, None, :] - fb[None, :, :]
    assert np.abs(prod.sum(3) - delta).max() < 1e-12
    assert np.abs(prod.sum(3)[1, 2]).max() == 0.0


def test_draws_like_shap_is_the_literal_double_loop():
    B, K, N, seed = 4, 7, 13, 42
    ridx, t = SE.draws_like_shap(seed, B, K, N)
    np.random.seed(seed)
    for j in range(B):
        for k in range(K):
            assert ridx[j, k] == np.random.choice(N)
            assert t[j, k] == np.float32(np.random.uniform())
    assert ridx.dtype == np.int32 and t.dtype == np.float32 and ridx.shape == t.shape == (B, K)
    again = SE.draws_like_shap(seed, B, K, N)        # shap reseeds per class: every class sees this table
    assert np.array_equal(again[0], ridx) and np.array_equal(again[1], t)
    np.random.seed(5)
    want_seed = np.random.randint(0, 1e6)
    np.random.seed(5)
    none = SE.draws_like_shap(None, B, K, N)
    seeded = SE.draws_like_shap(want_seed, B, K, N)
    assert np.array_equal(none[0], seeded[0]) and np.array_equal(none[1], seeded[1])


def test_draws_like_expected_gradients_are_the_existing_functions_draws(monkeypatch):
    B, N, K, D, H, C, seed = 3, 6, 8, 21, 7, 2, 9
    x, bg, w1, b1, w2, b2 = R.make_inputs(B, N, D, H, C, seed=4)
    seen = {}
    real_randint, real_rand = torch.randint, torch.rand

    def randint(*a, **kw):
        seen["bi"] = real_randint(*a, **kw)
        return seen["bi"]

    def rand(*a, **kw):
        seen["alpha"] = real_rand(*a, **kw)
        return seen["alpha"]

    monkeypatch.setattr(torch, "randint", randint)
    monkeypatch.setattr(torch, "rand", rand)
    net = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Linear(H, C)).double()
    with torch.no_grad():
        for p, v in zip(net.parameters(), (w1, b1, w2, b2)):
            p.copy_(torch.from_numpy(v.astype(np.float64)))
    xt, bgt = torch.from_numpy(x).double(), torch.from_numpy(bg).double()
    got = X.expected_gradients(net, bgt, xt, nsamples=K, seed=seed).numpy()
    monkeypatch.undo()
    ridx, t = SE.draws_like_expected_gradients(seed, K, B, N)
    assert np.array_equal(ridx, seen["bi"].numpy().T) and np.array_equal(t, seen["alpha"][:, :, 0].numpy().T)
    assert ridx.dtype == np.int32 and ridx.shape == t.shape == (B, K)
    want = R.expected_gradients(x, bg, ridx, t, w1, b1, w2)[0]
    assert np.abs(got - want).max() < 1e-6           # the function returns float32


def test_workspace_query_runs_without_a_gpu():
    lib = L.lib()
    small, large = lib.ecgmm_shap_mlp_workspace(1, 200, 768, 128, 2), lib.ecgmm_shap_mlp_workspace(16, 200, 768, 128, 2)
    assert 0 < small < large
    for bad in [(0, 200, 768, 128, 2), (1, 0, 768, 128, 2), (1, 4097, 768, 128, 2), (1, 200, 0, 128, 2),
                (1, 200, 4097, 128, 2), (1, 200, 768, 0, 2), (1, 200, 768, 257, 2), (1, 200, 768, 128, 0),
                (1, 200, 768, 128, 9)]:
        assert lib.ecgmm_shap_mlp_workspace(*bad) == 0
        assert b"shap_mlp_workspace" in lib.ecgmm_last_error()
    assert lib.ecgmm_shap_mlp_workspace(1, 4096, 4096, 256, 8) > 0


def _head(cls=torch.nn.Linear, p=0.3):
    return torch.nn.Sequential(cls(12, 6), torch.nn.ReLU(), torch.nn.Dropout(p), cls(6, 2)).eval()


def test_every_refusal_raises_before_any_launch():
    data, rows = torch.zeros(4, 12), torch.zeros(2, 12)
    for cls in (torch.nn.Linear, hnn.Linear):
        w1, b1, w2, b2 = SE.mlp_weights(X.FusionClassifierWrapper(_head(cls)))
        assert w1.shape == (6, 12) and b1.shape == (6,) and w2.shape == (2, 6) and b2.shape == (2,)
    assert len(SE.mlp_weights(torch.nn.Sequential(torch.nn.Linear(12, 6), torch.nn.ReLU(), torch.nn.Linear(6, 2)))) == 4
    deeper = torch.nn.Sequential(_head(), torch.nn.ReLU(), torch.nn.Linear(2, 2))
    other = torch.nn.Sequential(torch.nn.Linear(12, 6), torch.nn.Tanh(), torch.nn.Linear(6, 2))
    norm = torch.nn.Sequential(torch.nn.Linear(12, 6), torch.nn.ReLU(), torch.nn.LayerNorm(6), torch.nn.Linear(6, 2))
    for cls in (SE.GradientExplainer, SE.DeepExplainer):
        for model in (deeper, other, norm):
            with pytest.raises(NotImplementedError, match="Linear -> ReLU"):
                cls(model, data)
        with pytest.raises(RuntimeError, match="training mode"):
            cls(_head().train(), data)
        with pytest.raises(TypeError, match="nn.Module"):
            cls(lambda v: v, data)
        with pytest.raises(NotImplementedError, match="multi-input"):
            cls(_head(), [data])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(_head(), data)
        with pytest.raises(NotImplementedError, match="ranked_outputs"):
            cls.__new__(cls).shap_values(rows, ranked_outputs=2)
    assert SE.mlp_weights(_head(p=0.0).train())[0].shape == (6, 12)      # Dropout(0) in training mode is the identity
    with pytest.raises(NotImplementedError, match="local_smoothing"):
        SE.GradientExplainer(_head(), data, local_smoothing=0.1)
    from ecgmm.hip import functional as HF
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.shap_gradient(z(2, 12), z(4, 12), z(2, 3, dtype=torch.int32), z(2, 3), z(6, 12), z(6), z(2, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.shap_deep(z(2, 12), z(4, 12), z(6, 12), z(6), z(2, 6))
    with pytest.raises(ValueError, match="explainer must be one of"):
        X.main(explainer="kernel")


def _undecided_share(x, bg, ridx, t, w1, b1):
    p, pabs = R.points(x, bg, ridx, t)
    z = R.preact(p, w1, b1)
    return float((np.abs(z) <= Bd.z_bound(pabs, w1, b1, interpolated=True)).mean())


def test_cap_on_undecided_gates_holds_for_the_end_to_end_inputs():
    """tests/test_shap_gpu.py takes a gate from the device only where float64 cannot decide it; this is the share of such
    gates for its very inputs and draws, and for the small shapes of tests/test_shap_ops_gpu.py"""
    for B, N, D, H, C, seed in R.E2E_SHAPES:
        x, bg, w1, b1, _, _ = R.make_inputs(B, N, D, H, C, seed)
        for K in R.E2E_NSAMPLES:
            share = _undecided_share(x, bg, *SE.draws_like_shap(R.E2E_RSEED, B, K, N), w1, b1)
            print("undecided gates at D=%d H=%d B=%d K=%d: %.3g" % (D, H, B, K, share))
            assert share <= R.UNDECIDED_CAP
    for case in R.OPS_CASES[:2]:
        (x, bg, w1, b1, _, _), (ridx, t) = R.ops_inputs(case)
        assert _undecided_share(x, bg, ridx, t, w1, b1) == 0.0
