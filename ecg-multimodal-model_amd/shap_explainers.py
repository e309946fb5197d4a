"""``shap.GradientExplainer`` and ``shap.DeepExplainer`` for the fusion head, on csrc/shap.hip.

shap is not a dependency.  The reference applies both explainers to one network only, ``FusionClassifierWrapper`` around
``Linear(D, H) -> ReLU -> Dropout -> Linear(H, C)`` (shap_fusion_modal_balance.py:122-160, shap_fusion.py:62,
shap_fusion_paper.py:71), and for that network both estimators are one fused kernel.  The classes keep
shap's names and call shapes; anything the kernel does not cover is refused with a message, never computed another way.

The draws of ``GradientExplainer.shap_values`` are made on the host in shap's own order (``draws_like_shap``): they are
B * nsamples * 8 bytes, so there is no device generator.  The parity with the shap package is unpinned: the algorithm is
restated from its published source, not checked against an installed copy.
"""
import numpy as np
import torch
import torch.nn as nn

from .hip import functional as HF
from .hip import nn as hnn

__all__ = ["GradientExplainer", "DeepExplainer", "draws_like_shap", "draws_like_expected_gradients", "mlp_weights"]

WORKSPACE_BUDGET = 256 << 20   # bytes of kernel workspace one launch may ask for; larger batches run in chunks of B


def draws_like_shap(rseed, B, nsamples, N):
    """-> (ridx int32 [B, nsamples], t float32 [B, nsamples]) drawn as shap's PyTorch GradientExplainer draws them: one
    ``np.random.seed(rseed)``, then for each sample j and each k ``np.random.choice(N)`` followed by
    ``np.random.uniform()``.  shap reseeds with the same rseed for every class, so one table serves all classes.
    ``rseed=None`` draws ``np.random.randint(0, 1e6)`` first, as shap does.  Like shap, this moves numpy's global stream."""
    if rseed is None:
        rseed = np.random.randint(0, 1e6)
    np.random.seed(rseed)
    ridx = np.empty((B, nsamples), dtype=np.int32)
    t = np.empty((B, nsamples), dtype=np.float64)
    for j in range(B):
        for k in range(nsamples):
            ridx[j, k] = np.random.choice(N)
            t[j, k] = np.random.uniform()
    return ridx, t.astype(np.float32)


def draws_like_expected_gradients(seed, nsamples, B, N):
    """the draws of ``shap_fusion_modal_balance.expected_gradients(..., nsamples, seed)`` as (ridx [B, nsamples],
    t [B, nsamples]): its ``bi[k, b]`` and ``alpha[k, b]``"""
    g = torch.Generator().manual_seed(seed)
    bi = torch.randint(0, N, (nsamples, B), generator=g)
    alpha = torch.rand(nsamples, B, 1, generator=g)
    return bi.t().contiguous().to(torch.int32).numpy(), alpha[:, :, 0].t().contiguous().numpy()


def _leaves(module):
    kids = list(module.children())
    if not kids:
        return [module]
    out = []
    for k in kids:
        out.extend(_leaves(k))
    return out


def mlp_weights(model):
    """(w1 [H, D], b1 [H], w2 [C, H], b2 [C]) of a module whose flattened children are exactly Linear, ReLU, [Dropout],
    Linear (``hnn`` or ``torch.nn`` Linear); raises for anything else.  Reads the parameters, changes nothing."""
    if not isinstance(model, nn.Module):
        raise TypeError("the explainers take the model as an nn.Module (a (model, layer) tuple or a function is not supported)")
    mods = _leaves(model)
    kinds = [type(m).__name__ for m in mods]
    lin = (hnn.Linear, nn.Linear)
    ok = (len(mods) in (3, 4) and isinstance(mods[0], lin) and isinstance(mods[1], nn.ReLU) and isinstance(mods[-1], lin)
          and (len(mods) == 3 or isinstance(mods[2], nn.Dropout)))
    if not ok:
        raise NotImplementedError("the native SHAP explainers cover Linear -> ReLU -> [Dropout] -> Linear only; got "
                                  + " -> ".join(kinds))
    if len(mods) == 4 and mods[2].p > 0 and mods[2].training:
        raise RuntimeError("the model is in training mode with Dropout p > 0: call model.eval() before explaining it")
    l1, l2 = mods[0], mods[-1]
    if l1.weight.shape[0] != l2.weight.shape[1]:
        raise ValueError("the two Linear layers do not fit together")
    zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=l1.weight.device)
    b1 = l1.bias if l1.bias is not None else zeros(l1.weight.shape[0])
    b2 = l2.bias if l2.bias is not None else zeros(l2.weight.shape[0])
    return tuple(HF.f32c(p.detach()) for p in (l1.weight, b1, l2.weight, b2))


def _device_matrix(a, what):
    if isinstance(a, (list, tuple)):
        raise NotImplementedError(f"{what}: multi-input models (a list of tensors) are not supported")
    if not torch.is_tensor(a) or a.dim() != 2:
        raise TypeError(f"{what} must be a 2-D torch tensor on the ROCm device")
    if not a.is_cuda:
        raise RuntimeError(f"{what} is on {a.device}; the HIP library is the only compute path (no CPU fallback) -- move it "
                           "to a ROCm device")
    return HF.f32c(a.detach())


def _chunk_rows(B, K, D, H, C):
    from .hip import lib as L
    per = L.lib().ecgmm_shap_mlp_workspace(1, K, D, H, C)
    if per == 0:
        L.check(1, "shap workspace query")
    return max(1, min(B, WORKSPACE_BUDGET // per))


class _Explainer:
    def __init__(self, model, data):
        self.w1, self.b1, self.w2, self.b2 = mlp_weights(model)
        self.model = model
        self.data = _device_matrix(data, "data")
        if self.data.shape[1] != self.w1.shape[1]:
            raise ValueError(f"data has {self.data.shape[1]} columns, the model takes {self.w1.shape[1]}")
        if self.data.device != self.w1.device:
            raise RuntimeError("data and the model are on different devices")

    def _check(self, X, ranked_outputs):
        if ranked_outputs is not None:
            raise NotImplementedError("ranked_outputs is not supported: every class is explained")
        mlp_weights(self.model)   # the mode may have changed since construction
        X = _device_matrix(X, "X")
        if X.shape[1] != self.data.shape[1]:
            raise ValueError(f"X has {X.shape[1]} columns, the background {self.data.shape[1]}")
        return X


class GradientExplainer(_Explainer):
    """``shap.GradientExplainer(model, data)`` (expected gradients) of the two-Linear head."""

    def __init__(self, model, data, session=None, batch_size=50, local_smoothing=0):
        if local_smoothing != 0:
            raise NotImplementedError("local_smoothing > 0 is not supported")
        super().__init__(model, data)
        self.batch_size = batch_size   # shap's knob for its own batching; the kernel takes every pair of a chunk at once

    def shap_values(self, X, nsamples=200, ranked_outputs=None, output_rank_order="max", rseed=None,
                    return_variances=False, draws=None, return_z=False):
        """-> float32 numpy [B, D, C]; (values, variances) with ``return_variances``.  ``draws``: (ridx [B, nsamples],
        t [B, nsamples]) to use instead of ``draws_like_shap(rseed, ...)``.  ``return_z`` appends the device's
        pre-activations [B, nsamples, H] to the result."""
        X = self._check(X, ranked_outputs)
        B, D = X.shape
        H, C, N = self.w1.shape[0], self.w2.shape[0], self.data.shape[0]
        ridx, t = draws if draws is not None else draws_like_shap(rseed, B, int(nsamples), N)
        ridx = torch.as_tensor(np.ascontiguousarray(ridx), dtype=torch.int32).to(X.device)
        t = torch.as_tensor(np.ascontiguousarray(t), dtype=torch.float32).to(X.device)
        K = ridx.shape[1]
        step = _chunk_rows(B, K, D, H, C)
        phi, var, z = [], [], []
        for s in range(0, B, step):
            o = HF.shap_gradient(X[s:s + step], self.data, ridx[s:s + step], t[s:s + step], self.w1, self.b1, self.w2,
                                 want_var=return_variances, want_z=return_z)
            phi.append(o["phi"].cpu())
            if return_variances:
                var.append(o["var"].cpu())
            if return_z:
                z.append(o["z"].cpu())
        out = [torch.cat(phi).numpy()]
        if return_variances:
            out.append(torch.cat(var).numpy())
        if return_z:
            out.append(torch.cat(z).numpy())
        return out[0] if len(out) == 1 else tuple(out)


class DeepExplainer(_Explainer):
    """``shap.DeepExplainer(model, data)`` (DeepLIFT with the rescale rule, averaged over the background) of the head."""

    ADDITIVITY_TOLERANCE = 1e-2   # shap's own

    def __init__(self, model, data, session=None, learning_phase_flags=None):
        super().__init__(model, data)
        with torch.no_grad():
            self.expected_value = model(self.data).float().mean(0).cpu().numpy()

    def shap_values(self, X, ranked_outputs=None, output_rank_order="max", check_additivity=True, return_z=False):
        """-> float32 numpy [B, D, C]; with ``return_z`` also the device's zx [B, H] and zb [N, H]"""
        X = self._check(X, ranked_outputs)
        B, D = X.shape
        H, C, N = self.w1.shape[0], self.w2.shape[0], self.data.shape[0]
        step = _chunk_rows(B, N, D, H, C)
        phi, zx, zb = [], [], None
        for s in range(0, B, step):
            o = HF.shap_deep(X[s:s + step], self.data, self.w1, self.b1, self.w2, want_z=return_z)
            phi.append(o["phi"].cpu())
            if return_z:
                zx.append(o["zx"].cpu())
                zb = o["zb"].cpu()
        phi = torch.cat(phi).numpy()
        if check_additivity:
            with torch.no_grad():
                fx = self.model(X).float().cpu().numpy()
            diff = np.abs(fx - np.asarray(self.expected_value) - phi.sum(1)).max()
            if not diff <= self.ADDITIVITY_TOLERANCE:
                raise AssertionError(
                    "The SHAP explanations do not sum up to the model's output: max |model(X) - expected_value - "
                    f"phi.sum(1)| = {diff:.3g} > {self.ADDITIVITY_TOLERANCE}")
        return (phi, torch.cat(zx).numpy(), zb.numpy()) if return_z else phi
