"""torch.autograd glue over the C ABI: every op here launches HIP kernels from libecgmm_hip.so on
torch's current stream.  PyTorch only supplies device memory, the stream and the autograd graph.

Parameter gradients are written by the kernels straight into ``param.grad`` ("gradient sinks", see
:func:`grad_sink`) and the autograd Functions return ``None`` for parameters: a backward pass
OVERWRITES ``.grad`` (like ``zero_grad()`` + ``backward()`` in the reference loop, train.py:65-80)
instead of accumulating into it.  That keeps gradients inside one flat buffer for the RCCL
all-reduce and the fused Adam.
"""
import ctypes as C

import torch

from . import lib as L

vp = C.c_void_p
# debug switch: validate class indices on the host before the loss kernels (costs a device sync per call; without it an
# out-of-range label makes the loss NaN instead of raising like torch's CrossEntropyLoss)
_CHECK_LABELS = __import__("os").environ.get("ECGMM_CHECK_LABELS", "0") == "1"


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP library is the only compute path "
                           "(no CPU fallback) -- move the model and inputs to a ROCm device")


def ptr(t):
    return None if t is None else vp(t.data_ptr())


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def f32c(t):
    """contiguous fp32 view/copy of ``t`` (host-side plumbing only)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def grad_sink(p, accumulate=False):
    """The tensor the kernels write ``p``'s gradient into (allocated on first use, or the view of a
    flat gradient buffer installed by ``parallel.flatten``).  None when ``p`` is frozen.

    A backward pass OVERWRITES the sink.  Writing the same sink twice before the optimizer has consumed
    it (``FusedAdam.step()`` / ``zero_grad()``, ``module.zero_grad()`` or :func:`release_grads`) would
    silently drop the first gradient -- gradient accumulation over several backward passes, or a
    parameter used twice in one forward -- so that raises instead.  ``accumulate=True`` is for callers
    that add into the sink themselves (TabNet's shared layers)."""
    if p is None or not p.requires_grad:
        return None
    if p.grad is None:
        view = getattr(p, "_ecg_grad_view", None)
        p.grad = view if view is not None else torch.zeros_like(p, memory_format=torch.contiguous_format)
        p._ecg_dirty = False
    if getattr(p, "_ecg_dirty", False) and not accumulate:
        raise RuntimeError(
            "gradient sink written twice: backward passes of this library OVERWRITE .grad (train.py:65-81 pattern: "
            "zero_grad -> backward -> step).  Call optimizer.zero_grad() / optimizer.step() (or "
            "ecgmm.hip.functional.release_grads(model)) between backward passes; gradient accumulation and "
            f"parameters shared by several layers are not supported (parameter shape {tuple(p.shape)})")
    p._ecg_dirty = True
    p._ecg_written = True
    return p.grad


def release_grads(params):
    """Mark the gradients of ``params`` (an iterable of parameters or a module) as consumed: the next backward
    may overwrite them.  What ``FusedAdam.zero_grad()`` / ``step()`` do for their own parameters."""
    if isinstance(params, torch.nn.Module):
        params = params.parameters()
    for p in params:
        p._ecg_dirty = False


def new_bytes(n, device):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=device)


class _Scratch:
    """Grow-only per-device scratch buffers for transient workspaces (never freed mid-step, so the
    launches stay graph-capturable and allocator-quiet)."""
    _bufs = {}

    @classmethod
    def get(cls, key, nbytes, device):
        # one buffer per (use, device, STREAM): encoders may run concurrently on different streams
        k = (key, device.index, torch.cuda.current_stream(device).cuda_stream)
        b = cls._bufs.get(k)
        if b is None or b.numel() < nbytes:
            b = new_bytes(nbytes, device)
            cls._bufs[k] = b
        return b


# --------------------------------------------------------------------------------------------
# Linear (+bias, +activation)      reference: nn.Linear at PMB:221,257,261,269-271,284,288
# --------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act):
        _require_cuda(x, "linear")
        x = f32c(x)
        B, In = x.shape
        Out = weight.shape[0]
        y = torch.empty(B, Out, device=x.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_linear_fwd(ptr(x), ptr(weight), ptr(bias), ptr(y), B, In, Out, act, stream()), "linear_fwd")
        ctx.act = act
        ctx.params = (weight, bias)
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, bias = ctx.params
        B, In = x.shape
        Out = weight.shape[0]
        dy = f32c(dy)
        if ctx.act != L.ACT_NONE:
            dz = torch.empty_like(dy)
            L.check(L.lib().ecgmm_act_bwd(ptr(dy), ptr(y), ptr(dz), dy.numel(), ctx.act, stream()), "act_bwd")
        else:
            dz = dy
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        # sinks only for the gradients this backward was asked for (torch.autograd.grad w.r.t. inputs leaves .grad alone)
        dw = grad_sink(weight) if ctx.needs_input_grad[1] else None
        db = grad_sink(bias) if ctx.needs_input_grad[2] else None
        nb = L.lib().ecgmm_linear_bwd_scratch(B, In, Out)
        scratch = _Scratch.get("linear", nb, x.device)
        L.check(L.lib().ecgmm_linear_bwd(ptr(dz), ptr(x), ptr(weight), ptr(dx), ptr(dw), ptr(db), B, In, Out,
                                         ptr(scratch), scratch.numel(), stream()), "linear_bwd")
        return dx, None, None, None


def linear(x, weight, bias=None, act=L.ACT_NONE):
    return LinearFn.apply(x, weight, bias, act)


# --------------------------------------------------------------------------------------------
# LayerNorm / AttentionFusion        reference: PMB:31-46, 223, 239, 263
# --------------------------------------------------------------------------------------------
def _seg_arrays(segs):
    n = len(segs)
    arr = (vp * 3)(*[vp(s.data_ptr()) for s in segs] + [None] * (3 - n))
    dims = (C.c_int * 3)(*[s.shape[1] for s in segs] + [0] * (3 - n))
    return arr, dims


class LayerNormFn(torch.autograd.Function):
    """nseg == 1: plain LayerNorm.  nseg == 3 with fusion weights: softmax(w) * feats -> cat -> LN."""

    @staticmethod
    def forward(ctx, gamma, beta, fusion_w, eps, *segs):
        for s in segs:
            _require_cuda(s, "layernorm")
        segs = tuple(f32c(s) for s in segs)
        B = segs[0].shape[0]
        D = sum(s.shape[1] for s in segs)
        dev = segs[0].device
        out = torch.empty(B, D, device=dev, dtype=torch.float32)
        stat = torch.empty(B, 2, device=dev, dtype=torch.float32)
        soft = torch.empty(3, device=dev, dtype=torch.float32) if fusion_w is not None else None
        arr, dims = _seg_arrays(segs)
        L.check(L.lib().ecgmm_layernorm_fwd(arr, dims, len(segs), ptr(fusion_w), ptr(gamma), ptr(beta), ptr(out),
                                            ptr(stat), ptr(soft), B, eps, stream()), "layernorm_fwd")
        ctx.params = (gamma, beta, fusion_w)
        ctx.nseg = len(segs)
        ctx.save_for_backward(stat, *segs)
        if fusion_w is not None:
            ctx.mark_non_differentiable(soft)
            return out, soft
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        stat, *segs = ctx.saved_tensors
        gamma, beta, fusion_w = ctx.params
        B = segs[0].shape[0]
        D = sum(s.shape[1] for s in segs)
        dout = f32c(dout)
        dsegs = [torch.empty_like(s) if ctx.needs_input_grad[4 + i] else None for i, s in enumerate(segs)]
        arr, dims = _seg_arrays(segs)
        darr = (vp * 3)(*[ptr(d) for d in dsegs] + [None] * (3 - len(segs)))
        scratch = _Scratch.get("ln", L.lib().ecgmm_layernorm_bwd_scratch(B, D), dout.device)
        L.check(L.lib().ecgmm_layernorm_bwd(arr, dims, len(segs), ptr(fusion_w), ptr(gamma), ptr(stat), ptr(dout),
                                            darr, 0, ptr(grad_sink(gamma) if ctx.needs_input_grad[0] else None),
                                            ptr(grad_sink(beta) if ctx.needs_input_grad[1] else None),
                                            ptr(grad_sink(fusion_w) if ctx.needs_input_grad[2] else None), B, ptr(scratch),
                                            stream()), "layernorm_bwd")
        return (None, None, None, None, *dsegs)


def layer_norm(x, gamma, beta, eps=1e-5):
    return LayerNormFn.apply(gamma, beta, None, eps, x)


def attention_fusion(img, sig, clin, weights, gamma, beta, eps=1e-5):
    return LayerNormFn.apply(gamma, beta, weights, eps, img, sig, clin)


# --------------------------------------------------------------------------------------------
# var_loss                             reference: PMB:349-352
# --------------------------------------------------------------------------------------------
class VarLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f0, f1, f2):
        fs = tuple(f32c(f) for f in (f0, f1, f2))
        _require_cuda(fs[0], "var_loss")
        B = fs[0].shape[0]
        dev = fs[0].device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        scratch = torch.empty(3 * B + 4, device=dev, dtype=torch.float32)
        L.check(L.lib().ecgmm_varloss_fwd(ptr(fs[0]), ptr(fs[1]), ptr(fs[2]), B, fs[0].shape[1], fs[1].shape[1],
                                          fs[2].shape[1], ptr(loss), ptr(scratch), stream()), "varloss_fwd")
        ctx.save_for_backward(scratch, *fs)
        return loss

    @staticmethod
    def backward(ctx, gout):
        scratch, *fs = ctx.saved_tensors
        gout = f32c(gout).reshape(1)
        outs = []
        for m, f in enumerate(fs):
            if not ctx.needs_input_grad[m]:
                outs.append(None)
                continue
            df = torch.empty_like(f)
            L.check(L.lib().ecgmm_varloss_bwd(ptr(f), f.shape[0], f.shape[1], ptr(gout), ptr(scratch), m, ptr(df), 0,
                                              stream()), "varloss_bwd")
            outs.append(df)
        return tuple(outs)


def var_loss(f0, f1, f2):
    return VarLossFn.apply(f0, f1, f2)


# --------------------------------------------------------------------------------------------
# CrossEntropy / Focal                reference: train.py:31,69-72; signal_model.py:91-106
# --------------------------------------------------------------------------------------------
class CELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, focal, alpha, gamma):
        _require_cuda(logits, "cross_entropy")
        logits = f32c(logits)
        labels = labels.to(torch.int64).contiguous()
        B, Cn = logits.shape
        if labels.shape != (B,):
            raise ValueError(f"cross_entropy: expected {B} class indices, got shape {tuple(labels.shape)}")
        if _CHECK_LABELS and B > 0 and (int(labels.min()) < 0 or int(labels.max()) >= Cn):
            raise IndexError(f"Target {int(labels.max() if labels.max() >= Cn else labels.min())} is out of bounds.")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dcoef = torch.empty(B, device=logits.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_ce_fwd(ptr(logits), ptr(labels), B, Cn, int(focal), float(alpha), float(gamma),
                                     ptr(loss), ptr(dcoef), stream()), "ce_fwd")
        ctx.save_for_backward(logits, labels, dcoef)
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, labels, dcoef = ctx.saved_tensors
        B, Cn = logits.shape
        d = torch.empty_like(logits)
        gout = f32c(gout).reshape(1)
        L.check(L.lib().ecgmm_ce_bwd(ptr(logits), ptr(labels), B, Cn, ptr(dcoef), ptr(gout), ptr(d), stream()), "ce_bwd")
        return d, None, None, None, None


class CEPlusFn(torch.autograd.Function):
    """CrossEntropy(logits, labels) + w * extra  (the step loss of train.py:69-78: CE(fusion_logits) + 0.1 * var_loss)"""

    @staticmethod
    def forward(ctx, logits, labels, extra, w):
        _require_cuda(logits, "cross_entropy")
        logits, extra = f32c(logits), f32c(extra).reshape(1)
        labels = labels.to(torch.int64).contiguous()
        B, Cn = logits.shape
        if labels.shape != (B,):
            raise ValueError(f"cross_entropy: expected {B} class indices, got shape {tuple(labels.shape)}")
        if _CHECK_LABELS and B > 0 and (int(labels.min()) < 0 or int(labels.max()) >= Cn):
            raise IndexError("Target is out of bounds.")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dcoef = torch.empty(B, device=logits.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_ce_plus_fwd(ptr(logits), ptr(labels), B, Cn, ptr(extra), float(w), ptr(loss), ptr(dcoef),
                                          stream()), "ce_plus_fwd")
        ctx.w = float(w)
        ctx.save_for_backward(logits, labels, dcoef)
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, labels, dcoef = ctx.saved_tensors
        B, Cn = logits.shape
        d = torch.empty_like(logits)
        dextra = torch.empty((), device=logits.device, dtype=torch.float32)
        gout = f32c(gout).reshape(1)
        L.check(L.lib().ecgmm_ce_plus_bwd(ptr(logits), ptr(labels), B, Cn, ptr(dcoef), ptr(gout), ptr(d), ptr(dextra),
                                          ctx.w, stream()), "ce_plus_bwd")
        return d, None, dextra, None


def cross_entropy(logits, labels):
    return CELossFn.apply(logits, labels, False, 1.0, 0.0)


def cross_entropy_plus(logits, labels, extra, weight):
    """CrossEntropy(logits, labels) + weight * extra in one kernel per direction"""
    return CEPlusFn.apply(logits, labels, extra, weight)


def focal_loss(logits, labels, alpha=1.0, gamma=2.0):
    return CELossFn.apply(logits, labels, True, alpha, gamma)


# --------------------------------------------------------------------------------------------
# Dropout                              reference: nn.Dropout(0.3) at PMB:115,260,287
# --------------------------------------------------------------------------------------------
class _PhiloxState:
    """Seed/offset bookkeeping for the device Philox stream (advanced per call, like torch's)."""
    seed = 42
    offset = 0

    @classmethod
    def manual_seed(cls, seed):
        cls.seed, cls.offset = int(seed), 0

    @classmethod
    def take(cls, n):
        off = cls.offset
        cls.offset += (int(n) + 3) // 4
        return cls.seed, off


def manual_seed(seed):
    _PhiloxState.manual_seed(seed)


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        _require_cuda(x, "dropout")
        x = f32c(x)
        y = torch.empty_like(x)
        mask = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
        seed, off = _PhiloxState.take(x.numel())
        L.check(L.lib().ecgmm_dropout_fwd(ptr(x), ptr(y), ptr(mask), x.numel(), p, seed, off, stream()), "dropout_fwd")
        ctx.p = p
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = f32c(dy)
        dx = torch.empty_like(dy)
        L.check(L.lib().ecgmm_dropout_bwd(ptr(dy), ptr(mask), ptr(dx), dy.numel(), ctx.p, stream()), "dropout_bwd")
        return dx, None


def dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, float(p))


# --------------------------------------------------------------------------------------------
# BatchNorm1d over [B, C] fp32 (+ReLU)   reference: clinical_encoder[1:3], PMB:258-259
# --------------------------------------------------------------------------------------------
class BatchNorm1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, training, momentum, eps, relu):
        _require_cuda(x, "batchnorm1d")
        x = f32c(x)
        B, Cn = x.shape
        dev = x.device
        lib = L.lib()
        coef = torch.empty(4, Cn, device=dev, dtype=torch.float32)
        if training:
            if B < 2:
                raise ValueError("Expected more than 1 value per channel when training")  # torch's message
            rows = lib.ecgmm_col_stats_rows(L.F32, B, Cn)
            partial = torch.empty(rows + 64, 2, Cn, device=dev, dtype=torch.float32)  # + tail rows (ecgmm.h)
            L.check(lib.ecgmm_col_stats(L.F32, ptr(x), B, Cn, ptr(partial), stream()), "col_stats")
            L.check(lib.ecgmm_bn_finalize(ptr(partial), rows, Cn, float(B), ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                                          ptr(nbt), momentum, eps, ptr(coef), stream()), "bn_finalize")
        else:
            L.check(lib.ecgmm_bn_eval_coef(Cn, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), eps, ptr(coef), stream()),
                    "bn_eval_coef")
        y = torch.empty_like(x)
        L.check(lib.ecgmm_bn_act(L.F32, ptr(x), ptr(coef), None, None, None, 1, int(relu), ptr(y), B, Cn, stream()),
                "bn_act")
        ctx.params = (gamma, beta)
        ctx.relu, ctx.training = relu, training
        ctx.save_for_backward(x, y, coef)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, coef = ctx.saved_tensors
        gamma, beta = ctx.params
        B, Cn = x.shape
        dy = f32c(dy)
        lib = L.lib()
        dx = torch.empty_like(x)
        scratch = _Scratch.get("bn1d", lib.ecgmm_bn_bwd_scratch(L.F32, B, Cn), x.device)
        if not ctx.training:   # eval forward: a constant affine map (running statistics)
            L.check(lib.ecgmm_bn_eval_bwd(L.F32, ptr(dy), ptr(y) if ctx.relu else None, None, None, 1, ptr(x), ptr(coef),
                                          ptr(grad_sink(gamma) if ctx.needs_input_grad[1] else None),
                                          ptr(grad_sink(beta) if ctx.needs_input_grad[2] else None), ptr(dx), None, None, B,
                                          Cn, ptr(scratch), stream()), "bn_eval_bwd")
            return dx, None, None, None, None, None, None, None, None, None
        L.check(lib.ecgmm_bn_bwd(L.F32, ptr(dy), ptr(y) if ctx.relu else None, None, None, 1, ptr(x), ptr(coef),
                                 ptr(gamma), ptr(grad_sink(gamma) if ctx.needs_input_grad[1] else None),
                                 ptr(grad_sink(beta) if ctx.needs_input_grad[2] else None), ptr(dx), None, None, B, Cn,
                                 ptr(scratch), stream()), "bn_bwd")
        return dx, None, None, None, None, None, None, None, None, None


def batch_norm1d(x, gamma, beta, rm, rv, nbt, training, momentum=0.1, eps=1e-5, relu=False):
    return BatchNorm1dFn.apply(x, gamma, beta, rm, rv, nbt, training, momentum, eps, relu)


# --------------------------------------------------------------------------------------------
# LSTM (multi-layer, bidirectional)      reference: nn.LSTM at train_physionet2.py:75-76,94
# --------------------------------------------------------------------------------------------
def _ptr_table(tensors):
    return (vp * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _grad_wanted(p):
    """Inside a backward: does this pass accumulate into ``p.grad``?  ``ctx.needs_input_grad`` only says that ``p`` required
    grad at the forward; ``torch.autograd.grad(..., inputs)`` and ``backward(inputs=...)`` that do not name ``p`` run this
    node without ``p``'s AccumulateGrad node, which the engine reports.  Where it cannot tell, the sink is written."""
    with torch.enable_grad():
        node = p.view_as(p).grad_fn.next_functions[0][0]
    try:
        return torch._C._will_engine_execute_node(node)
    except RuntimeError:   # autograd.grad() naming a leaf itself: not answered by the engine
        return True


def check_lengths(lengths, B, T):
    """Sequence lengths of a padded ``[B, T, ...]`` batch -> an ``int32 [B]`` tensor (pure host code; the caller moves it).
    A list / tuple / array or a CPU integer tensor is validated as torch validates ``pack_padded_sequence``: shape ``[B]``,
    an integer dtype, ``1 <= len <= T``, else ``ValueError`` naming the first offending index.  A device integer tensor is
    taken as given (reading it would be a host sync) and converted to ``int32``: the kernels clamp its values to
    ``[0, T]``, and a clamped 0 is a row without live steps (``y = 0``, ``h_n = h_0``, a mean of 0)."""
    if isinstance(lengths, torch.Tensor):
        t = lengths
    else:
        try:
            t = torch.as_tensor(lengths)
        except Exception as e:
            raise ValueError(f"lengths: not convertible to a tensor ({e})") from None
    if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"lengths: dtype {t.dtype} is not an integer type")
    if tuple(t.shape) != (B,):
        raise ValueError(f"lengths: shape {tuple(t.shape)}, expected ({B},) (one length per batch row)")
    if t.device.type != "cpu":
        return t.to(torch.int32)
    bad = ((t < 1) | (t > T)).nonzero()
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"lengths[{i}] = {int(t[i])} is outside 1..T = {T}")
    return t.to(torch.int32)


def _lstm_dtype_code(name):
    """``"fp32"`` / ``"bf16"`` -> the library's dtype code (``ValueError`` otherwise)"""
    key = str(name).lower()
    if key not in ("fp32", "bf16"):
        raise ValueError(f"lstm: compute_dtype must be 'fp32' or 'bf16', got {name!r}")
    return L.BF16 if key == "bf16" else L.F32


class LSTMFn(torch.autograd.Function):
    """y, h_n, c_n = LSTM(x, h0, c0; params).  ``params`` in torch's ``_flat_weights`` order (per layer, per direction:
    w_ih, w_hh, b_ih, b_hh).  The forward keeps its workspace (activated gates, c_t, h_{t-1}) on ``ctx`` only when some
    input requires grad; the backward reads it and writes parameter gradients into their sinks.  ``cfg`` may carry a fifth
    entry, the device ``int32 [B]`` lengths (or ``None``): the ``_varlen`` entry points, else the fixed ones; and a sixth,
    the compute dtype code of the recurrence: ``ECGMM_BF16`` goes through the ``_dt`` entry points, fp32 through the ones
    it always went through."""

    @staticmethod
    def forward(ctx, x, h0, c0, cfg, *params):
        hidden, layers, bidirectional, batch_first = tuple(cfg)[:4]
        lengths = cfg[4] if len(cfg) > 4 else None
        dt = cfg[5] if len(cfg) > 5 else L.F32
        _require_cuda(x, "lstm")
        for t in (h0, c0) + params:
            if t is not None:
                _require_cuda(t, "lstm")
        D = 2 if bidirectional else 1
        if x.dim() != 3:
            raise RuntimeError(f"lstm: input must be 3-D (batched), got {x.dim()}-D")
        if len(params) != 4 * layers * D:
            raise RuntimeError(f"lstm: {len(params)} parameters, expected {4 * layers * D}")
        x = f32c(x)
        B, T = (x.shape[0], x.shape[1]) if batch_first else (x.shape[1], x.shape[0])
        In = x.shape[2]
        h0 = None if h0 is None else f32c(h0)
        c0 = None if c0 is None else f32c(c0)
        for t, name in ((h0, "h_0"), (c0, "c_0")):
            if t is not None and tuple(t.shape) != (layers * D, B, hidden):
                raise RuntimeError(f"lstm: {name} has shape {tuple(t.shape)}, expected {(layers * D, B, hidden)}")
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("lstm: parameters must be contiguous fp32")
        save = any(ctx.needs_input_grad)
        desc = L.LSTMDesc(B, T, In, hidden, layers, int(bidirectional), int(batch_first), int(save))
        lib = L.lib()
        nb = lib.ecgmm_lstm_fwd_workspace_dt(C.byref(desc), dt) if dt != L.F32 else lib.ecgmm_lstm_fwd_workspace(C.byref(desc))
        if nb == 0:
            raise RuntimeError("ecgmm lstm: " + lib.ecgmm_last_error().decode(errors="replace"))
        ws = new_bytes(nb, x.device) if save else _Scratch.get("lstm_fwd", nb, x.device)
        yshape = (B, T, D * hidden) if batch_first else (T, B, D * hidden)
        y = torch.empty(yshape, device=x.device, dtype=torch.float32)
        hn = torch.empty(layers * D, B, hidden, device=x.device, dtype=torch.float32)
        cn = torch.empty_like(hn)
        if lengths is not None:
            if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or lengths.device != x.device:
                raise RuntimeError(f"lstm: lengths must be int32 [{B}] on {x.device} (HF.check_lengths)")
            lengths = lengths.contiguous()
        if dt != L.F32:
            L.check(lib.ecgmm_lstm_forward_dt(C.byref(desc), dt, ptr(x), ptr(lengths), _ptr_table(params), ptr(h0), ptr(c0),
                                              ptr(y), ptr(hn), ptr(cn), ptr(ws), ws.numel(), stream()), "lstm_forward_dt")
        elif lengths is None:
            L.check(lib.ecgmm_lstm_forward(C.byref(desc), ptr(x), _ptr_table(params), ptr(h0), ptr(c0), ptr(y), ptr(hn),
                                           ptr(cn), ptr(ws), ws.numel(), stream()), "lstm_forward")
        else:
            L.check(lib.ecgmm_lstm_forward_varlen(C.byref(desc), ptr(x), ptr(lengths), _ptr_table(params), ptr(h0),
                                                  ptr(c0), ptr(y), ptr(hn), ptr(cn), ptr(ws), ws.numel(), stream()),
                    "lstm_forward_varlen")
        if save:
            ctx.desc, ctx.ws, ctx.params, ctx.lengths, ctx.dt = desc, ws, params, lengths, dt
            ctx.save_for_backward(x, h0, c0)
            ctx.set_materialize_grads(False)
        return y, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn, dcn):
        x, h0, c0 = ctx.saved_tensors
        desc, params = ctx.desc, ctx.params
        dy, dhn, dcn = (None if g is None else f32c(g) for g in (dy, dhn, dcn))
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None
        dh0 = torch.empty_like(h0) if h0 is not None and need[1] else None
        dc0 = torch.empty_like(c0) if c0 is not None and need[2] else None
        # sinks only for the gradients this backward was asked for (torch.autograd.grad w.r.t. inputs leaves .grad alone)
        sinks = [grad_sink(p) if need[4 + i] and _grad_wanted(p) else None for i, p in enumerate(params)]
        lib = L.lib()
        dt = ctx.dt
        nb = lib.ecgmm_lstm_bwd_workspace_dt(C.byref(desc), dt) if dt != L.F32 else lib.ecgmm_lstm_bwd_workspace(C.byref(desc))
        scratch = _Scratch.get("lstm_bwd", nb, x.device)
        if dt != L.F32:
            L.check(lib.ecgmm_lstm_backward_dt(C.byref(desc), dt, ptr(x), ptr(ctx.lengths), _ptr_table(params), ptr(h0),
                                               ptr(c0), ptr(dy), ptr(dhn), ptr(dcn), ptr(ctx.ws), ptr(dx), _ptr_table(sinks),
                                               ptr(dh0), ptr(dc0), ptr(scratch), scratch.numel(), stream()),
                    "lstm_backward_dt")
        elif ctx.lengths is None:
            L.check(lib.ecgmm_lstm_backward(C.byref(desc), ptr(x), _ptr_table(params), ptr(h0), ptr(c0), ptr(dy), ptr(dhn),
                                            ptr(dcn), ptr(ctx.ws), ptr(dx), _ptr_table(sinks), ptr(dh0), ptr(dc0),
                                            ptr(scratch), scratch.numel(), stream()), "lstm_backward")
        else:
            L.check(lib.ecgmm_lstm_backward_varlen(C.byref(desc), ptr(x), ptr(ctx.lengths), _ptr_table(params), ptr(h0),
                                                   ptr(c0), ptr(dy), ptr(dhn), ptr(dcn), ptr(ctx.ws), ptr(dx),
                                                   _ptr_table(sinks), ptr(dh0), ptr(dc0), ptr(scratch), scratch.numel(),
                                                   stream()), "lstm_backward_varlen")
        return (dx, dh0, dc0, None) + (None,) * len(params)


def lstm(x, hx, params, hidden_size, num_layers=1, bidirectional=False, batch_first=False, lengths=None,
         compute_dtype="fp32"):
    """``torch.nn.LSTM`` forward (with bias, no dropout, no projection): returns ``(output, (h_n, c_n))``.

    ``compute_dtype`` ``"fp32"`` (exact fp32 products, the default) or ``"bf16"``: the recurrent products ``h W_hh^T`` and
    ``dgates W_hh`` take their operands rounded to bf16 (fp32 sums, ``W_hh`` held on chip for all steps); the input
    projections, the gradient GEMMs, the parameters and everything stored stay fp32.  Anything else is a
    ``ValueError``.

    ``lengths`` (one per batch row, see :func:`check_lengths`): ``x`` stays padded and the result is
    ``pad_packed_sequence(lstm(pack_padded_sequence(x, lengths, enforce_sorted=False), hx), total_length=T)``: the output is
    exactly 0 from each row's length on, ``h_n / c_n`` are the states after each row's last own step, and no gradient sees
    the padding.  The padding of ``x`` must be finite (it meets exact zeros in the GEMMs).  A slice of 16 consecutive rows
    runs as many serial steps as its longest row: rows ordered by length free their CUs early, but a layer still lasts as
    long as the longest slice, and no time was gained at B = 256."""
    h0, c0 = (None, None) if hx is None else hx
    dt = _lstm_dtype_code(compute_dtype)
    cfg = (int(hidden_size), int(num_layers), bool(bidirectional), bool(batch_first))
    if lengths is not None:
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise RuntimeError("lstm: input must be a 3-D (batched) tensor")
        _require_cuda(x, "lstm")
        B, T = (x.shape[0], x.shape[1]) if batch_first else (x.shape[1], x.shape[0])
        cfg += (check_lengths(lengths, B, T).to(x.device),)
    if dt != L.F32:
        cfg = (cfg + (None,))[:5] + (dt,)
    y, hn, cn = LSTMFn.apply(x, h0, c0, cfg, *params)
    return y, (hn, cn)


class SeqMeanFn(torch.autograd.Function):
    """mean over the time axis of a [B, T, C] fp32 sequence (ecgmm_avgpool forward, ecgmm_bcast_rows backward)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x, "seq_mean")
        x = f32c(x)
        B, T, Cn = x.shape
        # the pooling kernel wants C / 4 to divide 256: wider rows are zero-padded to the next such width (plumbing copy)
        Cp = next((c for c in (4, 8, 16, 32, 64, 128, 256, 512, 1024) if c >= Cn), None) if (Cn % 4 or 256 % (Cn // 4)) else Cn
        if Cp is None:
            raise RuntimeError(f"seq_mean: C={Cn} above 1024 is not supported")
        if Cp != Cn:
            xp = torch.zeros(B, T, Cp, device=x.device, dtype=torch.float32)
            xp[:, :, :Cn] = x
            x = xp
        out = torch.empty(B, Cp, device=x.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_avgpool(L.F32, ptr(x), ptr(out), B, T, Cp, None, stream()), "avgpool")
        ctx.shape = (B, T, Cn)
        return out[:, :Cn].contiguous() if Cp != Cn else out

    @staticmethod
    def backward(ctx, dy):
        B, T, Cn = ctx.shape
        dy = f32c(dy)
        dx = torch.empty(B, T, Cn, device=dy.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_bcast_rows(L.F32, ptr(dy), ptr(dx), B, T, Cn, 1.0 / T, stream()), "bcast_rows")
        return dx


class SeqMeanVarlenFn(torch.autograd.Function):
    """mean over each row's own ``lengths[b]`` steps of a [B, T, C] fp32 sequence (ecgmm_seq_mean_varlen_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, lengths):
        _require_cuda(x, "seq_mean")
        x = f32c(x)
        B, T, Cn = x.shape
        out = torch.empty(B, Cn, device=x.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_seq_mean_varlen_fwd(ptr(x), ptr(lengths), ptr(out), B, T, Cn, stream()), "seq_mean_varlen_fwd")
        ctx.shape, ctx.lengths = (B, T, Cn), lengths
        return out

    @staticmethod
    def backward(ctx, dy):
        B, T, Cn = ctx.shape
        dy = f32c(dy)
        dx = torch.empty(B, T, Cn, device=dy.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_seq_mean_varlen_bwd(ptr(dy), ptr(ctx.lengths), ptr(dx), B, T, Cn, stream()),
                "seq_mean_varlen_bwd")
        return dx, None


def seq_mean(x, lengths=None):
    """mean over the time axis of ``x [B, T, C]``; with ``lengths`` (:func:`check_lengths`) over each row's own first
    ``lengths[b]`` steps, the gradient exactly 0 behind them."""
    if lengths is None:
        return SeqMeanFn.apply(x)
    _require_cuda(x, "seq_mean")
    if x.dim() != 3:
        raise RuntimeError(f"seq_mean: input must be [B, T, C], got {tuple(x.shape)}")
    return SeqMeanVarlenFn.apply(x, check_lengths(lengths, x.shape[0], x.shape[1]).to(x.device).contiguous())


# --------------------------------------------------------------------------------------------
# CRNN conv front end (three ConvBlocks as one plan)      reference: train_physionet2.py:55-65, 87-93
# --------------------------------------------------------------------------------------------
class CRNNFrontFn(torch.autograd.Function):
    """seq [B, T/8, 128*(F/8)] = front end(x [B,1,F,T]; 12 params, 9 buffers).  Holds the forward workspace on ``ctx``; the
    backward writes the parameter gradients into their sinks, and returns d / d x when the spectrogram requires a gradient
    (``ecgmm_crnn_front_backward_dx``: the Cin = 1 convolution's input gradient runs only then), behind a training-mode or
    an eval-mode forward."""

    @staticmethod
    def forward(ctx, x, cfg, buffers, *params):
        training, momentum, eps, dtype = cfg
        _require_cuda(x, "crnn_front")
        for t in tuple(params) + tuple(buffers):
            _require_cuda(t, "crnn_front parameter")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"crnn_front expects [B,1,F,T], got {tuple(x.shape)}")
        if len(params) != 12 or len(buffers) != 9:
            raise RuntimeError(f"crnn_front: {len(params)} parameters / {len(buffers)} buffers, expected 12 / 9")
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("crnn_front: parameters must be contiguous fp32")
        x = f32c(x)
        B, _, F, T = x.shape
        desc = L.CRNNFrontDesc(B, F, T, int(dtype), int(bool(training)), float(momentum), float(eps))
        lib = L.lib()
        nb = lib.ecgmm_crnn_front_fwd_workspace(C.byref(desc))
        if nb == 0:
            L.check(1, "crnn_front workspace query")
        ws = new_bytes(nb, x.device)
        seq = torch.empty(B, T // 8, 128 * (F // 8), device=x.device, dtype=torch.float32)
        L.check(lib.ecgmm_crnn_front_forward(C.byref(desc), ptr(x), _ptr_table(params), _ptr_table(buffers), ptr(seq),
                                             ptr(ws), ws.numel(), stream()), "crnn_front forward")
        ctx.desc, ctx.ws, ctx.x, ctx.params = desc, ws, x, params
        return seq

    @staticmethod
    def backward(ctx, dseq):
        desc, params = ctx.desc, ctx.params
        if ctx.ws is None:
            raise RuntimeError("crnn_front: second backward through a training-mode forward whose workspace was released")
        lib = L.lib()
        dseq = f32c(dseq)
        sinks = [grad_sink(p) if ctx.needs_input_grad[3 + i] else None for i, p in enumerate(params)]
        nb = lib.ecgmm_crnn_front_bwd_workspace(C.byref(desc))
        bws = _Scratch.get("crnn_front_bwd", nb, dseq.device)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(ctx.x)
            L.check(lib.ecgmm_crnn_front_backward_dx(C.byref(desc), ptr(ctx.x), ptr(dseq), _ptr_table(params),
                                                     _ptr_table(sinks), ptr(ctx.ws), ptr(bws), bws.numel(), ptr(dx), stream()),
                    "crnn_front backward")
        else:
            L.check(lib.ecgmm_crnn_front_backward(C.byref(desc), ptr(ctx.x), ptr(dseq), _ptr_table(params), _ptr_table(sinks),
                                                  ptr(ctx.ws), ptr(bws), bws.numel(), stream()), "crnn_front backward")
        if desc.training:
            ctx.ws = None
        return (dx, None, None) + (None,) * len(params)


def crnn_grad_cam(seq, dseq, steps, frames, F, T, channels=128):
    """Grad-CAM of the CRNN's last ConvBlock on the spectrogram (``ecgmm_crnn_gradcam``): ``seq``, ``dseq`` [B, Tp, C*Fp]
    fp32 (the front end's output, the chosen logit's gradient w.r.t. it), ``steps`` / ``frames`` int32 [B] or None (live
    steps 1..Tp, live spectrogram frames 1..T) -> ``[B, F, T]`` fp32 in [0, 1], exactly 0 at ``t >= frames[b]``."""
    _require_cuda(seq, "crnn_grad_cam seq")
    _require_cuda(dseq, "crnn_grad_cam dseq")
    seq, dseq = f32c(seq), f32c(dseq)
    if seq.dim() != 3 or seq.shape != dseq.shape or seq.shape[2] % channels:
        raise ValueError(f"crnn_grad_cam: seq {tuple(seq.shape)} / dseq {tuple(dseq.shape)} must both be "
                         f"[B, Tp, {channels}*Fp]")
    B, Tp, Fp = seq.shape[0], seq.shape[1], seq.shape[2] // channels
    tabs = []
    for t, what in ((steps, "steps"), (frames, "frames")):
        if t is not None:
            _require_cuda(t, "crnn_grad_cam " + what)
            if t.dtype != torch.int32 or t.shape != (B,):
                raise ValueError(f"crnn_grad_cam: {what} must be int32 [{B}], got {t.dtype} {tuple(t.shape)}")
            t = t.contiguous()
        tabs.append(t)
    lib = L.lib()
    nb = lib.ecgmm_crnn_gradcam_workspace(B, Tp, Fp, channels)
    if nb == 0:
        L.check(1, "crnn_gradcam workspace query")
    ws = _Scratch.get("crnn_gradcam", nb, seq.device)
    cam = torch.empty(B, F, T, device=seq.device, dtype=torch.float32)
    L.check(lib.ecgmm_crnn_gradcam(ptr(seq), ptr(dseq), ptr(tabs[0]), ptr(tabs[1]), ptr(ws), ws.numel(), ptr(cam), B, Tp,
                                   channels, Fp, int(F), int(T), stream()), "crnn_gradcam")
    return cam


def crnn_front(x, params, buffers, training, momentum=0.1, eps=1e-5, dtype=L.F32):
    """conv1..conv3 of the CRNN + permute + Flatten: ``params`` per block conv weight, conv bias, bn weight, bn bias;
    ``buffers`` per block running_mean, running_var, num_batches_tracked"""
    return CRNNFrontFn.apply(x, (training, momentum, eps, dtype), tuple(buffers), *params)


# --------------------------------------------------------------------------------------------
# LIME tabular (csrc/lime.hip)         reference: lime_fusion_modal_balance.py:118-160
# --------------------------------------------------------------------------------------------
LIME_TABLE_KEYS = ("qts", "cdf", "stats", "lim", "nbins")


def lime_perturb(x, table, num_samples, b0=0, seed_offset=None, return_uniforms=False):
    """Z uint8 [B, N, D], inverse fp32 [B, N, D], d2 int32 [B, N] (and the uniforms, double [B, N, D, 2]) of the rows
    ``x`` [B, D] under the discretiser ``table`` (``QuartileDiscretizer.table(device)``: qts, cdf [D, S] float64,
    stats [4, D, S] float64, lim [2, D, S] fp32, nbins [D] int32).  ``b0``: the index of x[0] in the caller's batch, which
    enters the Philox counter; ``seed_offset`` None takes one offset of the library's stream."""
    _require_cuda(x, "lime_perturb")
    for k in LIME_TABLE_KEYS:
        _require_cuda(table[k], "lime_perturb table")
    x = f32c(x)
    if x.dim() != 2:
        raise ValueError(f"lime_perturb expects rows [B, D], got {tuple(x.shape)}")
    B, D = x.shape
    N, S = int(num_samples), int(table["cdf"].shape[1])
    want = {"qts": ((D, S), torch.float64), "cdf": ((D, S), torch.float64), "stats": ((4, D, S), torch.float64),
            "lim": ((2, D, S), torch.float32), "nbins": ((D,), torch.int32)}
    for k, (shape, dt) in want.items():
        t = table[k]
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"lime_perturb: table[{k!r}] must be contiguous {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    seed, off = _PhiloxState.take(4) if seed_offset is None else seed_offset
    Z = torch.empty(B, max(N, 0), D, dtype=torch.uint8, device=x.device)
    inverse = torch.empty(B, max(N, 0), D, dtype=torch.float32, device=x.device)
    d2 = torch.empty(B, max(N, 0), dtype=torch.int32, device=x.device)
    u = torch.empty(B, max(N, 0), D, 2, dtype=torch.float64, device=x.device) if return_uniforms else None
    L.check(L.lib().ecgmm_lime_perturb(ptr(x), ptr(table["qts"]), ptr(table["cdf"]), ptr(table["stats"]), ptr(table["lim"]),
                                       ptr(table["nbins"]), S, B, int(b0), N, D, int(seed), int(off), ptr(Z), ptr(inverse),
                                       ptr(d2), ptr(u), stream()), "lime_perturb")
    return (Z, inverse, d2, u) if return_uniforms else (Z, inverse, d2)


def lime_ridge(Z, d2, y, kernel_width, alpha, cols=None, want=("w", "score", "local_pred")):
    """The weighted ridge fit of LIME for B samples and L labels at once: Z uint8 [B, N, D], d2 int32 [B, N],
    y fp32 [B, L, N], cols int32 [B, K] or None (all columns).  -> dict(coef [B, L, K], intercept [B, L]) plus the
    entries of ``want``: w [B, N], score [B, L], local_pred [B, L]."""
    _require_cuda(Z, "lime_ridge")
    _require_cuda(d2, "lime_ridge")
    _require_cuda(y, "lime_ridge")
    if Z.dtype != torch.uint8 or d2.dtype != torch.int32 or Z.dim() != 3 or y.dim() != 3:
        raise ValueError("lime_ridge expects Z uint8 [B, N, D], d2 int32 [B, N], y [B, L, N]")
    Z, d2, y = Z.contiguous(), d2.contiguous(), f32c(y)
    B, N, D = Z.shape
    Lb = y.shape[1]
    if tuple(d2.shape) != (B, N) or tuple(y.shape) != (B, Lb, N):
        raise ValueError(f"lime_ridge: d2 {tuple(d2.shape)} / y {tuple(y.shape)} do not match Z {tuple(Z.shape)}")
    K = D
    if cols is not None:
        _require_cuda(cols, "lime_ridge")
        if cols.dtype != torch.int32 or cols.dim() != 2 or cols.shape[0] != B:
            raise ValueError("lime_ridge: cols must be int32 [B, K]")
        cols = cols.contiguous()
        K = cols.shape[1]
    lib = L.lib()
    nb = lib.ecgmm_lime_ridge_workspace(B, N, D)
    if nb == 0:
        L.check(1, "lime_ridge workspace query")
    ws = _Scratch.get("lime_ridge", nb, Z.device)
    f32 = dict(dtype=torch.float32, device=Z.device)
    out = {"coef": torch.empty(B, Lb, K, **f32), "intercept": torch.empty(B, Lb, **f32)}
    if "w" in want:
        out["w"] = torch.empty(B, N, **f32)
    for k in ("score", "local_pred"):
        if k in want:
            out[k] = torch.empty(B, Lb, **f32)
    L.check(lib.ecgmm_lime_ridge(ptr(Z), ptr(d2), ptr(y), ptr(cols), B, N, D, K, Lb, float(kernel_width), float(alpha),
                                 ptr(out["coef"]), ptr(out["intercept"]), ptr(out.get("w")), ptr(out.get("score")),
                                 ptr(out.get("local_pred")), ptr(ws), ws.numel(), stream()), "lime_ridge")
    return out


def lime_prob(logits, label, out=None):
    """column ``label`` of softmax(logits, dim=1); ``out``: a 1-D view of M elements (any stride) to write into"""
    _require_cuda(logits, "lime_prob")
    logits = f32c(logits)
    M, Cn = logits.shape
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=logits.device)
    if out.dtype != torch.float32 or out.dim() != 1 or out.shape[0] != M or not out.is_cuda:
        raise ValueError("lime_prob: out must be a fp32 device vector of M elements")
    L.check(L.lib().ecgmm_lime_prob(ptr(logits), M, Cn, int(label), ptr(out), out.stride(0) if M > 1 else 1, stream()),
            "lime_prob")
    return out


def softmax_rows(logits):
    """softmax(logits, dim=1) [M, C], one ``lime_prob`` launch per class (C is the number of classes: 2)"""
    logits = f32c(logits)
    probs = torch.empty_like(logits)
    for c in range(logits.shape[1]):
        lime_prob(logits, c, probs[:, c])
    return probs


def _shap_operands(what, x, bg, w1, b1, w2):
    for t in (x, bg, w1, b1, w2):
        _require_cuda(t, what)
    x, bg, w1, b1, w2 = (f32c(t.detach()) for t in (x, bg, w1, b1, w2))
    if x.dim() != 2 or bg.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or b1.dim() != 1:
        raise ValueError(f"{what} expects x [B, D], bg [N, D], w1 [H, D], b1 [H], w2 [C, H]")
    (B, D), N, (H, C) = x.shape, bg.shape[0], (w1.shape[0], w2.shape[0])
    if bg.shape[1] != D or w1.shape[1] != D or b1.shape[0] != H or w2.shape[1] != H:
        raise ValueError(f"{what}: x {tuple(x.shape)}, bg {tuple(bg.shape)}, w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, "
                         f"w2 {tuple(w2.shape)} do not fit together")
    return x, bg, w1, b1, w2, B, N, D, H, C


def _shap_workspace(B, K, D, H, C, device):
    nb = L.lib().ecgmm_shap_mlp_workspace(B, K, D, H, C)
    if nb == 0:
        L.check(1, "shap workspace query")
    return _Scratch.get("shap_mlp", nb, device)


def shap_gradient(x, bg, ridx, t, w1, b1, w2, want_var=False, want_z=False):
    """Expected gradients of Linear(D, H) -> ReLU -> Linear(H, C) for B samples at once on the caller's draws: x [B, D],
    bg [N, D], ridx int32 [B, K] (background row of pair k), t fp32 [B, K] (its point t x + (1 - t) bg).
    -> dict(phi [B, D, C]) plus var [B, D, C] (population variance over k / sqrt(K)) and z [B, K, H] where asked for."""
    x, bg, w1, b1, w2, B, N, D, H, C = _shap_operands("shap_gradient", x, bg, w1, b1, w2)
    _require_cuda(ridx, "shap_gradient")
    _require_cuda(t, "shap_gradient")
    if ridx.dtype != torch.int32 or ridx.dim() != 2 or ridx.shape[0] != B or tuple(t.shape) != tuple(ridx.shape):
        raise ValueError("shap_gradient: ridx must be int32 [B, K] and t fp32 [B, K]")
    ridx, t = ridx.contiguous(), f32c(t)
    K = ridx.shape[1]
    ws = _shap_workspace(B, K, D, H, C, x.device)
    f32 = dict(dtype=torch.float32, device=x.device)
    out = {"phi": torch.empty(B, D, C, **f32)}
    if want_var:
        out["var"] = torch.empty(B, D, C, **f32)
    if want_z:
        out["z"] = torch.empty(B, K, H, **f32)
    L.check(L.lib().ecgmm_shap_gradient(ptr(x), ptr(bg), ptr(ridx), ptr(t), ptr(w1), ptr(b1), ptr(w2), B, N, K, D, H, C,
                                        ptr(out["phi"]), ptr(out.get("var")), ptr(out.get("z")), ptr(ws), ws.numel(),
                                        stream()), "shap_gradient")
    return out


def shap_deep(x, bg, w1, b1, w2, want_z=False):
    """DeepLIFT (rescale rule) of Linear(D, H) -> ReLU -> Linear(H, C) against every background row: x [B, D], bg [N, D].
    -> dict(phi [B, D, C]) plus zx [B, H], zb [N, H] where asked for."""
    x, bg, w1, b1, w2, B, N, D, H, C = _shap_operands("shap_deep", x, bg, w1, b1, w2)
    ws = _shap_workspace(B, N, D, H, C, x.device)
    f32 = dict(dtype=torch.float32, device=x.device)
    out = {"phi": torch.empty(B, D, C, **f32)}
    if want_z:
        out["zx"], out["zb"] = torch.empty(B, H, **f32), torch.empty(N, H, **f32)
    L.check(L.lib().ecgmm_shap_deep(ptr(x), ptr(bg), ptr(w1), ptr(b1), ptr(w2), B, N, D, H, C, ptr(out["phi"]),
                                    ptr(out.get("zx")), ptr(out.get("zb")), ptr(ws), ws.numel(), stream()), "shap_deep")
    return out


# --------------------------------------------------------------------------------------------
# Transformer encoder pieces      reference: train_physionet.py:216-220, 233-236 (nn.TransformerEncoderLayer);
#                                 multimodal_paper_modal_balance.py:127-194
# --------------------------------------------------------------------------------------------
def _aligned16(t):
    """the attention kernels read rows as float4: a view that starts off a 16-byte boundary is copied (plumbing)"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class MultiHeadAttentionFn(torch.autograd.Function):
    """out [rows, E] = concat_heads(softmax(Q K^T / sqrt(d)) V) of the packed projection qkv [rows, 3E] (csrc/attention.hip).
    Saves qkv, out and one log-sum-exp per score row; the backward recomputes the probabilities and, with dropout, the keep
    decisions from the call's (seed, offset).  ``cfg`` may carry a sixth entry, the device ``int32 [N]`` lengths (or
    ``None``): the ``_varlen`` entry points, else the fixed ones; the lengths are kept for the backward.  A true seventh
    entry also returns the log-sum-exp ``[N * heads * S]``, marked non-differentiable (the attention maps are rebuilt from
    it); the launches are the same."""

    @staticmethod
    def forward(ctx, qkv, cfg):
        S, N, heads, batch_first, p, lengths, want_lse = (tuple(cfg) + (None, False))[:7]
        _require_cuda(qkv, "multi_head_attention")
        if qkv.dim() != 2 or qkv.shape[0] != S * N or qkv.shape[1] % (3 * heads):
            raise RuntimeError(f"multi_head_attention: qkv must be [S * N, 3 * E] with E a multiple of heads, got "
                               f"{tuple(qkv.shape)} for S={S} N={N} heads={heads}")
        qkv = _aligned16(f32c(qkv))
        E = qkv.shape[1] // 3
        desc = L.MHADesc(S, N, heads, E // heads, int(batch_first), float(p))
        out = torch.empty(S * N, E, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(N * heads * S, device=qkv.device, dtype=torch.float32)
        seed, off = _PhiloxState.take(4) if p > 0 else (0, 0)
        if lengths is None:
            L.check(L.lib().ecgmm_mha_forward(C.byref(desc), ptr(qkv), ptr(out), ptr(lse), seed, off, stream()), "mha_forward")
        else:
            if lengths.dtype != torch.int32 or tuple(lengths.shape) != (N,) or lengths.device != qkv.device:
                raise RuntimeError(f"multi_head_attention: lengths must be int32 [{N}] on {qkv.device} (HF.check_lengths)")
            lengths = lengths.contiguous()
            L.check(L.lib().ecgmm_mha_forward_varlen(C.byref(desc), ptr(qkv), ptr(lengths), ptr(out), ptr(lse), seed, off,
                                                     stream()), "mha_forward_varlen")
        ctx.desc, ctx.rng, ctx.lengths = desc, (seed, off), lengths
        ctx.save_for_backward(qkv, out, lse)
        if want_lse:
            ctx.mark_non_differentiable(lse)
            return out, lse
        return out

    @staticmethod
    def backward(ctx, dout, _dlse=None):
        qkv, out, lse = ctx.saved_tensors
        desc = ctx.desc
        dout = _aligned16(f32c(dout))
        dqkv = torch.empty_like(qkv)
        lib = L.lib()
        ws = _Scratch.get("mha_bwd", lib.ecgmm_mha_bwd_workspace(C.byref(desc)), qkv.device)
        if ctx.lengths is None:
            L.check(lib.ecgmm_mha_backward(C.byref(desc), ptr(qkv), ptr(out), ptr(lse), ptr(dout), ptr(dqkv), ptr(ws),
                                           ws.numel(), ctx.rng[0], ctx.rng[1], stream()), "mha_backward")
        else:
            L.check(lib.ecgmm_mha_backward_varlen(C.byref(desc), ptr(qkv), ptr(ctx.lengths), ptr(out), ptr(lse), ptr(dout),
                                                  ptr(dqkv), ptr(ws), ws.numel(), ctx.rng[0], ctx.rng[1], stream()),
                    "mha_backward_varlen")
        return dqkv, None


def multi_head_attention(qkv, S, N, heads, batch_first=False, p=0.0, training=False, *, return_lse=False, lengths=None):
    """Self-attention on the packed projection ``qkv`` [S * N, 3E] (row ``s * N + n``, or ``n * S + s`` with
    ``batch_first``) -> [S * N, E], heads concatenated.  ``p``: dropout on the attention weights, in training only; its
    Philox offset comes from :func:`manual_seed`'s stream.

    ``lengths`` (one per attention-batch element ``n``, see :func:`check_lengths`): positions ``s >= lengths[n]`` are padding,
    torch's ``key_padding_mask[n, s] = s >= lengths[n]``: no query attends to them, their own output rows are exact zeros and
    so are their rows of the gradient.  Padded rows of ``qkv`` (and of the incoming gradient) are never read and may hold
    anything.  A device tensor is not synced: the kernels clamp it to ``[0, S]`` (a 0 makes everything of ``n`` zero).

    ``return_lse`` (keyword only, as ``lengths`` now is beside it): -> ``(out, lse)``, ``lse`` [N * heads * S] the log-sum-exp of every score row as the forward wrote it
    (non-differentiable): what :func:`attention_weights` and :func:`attention_rollout_step` rebuild the maps from.  Off, the
    call is what it always was."""
    p = float(p) if training else 0.0
    cfg = (int(S), int(N), int(heads), bool(batch_first), p)
    lengths = _mha_lengths(lengths, qkv, N, S)
    if lengths is not None or return_lse:
        cfg += (lengths,)
    if return_lse:
        cfg += (True,)
    return MultiHeadAttentionFn.apply(qkv, cfg)


def _mha_lengths(lengths, qkv, N, S):
    """``None`` or the device ``int32 [N]`` tensor the attention kernels take (validated unless it already is one)"""
    if lengths is None:
        return None
    if not (isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and tuple(lengths.shape) == (int(N),)
            and lengths.device == qkv.device):
        lengths = check_lengths(lengths, int(N), int(S)).to(qkv.device)
    return lengths.contiguous()


def _maps_operands(what, qkv, lse, S, N, heads, batch_first, lengths):
    """the checked operands of the two map entry points -> (qkv, lse, desc, lengths)"""
    _require_cuda(qkv, what)
    _require_cuda(lse, what)
    S, N, heads = int(S), int(N), int(heads)
    if qkv.dim() != 2 or qkv.shape[0] != S * N or qkv.shape[1] % (3 * heads):
        raise RuntimeError(f"{what}: qkv must be [S * N, 3 * E] with E a multiple of heads, got {tuple(qkv.shape)} for "
                           f"S={S} N={N} heads={heads}")
    if lse.numel() != N * heads * S:
        raise RuntimeError(f"{what}: lse must hold N * heads * S = {N * heads * S} values, got {tuple(lse.shape)}")
    qkv, lse = _aligned16(f32c(qkv.detach())), f32c(lse.detach())
    desc = L.MHADesc(S, N, heads, qkv.shape[1] // 3 // heads, int(bool(batch_first)), 0.0)
    return qkv, lse, desc, _mha_lengths(lengths, qkv, N, S)


def attention_weights(qkv, lse, S, N, heads, batch_first=False, lengths=None, average=True):
    """The attention weights of :func:`multi_head_attention` on ``qkv``, rebuilt from the ``lse`` it returned
    (``return_lse=True``; ``ecgmm_mha_weights``): ``[N, S, S]`` averaged over the heads (``average``, torch's
    ``average_attn_weights``) or ``[N, heads, S, S]``, always (query row, key column).  These are the probabilities before
    dropout.  With ``lengths`` the padded query rows and key columns are exact zeros (torch's padded query rows still attend).
    ``4 * N * S * S`` bytes (times ``heads`` per head).  The result is detached and carries no gradient."""
    qkv, lse, desc, lengths = _maps_operands("attention_weights", qkv, lse, S, N, heads, batch_first, lengths)
    shape = (desc.N, desc.S, desc.S) if average else (desc.N, desc.heads, desc.S, desc.S)
    w = torch.empty(shape, device=qkv.device, dtype=torch.float32)
    L.check(L.lib().ecgmm_mha_weights(C.byref(desc), ptr(qkv), ptr(lse), ptr(lengths), ptr(w), 0 if average else 1, stream()),
            "mha_weights")
    return w


def attention_rollout_step(qkv, lse, v, S, N, heads, batch_first=False, lengths=None, residual=0.5):
    """One step of attention rollout of the row vectors ``v`` [N, S] through one attention layer (``ecgmm_mha_rollout_step``):
    ``residual * v + (1 - residual) * v @ mean_h P`` with ``P`` the layer's attention weights, rebuilt from ``qkv`` and the
    ``lse`` of its forward without forming them.  ``0 <= residual < 1``.  With ``lengths`` padded ``v`` is never read and the
    padded result is exact 0.  The result is detached and carries no gradient."""
    residual = float(residual)
    if not 0.0 <= residual < 1.0:
        raise ValueError(f"attention_rollout_step: residual={residual} must lie in [0, 1)")
    qkv, lse, desc, lengths = _maps_operands("attention_rollout_step", qkv, lse, S, N, heads, batch_first, lengths)
    _require_cuda(v, "attention_rollout_step")
    if tuple(v.shape) != (desc.N, desc.S):
        raise RuntimeError(f"attention_rollout_step: v must be [N, S] = [{desc.N}, {desc.S}], got {tuple(v.shape)}")
    v = f32c(v.detach())
    y = torch.empty_like(v)
    L.check(L.lib().ecgmm_mha_rollout_step(C.byref(desc), ptr(qkv), ptr(lse), ptr(lengths), ptr(v), ptr(y), residual,
                                           stream()), "mha_rollout_step")
    return y


class AddFn(torch.autograd.Function):
    """a + b through ecgmm_ew (the residual connections of the encoder layer)."""

    @staticmethod
    def forward(ctx, a, b):
        _require_cuda(a, "add")
        _require_cuda(b, "add")
        a, b = f32c(a), f32c(b)
        if a.shape != b.shape:
            raise RuntimeError(f"add: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
        out = torch.empty_like(a)
        L.check(L.lib().ecgmm_ew(7, ptr(a), ptr(b), ptr(out), a.numel(), 0.0, stream()), "ew add")   # ECGMM_EW_ADD
        return out

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return AddFn.apply(a, b)


class Embed1dFn(torch.autograd.Function):
    """[B, Cin, L] -> [B, L, D]: Conv1d(Cin, D, 3, padding=1) + bias, channels last, + pos[0, :L] in one launch."""

    @staticmethod
    def forward(ctx, x, weight, bias, pos):
        for t in (x, weight, bias, pos):
            _require_cuda(t, "embed1d")
        x = f32c(x)
        if x.dim() != 3 or weight.dim() != 3 or weight.shape[1] != x.shape[1] or weight.shape[2] != 3:
            raise RuntimeError(f"embed1d: x {tuple(x.shape)} / weight {tuple(weight.shape)}: need [B, Cin, L] and [D, Cin, 3]")
        B, Cin, Ln = x.shape
        D = weight.shape[0]
        if pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[2] != D or pos.shape[1] < Ln:
            raise RuntimeError(f"embed1d: pos {tuple(pos.shape)} must be [1, >= {Ln}, {D}]")
        for p in (weight, bias, pos):
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("embed1d: parameters must be contiguous fp32")
        y = torch.empty(B, Ln, D, device=x.device, dtype=torch.float32)
        L.check(L.lib().ecgmm_embed1d_fwd(ptr(x), ptr(weight), ptr(bias), ptr(pos), ptr(y), B, Cin, Ln, D, stream()),
                "embed1d_fwd")
        ctx.params = (weight, bias, pos)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        weight, bias, pos = ctx.params
        B, Cin, Ln = x.shape
        D = weight.shape[0]
        dy = f32c(dy)
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None
        dw = grad_sink(weight) if need[1] else None
        db = grad_sink(bias) if need[2] else None
        dpos = grad_sink(pos) if need[3] else None
        lib = L.lib()
        ws = _Scratch.get("embed1d", lib.ecgmm_embed1d_bwd_workspace(B, Cin, Ln, D), x.device)
        L.check(lib.ecgmm_embed1d_bwd(ptr(x), ptr(weight), ptr(dy), ptr(dw), ptr(db), ptr(dpos), ptr(dx), B, Cin, Ln, D,
                                      pos.shape[1], ptr(ws), ws.numel(), stream()), "embed1d_bwd")
        return dx, None, None, None


def embed1d(x, weight, bias, pos):
    return Embed1dFn.apply(x, weight, bias, pos)


# --------------------------------------------------------------------------------------------
# forward-only tails of a post-norm encoder layer (csrc/transformer_infer.hip)     reference: train_physionet.py:219-220, 236
# --------------------------------------------------------------------------------------------
def _forward_only(what, tensors):
    """the fused tails keep nothing for a backward: refuse an input that would want one"""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is forward-only (it saves nothing for a backward): call it under torch.no_grad() or "
                           "detach its inputs; training goes through ecgmm.hip.nn.TransformerEncoderLayer")
    out = []
    for t in tensors:
        _require_cuda(t, what)
        out.append(_aligned16(f32c(t.detach())))
    return out


def linear_res_ln(a, weight, bias, res, gamma, beta, eps=1e-5):
    """``LayerNorm(res + a @ weight.T + bias)`` over the last axis as ONE launch (``ecgmm_linear_res_ln``): ``a`` [R, K],
    ``weight`` [E, K], ``res`` [R, E] -> [R, E] -- ``out_proj`` + residual + ``norm1`` of an encoder layer in eval mode.
    Forward-only.  ``E`` a multiple of 16 up to 256, ``K`` a multiple of 16 up to 4096."""
    a, weight, bias, res, gamma, beta = _forward_only("linear_res_ln", (a, weight, bias, res, gamma, beta))
    if a.dim() != 2 or weight.dim() != 2 or res.dim() != 2 or a.shape[1] != weight.shape[1] or \
            tuple(res.shape) != (a.shape[0], weight.shape[0]):
        raise RuntimeError(f"linear_res_ln: a {tuple(a.shape)}, weight {tuple(weight.shape)}, res {tuple(res.shape)}: need "
                           "[R, K], [E, K] and [R, E]")
    E = weight.shape[0]
    for name, t in (("bias", bias), ("gamma", gamma), ("beta", beta)):
        if tuple(t.shape) != (E,):
            raise RuntimeError(f"linear_res_ln: {name} {tuple(t.shape)} must be [{E}]")
    out = torch.empty_like(res)
    L.check(L.lib().ecgmm_linear_res_ln(ptr(a), ptr(weight), ptr(bias), ptr(res), ptr(gamma), ptr(beta), ptr(out), a.shape[0],
                                        a.shape[1], E, float(eps), stream()), "linear_res_ln")
    return out


def ffn_res_ln(x, w1, b1, w2, b2, gamma, beta, eps=1e-5):
    """``LayerNorm(x + relu(x @ w1.T + b1) @ w2.T + b2)`` as ONE launch (``ecgmm_ffn_res_ln``): ``x`` [R, E], ``w1`` [ff, E],
    ``w2`` [E, ff] -> [R, E] -- the feed-forward block + residual + ``norm2`` of an encoder layer in eval mode; the hidden
    activation is never stored.  Forward-only.  ``E`` a multiple of 16 up to 256, ``ff`` a multiple of 16 up to 4096."""
    x, w1, b1, w2, b2, gamma, beta = _forward_only("ffn_res_ln", (x, w1, b1, w2, b2, gamma, beta))
    if x.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != x.shape[1] or \
            tuple(w2.shape) != (x.shape[1], w1.shape[0]):
        raise RuntimeError(f"ffn_res_ln: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}: need [R, E], [ff, E] "
                           "and [E, ff]")
    E, ff = x.shape[1], w1.shape[0]
    for name, t, n in (("b1", b1, ff), ("b2", b2, E), ("gamma", gamma, E), ("beta", beta, E)):
        if tuple(t.shape) != (n,):
            raise RuntimeError(f"ffn_res_ln: {name} {tuple(t.shape)} must be [{n}]")
    out = torch.empty_like(x)
    L.check(L.lib().ecgmm_ffn_res_ln(ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(gamma), ptr(beta), ptr(out), x.shape[0], E,
                                     ff, float(eps), stream()), "ffn_res_ln")
    return out
