"""Inference path: ``Predictor(model)(...)`` returns what ``model.eval()(...)`` returns under ``torch.no_grad()``, through
the encoders' *inference plans* (csrc/plan_infer.hip) instead of the training plans' eval mode.

What the reference does at every validation / test pass (train.py:92-95, 175-182; train_kfold.py:72-74, 118-121;
train_image_only.py:142-144; signal_model.py:174-176) and for embedding extraction (shap_fusion_modal_balance.py:54-59)::

    model.eval()
    with torch.no_grad():
        out = model(images, ecg, clinical)

becomes::

    predict = Predictor(model)          # folds every BatchNorm into its convolution, once
    out = predict(images, ecg, clinical)

An inference plan keeps nothing for a backward: no saved activations, no ReLU bits, no pool indices, no statistics rows.
Grad-CAM and input gradients (ecgmm/explain.py) therefore keep using the model's own eval forward.

**Stale weights.**  The folded weights are a snapshot.  ``FusedAdam`` (and the HIP backward) write parameters and
gradients through raw pointers, so tensor version counters do not move and a ``Predictor`` cannot notice that the model
was trained further: call :meth:`Predictor.refresh` after the weights changed (``load_state_dict``, an optimizer step).
Until then it keeps returning the answer of the weights it was prepared from.  The snapshot covers both encoders and
the multimodal head; the clinical branch of the MLP variant (a few small dense layers) runs the model's own eval forward on
the live parameters.

**TabNet** (``ecgmm.tabnet.ClinicalTabNetEncoder``): ``Predictor(encoder)(x) -> z``, and inside
``Predictor(model, clinical_plan=True)`` the TabNet variant's clinical branch: the whole eval forward is ONE launch of
``ecgmm_tabnet_infer`` (csrc/tabnet_infer.hip) on a blob in which every BatchNorm is folded into the ``fc`` in front of it
(a shared ``fc`` once per FeatTransformer, with that FeatTransformer's statistics), where the module's forward issues about
110.  The blob is a snapshot like every other part of a predictor.  ``clinical_plan=False`` keeps the module's own forward;
the MLP variant and a TabNet shape outside the fused path (``ecgmm.tabnet.FUSED_LIMITS``) do so silently.

**The spectrogram CRNN** (``ecgmm.crnn.CRNN``, ``train_physionet2``): ``Predictor(model)(x, lengths=None)``.  The three
ConvBlocks run as ``ecgmm_crnn_front_infer`` (csrc/plan_infer.hip: block 1 as one conv + ReLU + pool kernel, no
``[B, F, T, 32]`` tensor, no argmax bytes, no per-call weight packs); the LSTM (no saves), the mean over time and the
classifier run on snapshots of their parameters, so the whole answer is stale until ``refresh()``.

**The transformer** (``ecgmm.train_physionet.ECGTransformer1D``, both ``time_attention`` modes):
``Predictor(model)(x, lengths=None)``.  The whole forward is ONE call of ``ecgmm_transformer_infer`` on a blob that holds a
copy of every parameter: embed, then four launches per encoder layer (``in_proj``, attention, ``out_proj`` + residual +
``norm1`` as ``ecgmm_linear_res_ln``, the feed-forward block + residual + ``norm2`` as ``ecgmm_ffn_res_ln``) where the
model's own eval forward takes nine, the mean over the positions and the classifier.  The workspace rotates three
``[B L, d_model]`` buffers through all layers; the ``[B L, dim_feedforward]`` hidden activation is never stored.  The
attention records ``ecgmm.explain`` works from (``attention_sink``) are not offered: it keeps using the model's forward.
"""
import ctypes as C

import torch

from .crnn import CRNN
from .hip import encoders as E
from .hip import lib as L
from .hip.functional import _Scratch, _require_cuda, f32c, new_bytes, ptr, stream
from .image_encoder import ResNet18
from .multimodal_paper_modal_balance import ECGMultimodalModel, ResNet1D_SE
from . import tabnet as T
from .train_physionet import ECGTransformer1D

__all__ = ["Predictor"]


class _EncoderPlan:
    """Prepared blob + launch of one encoder (``ResNet18`` or ``ResNet1D_SE``)."""

    def __init__(self, module):
        if isinstance(module, ResNet18):
            self.prefix, self.name, self.n_params, self.n_buffers = "ecgmm_resnet18", "resnet18", 62, 60
        elif isinstance(module, ResNet1D_SE):
            self.prefix, self.name, self.n_params, self.n_buffers = "ecgmm_resnet1d", "resnet1d_se", 52, 27
        else:
            raise TypeError(f"no inference plan for {type(module).__name__}")
        self.module = module
        self.blob = None
        self.refresh()

    def _desc(self, N, a, b):
        m = self.module
        if self.name == "resnet18":
            return L.ResNet18Desc(N, a, b, self.out_dim, self.dtype, 0, 0.0, self.eps)
        return L.ResNet1DDesc(N, m.input_channels, a, self.out_dim, self.dtype, 0, 0.0, self.eps, 0.0, 0, 0)

    def refresh(self):
        m = self.module
        params, buffers = list(m.parameters()), list(m.buffers())
        if len(params) != self.n_params or len(buffers) != self.n_buffers:
            raise RuntimeError(f"{self.name}: expected {self.n_params} parameters / {self.n_buffers} buffers, found "
                               f"{len(params)} / {len(buffers)}")
        for t in params + buffers:
            _require_cuda(t, f"Predictor({self.name}) parameter")
        self.dtype = E.dtype_code(m.compute_dtype)
        if self.name == "resnet18":
            self.out_dim, self.eps = m.fc.weight.shape[0], float(m.bn1.eps)
        else:
            self.out_dim, self.eps = m.classifier[4].weight.shape[0], float(m.initial[1].eps)
        lib = L.lib()
        desc = self._desc(0, 0, 0)
        nb = getattr(lib, self.prefix + "_infer_prepared_bytes")(C.byref(desc))
        if nb == 0:
            L.check(1, self.name + " prepared-size query")
        dev = params[0].device
        with torch.cuda.device(dev):
            # a NEW blob: a forward already enqueued with the old one (another stream) keeps reading consistent weights
            blob = new_bytes(nb, dev)
            L.check(getattr(lib, self.prefix + "_infer_prepare")(C.byref(desc), E._table(params), E._table(buffers), ptr(blob),
                                                                 blob.numel(), stream()), self.name + " infer prepare")
        self.blob = blob

    def __call__(self, x):
        m = self.module
        _require_cuda(x, f"Predictor({self.name})")
        if E.dtype_code(m.compute_dtype) != self.dtype:
            raise RuntimeError(f"Predictor({self.name}): the model's compute dtype is now {m.compute_dtype!r} but the weights "
                               "were prepared in another one -- call refresh()")
        if self.name == "resnet18":
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError(f"image encoder expects [B,3,H,W], got {tuple(x.shape)}")
            desc = self._desc(x.shape[0], x.shape[2], x.shape[3])
        else:
            if x.dim() != 3 or x.shape[1] != m.input_channels:
                raise ValueError(f"signal encoder expects [B,{m.input_channels},L], got {tuple(x.shape)}")
            desc = self._desc(x.shape[0], x.shape[2], 0)
        x = f32c(x)
        lib = L.lib()
        nb = getattr(lib, self.prefix + "_infer_workspace")(C.byref(desc))
        if nb == 0:
            L.check(1, self.name + " infer workspace query")
        ws = _Scratch.get(self.prefix + "_infer", nb, x.device)   # transient: nothing in it outlives the call
        self.blob.record_stream(torch.cuda.current_stream(x.device))
        feat = torch.empty(x.shape[0], self.out_dim, device=x.device, dtype=torch.float32)
        L.check(getattr(lib, self.prefix + "_infer")(C.byref(desc), ptr(x), ptr(self.blob), self.blob.numel(), ptr(feat),
                                                     ptr(ws), ws.numel(), stream()), self.name + " infer")
        return feat

    def workspace_bytes(self, *shape):
        """Bytes of the inference workspace for an input of ``shape`` (no GPU work)."""
        desc = self._desc(shape[0], shape[2], shape[3] if self.name == "resnet18" else 0)
        return int(getattr(L.lib(), self.prefix + "_infer_workspace")(C.byref(desc)))


class _CRNNPlan:
    """The spectrogram ``CRNN`` (ecgmm/crnn.py): the three ConvBlocks through ``ecgmm_crnn_front_infer`` (folded blob, 5
    launches, no ``[B, F, T, 32]`` tensor), then the LSTM, the mean over time and the classifier on ``detach().clone()``
    snapshots of their parameters -- so the WHOLE answer is that of the weights the plan was prepared from."""

    def __init__(self, model):
        self.model = model
        cls = list(model.classifier)
        if len(cls) != 4 or not isinstance(cls[1], torch.nn.ReLU) or not isinstance(cls[2], torch.nn.Dropout):
            raise RuntimeError("Predictor(CRNN): the classifier is not the Linear-ReLU-Dropout-Linear layout")
        self.blob = None
        self.refresh()

    def _desc(self, B, F, T):
        return L.CRNNFrontDesc(B, F, T, self.dtype, 0, 0.0, self.eps)

    def refresh(self):
        m = self.model
        params, buffers = m._front_tables()
        lstm = [getattr(m.bilstm, n) for n in m.bilstm._flat_names]
        dense = [m.classifier[0].weight, m.classifier[0].bias, m.classifier[3].weight, m.classifier[3].bias]
        for t in params + buffers + lstm + dense:
            _require_cuda(t, "Predictor(CRNN) parameter")
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("Predictor(CRNN): parameters must be contiguous fp32")
        self.dtype, self.eps = E.dtype_code(m.compute_dtype), float(m.conv1.block[1].eps)
        lib = L.lib()
        desc = self._desc(0, 0, 0)
        nb = lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(desc))
        if nb == 0:
            L.check(1, "crnn_front prepared-size query")
        dev = params[0].device
        with torch.cuda.device(dev), torch.no_grad():
            # a NEW blob and new snapshots: a forward already enqueued with the old ones keeps reading consistent weights
            blob = new_bytes(nb, dev)
            L.check(lib.ecgmm_crnn_front_infer_prepare(C.byref(desc), E._table(params), E._table(buffers), ptr(blob),
                                                       blob.numel(), stream()), "crnn_front infer prepare")
            self._lstm = [p.detach().clone() for p in lstm]
            self._dense = [p.detach().clone() for p in dense]
        self.blob = blob

    def front(self, x):
        """``x [B, 1, F, T]`` -> ``seq [B, T // 8, 128 * (F // 8)]`` fp32; the shape errors are ``CRNN._front``'s"""
        m = self.model
        _require_cuda(x, "Predictor(CRNN)")
        if E.dtype_code(m.compute_dtype) != self.dtype:
            raise RuntimeError(f"Predictor(CRNN): the model's compute dtype is now {m.compute_dtype!r} but the weights "
                               "were prepared in another one -- call refresh()")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"CRNN expects a log-spectrogram [B,1,F,T], got {tuple(x.shape)}")
        B, _, F, T = x.shape
        if 128 * (F // 8) != m.bilstm.input_size:
            raise ValueError(f"CRNN: F={F} frequency bins give {128 * (F // 8)} features per time step after three 2x2 "
                             f"pools, but the LSTM takes {m.bilstm.input_size} (F must be 32..39)")
        if T < 8:
            raise ValueError(f"CRNN: T={T} time bins; three 2x2 pools need at least 8")
        x = f32c(x)
        desc = self._desc(B, F, T)
        lib = L.lib()
        nb = lib.ecgmm_crnn_front_infer_workspace(C.byref(desc))
        if nb == 0:
            L.check(1, "crnn_front infer workspace query")
        ws = _Scratch.get("ecgmm_crnn_front_infer", nb, x.device)   # transient: nothing in it outlives the call
        self.blob.record_stream(torch.cuda.current_stream(x.device))
        seq = torch.empty(B, T // 8, 128 * (F // 8), device=x.device, dtype=torch.float32)
        L.check(lib.ecgmm_crnn_front_infer(C.byref(desc), ptr(x), ptr(self.blob), self.blob.numel(), ptr(seq), ptr(ws),
                                           ws.numel(), stream()), "crnn_front infer")
        return seq

    def __call__(self, x, lengths=None):
        from .hip import functional as HF
        m = self.model
        seq = self.front(x)
        rnn = m.bilstm
        if lengths is not None:   # CRNN._tail's rule: three floor pools give exactly // 8
            lengths = HF.check_lengths(lengths, seq.shape[0], x.shape[3]).to(seq.device)
            lengths = torch.clamp(lengths // 8, 1, seq.shape[1]).to(torch.int32)
        # under no_grad nothing requires a gradient, so the LSTM keeps no saves (save = 0)
        out, _ = HF.lstm(seq, None, self._lstm, rnn.hidden_size, rnn.num_layers, rnn.bidirectional, rnn.batch_first, lengths)
        w1, b1, w2, b2 = self._dense
        return HF.linear(HF.linear(HF.seq_mean(out, lengths), w1, b1, L.ACT_RELU), w2, b2)   # eval: no dropout


class _TransformerPlan:
    """``ECGTransformer1D`` (ecgmm/train_physionet.py) through ``ecgmm_transformer_infer`` (csrc/plan_infer.hip): one blob
    with a copy of every parameter, four launches per encoder layer, rotating buffers -- the WHOLE answer is that of the
    weights the plan was prepared from."""

    LAYER = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
             "norm2.bias")

    def __init__(self, model):
        self.model = model
        layers = list(model.transformer_encoder.layers)
        attn = layers[0].self_attn
        self.E, self.heads, self.ff = attn.embed_dim, attn.num_heads, layers[0].linear1.out_features
        if self.E > 256 or self.E % 16:
            raise ValueError(f"Predictor(ECGTransformer1D): d_model={self.E} is not supported by the fused layer tails (a "
                             "multiple of 16 with d_model <= 256)")
        if self.ff % 16 or self.ff > 4096:
            raise ValueError(f"Predictor(ECGTransformer1D): dim_feedforward={self.ff} is not supported by the fused layer "
                             "tails (a multiple of 16 with dim_feedforward <= 4096)")
        cls = list(model.classifier)
        if len(cls) != 5 or not isinstance(cls[2], torch.nn.ReLU) or not isinstance(cls[3], torch.nn.Dropout) or \
                cls[1].out_features != 64:
            raise RuntimeError("Predictor(ECGTransformer1D): the classifier is not the Flatten-Linear(64)-ReLU-Dropout-Linear "
                               "layout")
        self.blob = None
        self.refresh()

    def _params(self):
        m = self.model
        sd = dict(m.named_parameters())
        names = ["conv.weight", "conv.bias", "pos_embedding"]
        for i in range(len(m.transformer_encoder.layers)):
            names += [f"transformer_encoder.layers.{i}.{n}" for n in self.LAYER]
        names += ["classifier.1.weight", "classifier.1.bias", "classifier.4.weight", "classifier.4.bias"]
        return [sd[n] for n in names]

    def _desc(self, B, L_):
        return L.TransformerInferDesc(B, L_, self.input_dim, self.E, self.heads, self.ff, self.layers, self.classes,
                                      int(self.batch_first), self.eps)

    def refresh(self):
        m = self.model
        params = self._params()
        for p in params:
            _require_cuda(p, "Predictor(ECGTransformer1D) parameter")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("Predictor(ECGTransformer1D): parameters must be contiguous fp32")
        layers = list(m.transformer_encoder.layers)
        eps = {float(n.eps) for k in layers for n in (k.norm1, k.norm2)}
        if len(eps) != 1:
            raise RuntimeError("Predictor(ECGTransformer1D): the LayerNorms do not share one eps")
        self.input_dim, self.layers, self.classes = m.conv.in_channels, len(layers), m.classifier[4].out_features
        self.batch_first, self.eps, self.seq_len = bool(m.time_attention), eps.pop(), m.pos_embedding.shape[1]
        lib = L.lib()
        desc = self._desc(0, self.seq_len)
        nb = lib.ecgmm_transformer_infer_prepared_bytes(C.byref(desc))
        if nb == 0:
            L.check(1, "transformer prepared-size query")
        dev = params[0].device
        with torch.cuda.device(dev), torch.no_grad():
            # a NEW blob: a forward already enqueued with the old one (another stream) keeps reading consistent weights
            blob = new_bytes(nb, dev)
            L.check(lib.ecgmm_transformer_infer_prepare(C.byref(desc), E._table(params), ptr(blob), blob.numel(), stream()),
                    "transformer infer prepare")
        self.blob, self._blob_len = blob, self.seq_len

    def __call__(self, x, lengths=None):
        from .hip import functional as HF
        m = self.model
        if lengths is not None and not self.batch_first:
            raise ValueError("ECGTransformer1D: lengths needs time_attention=True (attention across the batch has no "
                             "per-sample length)")
        _require_cuda(x, "Predictor(ECGTransformer1D)")
        if bool(m.time_attention) != self.batch_first:
            raise RuntimeError("Predictor(ECGTransformer1D): the model's time_attention changed since the plan was prepared "
                               "-- call refresh()")
        if x.dim() != 3 or x.shape[1] != self.input_dim:
            raise ValueError(f"ECGTransformer1D expects [B, {self.input_dim}, L], got {tuple(x.shape)}")
        B, _, Ln = x.shape
        if Ln > self._blob_len:
            raise ValueError(f"ECGTransformer1D: L={Ln} exceeds seq_len={self._blob_len}")
        if lengths is not None:
            lengths = HF.check_lengths(lengths, B, Ln).to(x.device).contiguous()
        x = f32c(x)
        # the blob's positional table has seq_len rows and is its last entry: a shorter L reads the same blob
        desc = self._desc(B, Ln)
        lib = L.lib()
        nb = lib.ecgmm_transformer_infer_workspace(C.byref(desc))
        if nb == 0:
            L.check(1, "transformer infer workspace query")
        ws = _Scratch.get("ecgmm_transformer_infer", nb, x.device)   # transient: nothing in it outlives the call
        self.blob.record_stream(torch.cuda.current_stream(x.device))
        logits = torch.empty(B, self.classes, device=x.device, dtype=torch.float32)
        L.check(lib.ecgmm_transformer_infer(C.byref(desc), ptr(x), ptr(lengths), ptr(self.blob), self.blob.numel(), ptr(logits),
                                            ptr(ws), ws.numel(), stream()), "transformer infer")
        return logits

    def workspace_bytes(self, B, Ln):
        """Bytes of the inference workspace for ``B`` records of ``Ln`` samples (no GPU work)."""
        return int(L.lib().ecgmm_transformer_infer_workspace(C.byref(self._desc(B, Ln))))


class _TabNetPlan:
    """``ClinicalTabNetEncoder`` through ``ecgmm_tabnet_infer`` (csrc/tabnet_infer.hip): one folded blob, one launch per
    forward -- the answer is that of the parameters and running statistics the plan was prepared from."""

    def __init__(self, module):
        if not isinstance(module, T.ClinicalTabNetEncoder):
            raise TypeError(f"no TabNet inference plan for {type(module).__name__}")
        self.module = module
        self.blob = None
        self.refresh()

    def refresh(self):
        net = self.module.tabnet
        self.desc, self.blob = T.fused_fold(net.encoder, net.final_mapping.weight)
        return self

    def __call__(self, x):
        """``x [B, D]`` -> ``z [B, latent_dim]`` (the module's forward also returns M_loss; a predictor has no use for it)"""
        return T.fused_run(self.desc, self.blob, x)[0]

    def masks(self, x):
        """``(M_explain [B, D], {step: M [B, D]})`` of the snapshot (``forward_masks`` of the module folds per call)"""
        _, mexp, masks, _ = T.fused_run(self.desc, self.blob, x, explain=True)
        return mexp, {step: masks[step] for step in range(self.desc.n_steps)}


def _find_encoder(model):
    if isinstance(model, (ResNet18, ResNet1D_SE)):
        return model
    enc = getattr(model, "image_encoder", None)       # ImageOnlyClassifier and the like: a wrapper around one encoder
    if isinstance(enc, ResNet18) and not isinstance(model, ECGMultimodalModel):
        return enc
    return None


class Predictor:
    """Eval-mode forward of ``model`` through the inference plans.

    ``model``: an ``ECGMultimodalModel`` (either variant), a ``ResNet18`` / ``ImageOnlyClassifier``, a ``ResNet1D_SE``,
    the spectrogram ``CRNN``, an ``ECGTransformer1D`` (either ``time_attention`` mode) or a ``ClinicalTabNetEncoder``
    (``predictor(x) -> z``), on a ROCm device.  ``clinical_plan`` (multimodal TabNet variant only): the clinical branch as one
    fused launch on a folded snapshot instead of the module's own forward.  Construction prepares the folded weights; :meth:`refresh` prepares them
    again (see the module docstring: nothing can detect stale weights for you).  Calling the predictor never changes
    ``model.training``, a running statistic or a ``.grad``.  A ``CRNN`` predictor is called as the model is,
    ``predictor(x, lengths=None)``; its snapshot covers the front end, the LSTM and the classifier.  So is an
    ``ECGTransformer1D`` predictor (``lengths`` only with ``time_attention``); its snapshot covers every parameter.  It
    refuses ``d_model > 256`` and a ``dim_feedforward`` that is no multiple of 16 or exceeds 4096 with a ``ValueError``.
    """

    def __init__(self, model, clinical_plan=True):
        self.model = model
        self.multimodal = isinstance(model, ECGMultimodalModel)
        self.crnn = isinstance(model, CRNN)
        self.transformer = isinstance(model, ECGTransformer1D)
        self.clinical = None
        if isinstance(model, T.ClinicalTabNetEncoder):
            self.encoder = _TabNetPlan(model)
        elif self.crnn:
            self.encoder = _CRNNPlan(model)
        elif self.transformer:
            self.encoder = _TransformerPlan(model)
        elif self.multimodal:
            self.image, self.signal = _EncoderPlan(model.image_encoder), _EncoderPlan(model.signal_encoder)
            clin = model.clinical_encoder
            if clinical_plan and isinstance(clin, T.ClinicalTabNetEncoder) and \
                    T.fused_refusal(clin.tabnet.encoder, clin.tabnet.final_mapping.weight.shape[0]) is None:
                self.clinical = _TabNetPlan(clin)
            self._snapshot_head()
        else:
            enc = _find_encoder(model)
            if enc is None:
                raise TypeError(f"Predictor: unsupported model {type(model).__name__} (ECGMultimodalModel, ResNet18, "
                                "ImageOnlyClassifier, ResNet1D_SE, CRNN, ECGTransformer1D or ClinicalTabNetEncoder)")
            self.encoder = _EncoderPlan(enc)

    def _snapshot_head(self):
        with torch.no_grad():
            self._head_params = [p.detach().clone() for p in self.model._head_params()]

    def refresh(self):
        """Prepare the folded weights again from the model's current parameters and running statistics."""
        if self.multimodal:
            self.image.refresh()
            self.signal.refresh()
            if self.clinical is not None:
                self.clinical.refresh()
            self._snapshot_head()
        else:
            self.encoder.refresh()
        return self

    @torch.no_grad()
    def __call__(self, *inputs, lengths=None):
        if self.crnn or self.transformer:
            if len(inputs) == 2 and lengths is None:
                inputs, lengths = inputs[:1], inputs[1]
            if len(inputs) != 1:
                raise TypeError(f"Predictor({type(self.model).__name__}) takes ({'spectrogram' if self.crnn else 'signal'}, "
                                f"lengths=None), got {len(inputs)} inputs")
            return self.encoder(inputs[0], lengths)
        if lengths is not None:
            raise TypeError(f"Predictor({type(self.model).__name__}) takes no lengths")
        if not self.multimodal:
            if len(inputs) != 1:
                raise TypeError(f"Predictor({type(self.model).__name__}) takes one input, got {len(inputs)}")
            return self.encoder(inputs[0])
        if len(inputs) != 3:
            raise TypeError(f"Predictor({type(self.model).__name__}) takes (image, ecg_signal, clinical), got {len(inputs)} inputs")
        model = self.model
        image, ecg_signal, clinical = inputs
        for t, what in ((image, "image"), (ecg_signal, "ecg_signal"), (clinical, "clinical")):
            _require_cuda(t, f"Predictor {what}")
        if model.clinical_encoder.training:
            raise RuntimeError("Predictor: the clinical branch runs the model's own forward, which is in training mode "
                               "(batch statistics, dropout) -- call model.eval() first; the predictor does not change it")
        spec = model._head_spec()
        if spec is None:
            raise RuntimeError("Predictor: this model's head is not the fused Linear-ReLU-Dropout-Linear / LayerNorm layout")
        spec.training = False
        ecg_signal = ecg_signal.unsqueeze(1)
        from . import multimodal_paper_modal_balance as pmb
        if getattr(model.config, "overlap_encoders", True) and pmb._OVERLAP_ENV:
            # as ECGMultimodalModel.forward: the small-kernel branches on a side stream underneath the image encoder
            main = torch.cuda.current_stream(image.device)
            side = model._side_stream = getattr(model, "_side_stream", None) or torch.cuda.Stream(image.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                signal_raw = self.signal(ecg_signal)
                clinical_raw = self._clinical_forward(clinical)
            image_raw = self.image(image)
            main.wait_stream(side)
            signal_raw.record_stream(main)
            clinical_raw.record_stream(main)
        else:
            image_raw = self.image(image)
            signal_raw = self.signal(ecg_signal)
            clinical_raw = self._clinical_forward(clinical)
        return E.run_head(image_raw, signal_raw, clinical_raw, spec, self._head_params)

    def _clinical_forward(self, clinical):
        return self.clinical(clinical) if self.clinical is not None else self.model._clinical_forward(clinical)

    def logits(self, *inputs):
        """The class logits of a forward: ``fusion_logits`` of the multimodal 6-tuple, the output itself otherwise."""
        out = self(*inputs)
        return out[3] if self.multimodal else out

    def predict_proba(self, loader, device=None):
        """Softmax probabilities of a whole loader, in loader order.

        Batches are ``(*inputs, labels)`` or ``(*inputs, labels, index)`` with three inputs for the multimodal model and
        one otherwise (the dataset classes of this package); for a ``CRNN`` the one input is the spectrogram or the pair
        ``(spectrogram, frames)`` a loader with lengths yields (``train_physionet2.DeviceSpectrogramLoader``); for an
        ``ECGTransformer1D`` the signals ``[B, L]`` (given their channel axis here) or the pair ``(signals, lengths)`` of
        ``train_physionet.DeviceSignalLoader``.
        -> ``(prob [n, classes], labels [n], index [n])`` CPU tensors; without an index column the index is the running
        position."""
        n_in = 3 if self.multimodal else 1
        device = device or next(self.model.parameters()).device
        probs, labels, index, seen = [], [], [], 0
        for batch in loader:
            if len(batch) not in (n_in + 1, n_in + 2):
                raise ValueError(f"predict_proba: a batch of {len(batch)} tensors; expected {n_in} inputs, labels[, index]")
            inputs = batch[:n_in]
            if (self.crnn or self.transformer) and isinstance(inputs[0], (tuple, list)):   # ((input, lengths), labels)
                inputs = tuple(inputs[0])
            inputs = [t.to(device) for t in inputs]
            if self.transformer and inputs[0].dim() == 2:   # the loaders yield [B, L]; the model takes [B, 1, L]
                inputs[0] = inputs[0].unsqueeze(1)
            logits = self.logits(*inputs)
            probs.append(torch.softmax(logits.float().cpu(), dim=1))
            labels.append(torch.as_tensor(batch[n_in]).cpu())
            b = probs[-1].shape[0]
            index.append(torch.as_tensor(batch[n_in + 1]).cpu() if len(batch) == n_in + 2 else torch.arange(seen, seen + b))
            seen += b
        if not probs:
            return torch.empty(0, 0), torch.empty(0, dtype=torch.long), torch.empty(0, dtype=torch.long)
        return torch.cat(probs), torch.cat(labels), torch.cat(index)
