"""Inference path: ``Predictor(model)(...)`` returns what ``model.eval()(...)`` returns under ``torch.no_grad()`` -- what the
reference does at every validation / test pass (train.py:92-95, 175-182; train_kfold.py:72-74, 118-121;
train_image_only.py:142-144; signal_model.py:174-176) and for embedding extraction (shap_fusion_modal_balance.py:54-59) --
through an *inference plan* instead of the training plans' eval mode::

    predict = Predictor(model)          # prepares the weights once (every BatchNorm folded into its convolution / fc)
    out = predict(images, ecg, clinical)

A plan keeps nothing for a backward (no saved activations, ReLU bits, pool indices, statistics rows, attention records), so
Grad-CAM, input gradients and the attention maps (ecgmm/explain.py) keep using the model's own eval forward.

**Stale weights.**  The prepared weights are a snapshot.  ``FusedAdam`` (and the HIP backward) write parameters through raw
pointers, so tensor version counters do not move and a ``Predictor`` cannot notice that the model was trained further: call
:meth:`Predictor.refresh` after the weights changed (``load_state_dict``, an optimizer step).  Until then it keeps returning
the answer of the weights it was prepared from.

**The plans** (each a ``PreparedPlan``, ecgmm/hip/prepared.py: one blob, one prepare step, one launch procedure):
``ResNet18`` / ``ImageOnlyClassifier`` and ``ResNet1D_SE`` -- the folded encoders of csrc/plan_infer.hip;
``CRNN`` -- ``(x, lengths=None)``: the three ConvBlocks as ``ecgmm_crnn_front_infer``, then the LSTM (no saves), the mean over
time and the classifier on snapshots of their parameters;
``ECGTransformer1D`` (both ``time_attention`` modes) -- ``(x, lengths=None)``: ONE call of ``ecgmm_transformer_infer`` on a copy
of every parameter, four launches per encoder layer where the model's eval forward takes nine;
``ClinicalTabNetEncoder`` -- ``(x) -> z``: ONE launch of ``ecgmm_tabnet_infer`` (csrc/tabnet_infer.hip) where the module issues
about 110;
``ECGMultimodalModel`` -- both encoders, a snapshot of the head and, for the TabNet variant with ``clinical_plan=True``, the
clinical branch as a TabNet plan.  The MLP variant's clinical branch, ``clinical_plan=False`` and a TabNet shape outside
``ecgmm.tabnet.FUSED_LIMITS`` run the module's own eval forward on the live parameters.
"""
import torch

from .crnn import CRNN
from .hip import encoders as E
from .hip import functional as HF
from .hip import lib as L
from .hip.functional import _require_cuda, f32c
from .hip.prepared import PreparedPlan
from .image_encoder import ResNet18
from .multimodal_paper_modal_balance import ECGMultimodalModel, ResNet1D_SE
from . import tabnet as T
from .train_physionet import ECGTransformer1D

__all__ = ["Predictor"]


class _EncoderPlan(PreparedPlan):
    """Prepared blob + launch of one BatchNorm-folded encoder; a subclass names the encoder, its table sizes, its descriptor
    and its input-shape check."""
    n_params = n_buffers = None

    def refresh(self):
        m = self.module
        params, buffers = list(m.parameters()), list(m.buffers())
        if len(params) != self.n_params or len(buffers) != self.n_buffers:
            raise RuntimeError(f"{self.name}: expected {self.n_params} parameters / {self.n_buffers} buffers, found "
                               f"{len(params)} / {len(buffers)}")
        self.check_params(params + buffers, self.who + " parameter")
        self.dtype = E.dtype_code(m.compute_dtype)
        self.out_dim, self.eps = self._head(m)
        self.blob = self.prepare(self._desc(), [params, buffers], params[0].device)

    def __call__(self, x):
        _require_cuda(x, self.who)
        self.check_compute_dtype()
        self._check_input(x)
        x = f32c(x)
        return self.run(self._desc(*x.shape), self.blob, (x,), [(x.shape[0], self.out_dim)], x.device)[0]


class _ResNet18Plan(_EncoderPlan):
    prefix, name, who = "ecgmm_resnet18", "resnet18", "Predictor(resnet18)"
    n_params, n_buffers = L.RESNET18_NPARAMS, L.RESNET18_NBUFFERS

    _head = staticmethod(lambda m: (m.fc.weight.shape[0], float(m.bn1.eps)))      # (out_dim, BatchNorm eps)

    def _desc(self, N=0, C=3, H=0, W=0):
        return L.ResNet18Desc(N, H, W, self.out_dim, self.dtype, 0, 0.0, self.eps)

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"image encoder expects [B,3,H,W], got {tuple(x.shape)}")


class _ResNet1DPlan(_EncoderPlan):
    prefix, name, who = "ecgmm_resnet1d", "resnet1d_se", "Predictor(resnet1d_se)"
    n_params, n_buffers = L.RESNET1D_NPARAMS, L.RESNET1D_NBUFFERS

    _head = staticmethod(lambda m: (m.classifier[4].weight.shape[0], float(m.initial[1].eps)))

    def _desc(self, N=0, C=None, Ln=0):
        return L.ResNet1DDesc(N, self.module.input_channels, Ln, self.out_dim, self.dtype, 0, 0.0, self.eps, 0.0, 0, 0)

    def _check_input(self, x):
        if x.dim() != 3 or x.shape[1] != self.module.input_channels:
            raise ValueError(f"signal encoder expects [B,{self.module.input_channels},L], got {tuple(x.shape)}")


class _CRNNPlan(PreparedPlan):
    """The spectrogram ``CRNN`` (ecgmm/crnn.py): the three ConvBlocks through ``ecgmm_crnn_front_infer`` (folded blob, 5
    launches, no ``[B, F, T, 32]`` tensor), then the LSTM, the mean over time and the classifier on ``detach().clone()``
    snapshots of their parameters -- so the WHOLE answer is that of the weights the plan was prepared from."""
    prefix, name, who = "ecgmm_crnn_front", "crnn_front", "Predictor(CRNN)"
    inputs, takes_lengths = ("spectrogram",), True

    def __init__(self, model):
        cls = list(model.classifier)
        if len(cls) != 4 or not isinstance(cls[1], torch.nn.ReLU) or not isinstance(cls[2], torch.nn.Dropout):
            raise RuntimeError("Predictor(CRNN): the classifier is not the Linear-ReLU-Dropout-Linear layout")
        super().__init__(model)

    def _desc(self, B=0, C=1, F=0, T=0):
        return L.CRNNFrontDesc(B, F, T, self.dtype, 0, 0.0, self.eps)

    def refresh(self):
        m = self.module
        params, buffers = m._front_tables()
        lstm = [getattr(m.bilstm, n) for n in m.bilstm._flat_names]
        dense = [m.classifier[0].weight, m.classifier[0].bias, m.classifier[3].weight, m.classifier[3].bias]
        self.check_params(params + buffers + lstm + dense, self.who + " parameter")
        self.check_params(params, self.who + " parameter", fp32=self.who)
        self.dtype, self.eps = E.dtype_code(m.compute_dtype), float(m.conv1.block[1].eps)
        blob = self.prepare(self._desc(), [params, buffers], params[0].device)
        with torch.no_grad():   # new snapshots beside the new blob: an enqueued forward keeps the old ones
            self._lstm = [p.detach().clone() for p in lstm]
            self._dense = [p.detach().clone() for p in dense]
        self.blob = blob

    def front(self, x):
        """``x [B, 1, F, T]`` -> ``seq [B, T // 8, 128 * (F // 8)]`` fp32; the shape errors are ``CRNN._front``'s"""
        m = self.module
        _require_cuda(x, self.who)
        self.check_compute_dtype()
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"CRNN expects a log-spectrogram [B,1,F,T], got {tuple(x.shape)}")
        B, _, F, T = x.shape
        if 128 * (F // 8) != m.bilstm.input_size:
            raise ValueError(f"CRNN: F={F} frequency bins give {128 * (F // 8)} features per time step after three 2x2 "
                             f"pools, but the LSTM takes {m.bilstm.input_size} (F must be 32..39)")
        if T < 8:
            raise ValueError(f"CRNN: T={T} time bins; three 2x2 pools need at least 8")
        x = f32c(x)
        return self.run(self._desc(*x.shape), self.blob, (x,), [(B, T // 8, 128 * (F // 8))], x.device)[0]

    def __call__(self, x, lengths=None):
        seq = self.front(x)
        rnn = self.module.bilstm
        if lengths is not None:   # CRNN._tail's rule: three floor pools give exactly // 8
            lengths = HF.check_lengths(lengths, seq.shape[0], x.shape[3]).to(seq.device)
            lengths = torch.clamp(lengths // 8, 1, seq.shape[1]).to(torch.int32)
        # under no_grad nothing requires a gradient, so the LSTM keeps no saves (save = 0)
        out, _ = HF.lstm(seq, None, self._lstm, rnn.hidden_size, rnn.num_layers, rnn.bidirectional, rnn.batch_first, lengths,
                         getattr(rnn, "compute_dtype", "fp32"))   # the model's lstm_dtype
        w1, b1, w2, b2 = self._dense
        return HF.linear(HF.linear(HF.seq_mean(out, lengths), w1, b1, L.ACT_RELU), w2, b2)   # eval: no dropout


class _TransformerPlan(PreparedPlan):
    """``ECGTransformer1D`` (ecgmm/train_physionet.py) through ``ecgmm_transformer_infer`` (csrc/plan_infer.hip): one blob
    with a copy of every parameter, four launches per encoder layer, rotating buffers -- the WHOLE answer is that of the
    weights the plan was prepared from."""
    prefix, name, who = "ecgmm_transformer", "transformer", "Predictor(ECGTransformer1D)"
    inputs, takes_lengths = ("signal",), True

    LAYER = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
             "norm2.bias")

    def __init__(self, model):
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
        super().__init__(model)

    def _params(self):
        m = self.module
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
        m = self.module
        params = self._params()
        self.check_params(params, self.who + " parameter", fp32=self.who)
        layers = list(m.transformer_encoder.layers)
        eps = {float(n.eps) for k in layers for n in (k.norm1, k.norm2)}
        if len(eps) != 1:
            raise RuntimeError("Predictor(ECGTransformer1D): the LayerNorms do not share one eps")
        self.input_dim, self.layers, self.classes = m.conv.in_channels, len(layers), m.classifier[4].out_features
        self.batch_first, self.eps, self.seq_len = bool(m.time_attention), eps.pop(), m.pos_embedding.shape[1]
        blob = self.prepare(self._desc(0, self.seq_len), [params], params[0].device)
        self.blob, self._blob_len = blob, self.seq_len

    def batch_args(self, columns):
        x, *rest = super().batch_args(columns)
        return (x.unsqueeze(1) if x.dim() == 2 else x, *rest)   # the loaders yield [B, L]; the model takes [B, 1, L]

    def __call__(self, x, lengths=None):
        if lengths is not None and not self.batch_first:
            raise ValueError("ECGTransformer1D: lengths needs time_attention=True (attention across the batch has no "
                             "per-sample length)")
        _require_cuda(x, self.who)
        if bool(self.module.time_attention) != self.batch_first:
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
        return self.run(self._desc(B, Ln), self.blob, (x, lengths), [(B, self.classes)], x.device)[0]


class _TabNetPlan(T.FusedPlan):
    """``ClinicalTabNetEncoder`` through ``ecgmm_tabnet_infer`` (csrc/tabnet_infer.hip): one folded blob, one launch per
    forward -- the answer is that of the parameters and running statistics the plan was prepared from."""

    def __init__(self, module):
        if not isinstance(module, T.ClinicalTabNetEncoder):
            raise TypeError(f"no TabNet inference plan for {type(module).__name__}")
        super().__init__(module)

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


class _MultimodalPlan(PreparedPlan):
    """``ECGMultimodalModel`` (either variant): the image and signal plans, the clinical plan (None: the module's own eval
    forward on the live parameters) and a snapshot of the head, composed as ``ECGMultimodalModel.forward`` composes them."""
    inputs, logits = ("image", "ecg_signal", "clinical"), 3     # fusion_logits of the 6-tuple

    def __init__(self, model, clinical_plan=True):
        self.module = model
        self.image, self.signal = _ResNet18Plan(model.image_encoder), _ResNet1DPlan(model.signal_encoder)
        clin = model.clinical_encoder
        fused = clinical_plan and isinstance(clin, T.ClinicalTabNetEncoder) and \
            T.fused_refusal(clin.tabnet.encoder, clin.tabnet.final_mapping.weight.shape[0]) is None
        self.clinical = _TabNetPlan(clin) if fused else None
        self._snapshot_head()

    def _snapshot_head(self):
        with torch.no_grad():
            self._head_params = [p.detach().clone() for p in self.module._head_params()]

    def refresh(self):
        for plan in (self.image, self.signal, self.clinical):
            if plan is not None:
                plan.refresh()
        self._snapshot_head()

    def _clinical_forward(self, clinical):
        return self.clinical(clinical) if self.clinical is not None else self.module._clinical_forward(clinical)

    def __call__(self, image, ecg_signal, clinical):
        model = self.module
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


def _find_encoder(model):
    """``model`` itself, or the one encoder a wrapper such as ``ImageOnlyClassifier`` is around"""
    enc = getattr(model, "image_encoder", None)
    if isinstance(enc, ResNet18) and not isinstance(model, ECGMultimodalModel):
        return enc
    return model


# model type -> plan class, first match (what a new plan adds: see DESIGN.md, "adding an inference plan")
PLANS = ((T.ClinicalTabNetEncoder, _TabNetPlan), (CRNN, _CRNNPlan), (ECGTransformer1D, _TransformerPlan),
         (ECGMultimodalModel, _MultimodalPlan), (ResNet18, _ResNet18Plan), (ResNet1D_SE, _ResNet1DPlan))


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
        target = _find_encoder(model)
        plan = next((p for kind, p in PLANS if isinstance(target, kind)), None)
        if plan is None:
            raise TypeError(f"Predictor: unsupported model {type(model).__name__} (ECGMultimodalModel, ResNet18, "
                            "ImageOnlyClassifier, ResNet1D_SE, CRNN, ECGTransformer1D or ClinicalTabNetEncoder)")
        self.encoder = plan(target, clinical_plan) if plan is _MultimodalPlan else plan(target)
        self.multimodal = plan is _MultimodalPlan
        # the parts of a composed plan (None otherwise; ``clinical`` also when the module's own forward is used)
        self.image, self.signal, self.clinical = (getattr(self.encoder, n, None) for n in ("image", "signal", "clinical"))

    def refresh(self):
        """Prepare the folded weights again from the model's current parameters and running statistics."""
        self.encoder.refresh()
        return self

    @torch.no_grad()
    def __call__(self, *inputs, lengths=None):
        plan = self.encoder
        if plan.takes_lengths:
            if len(inputs) == len(plan.inputs) + 1 and lengths is None:
                inputs, lengths = inputs[:-1], inputs[-1]
        elif lengths is not None:
            raise TypeError(f"Predictor({type(self.model).__name__}) takes no lengths")
        if len(inputs) != len(plan.inputs):
            names = plan.inputs + ("lengths=None",) * plan.takes_lengths
            raise TypeError(f"Predictor({type(self.model).__name__}) takes " + (
                f"one input, got {len(inputs)}" if len(names) == 1 else f"({', '.join(names)}), got {len(inputs)} inputs"))
        return plan(*inputs, lengths) if plan.takes_lengths else plan(*inputs)

    def logits(self, *inputs):
        """The class logits of a forward: ``fusion_logits`` of the multimodal 6-tuple, the output itself otherwise."""
        out = self(*inputs)
        return out if self.encoder.logits is None else out[self.encoder.logits]

    def predict_proba(self, loader, device=None):
        """Softmax probabilities of a whole loader, in loader order.

        Batches are ``(*inputs, labels)`` or ``(*inputs, labels, index)`` with three inputs for the multimodal model and
        one otherwise (the dataset classes of this package); for a ``CRNN`` the one input is the spectrogram or the pair
        ``(spectrogram, frames)`` a loader with lengths yields (``train_physionet2.DeviceSpectrogramLoader``); for an
        ``ECGTransformer1D`` the signals ``[B, L]`` (given their channel axis here) or the pair ``(signals, lengths)`` of
        ``train_physionet.DeviceSignalLoader``.
        -> ``(prob [n, classes], labels [n], index [n])`` CPU tensors; without an index column the index is the running
        position."""
        n_in = len(self.encoder.inputs)
        device = device or next(self.model.parameters()).device
        probs, labels, index, seen = [], [], [], 0
        for batch in loader:
            if len(batch) not in (n_in + 1, n_in + 2):
                raise ValueError(f"predict_proba: a batch of {len(batch)} tensors; expected {n_in} inputs, labels[, index]")
            logits = self.logits(*(t.to(device) for t in self.encoder.batch_args(batch[:n_in])))
            probs.append(torch.softmax(logits.float().cpu(), dim=1))
            labels.append(torch.as_tensor(batch[n_in]).cpu())
            b = probs[-1].shape[0]
            index.append(torch.as_tensor(batch[n_in + 1]).cpu() if len(batch) == n_in + 2 else torch.arange(seen, seen + b))
            seen += b
        if not probs:
            return torch.empty(0, 0), torch.empty(0, dtype=torch.long), torch.empty(0, dtype=torch.long)
        return torch.cat(probs), torch.cat(labels), torch.cat(index)
