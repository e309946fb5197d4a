"""Saliency of the trained model down to its inputs: input gradients and Grad-CAM.

The reference's users explain a decision after training -- ``gpt/gpt_analysis.py`` is fed Grad-CAM overlays of the ECG
picture (``gpt/abnormal_gradcam_15_overlay.png`` and friends; the script that drew them is not in its tree, only the
pictures).  Every reference module is an ordinary autograd module, so ``image.requires_grad_(True)`` on an ``eval()``
model is all it takes there; here the encoders are native launch plans, whose backward produces the input gradient and
runs behind an eval-mode forward (csrc/plan_resnet18.hip, plan_resnet1d.hip, conv_stem_dgrad.hip, bn_eval_bwd.hip).

  * ``input_gradients``  d (class logit) / d (image, signal, clinical vector) per sample;
  * ``grad_cam``         the [N, H, W] map over the picture from the image encoder's last stage and the [N, L] map over the
                         signal from the signal encoder's last block: relu(sum_c a_c A_c) / max, a_c = the spatial mean of
                         d logit / d A_c, bilinearly upsampled to the input size (align_corners=False).  After a global
                         average pool that gradient is constant over space, so only the head's backward runs, not the
                         convolutions' (csrc/gradcam.hip);
  * ``encoder_grad_cam`` the same for a stand-alone ``ResNet18`` / ``ResNet1D_SE`` classifier;
  * ``attention_maps``   the attention weights of every encoder layer of an ``ECGTransformer1D``, rebuilt from what its
                         forward stored (csrc/attention.hip: ``ecgmm_mha_weights``);
  * ``attention_rollout`` the relevance of each input sample to the mean-pooled representation of an ``ECGTransformer1D``
                         with ``time_attention`` (Abnar & Zuidema 2020), one row vector per record and no S x S matrix
                         (``ecgmm_mha_rollout_step``);
  * ``spectrogram_gradients`` d (class logit) / d (log-spectrogram) of the ``CRNN`` of ``train_physionet2`` -- what
                         ``spectrogram.requires_grad_()`` gives in the reference (train_physionet2.py:59, 70): the front
                         end's plan returns the input gradient (csrc/crnn_front.hip: ``ecgmm_conv5_in1_bwd_data``);
  * ``spectrogram_grad_cam`` the [B, F, T] map over the spectrogram from the CRNN's last ConvBlock.  No average pool
                         stands in front of that head, so the gradient varies over space and is read
                         (csrc/gradcam.hip: ``ecgmm_crnn_gradcam``); only the LSTM's and the head's backward run.
Everything numeric runs in libecgmm_hip.so; there is no CPU path.
"""
import os

import torch

from .config import Config
from .hip import encoders as E
from .hip.functional import _require_cuda

OUTPUTS = {"image": 0, "signal": 1, "clinical": 2, "fusion": 3}


class _Frozen:
    """eval() + parameters frozen for the duration (no weight gradient is computed, no ``.grad`` sink is touched), as
    ``shap_fusion_modal_balance.expected_gradients`` does; both restored on exit."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was_training = self.model.training
        self.model.eval()
        self.frozen = [p for p in self.model.parameters() if p.requires_grad]
        for p in self.frozen:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.frozen:
            p.requires_grad_(True)
        self.model.train(self.was_training)


def _seed(logits, target):
    """one-hot d / d logits of the chosen class per sample (default: the predicted class)"""
    if target is None:
        target = logits.detach().argmax(dim=1)
    elif not torch.is_tensor(target):
        target = torch.full((logits.shape[0],), int(target), dtype=torch.long)
    target = target.to(logits.device).long().view(-1, 1)
    return torch.zeros_like(logits).scatter_(1, target, 1.0)


def _logits(outputs, output):
    if output not in OUTPUTS:
        raise ValueError(f"output must be one of {sorted(OUTPUTS)}, got {output!r}")
    return outputs[OUTPUTS[output]]


def input_gradients(model, image, ecg_signal, clinical, target=None, output="fusion"):
    """-> (d_image [N,3,H,W], d_signal [N,L], d_clinical [N,D]) of ``output``'s logit of class ``target`` (int, [N] tensor,
    or None = the predicted class), each sample its own.  A modality that ``output`` does not depend on gets zeros."""
    for t, what in ((image, "image"), (ecg_signal, "ecg_signal"), (clinical, "clinical")):
        _require_cuda(t, "input_gradients " + what)
    with _Frozen(model):
        xs = [t.detach().requires_grad_(True) for t in (image, ecg_signal, clinical)]
        logits = _logits(model(*xs), output)
        grads = torch.autograd.grad(logits, xs, grad_outputs=_seed(logits, target), allow_unused=True)
    return tuple(torch.zeros_like(x) if g is None else g for g, x in zip(grads, xs))


def _recorded(encoders):
    class _Rec:
        def __enter__(self):
            for e in encoders:
                e._spec.keep_last, e._spec.last = True, None

        def __exit__(self, *exc):
            for e in encoders:
                e._spec.keep_last, e._spec.last = False, None
    return _Rec()


def grad_cam(model, image, ecg_signal, clinical, target=None, output="fusion"):
    """-> (cam_image [N,H,W], cam_signal [N,L]) fp32 in [0, 1] for ``output``'s logit of class ``target``."""
    for t, what in ((image, "image"), (ecg_signal, "ecg_signal"), (clinical, "clinical")):
        _require_cuda(t, "grad_cam " + what)
    encoders = (model.image_encoder, model.signal_encoder)
    feats = {}
    hooks = [e.register_forward_hook(lambda _m, _i, out, k=k: feats.__setitem__(k, out)) for k, e in enumerate(encoders)]
    try:
        with _Frozen(model), _recorded(encoders):
            # (inputs that require a gradient make the encoders' outputs part of the graph; only the head's backward runs)
            xs = [image.detach().requires_grad_(True), ecg_signal.detach().requires_grad_(True), clinical.detach()]
            logits = _logits(model(*xs), output)
            dfeat = torch.autograd.grad(logits, [feats[0], feats[1]], grad_outputs=_seed(logits, target), allow_unused=True)
            cams = []
            for e, g, f in zip(encoders, dfeat, (feats[0], feats[1])):
                cams.append(E.plan_grad_cam(e._spec, torch.zeros_like(f) if g is None else g))
    finally:
        for h in hooks:
            h.remove()
    return cams[0], cams[1]


def encoder_grad_cam(encoder, x, target=None):
    """Grad-CAM of a stand-alone ``ResNet18`` ([N,3,H,W] -> [N,H,W]) or ``ResNet1D_SE`` ([N,cin,L] -> [N,L]) whose output
    are the class logits."""
    _require_cuda(x, "encoder_grad_cam input")
    with _Frozen(encoder), _recorded((encoder,)), torch.no_grad():
        logits = encoder(x)
        return E.plan_grad_cam(encoder._spec, _seed(logits, target))


def _attention_records(model, x, lengths):
    """one eval-mode forward of an ``ECGTransformer1D`` with a sink -> the attention record of every layer, first to last"""
    _require_cuda(x, "attention maps input")
    if not hasattr(model, "transformer_encoder"):
        raise ValueError("attention maps need an ECGTransformer1D (a model with a transformer_encoder)")
    sink = []
    with _Frozen(model), torch.no_grad():
        model(x, lengths, attention_sink=sink) if lengths is not None else model(x, attention_sink=sink)
    return sink


def attention_maps(model, x, lengths=None, average=True):
    """The attention weights of every encoder layer of an ``ECGTransformer1D`` on ``x`` [B, input_dim, L], in eval mode
    (no dropout): a list with one ``[N, S, S]`` tensor per layer (``average``: the mean over the heads, torch's
    ``average_attn_weights``) or ``[N, heads, S, S]``, rows = queries, columns = keys.  With ``time_attention`` N = B and
    S = L: a map over the record's positions, with ``lengths`` exact zeros in the padded rows and columns; without it the
    model attends across the batch, N = L and S = B.  Each layer's map takes ``4 * N * S * S`` bytes (times ``heads`` per
    head) -- 36 MB per record at L = 3000: for long records use :func:`attention_rollout`, which never forms it.
    Detached, no gradient."""
    from .hip import functional as HF
    return [HF.attention_weights(**rec, average=average) for rec in _attention_records(model, x, lengths)]


def attention_rollout(model, x, lengths=None, residual=0.5):
    """Attention rollout (Abnar & Zuidema 2020) of the mean-pooled representation of an ``ECGTransformer1D`` with
    ``time_attention`` -> ``[B, L]`` fp32: the relevance of each input sample, >= 0, summing to 1 per record, exactly 0 behind
    ``lengths``.  Each layer is taken as ``residual * I + (1 - residual) * A`` with ``A`` its head-averaged attention map
    (``residual`` in [0, 1); 0.5 is the paper's equal weighting of the skip connection); the model ends in the mean over
    the live positions, so the row vector ``1 / len`` is carried from the last layer to the first, one
    ``ecgmm_mha_rollout_step`` per layer, and no S x S matrix is formed.  The embedding (a 3-tap convolution plus the
    positional embedding) keeps positions, so the vector lies over the raw signal.  One eval-mode forward.  Detached."""
    from .hip import functional as HF
    residual = float(residual)
    if not 0.0 <= residual < 1.0:
        raise ValueError(f"attention_rollout: residual={residual} must lie in [0, 1)")
    if not getattr(model, "time_attention", False):
        raise ValueError("attention_rollout needs time_attention=True (attention across the batch has no per-record map)")
    records = _attention_records(model, x, lengths)
    B, Ln = x.shape[0], x.shape[2]
    if lengths is None:
        v = torch.full((B, Ln), 1.0 / Ln, device=x.device, dtype=torch.float32)
    else:
        n = records[0]["lengths"].to(torch.float32)[:, None]                  # validated by the forward: 1 <= n <= L
        v = torch.where(torch.arange(Ln, device=x.device)[None, :] < n, 1.0 / n, torch.zeros_like(n))
    for rec in reversed(records):
        v = HF.attention_rollout_step(rec["qkv"], rec["lse"], v, rec["S"], rec["N"], rec["heads"], rec["batch_first"],
                                      rec["lengths"], residual)
    return v


def _require_crnn(model, who):
    if not all(hasattr(model, name) for name in ("conv1", "conv2", "conv3", "bilstm")):
        raise ValueError(f"{who} needs a CRNN (a model with conv1..conv3 and a bilstm), got {type(model).__name__}")


def spectrogram_gradients(model, x, lengths=None, target=None):
    """d (logit of ``target``) / d ``x`` of a ``CRNN`` on log-spectrograms ``x [B, 1, F, T]`` -> ``[B, 1, F, T]`` fp32,
    each record its own: which time and which frequency band carried the decision.  ``lengths`` as in ``CRNN.forward``
    (the gradient just behind a record's end is not zero: the convolutions see the padding); ``target`` an int, a [B]
    tensor, or None = the predicted class.  Eval mode, parameters frozen, no ``.grad`` touched: the chain of input
    gradients alone runs (``ecgmm_crnn_front_backward_dx``), no weight gradient."""
    _require_crnn(model, "spectrogram_gradients")
    _require_cuda(x, "spectrogram_gradients input")
    with _Frozen(model):
        xs = x.detach().float().requires_grad_(True)
        logits = model(xs) if lengths is None else model(xs, lengths)
        (grad,) = torch.autograd.grad(logits, [xs], grad_outputs=_seed(logits, target))
    return grad


def spectrogram_grad_cam(model, x, lengths=None, target=None):
    """Grad-CAM of a ``CRNN``'s last ConvBlock over the log-spectrogram ``x [B, 1, F, T]`` -> ``[B, F, T]`` fp32 in [0, 1],
    exactly 0 at ``t >= lengths[b]``.  The front end runs without a graph; the graph starts at its output ``seq``, so only
    the LSTM's, the mean's and the classifier's backward run, no convolution's.  There is no global average pool in front
    of this head: the gradient varies over space and ``ecgmm_crnn_gradcam`` takes its mean per channel itself."""
    from .hip import functional as HF
    _require_crnn(model, "spectrogram_grad_cam")
    _require_cuda(x, "spectrogram_grad_cam input")
    with _Frozen(model):
        with torch.no_grad():
            seq = model._front(x)
        seq = seq.detach().requires_grad_(True)
        logits, steps = model._tail(seq, lengths, x.shape[3])
        (dseq,) = torch.autograd.grad(logits, [seq], grad_outputs=_seed(logits, target))
        frames = None
        if lengths is not None:
            frames = HF.check_lengths(lengths, x.shape[0], x.shape[3]).to(x.device)
            frames = torch.clamp(frames, 1, x.shape[3]).to(torch.int32)
        channels = model.conv3.block[0].weight.shape[0]
        return HF.crnn_grad_cam(seq.detach(), dseq, steps, frames, x.shape[2], x.shape[3], channels)


def overlay(image, cam, alpha=0.5):
    """uint8 [H, W, 3] pictures of one sample: the map on a fixed blue -> red ramp, and blended over the image (a [3,H,W]
    tensor scaled to its own range).  Host-side drawing only."""
    cam = cam.detach().float().cpu().clamp(0, 1)
    img = image.detach().float().cpu()
    lo, hi = img.min(), img.max()
    img = ((img - lo) / (hi - lo if hi > lo else 1.0)).permute(1, 2, 0)
    cold, hot = torch.tensor([0.0, 0.0, 0.6]), torch.tensor([1.0, 0.1, 0.0])
    heat = cold + cam[..., None] * (hot - cold)
    mixed = (1 - alpha * cam[..., None]) * img + alpha * cam[..., None] * heat
    as_u8 = lambda t: (t * 255).round().clamp(0, 255).to(torch.uint8).numpy()
    return as_u8(heat), as_u8(mixed)


def main(config=Config, model_path=None, out_dir="./gradcam", samples=4, output="fusion", quiet=False, model_cls=None):
    """writes gradcam_<i>.png + gradcam_<i>_overlay.png for the first ``samples`` test samples; -> list of file paths.
    ``model_cls``: the model class (default: the paper_modal_balance ``ECGMultimodalModel``).  With the TabNet variant
    (``ecgmm.multimodal.ECGMultimodalModel``) the step masks of the same samples' clinical rows are written too, as
    ``clinical_masks.npz`` (``ClinicalTabNetEncoder.visualize_masks``), the last path of the list."""
    from PIL import Image

    from .dataset import get_dataloaders
    from .multimodal_paper_modal_balance import ECGMultimodalModel
    from .tabnet import ClinicalTabNetEncoder
    device = torch.device(config.device)
    _train_loader, _val_loader, test_loader = get_dataloaders(config)
    model = (model_cls or ECGMultimodalModel)(config).to(device)
    if model_path:
        model.load_state_dict(torch.load(model_path, map_location=device))
    model.eval()
    os.makedirs(out_dir, exist_ok=True)
    written, clin_rows = [], []
    for *batch, _index in test_loader:
        images, ecg_signals, clinical, labels = (t.to(device) for t in batch)
        cam_img, _cam_sig = grad_cam(model, images, ecg_signals, clinical, output=output)
        for b in range(images.shape[0]):
            if len(written) >= 2 * samples:
                break
            i = len(written) // 2
            heat, mixed = overlay(images[b], cam_img[b])
            for name, arr in ((f"gradcam_{i}.png", heat), (f"gradcam_{i}_overlay.png", mixed)):
                path = os.path.join(out_dir, name)
                Image.fromarray(arr).save(path)
                written.append(path)
            clin_rows.append(clinical[b])
            if not quiet:
                print(f"sample {i}: label {int(labels[b])}, map mean {float(cam_img[b].mean()):.3f} -> {written[-1]}")
        if len(written) >= 2 * samples:
            break
    if clin_rows and isinstance(model.clinical_encoder, ClinicalTabNetEncoder):
        model.clinical_encoder.visualize_masks(torch.stack(clin_rows), None, out_dir, "clinical")
        written.append(os.path.join(out_dir, "clinical_masks.npz"))
        if not quiet:
            print(f"clinical step masks of {len(clin_rows)} samples -> {written[-1]}")
    return written


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="Grad-CAM overlays of the ECG picture")
    ap.add_argument("--model", default=None)
    ap.add_argument("--out-dir", default="./gradcam")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--output", default="fusion", choices=sorted(OUTPUTS))
    a = ap.parse_args()
    main(model_path=a.model, out_dir=a.out_dir, samples=a.samples, output=a.output)
