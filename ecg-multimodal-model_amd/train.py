"""Multimodal training entry point (reference: train.py:22-336; ``train_paper_modal_balance`` wraps it for the
paper_modal_balance model).  Like the reference's train.py:14 it builds ``multimodal.ECGMultimodalModel`` (TabNet
clinical branch, widths 512 / 128 / 32) unless another ``model_cls`` is passed.

This module holds the step (``step_loss``, ``run_epoch``), the test metrics (``evaluate``) and the policy values; the epoch
loop, the checkpoint test loop and the metric helpers are ``ecgmm.training``'s.
Reproduces the reference loop: seed 42; encoders frozen by default as train.py:35-40 does (pass
``freeze_encoders=False`` for the end-to-end step of train_kfold.py:42); Adam(lr=Config.lr) on the
trainable parameters; per step zero_grad -> forward -> CE(fusion_logits) + 0.1 * var_loss ->
backward -> step; accuracy from fusion_logits.argmax; validation under no_grad; last/best/epochN.pth
state_dict checkpoints under checkpoints/<MMDD_HHMMSS>/; LR / 10 after 2 non-improving epochs; early
stop after ``Config.patience``; final test with softmax[:, 1], accuracy / F1 / AUC.
The reference's 4-vs-5 tuple unpacking defect (train.py:60 vs dataset.py:74) is not replicated:
loops unpack ``*batch, index``.  TensorBoard is optional (not installed in this image).
"""
import os

import torch

from . import training as T
from .config import Config
from .dataset import get_dataloaders
from .hip import functional as HF
from .multimodal import ECGMultimodalModel      # train.py:14
from .optim import FusedAdam


def _writer(logdir):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(logdir)
    except Exception:
        return None


def step_loss(outputs, labels):
    """train.py:69-78: total = CE(fusion_logits) + 0.1 * var_loss (branch CE terms are computed by the
    reference but not part of total_loss)."""
    return HF.cross_entropy_plus(outputs[3], labels, outputs[4], 0.1)


def run_epoch(model, loader, device, optimizer=None, predictor=None):
    """``predictor`` (optional, validation only): an ``ecgmm.inference.Predictor`` of ``model`` whose weights are current
    (``refresh()`` after training); the forward then runs through the inference plans.  Default: the model's own forward.
    -> (mean loss, mean var_loss, accuracy)."""
    train = optimizer is not None
    if train and predictor is not None:
        raise ValueError("run_epoch: a Predictor has no backward; pass it for validation passes only")
    model.train(train)
    forward = model if predictor is None else predictor

    def step(batch):
        *inputs, _index = batch
        images, ecg, clinical, labels = (t.to(device) for t in inputs)
        outputs = forward(images, ecg, clinical)
        return step_loss(outputs, labels), outputs[3], labels, {"var_loss": outputs[4]}

    loss, acc, extras = T.run_epoch(loader, step, optimizer)
    return loss, extras.get("var_loss", 0.0), acc


def evaluate(model, loader, device, predictor=None):
    """train.py:173-260: softmax[:,1] probabilities, accuracy / F1 / AUC on the test split.
    ``predictor`` (optional): an ``ecgmm.inference.Predictor`` of ``model`` with current weights; default: ``model`` itself."""
    model.eval()
    y_true, y_prob, y_pred = [], [], []
    with torch.no_grad():
        for *batch, _index in loader:
            images, ecg, clinical, labels = (t.to(device) for t in batch)
            logits = (model if predictor is None else predictor)(images, ecg, clinical)[3]
            prob = torch.softmax(logits.float().cpu(), dim=1)   # host-side metrics, as in the reference
            y_true += labels.cpu().tolist()
            y_prob += prob[:, 1].tolist()
            y_pred += prob.argmax(1).tolist()
    return T.binary_metrics(y_true, y_prob, y_pred)


def main(config=Config, freeze_encoders=True, num_epochs=None, quiet=False, model_cls=None, use_predictor=False):
    """``use_predictor``: run the validation and test passes through an ``ecgmm.inference.Predictor`` (BatchNorm-folded
    inference plans), refreshed after every training epoch and after every checkpoint load.  Default off."""
    T.seed_all(config.seed)
    device = torch.device(config.device)
    if not quiet:
        print(f"Using device: {device}")
    model = (model_cls or ECGMultimodalModel)(config).to(device)
    if getattr(config, "synthetic", True):   # synthetic batches carry the clinical width the model expects
        config = type(config.__name__, (config,), {"clinical_input_dim": model.get_clinical_feature_dim()})
    train_loader, val_loader, test_loader = get_dataloaders(config)

    if freeze_encoders:  # train.py:35-40
        for enc in (model.image_encoder, model.signal_encoder, model.clinical_encoder):
            for p in enc.parameters():
                p.requires_grad = False
    optimizer = FusedAdam(filter(lambda p: p.requires_grad, model.parameters()), lr=config.lr)

    ckpt_dir = T.run_dir(config.checkpoint_dir)
    writer = _writer(f"runs/{os.path.basename(ckpt_dir)}")
    predictor = None
    if use_predictor:
        from .inference import Predictor
        predictor = Predictor(model)

    def on_epoch(h, extras):
        if not quiet:
            print(f"[{h['epoch']}] train {h['train_loss']:.4f}/{h['train_acc']:.4f}  val {h['val_loss']:.4f}/{h['val_acc']:.4f}")
        if writer is not None:
            epoch = h["epoch"] - 1
            writer.add_scalar("Loss/Train", h["train_loss"], epoch)
            writer.add_scalar("Loss/Val", h["val_loss"], epoch)
            writer.add_scalar("VarLoss/Val", extras["var_loss"], epoch)
            writer.add_scalar("Accuracy/Train", h["train_acc"], epoch)
            writer.add_scalar("Accuracy/Val", h["val_acc"], epoch)
            w = torch.softmax(model.attention_fusion.weights.detach().float().cpu(), 0)
            for name, v in zip(("Image", "Signal", "Clinical"), w.tolist()):
                writer.add_scalar(f"AttentionWeights/{name}", v, epoch)

    def one_pass(loader, **kw):
        loss, var, acc = run_epoch(model, loader, device, **kw)
        return loss, acc, {"var_loss": var}

    # train.py:145-151: epochN.pth and best.pth only on improvement; :157-163: manual LR / 10 after 2 non-improving epochs
    history = T.fit(model, optimizer, lambda: one_pass(train_loader, optimizer=optimizer),
                    lambda: one_pass(val_loader, predictor=predictor), ckpt_dir, num_epochs or config.num_epochs,
                    patience=config.patience, lr_decay_after=2, best_names=("epoch{epoch}.pth", "best.pth"),
                    predictor=predictor, on_epoch=on_epoch)
    # (best.pth is missing when no epoch improved on inf: that raises here, as it always did)
    results = T.test_checkpoints(model, ckpt_dir, ("best", "last"), lambda: evaluate(model, test_loader, device, predictor),
                                 predictor, skip_missing=False)
    if not quiet:
        for tag, res in results.items():
            print(f"test[{tag}]: {res}")
    if writer is not None:
        writer.close()
    return history, results, ckpt_dir


if __name__ == "__main__":
    main()
