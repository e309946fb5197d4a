"""What every trainer of this package shares on the host: the device-resident loader base, one pass over a loader, the
epoch loop with its checkpoint / patience / LR policy, the checkpoint test loop and the metrics.  A trainer module keeps
what is its own: data, model, loss, the policy values and the reference citations that justify them.

Nothing here launches a kernel or imports the HIP library; ``sklearn`` is imported by the functions that need it.
"""
import os
import time

import numpy as np
import torch


# --------------------------------------------------------------------------------------------
# small helpers
# --------------------------------------------------------------------------------------------
def seed_all(seed, numpy=False):
    """Seed torch, the Philox stream of ``ecgmm.hip.functional`` and, where the trainer's reference does, numpy."""
    from .hip import functional as HF
    torch.manual_seed(seed)
    if numpy:
        np.random.seed(seed)
    HF.manual_seed(seed)


def run_dir(*parts):
    """``os.path.join(*parts, <MMDD_HHMMSS>)``, created."""
    path = os.path.join(*parts, time.strftime("%m%d_%H%M%S"))
    os.makedirs(path, exist_ok=True)
    return path


def split_indices(labels, seed=42, split=(0.2, 0.5)):
    """Stratified train / val / test indices: ``train_test_split(test_size=split[0])`` then the held-out part split again
    with ``test_size=split[1]``, both seeded with ``seed`` (train_physionet.py:112-118)."""
    from sklearn.model_selection import train_test_split
    labels = np.asarray(labels)
    idx = np.arange(len(labels))
    train_idx, temp_idx, _, temp_y = train_test_split(idx, labels, test_size=split[0], stratify=labels, random_state=seed)
    val_idx, test_idx = train_test_split(temp_idx, test_size=split[1], stratify=temp_y, random_state=seed)
    return train_idx, val_idx, test_idx


# --------------------------------------------------------------------------------------------
# loader over a dataset that is resident on the device
# --------------------------------------------------------------------------------------------
class ResidentLoader:
    """Batches of a dataset whose tensors already live on the device (``dataset.labels`` says which).  One draw per epoch:
    ``sampler.sample()`` (device indices, ``len(sampler)`` of them), a ``torch.randperm`` of the seeded ``generator`` when
    ``shuffle``, else ``arange``.  The order is kept in ``last_order`` (host), uploaded once and sliced per batch; the
    indices are in range by construction, so nothing checks them per batch.  A subclass implements ``batch(idx)``."""

    def __init__(self, dataset, batch_size, shuffle=False, generator=None, drop_last=False, sampler=None):
        if sampler is not None and shuffle:
            raise ValueError(f"{type(self).__name__}: sampler and shuffle are mutually exclusive")   # as torch's DataLoader
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.generator, self.sampler = generator, sampler
        self.last_order = None

    def __len__(self):
        n, b = len(self.dataset if self.sampler is None else self.sampler), self.batch_size
        return n // b if self.drop_last else (n + b - 1) // b

    def __iter__(self):
        if self.sampler is not None:
            order_dev = self.sampler.sample()
            self.last_order = order_dev.cpu()
        else:
            n = len(self.dataset)
            self.last_order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
            order_dev = self.last_order.to(self.dataset.labels.device)
        for k in range(len(self)):
            yield self.batch(order_dev[k * self.batch_size:(k + 1) * self.batch_size])

    def batch(self, idx):
        """device index vector -> the batch the loader yields"""
        raise NotImplementedError


# --------------------------------------------------------------------------------------------
# one pass, the epoch loop, the checkpoint test loop
# --------------------------------------------------------------------------------------------
def run_epoch(loader, step, optimizer=None, scheduler=None, count_correct=True):
    """One pass over ``loader``.  ``step(batch) -> (loss, logits, labels[, {name: 0-dim tensor}])`` does everything between
    the batch and the loss.  With an ``optimizer`` every batch runs zero_grad -> step -> backward -> optimizer.step() ->
    scheduler.step(); without one the pass runs under ``torch.no_grad()``.  The caller sets the model's mode.
    -> (mean loss per batch, accuracy or ``None`` without ``count_correct``, {name: mean per batch})."""
    train = optimizer is not None
    tot, correct, n, extras = 0.0, 0, 0, {}
    with torch.enable_grad() if train else torch.no_grad():
        for batch in loader:
            if train:
                optimizer.zero_grad()
            loss, logits, labels, *more = step(batch)
            if train:
                loss.backward()
                optimizer.step()
                if scheduler is not None:
                    scheduler.step()
            tot += loss.item()
            for name, value in (more[0] if more else {}).items():
                extras[name] = extras.get(name, 0.0) + value.item()
            if count_correct:
                correct += logits.argmax(1).eq(labels).sum().item()
                n += labels.size(0)
    k = max(len(loader), 1)
    return tot / k, correct / max(n, 1) if count_correct else None, {name: v / k for name, v in extras.items()}


def fit(model, optimizer, train_pass, val_pass, ckpt_dir, num_epochs, patience=None, lr_decay_after=None,
        save_last="last.pth", best_names=("best.pth",), predictor=None, on_epoch=None):
    """The epoch loop.  ``train_pass()`` and ``val_pass()`` return what :func:`run_epoch` returns; ``predictor`` (an
    ``ecgmm.inference.Predictor`` of ``model``) is refreshed between the two, since the optimizer writes the weights through
    raw pointers and nothing else can tell.  Each epoch appends ``{epoch, train_loss, train_acc, val_loss, val_acc}`` (1-based
    epoch; an accuracy that is ``None`` is left out) to the history and calls ``on_epoch(record, extras of val_pass)``.

    ``save_last`` is written every epoch; every name of ``best_names``, formatted with ``epoch``, when the validation loss
    is strictly below the best so far (starting from inf, so a NaN loss never writes one).  After ``lr_decay_after``
    non-improving epochs in a row every param group's lr is divided by 10 and that count starts again; after ``patience``
    non-improving epochs in a row the loop stops.  -> history."""
    save = lambda name: torch.save(model.state_dict(), os.path.join(ckpt_dir, name))
    best, misses, since_decay, history = float("inf"), 0, 0, []
    for epoch in range(1, num_epochs + 1):
        train_loss, train_acc, _ = train_pass()
        if predictor is not None:
            predictor.refresh()
        val_loss, val_acc, extras = val_pass()
        record = dict(epoch=epoch, train_loss=train_loss, train_acc=train_acc, val_loss=val_loss, val_acc=val_acc)
        record = {k: v for k, v in record.items() if v is not None}
        history.append(record)
        if on_epoch is not None:
            on_epoch(record, extras)
        if save_last is not None:
            save(save_last)
        if val_loss < best:
            best, misses, since_decay = val_loss, 0, 0
            for name in best_names:
                save(name.format(epoch=epoch))
        else:
            misses += 1
            since_decay += 1
            if lr_decay_after is not None and since_decay >= lr_decay_after:
                for g in optimizer.param_groups:
                    g["lr"] /= 10
                since_decay = 0
            if patience is not None and misses >= patience:
                break
    return history


def test_checkpoints(model, ckpt_dir, tags, evaluate, predictor=None, skip_missing=True):
    """``{tag: evaluate()}`` with ``{tag}.pth`` of ``ckpt_dir`` loaded into ``model`` (and ``predictor`` refreshed) first.
    A missing file -- no epoch improved on inf, i.e. a NaN validation loss -- is skipped, or raises without ``skip_missing``."""
    device = next(model.parameters()).device
    results = {}
    for tag in tags:
        path = os.path.join(ckpt_dir, f"{tag}.pth")
        if skip_missing and not os.path.exists(path):
            continue
        model.load_state_dict(torch.load(path, map_location=device))
        if predictor is not None:
            predictor.refresh()
        results[tag] = evaluate()
    return results


# --------------------------------------------------------------------------------------------
# metrics
# --------------------------------------------------------------------------------------------
def auc_or_nan(y_true, score, **kw):
    """``roc_auc_score``, NaN where sklearn cannot define it (one class only, NaN scores)."""
    from sklearn.metrics import roc_auc_score
    try:
        return float(roc_auc_score(y_true, score, **kw))
    except ValueError:
        return float("nan")


def binary_metrics(y_true, y_prob, y_pred):
    """labels, class-1 probabilities, predictions -> ``{"accuracy", "f1", "auc"}``"""
    from sklearn.metrics import f1_score
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    return {"accuracy": float((y_true == y_pred).mean()), "f1": float(f1_score(y_true, y_pred, zero_division=0)),
            "auc": auc_or_nan(y_true, y_prob)}


def predict(forward, loader, prepare=None, criterion=None):
    """``forward`` over a loader of ``(inputs, labels)`` batches under ``torch.no_grad()``; ``prepare(inputs)`` shapes the
    inputs first.  The softmax and the argmax of the logits are taken on the device.  The caller sets the model's mode.
    -> (labels [n], probabilities [n, classes] fp32, argmax of the logits [n], mean batch loss or ``None``), numpy."""
    y_true, y_prob, y_pred, loss = [], [], [], 0.0
    with torch.no_grad():
        for inputs, labels in loader:
            logits = forward(inputs if prepare is None else prepare(inputs))
            if criterion is not None:
                loss += criterion(logits, labels).item()
            y_prob.append(torch.softmax(logits.float(), dim=1).cpu().numpy())
            y_pred.append(logits.argmax(1))          # stays on the device: one copy after the loop
            y_true.append(labels.cpu().numpy())
    return (np.concatenate(y_true), np.concatenate(y_prob), torch.cat(y_pred).cpu().numpy(),
            loss / max(len(loader), 1) if criterion is not None else None)
