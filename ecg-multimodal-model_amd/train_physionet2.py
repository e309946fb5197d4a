"""PhysioNet-2017 spectrogram CRNN trainer, N vs AF/O (reference: train_physionet2.py:30-34, 124-261).

The reference runs ``scipy.signal.stft`` per record on the CPU, zero-pads every log-spectrogram along time to the longest
one, stacks ``[N, 1, 33, max_time]`` on the host and splits that 80 / 10 / 10.  Here the records are padded to the longest
one on the host and transformed on the device in chunks (:func:`build_spectrograms`, one ``log_spectrogram`` launch per
chunk) into ONE resident tensor; the STFT of a zero-padded record is the record's own STFT followed by exact zeros, so this
is the same array.  A split is an index set over that tensor.  Model, loss and optimizer are the reference's: ``CRNN()``,
``FocalLoss()``, Adam(``Config.lr``) without a scheduler, ``Config.batch_size``, ``Config.num_epochs``, no augmentation;
``last.pth`` every epoch, ``best.pth`` on a better validation loss; the test split is scored with argmax predictions and
the class-1 softmax probability.

Not carried over: the plots and the classification report.  The validation loader is not shuffled (the reference's
``shuffle=True`` at :164 changes nothing it reports: it only permutes the rows the validation loss and accuracy are
accumulated over).  ``wfdb`` / ``pandas`` are replaced by :mod:`ecgmm.train_physionet`'s record
reader and label table, which this module reuses.  NEW: ``config.physionet2_max_len`` (default ``None``) truncates longer
records at the end before the transform.
"""
import os
import time

import numpy as np
import torch

from .config import Config
from .crnn import CRNN, FocalLoss
from .hip import functional as HF
from .optim import FusedAdam
from .spectrogram import NPERSEG, compute_log_spectrogram, stft_frames
from .train_physionet import LABEL_MAP, SPLIT, load_records, pad_sequences, read_labels, split_indices  # noqa: F401


def build_spectrograms(signals, device, chunk=1024):
    """Variable-length 1-D records -> the resident ``[N, 1, 33, T(Lmax)]`` fp32 log-spectrogram tensor on ``device``
    (train_physionet2.py:134-155).  The records are zero-padded to the longest one on the host, ``chunk`` records at a time,
    uploaded and transformed; the padded raw array is never resident as a whole."""
    if len(signals) < 1:
        raise ValueError("build_spectrograms: no records")
    lengths = [len(s) for s in signals]
    if min(lengths) < NPERSEG:
        raise ValueError(f"build_spectrograms: record {int(np.argmin(lengths))} has {min(lengths)} samples, fewer than "
                         f"nperseg={NPERSEG}; scipy would shrink the segment for it (another number of bins) or raise")
    lmax, chunk = max(lengths), max(int(chunk), 1)
    out = torch.empty(len(signals), 1, NPERSEG // 2 + 1, stft_frames(lmax), dtype=torch.float32, device=device)
    for i in range(0, len(signals), chunk):
        raw = pad_sequences(signals[i:i + chunk], maxlen=lmax, dtype="float32", padding="post", truncating="post")
        out[i:i + chunk, 0] = compute_log_spectrogram(torch.from_numpy(raw).to(device))
    return out


class SpectrogramDataset:
    """One split as an index set over the shared spectrogram tensor (train_physionet2.py:41-48, 163-165 copy the rows)."""

    def __init__(self, indices, labels, spectrograms):
        device = spectrograms.device
        self.spectrograms = spectrograms
        self.indices = torch.as_tensor(np.asarray(indices), dtype=torch.long, device=device)
        self.labels_host = torch.as_tensor(np.asarray(labels)[np.asarray(indices)], dtype=torch.long)
        self.labels = self.labels_host.to(device)

    def __len__(self):
        return self.labels_host.numel()

    def __getitem__(self, idx):
        return self.spectrograms[self.indices[idx]], self.labels[idx]


class DeviceSpectrogramLoader:
    """Batches of a :class:`SpectrogramDataset`: ``(spectrograms [B, 1, 33, T] fp32, labels [B])``, both on the device.
    ``shuffle``: a ``torch.randperm`` of the seeded ``generator`` per epoch, kept in ``last_order``.  The last partial batch
    is kept (``DataLoader``'s default, which the reference uses)."""

    def __init__(self, dataset, batch_size=Config.batch_size, shuffle=False, generator=None):
        self.dataset, self.batch_size, self.shuffle, self.generator = dataset, int(batch_size), shuffle, generator
        self.last_order = None

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds, n = self.dataset, len(self.dataset)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        self.last_order = order
        order_dev = order.to(ds.indices.device)
        for k in range(len(self)):
            idx = order_dev[k * self.batch_size:(k + 1) * self.batch_size]
            yield ds.spectrograms.index_select(0, ds.indices[idx]), ds.labels[idx]


def get_spectrogram_dataloaders(config=Config, batch_size=None, label_map=LABEL_MAP, split=SPLIT, chunk=1024):
    """train / val / test :class:`DeviceSpectrogramLoader` over one resident tensor (train_physionet2.py:128-165): labels
    N -> 0, AF / O -> 1, '~' dropped; stratified 80 / 10 / 10 with ``config.seed``; only the train split is shuffled."""
    batch_size = config.batch_size if batch_size is None else batch_size
    signals, labels = load_records(config, label_map)
    max_len = getattr(config, "physionet2_max_len", None)
    if max_len is not None:
        signals = [s[:max_len] for s in signals]
    train_idx, val_idx, test_idx = split_indices(labels, config.seed, split)
    spec = build_spectrograms(signals, torch.device(config.device), chunk)
    gen = torch.Generator().manual_seed(config.seed)
    return (DeviceSpectrogramLoader(SpectrogramDataset(train_idx, labels, spec), batch_size, shuffle=True, generator=gen),
            DeviceSpectrogramLoader(SpectrogramDataset(val_idx, labels, spec), batch_size),
            DeviceSpectrogramLoader(SpectrogramDataset(test_idx, labels, spec), batch_size))


def evaluate(model, loader):
    """train_physionet2.py:233-257: argmax predictions and the class-1 softmax probability of the split ->
    accuracy / binary F1 / ROC-AUC (NaN where sklearn cannot define it: one class only)."""
    from sklearn.metrics import f1_score, roc_auc_score
    model.eval()
    y_true, y_pred, y_prob = [], [], []
    with torch.no_grad():
        for spec, labels in loader:
            logits = model(spec).float()
            y_prob.append(torch.softmax(logits, dim=1)[:, 1].cpu().numpy())
            y_pred.append(logits.argmax(1).cpu().numpy())
            y_true.append(labels.cpu().numpy())
    y_true, y_pred, y_prob = np.concatenate(y_true), np.concatenate(y_pred), np.concatenate(y_prob)
    try:
        auc = float(roc_auc_score(y_true, y_prob))
    except ValueError:
        auc = float("nan")
    return {"accuracy": float((y_true == y_pred).mean()), "f1": float(f1_score(y_true, y_pred, zero_division=0)), "auc": auc}


def main(config=Config, num_epochs=None, batch_size=None, quiet=False):
    """-> (history, {"best": metrics, "last": metrics}, checkpoint directory)."""
    num_epochs = config.num_epochs if num_epochs is None else num_epochs
    batch_size = config.batch_size if batch_size is None else batch_size
    torch.manual_seed(config.seed)
    np.random.seed(config.seed)
    HF.manual_seed(config.seed)
    device = torch.device(config.device)
    if not quiet:
        print(f"Using device: {device}")
    train_loader, val_loader, test_loader = get_spectrogram_dataloaders(config, batch_size)
    model = CRNN(compute_dtype=getattr(config, "compute_dtype", "bf16")).to(device)
    criterion = FocalLoss()
    optimizer = FusedAdam(model.parameters(), lr=config.lr)
    ckpt_dir = os.path.join(config.checkpoint_dir, time.strftime("%m%d_%H%M%S"))
    os.makedirs(ckpt_dir, exist_ok=True)
    min_val, history = float("inf"), []
    for epoch in range(num_epochs):
        model.train()
        tl, correct, total = 0.0, 0, 0
        for spec, labels in train_loader:
            optimizer.zero_grad()
            out = model(spec)
            loss = criterion(out, labels)
            loss.backward()
            optimizer.step()
            tl += loss.item()
            correct += out.argmax(1).eq(labels).sum().item()
            total += labels.size(0)
        torch.save(model.state_dict(), os.path.join(ckpt_dir, "last.pth"))
        model.eval()
        vl, vc, vt = 0.0, 0, 0
        with torch.no_grad():
            for spec, labels in val_loader:
                out = model(spec)
                vl += criterion(out, labels).item()
                vc += out.argmax(1).eq(labels).sum().item()
                vt += labels.size(0)
        avg = vl / max(len(val_loader), 1)
        history.append(dict(epoch=epoch + 1, train_loss=tl / max(len(train_loader), 1), train_acc=correct / max(total, 1),
                            val_loss=avg, val_acc=vc / max(vt, 1)))
        if not quiet:
            h = history[-1]
            print(f"[{epoch + 1}] train {h['train_loss']:.4f}/{h['train_acc']:.4f}  val {avg:.4f}/{h['val_acc']:.4f}")
        if avg < min_val:   # train_physionet2.py:220-222
            min_val = avg
            torch.save(model.state_dict(), os.path.join(ckpt_dir, "best.pth"))
    results = {}
    for tag in ("best", "last"):
        path = os.path.join(ckpt_dir, f"{tag}.pth")
        if not os.path.exists(path):   # no epoch improved on inf (a NaN validation loss): nothing was saved as best
            continue
        model.load_state_dict(torch.load(path, map_location=device))
        results[tag] = evaluate(model, test_loader)
        if not quiet:
            print(f"test[{tag}]: {results[tag]}")
    return history, results, ckpt_dir


if __name__ == "__main__":
    main()
