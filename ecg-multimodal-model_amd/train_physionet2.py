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
reader and label table, which this module reuses; the loader base, the epoch loop and the metrics are ``ecgmm.training``'s.  NEW: ``config.physionet2_max_len`` (default ``None``) truncates longer
records at the end before the transform.  NEW: ``main(use_lengths=True)`` / ``config.physionet2_use_lengths`` hands each
record's own frame count to ``CRNN.forward(x, lengths)``, so the BiLSTM stops where the record does and the mean over time
leaves the padding out; each batch's rows are then ordered by length (:class:`DeviceSpectrogramLoader`).  Off by default:
the reference runs through the padding.  NEW: ``main(saliency_samples=k)`` / ``config.physionet2_saliency_samples`` writes the
input gradients and the Grad-CAM maps of the first ``k`` test spectrograms beside the checkpoints (off by default).
NEW: ``main(use_predictor=True)`` / ``config.physionet2_use_predictor`` runs the validation and test passes through
``ecgmm.inference.Predictor`` (the front end's BatchNorm-folded inference plan) instead of the training plan's eval mode
(off by default).
"""
import numpy as np
import torch

from . import training as T
from .config import Config
from .crnn import CRNN, FocalLoss
from .optim import FusedAdam
from .spectrogram import NPERSEG, compute_log_spectrogram, stft_frames
from .train_physionet import LABEL_MAP, SPLIT, load_records, pad_sequences, read_labels  # noqa: F401 -- the record reader
from .training import split_indices


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


def spectrogram_frames(signals):
    """``stft_frames(len(record))`` per record, int64 (host): the frames of :func:`build_spectrograms`' rows that are the
    record's own; those behind them are the transform of the zero padding."""
    return np.asarray([stft_frames(len(s)) for s in signals], dtype=np.int64)


class SpectrogramDataset:
    """One split as an index set over the shared spectrogram tensor (train_physionet2.py:41-48, 163-165 copy the rows).
    ``frames`` (optional): the valid frames of every row of ``spectrograms``, as :func:`spectrogram_frames` gives them."""

    def __init__(self, indices, labels, spectrograms, frames=None):
        device = spectrograms.device
        self.spectrograms = spectrograms
        self.frames_host = self.frames = None
        if frames is not None:
            frames = np.asarray(frames)
            if frames.shape != (spectrograms.shape[0],) or frames.dtype.kind not in "iu":
                raise ValueError(f"SpectrogramDataset: frames must be {spectrograms.shape[0]} integers, one per spectrogram")
            if frames.min() < 1 or frames.max() > spectrograms.shape[-1]:
                raise ValueError(f"SpectrogramDataset: frames outside 1..{spectrograms.shape[-1]}")
            self.frames_host = torch.as_tensor(frames[np.asarray(indices)], dtype=torch.int32)   # per split row, as labels
            self.frames = self.frames_host.to(device)
        self.indices = torch.as_tensor(np.asarray(indices), dtype=torch.long, device=device)
        self.labels_host = torch.as_tensor(np.asarray(labels)[np.asarray(indices)], dtype=torch.long)
        self.labels = self.labels_host.to(device)

    def __len__(self):
        return self.labels_host.numel()

    def __getitem__(self, idx):
        return self.spectrograms[self.indices[idx]], self.labels[idx]


class DeviceSpectrogramLoader(T.ResidentLoader):
    """Batches of a :class:`SpectrogramDataset`: ``(spectrograms [B, 1, 33, T] fp32, labels [B])``, both on the device.
    ``shuffle``: a ``torch.randperm`` of the seeded ``generator`` per epoch, kept in ``last_order``.  The last partial batch
    is kept (``DataLoader``'s default, which the reference uses).

    A dataset with ``frames`` yields ``((spectrograms, frames [B] int32), labels)``.  ``sort_by_length`` (default: on exactly
    then) orders the rows of each batch by descending frames, a stable sort of the batch's index slice: the batches hold the
    rows they would hold anyway, and the LSTM's slices of 16 consecutive rows become homogeneous in length, so that the short
    slices leave their CUs early.  That saves CU time, not latency: a layer lasts as long as the batch's longest slice, and
    at B = 256 no time was gained.  Without frames the batches are as before."""

    def __init__(self, dataset, batch_size=Config.batch_size, shuffle=False, generator=None, sort_by_length=None):
        super().__init__(dataset, batch_size, shuffle, generator)
        has = getattr(dataset, "frames", None) is not None
        if sort_by_length and not has:
            raise ValueError("DeviceSpectrogramLoader: sort_by_length needs a dataset with frames")
        self.sort_by_length = has if sort_by_length is None else bool(sort_by_length)

    def batch(self, idx):
        ds = self.dataset
        if getattr(ds, "frames", None) is None:
            return ds.spectrograms.index_select(0, ds.indices[idx]), ds.labels[idx]
        if self.sort_by_length:
            idx = idx[torch.sort(ds.frames[idx], descending=True, stable=True).indices]
        return (ds.spectrograms.index_select(0, ds.indices[idx]), ds.frames[idx]), ds.labels[idx]


def get_spectrogram_dataloaders(config=Config, batch_size=None, label_map=LABEL_MAP, split=SPLIT, chunk=1024,
                                use_lengths=False, target_fs=None):
    """train / val / test :class:`DeviceSpectrogramLoader` over one resident tensor (train_physionet2.py:128-165): labels
    N -> 0, AF / O -> 1, '~' dropped; stratified 80 / 10 / 10 with ``config.seed``; only the train split is shuffled.
    ``use_lengths``: the datasets carry :func:`spectrogram_frames` and the loaders yield ``((spec, frames), labels)``.
    ``target_fs`` (or ``config.physionet_target_fs``): ``train_physionet.load_records``."""
    batch_size = config.batch_size if batch_size is None else batch_size
    target_fs = target_fs if target_fs is not None else getattr(config, "physionet_target_fs", None)
    signals, labels = load_records(config, label_map, **({} if target_fs is None else {"target_fs": target_fs}))
    max_len = getattr(config, "physionet2_max_len", None)
    if max_len is not None:
        signals = [s[:max_len] for s in signals]
    train_idx, val_idx, test_idx = split_indices(labels, config.seed, split)
    spec = build_spectrograms(signals, torch.device(config.device), chunk)
    gen = torch.Generator().manual_seed(config.seed)
    frames = spectrogram_frames(signals) if use_lengths else None
    return (DeviceSpectrogramLoader(SpectrogramDataset(train_idx, labels, spec, frames), batch_size, shuffle=True,
                                    generator=gen),
            DeviceSpectrogramLoader(SpectrogramDataset(val_idx, labels, spec, frames), batch_size),
            DeviceSpectrogramLoader(SpectrogramDataset(test_idx, labels, spec, frames), batch_size))


def predict_split(model, loader, predictor=None):
    """-> (labels [n], softmax probabilities [n, 2], argmax predictions [n]) of the split, numpy, from the model's eval
    forward or, with ``predictor`` (an ``ecgmm.inference.Predictor`` of ``model``), from its inference plan."""
    model.eval()
    forward = model if predictor is None else predictor
    # a loader with frames yields (spec, frames) as the inputs
    y_true, y_prob, y_pred, _ = T.predict(lambda inputs: forward(*inputs) if isinstance(inputs, tuple) else forward(inputs), loader)
    return y_true, y_prob, y_pred


def evaluate(model, loader, predictor=None):
    """train_physionet2.py:233-257: argmax predictions and the class-1 softmax probability of the split ->
    accuracy / binary F1 / ROC-AUC (NaN where sklearn cannot define it: one class only)."""
    y_true, y_prob, y_pred = predict_split(model, loader, predictor)
    return T.binary_metrics(y_true, y_prob[:, 1], y_pred)


def main(config=Config, num_epochs=None, batch_size=None, quiet=False, use_lengths=False, saliency_samples=0,
         use_predictor=False, lstm_dtype=None):
    """-> (history, {"best": metrics, "last": metrics}, checkpoint directory).  ``use_lengths`` or
    ``config.physionet2_use_lengths`` (both off by default): the CRNN gets every record's own length (module docstring).
    ``saliency_samples=k`` > 0 (or ``config.physionet2_saliency_samples``): after the test pass, with the weights it ended
    on, ``spectrogram_saliency.npz`` is written into the run directory for the first ``k`` test records
    (:func:`write_spectrogram_saliency`).  The default 0 writes nothing.
    ``use_predictor`` or ``config.physionet2_use_predictor`` (both off by default): the validation and test passes run
    through an ``ecgmm.inference.Predictor`` (BatchNorm-folded inference plan of the front end, no saves), refreshed after
    every training epoch and after every checkpoint load; the saliency dump keeps the model's own forward, which is what
    a backward needs.
    ``lstm_dtype`` (``None``: ``config.physionet2_lstm_dtype``, default ``"fp32"``): ``"bf16"`` runs the BiLSTM's recurrent
    products on bf16 operands (``CRNN(lstm_dtype=...)``), in training, evaluation and the predictor alike."""
    lstm_dtype = lstm_dtype or getattr(config, "physionet2_lstm_dtype", "fp32")
    use_lengths = bool(use_lengths or getattr(config, "physionet2_use_lengths", False))
    use_predictor = bool(use_predictor or getattr(config, "physionet2_use_predictor", False))
    saliency_samples = int(saliency_samples or getattr(config, "physionet2_saliency_samples", 0) or 0)
    if saliency_samples < 0:
        raise ValueError(f"saliency_samples={saliency_samples} must be >= 0")
    num_epochs = config.num_epochs if num_epochs is None else num_epochs
    batch_size = config.batch_size if batch_size is None else batch_size
    T.seed_all(config.seed, numpy=True)
    device = torch.device(config.device)
    if not quiet:
        print(f"Using device: {device}")
    train_loader, val_loader, test_loader = get_spectrogram_dataloaders(config, batch_size, use_lengths=use_lengths)
    model = CRNN(compute_dtype=getattr(config, "compute_dtype", "bf16"), lstm_dtype=lstm_dtype).to(device)
    criterion = FocalLoss()
    optimizer = FusedAdam(model.parameters(), lr=config.lr)
    ckpt_dir = T.run_dir(config.checkpoint_dir)

    predictor = None
    if use_predictor:
        from .inference import Predictor
        predictor = Predictor(model)

    def step(batch, forward=model):
        spec, labels = batch
        out = forward(*spec) if use_lengths else forward(spec)
        return criterion(out, labels), out, labels

    def train_pass():
        model.train()
        return T.run_epoch(train_loader, step, optimizer)

    def val_pass():
        model.eval()
        return T.run_epoch(val_loader, step if predictor is None else lambda batch: step(batch, predictor))

    def on_epoch(h, _extras):
        if not quiet:
            print(f"[{h['epoch']}] train {h['train_loss']:.4f}/{h['train_acc']:.4f}  val {h['val_loss']:.4f}/{h['val_acc']:.4f}")

    # train_physionet2.py:220-222: best.pth on a lower validation loss; no scheduler, no early stop
    history = T.fit(model, optimizer, train_pass, val_pass, ckpt_dir, num_epochs, predictor=predictor, on_epoch=on_epoch)
    results = T.test_checkpoints(model, ckpt_dir, ("best", "last"),
                                 lambda: evaluate(model, test_loader, predictor=predictor), predictor)
    if not quiet:
        for tag, res in results.items():
            print(f"test[{tag}]: {res}")
    if saliency_samples:
        path = write_spectrogram_saliency(model, test_loader.dataset, saliency_samples, ckpt_dir)
        if not quiet:
            print(f"spectrogram saliency of the first test records -> {path}")
    return history, results, ckpt_dir


def write_spectrogram_saliency(model, dataset, k, out_dir):
    """``spectrogram_saliency.npz`` in ``out_dir`` for the first ``k`` records of ``dataset`` (a
    :class:`SpectrogramDataset`): ``grad_cam`` [k, F, T] and ``gradients`` [k, F, T] of the predicted class
    (``ecgmm.explain.spectrogram_grad_cam`` / ``spectrogram_gradients``), ``frames`` [k] (T without frames in the dataset),
    ``labels`` [k], ``probs`` [k, 2] -> the file's path"""
    import os

    from .explain import spectrogram_grad_cam, spectrogram_gradients
    k = min(int(k), len(dataset))
    x = dataset.spectrograms.index_select(0, dataset.indices[:k])
    frames = None if dataset.frames is None else dataset.frames[:k]
    was_training = model.training
    model.eval()
    with torch.no_grad():
        logits = model(x) if frames is None else model(x, frames)
    model.train(was_training)
    target = logits.argmax(dim=1)       # one class for both maps
    cam = spectrogram_grad_cam(model, x, frames, target)
    grads = spectrogram_gradients(model, x, frames, target)
    path = os.path.join(out_dir, "spectrogram_saliency.npz")
    np.savez(path, grad_cam=cam.cpu().numpy(), gradients=grads[:, 0].cpu().numpy(),
             frames=(np.full(k, x.shape[3], dtype=np.int32) if frames is None else dataset.frames_host[:k].numpy()),
             labels=dataset.labels_host[:k].numpy(), probs=torch.softmax(logits.float(), dim=1).cpu().numpy())
    return path


if __name__ == "__main__":
    main()
