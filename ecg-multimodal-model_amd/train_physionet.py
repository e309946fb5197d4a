"""PhysioNet-2017 single-lead trainer, N vs AF/O (reference: train_physionet.py:22-132, 267-451).

The reference filters every sample again at every ``__getitem__`` on the CPU (4th-order Butterworth band-pass ``filtfilt``
-> z-score -> random augmentation).  Here each split is padded on the host, uploaded once and pre-processed once by ONE
``filter_zscore`` launch (the result is a pure function of the record, so caching it changes nothing); per batch one
``gather_augment`` launch gathers the rows and applies ``augment_signal`` on the device.  The model, loss, optimizer and
schedule are the reference's: ``ResNet1D_SE`` on ``[B, 1, 3000]``, ``FocalLoss(1, 2)``, Adam(1e-3), OneCycleLR per batch.
``main(model="transformer")`` trains the reference's one-line alternative instead (train_physionet.py:276),
:class:`ECGTransformer1D` on the native attention kernels; ``time_attention=True`` lets it attend along each record's
positions instead of across the batch, and ``use_lengths=True`` then hands it every record's own length, so that the zero
padding of a short record is neither attended to nor averaged.

This module holds the model alternative, the device pre-processing, the record reader, the resident dataset and loader and
the policy values; the epoch loop, the checkpoint test loop and the metrics are ``ecgmm.training``'s, the gather launch is
``ecgmm.preprocess.gather_augment``.

``resample_signal`` (train_physionet.py:35-39) is :func:`resample_signal` on the device (``ecgmm.preprocess.resample``,
csrc/resample.hip); the reference's three steps for unequal rates are :func:`preprocess_resampled`, and
``load_records(target_fs=...)`` moves every record whose header names another sampling rate to ``target_fs`` before it is
padded.  Not carried over: plots.  ``wfdb`` is replaced by :func:`read_record`, ``keras`` by :func:`pad_sequences`.
"""
import csv
import os
import re

import numpy as np
import torch

from . import preprocess as PP
from . import training as T
from .config import Config
from .hip import functional as HF
from .hip import nn as HN
from .hip.functional import _require_cuda
from .optim import FusedAdam
from .preprocess import gather_augment   # noqa: F401 -- its home is ecgmm.preprocess; this name is part of this module
from .signal_model import FocalLoss, ResNet1D_SE
from .training import split_indices      # noqa: F401 -- train_physionet.py:112-118; shared with the other PhysioNet / PTB-XL trainers

LABEL_MAP = {"N": 0, "AF": 1, "O": 1}      # train_physionet.py:93 ('~' records are dropped at :92)
MAX_LEN = 3000
# train_physionet.py:113-118: 80 % train, the remaining 20 % halved into validation and test
SPLIT = (0.2, 0.5)
AUG_DEFAULTS = dict(p=0.5, sigma=0.01, scale=(0.8, 1.2), shift=(-10, 10))   # train_physionet.py:47-58


# --------------------------------------------------------------------------------------------
# the Transformer alternative                               reference: train_physionet.py:211-240, 276
# --------------------------------------------------------------------------------------------
class ECGTransformer1D(torch.nn.Module):
    """``ECGTransformer1D`` of the reference with its attribute names, shapes and initialisation, so ``state_dict``s move in
    both directions: Conv1d(input_dim, d_model, 3, padding=1) + ``pos_embedding`` (one launch, ``HF.embed1d``) -> a post-norm
    ``TransformerEncoder`` -> mean over the positions -> Linear-ReLU-Dropout-Linear.

    The reference builds its encoder layers with torch's default ``batch_first=False`` and feeds them ``[B, L, d_model]``
    (:219, :236), so attention runs ACROSS THE BATCH: the sequence is the B samples of the batch and each of the L positions
    is an independent attention "batch" element.  A sample's logits therefore depend on the other samples of its batch, in
    eval mode too.  That is reproduced here as it is, not corrected: it is the default.

    ``time_attention=True`` builds the layers with ``batch_first=True`` instead, the reference's own intended design
    (multimodal_paper_modal_balance.py:133-140): every sample attends along its own L positions and its logits depend on
    nothing else in the batch.  Parameter names and shapes are the same in both modes, so checkpoints move between them.
    Only then does ``forward(x, lengths=...)`` make sense: one length per sample (``HF.check_lengths``), the positions behind
    it are never keys and do not enter the mean over the positions, and the padded samples of ``x`` are replaced by zeros
    before the convolution (its 3-tap window at the last live position reaches one sample into the padding).  A sample's
    logits then depend on its own live samples alone, bit for bit.

    ``forward(x, lengths, attention_sink=[])``: every encoder layer appends the record of its attention to the list
    (``ecgmm.hip.nn.TransformerEncoderLayer``), what ``ecgmm.explain.attention_maps`` / ``attention_rollout`` work from; the
    logits are bit-identical with and without it."""

    def __init__(self, input_dim=1, seq_len=3000, num_classes=2, d_model=128, nhead=4, num_layers=2, dim_feedforward=256,
                 time_attention=False):
        super().__init__()
        self.time_attention = bool(time_attention)
        self.conv = HN.Conv1d(input_dim, d_model, kernel_size=3, padding=1)
        self.pos_embedding = torch.nn.Parameter(torch.zeros(1, seq_len, d_model))
        encoder_layer = HN.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward,
                                                   batch_first=self.time_attention)
        self.transformer_encoder = HN.TransformerEncoder(encoder_layer, num_layers=num_layers)
        self.global_pool = torch.nn.AdaptiveAvgPool1d(1)   # (executed as HF.seq_mean over the positions)
        self.classifier = HN.Sequential(torch.nn.Flatten(), HN.Linear(d_model, 64), torch.nn.ReLU(), torch.nn.Dropout(0.3),
                                        HN.Linear(64, num_classes))

    def forward(self, x, lengths=None, attention_sink=None):
        if lengths is not None and not self.time_attention:
            raise ValueError("ECGTransformer1D: lengths needs time_attention=True (attention across the batch has no "
                             "per-sample length)")
        if lengths is not None and isinstance(x, torch.Tensor) and x.dim() == 3:
            lengths = HF.check_lengths(lengths, x.shape[0], x.shape[2]).to(x.device)
        _require_cuda(x, "ECGTransformer1D")
        if x.dim() != 3 or x.shape[1] != self.conv.in_channels:
            raise ValueError(f"ECGTransformer1D expects [B, {self.conv.in_channels}, L], got {tuple(x.shape)}")
        if x.shape[2] > self.pos_embedding.shape[1]:
            raise ValueError(f"ECGTransformer1D: L={x.shape[2]} exceeds seq_len={self.pos_embedding.shape[1]}")
        if lengths is not None:
            # the conv's right tap at a record's last live position reads the first padded sample: the padding of the raw
            # input is set to zero (plumbing on [B, C, L]), so that nothing live depends on what the padding holds
            live = torch.arange(x.shape[2], device=x.device)[None, None, :] < lengths[:, None, None]
            x = x.masked_fill(~live, 0.0)
        x = HF.embed1d(x, self.conv.weight, self.conv.bias, self.pos_embedding)   # [B, L, d_model]
        sink = {} if attention_sink is None else {"attention_sink": attention_sink}
        if lengths is None:
            x = self.transformer_encoder(x, **sink)         # sequence axis = B as the reference, or L with time_attention
            return self.classifier(HF.seq_mean(x))
        x = self.transformer_encoder(x, lengths=lengths, **sink)
        return self.classifier(HF.seq_mean(x, lengths))


def build_model(model="resnet", num_classes=2, config=Config, seq_len=MAX_LEN, time_attention=False):
    """The network ``main`` trains: ``"resnet"`` = ``ResNet1D_SE`` (train_physionet.py:275), ``"transformer"`` =
    :class:`ECGTransformer1D` (:276), with ``time_attention`` attending along the positions."""
    if model == "resnet":
        if time_attention:
            raise ValueError("time_attention=True needs model='transformer'")
        return ResNet1D_SE(num_classes=num_classes, compute_dtype=getattr(config, "compute_dtype", "bf16"))
    if model == "transformer":
        return ECGTransformer1D(seq_len=seq_len, num_classes=num_classes, time_attention=time_attention)
    raise ValueError(f"model={model!r}: expected 'resnet' or 'transformer'")


# --------------------------------------------------------------------------------------------
# pre-processing (device)                                   reference: train_physionet.py:23-45
# --------------------------------------------------------------------------------------------
def z_score_normalize(signal, eps=1e-8):
    """(x - mean) / (std + eps) per record of a CUDA tensor [..., L] (population std, fp64 inside)."""
    return PP.filter_zscore(signal, [1.0, 0.0], [1.0, 0.0], zscore=True, eps=eps)   # identity filter: y = x exactly


def _band(lowcut, highcut, fs, order):
    nyq = 0.5 * fs
    return PP.butter_bandpass(order, lowcut / nyq, highcut / nyq)


def bandpass_filter(signal, lowcut=16, highcut=149, fs=300, order=4):
    """filtfilt(butter(order, [low, high], 'band'), signal) per record of a CUDA tensor [..., L]."""
    b, a = _band(lowcut, highcut, fs, order)
    return PP.filter_zscore(signal, b, a, zscore=False)


def preprocess_signal(raw_signal, orig_fs=300, target_fs=300):
    """bandpass_filter -> z_score_normalize in one launch.  raw_signal: CUDA float tensor [..., L]."""
    if orig_fs != target_fs:
        raise NotImplementedError("preprocess_signal: this is the one-launch filter + z-score of equal rates; for "
                                  "orig_fs != target_fs use preprocess_resampled (band-pass, resample_signal, z-score) or "
                                  "resample_signal itself")
    _require_cuda(raw_signal, "preprocess_signal")
    b, a = _band(16, 149, orig_fs, 4)
    return PP.filter_zscore(raw_signal, b, a, zscore=True, eps=1e-8)


def _rate_ratio(orig_fs, target_fs):
    if not (np.isfinite(orig_fs) and np.isfinite(target_fs) and orig_fs > 0 and target_fs > 0):
        raise ValueError(f"resample_signal: sampling rates must be finite and > 0 (orig_fs={orig_fs}, target_fs={target_fs})")
    return target_fs / orig_fs      # in Python floats, as the reference writes it


def resample_signal(signal, orig_fs, target_fs=300):
    """train_physionet.py:35-39 per record of a CUDA tensor [..., L]: ``signal`` itself when the rates are equal, else
    ``scipy.signal.resample(signal, int(L * (target_fs / orig_fs)))`` (``ecgmm.preprocess.resample``: fp64 inside)."""
    if orig_fs == target_fs:
        return signal
    ratio = _rate_ratio(orig_fs, target_fs)
    _require_cuda(signal, "resample_signal")
    return PP.resample(signal, ratio=ratio)


def preprocess_resampled(raw_signal, orig_fs, target_fs=300):
    """The reference's three steps for unequal rates (train_physionet.py:41-45): bandpass_filter at ``orig_fs`` ->
    resample_signal -> z_score_normalize.  raw_signal: CUDA float tensor [..., L] -> [..., int(L * (target_fs / orig_fs))]."""
    _require_cuda(raw_signal, "preprocess_resampled")
    filtered = bandpass_filter(raw_signal, 16, 149, orig_fs, 4)
    return z_score_normalize(resample_signal(filtered, orig_fs, target_fs))


def augment_signal(signal, **kw):
    """train_physionet.py:47-60 per record of a CUDA tensor [..., L]: three independent coin flips -- N(0, 0.01^2) noise,
    a U(0.8, 1.2) gain, a circular roll by -10 .. 9 samples.  Draws from ``HF``'s Philox state."""
    _require_cuda(signal, "augment_signal")
    shape = signal.shape
    x = signal.reshape(-1, shape[-1]).float().contiguous()
    idx = torch.arange(x.shape[0], dtype=torch.int64, device=x.device)
    return gather_augment(x, idx, augment=True, check_index=False, **{**AUG_DEFAULTS, **kw}).reshape(shape)


# --------------------------------------------------------------------------------------------
# host side: records, padding, labels, split
# --------------------------------------------------------------------------------------------
def pad_sequences(sequences, maxlen, dtype="float32", padding="post", truncating="post", value=0.0):
    """keras ``pad_sequences`` for the arguments the reference uses (train_physionet.py:72-74): zero padding at the end,
    truncation at the end.  -> numpy [len(sequences), maxlen]."""
    if padding != "post" or truncating != "post":
        raise NotImplementedError("pad_sequences: only padding='post', truncating='post' (the reference's call)")
    out = np.full((len(sequences), int(maxlen)), value, dtype=dtype)
    for i, s in enumerate(sequences):
        s = np.asarray(s)[:maxlen]
        out[i, :len(s)] = s
    return out


_GAIN = re.compile(r"^([0-9.eE+-]+)(?:\((-?\d+)\))?(?:/.*)?$")


def read_record(path):
    """Physical signal ``p_signal`` [samples, signals] (float64) of one challenge record, as ``wfdb.rdrecord(path).p_signal``:
    ``path`` names the ``NAME.hea`` + ``NAME.mat`` pair without extension (``val`` int16 [signals, samples]; gain and
    baseline from each signal line of the header, gain 200 when absent or 0, baseline = ADC zero when not in parentheses;
    ``(val - baseline) / gain``).  A ``.npy`` path (or ``NAME.npy`` next to no header) is loaded as is."""
    if path.endswith(".npy") or (not os.path.exists(path + ".hea") and os.path.exists(path + ".npy")):
        x = np.load(path if path.endswith(".npy") else path + ".npy").astype(np.float64)
        return x.reshape(-1, 1) if x.ndim == 1 else x
    from scipy.io import loadmat
    with open(path + ".hea") as f:
        lines = [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]
    nsig = int(lines[0].split()[1])
    gains, baselines = [], []
    for ln in lines[1:1 + nsig]:
        fld = ln.split()
        gain, base = 200.0, None
        if len(fld) > 2:
            m = _GAIN.match(fld[2])
            if m is None:
                raise ValueError(f"{path}.hea: cannot parse the gain field {fld[2]!r}")
            gain = float(m.group(1)) or 200.0
            base = None if m.group(2) is None else int(m.group(2))
        if base is None:
            base = int(fld[4]) if len(fld) > 4 else 0
        gains.append(gain)
        baselines.append(base)
    val = np.asarray(loadmat(path + ".mat")["val"], dtype=np.float64)
    if val.shape[0] != nsig:
        raise ValueError(f"{path}.mat: {val.shape[0]} signals, the header declares {nsig}")
    return ((val - np.array(baselines, dtype=np.float64)[:, None]) / np.array(gains)[:, None]).T


def read_fs(path):
    """Sampling frequency of one record: field 3 of the first line of ``NAME.hea`` (``NAME nsig fs[/counter] nsamp ...``);
    ``None`` for a ``.npy`` record, which carries none."""
    if path.endswith(".npy") or (not os.path.exists(path + ".hea") and os.path.exists(path + ".npy")):
        return None
    with open(path + ".hea") as f:
        lines = [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]
    fld = lines[0].split()
    if len(fld) < 3:
        return 250.0                # WFDB's default where the record line names no frequency
    return float(fld[2].split("/")[0])


def read_labels(label_file, label_map=LABEL_MAP):
    """REFERENCE.csv (``record,label``, no header) -> [(record, class)] for the labels in ``label_map``; the rest ('~') dropped."""
    rows = []
    with open(label_file, newline="") as f:
        for rec in csv.reader(f):
            if len(rec) >= 2 and rec[1].strip() in label_map:
                rows.append((rec[0].strip(), label_map[rec[1].strip()]))
    return rows


def synthetic_records(config=Config, label_map=LABEL_MAP):
    """Generated variable-length single-lead records (2000 .. 18000 samples at 300 Hz) in place of the challenge data:
    a beat train whose regularity depends on the class, baseline wander and noise, in mV."""
    n = config.synthetic_train_size + config.synthetic_val_size + config.synthetic_test_size
    rng = np.random.RandomState(config.seed)
    names = sorted(label_map, key=lambda k: (label_map[k], k))
    signals, labels = [], []
    for i in range(n):
        name = names[i % len(names)]
        length = int(rng.randint(2000, 18001))
        t = np.arange(length) / 300.0
        rate = {"N": 1.1, "AF": 1.9, "O": 1.4}.get(name, 1.0)
        jitter = {"N": 0.0, "AF": 0.35, "O": 0.1}.get(name, 0.0)
        phase = 2 * np.pi * rate * t + jitter * np.cumsum(rng.randn(length)) * 0.2
        beat = np.exp(8.0 * (np.cos(phase) - 1.0))
        x = 0.9 * beat + 0.1 * np.sin(2 * np.pi * 0.3 * t + rng.rand() * 6.28) + 0.02 * rng.randn(length)
        signals.append(x)
        labels.append(label_map[name])
    return signals, np.array(labels, dtype=np.int64)


def load_records(config=Config, label_map=LABEL_MAP, quiet=True, target_fs=None):
    """-> (list of 1-D float64 signals, int64 labels): lead 0 of every record of REFERENCE.csv that loads
    (train_physionet.py:91-109; a record that fails to load is skipped with a warning).
    ``target_fs=None``: the records as they are read (host code only).  A number: every record whose header (:func:`read_fs`)
    names another sampling rate is resampled over its own length to ``int(len * (target_fs / fs))`` samples on
    ``config.device`` (:func:`resample_records`); the synthetic records and ``.npy`` records carry no rate and stay."""
    if getattr(config, "synthetic", False):
        return synthetic_records(config, label_map)
    signals, labels, rates = [], [], []
    for name, lab in read_labels(config.physionet_label_file, label_map):
        try:
            path = os.path.join(config.physionet_data_dir, name)
            signals.append(read_record(path)[:, 0])
            labels.append(lab)
            rates.append(None if target_fs is None else read_fs(path))
        except Exception as e:   # noqa: BLE001 -- as the reference: any failure skips the record
            if not quiet:
                print(f"Warning: Failed to load record {name}: {e}")
    if target_fs is not None:
        signals = resample_records(signals, rates, target_fs, torch.device(config.device))
    return signals, np.array(labels, dtype=np.int64)


def resample_records(signals, rates, target_fs, device, chunk=256):
    """Every record i with ``rates[i]`` neither ``None`` nor ``target_fs`` -> ``resample_signal`` over its own length, the
    others untouched.  Records of one rate go up in chunks of ``chunk`` rows, zero-padded to the chunk's longest record, and
    come back through the lengths form of ``ecgmm.preprocess.resample`` as float64 numpy like the rest."""
    out = list(signals)
    by_rate = {}
    for i, fs in enumerate(rates):
        if fs is not None and fs != target_fs and len(signals[i]) > 0:
            by_rate.setdefault(fs, []).append(i)
    for fs, idx in sorted(by_rate.items()):
        ratio = _rate_ratio(fs, target_fs)
        for c0 in range(0, len(idx), chunk):
            part = idx[c0:c0 + chunk]
            lens = [len(signals[i]) for i in part]
            rows = pad_sequences([signals[i] for i in part], maxlen=max(lens), dtype="float32")
            y, n = PP.resample(torch.from_numpy(rows).to(device), ratio=ratio, lengths=lens)
            y, n = y.cpu().numpy(), n.cpu().numpy()
            for row, i in enumerate(part):
                out[i] = y[row, :n[row]].astype(np.float64)
    return out


# --------------------------------------------------------------------------------------------
# dataset + loader (device resident)
# --------------------------------------------------------------------------------------------
class SignalOnlyDataset:
    """One split, resident on the device: padded to ``max_len`` on the host, uploaded once, band-pass filtered and
    z-scored once (train_physionet.py:63-86 does both per sample per epoch).  ``signals`` [n, max_len] fp32, ``labels`` [n].
    ``with_lengths``: the dataset also carries ``lengths`` [n] int32 on the device (``lengths_host`` on the host),
    ``min(len(record), max_len)`` per record: the samples of a row that are the record's own.  The filter and the z-score
    still run over the padded row, as the reference's do."""

    def __init__(self, indices, labels, ecg_signals, augment=True, max_len=MAX_LEN, split="train", device=None,
                 with_lengths=False):
        device = torch.device(device or Config.device)
        self.labels_host = torch.as_tensor(np.asarray(labels)[np.asarray(indices)], dtype=torch.long)
        self.ecg_signals_padded = pad_sequences([ecg_signals[i] for i in indices], maxlen=max_len, dtype="float32",
                                                padding="post", truncating="post")
        self.lengths_host = self.lengths = None
        if with_lengths:
            self.lengths_host = torch.as_tensor([min(len(ecg_signals[i]), int(max_len)) for i in indices], dtype=torch.int32)
            if self.lengths_host.numel() and int(self.lengths_host.min()) < 1:
                raise ValueError("SignalOnlyDataset: an empty record has no length to attend over")
            self.lengths = self.lengths_host.to(device)
        self.max_len, self.split = max_len, split
        self.augment = bool(augment) and split == "train"
        self.signals = preprocess_signal(torch.from_numpy(self.ecg_signals_padded).to(device), orig_fs=300, target_fs=300)
        self.labels = self.labels_host.to(device)

    def __len__(self):
        return self.labels_host.numel()

    def __getitem__(self, idx):
        sig = self.signals[idx]
        if self.augment:
            sig = augment_signal(sig)
        return sig, self.labels[idx]


class DeviceSignalLoader(T.ResidentLoader):
    """Batches of a :class:`SignalOnlyDataset`: ``(signals [B, L] fp32 on the device, labels [B] on the device)``, one
    ``gather_augment`` launch per batch (augmentation as the dataset says).  ``shuffle``: a ``torch.randperm`` of the seeded
    ``generator`` per epoch, kept in ``last_order``.

    A dataset with ``lengths`` yields ``((signals, lengths [B] int32), labels)``, the shape ``train_physionet2``'s loader
    uses.  The augmentation is unchanged: its circular roll of at most 10 samples turns the whole padded row, so it moves at
    most 10 samples across the record's end (up to 10 samples of the record into the padding's far end or the start, and as
    many zeros of the padding into the live part); the length is not adjusted for it."""

    def __init__(self, dataset, batch_size=8, shuffle=False, generator=None, drop_last=False):
        super().__init__(dataset, batch_size, shuffle, generator, drop_last)

    def batch(self, idx):
        ds = self.dataset
        signals = gather_augment(ds.signals, idx, augment=ds.augment, check_index=False, **AUG_DEFAULTS)
        if getattr(ds, "lengths", None) is None:
            return signals, ds.labels[idx]
        return (signals, ds.lengths[idx]), ds.labels[idx]


def get_signalonly_dataloaders(config=Config, batch_size=8, label_map=LABEL_MAP, augment=True, split=SPLIT, max_len=MAX_LEN,
                               use_lengths=False, target_fs=None):
    """train / val / test :class:`DeviceSignalLoader` (train_physionet.py:89-132; batch 8, only the train split shuffled).
    ``use_lengths``: the datasets carry every record's ``min(len(record), max_len)`` and the loaders yield
    ``((signals, lengths), labels)``.  ``target_fs``: :func:`load_records`."""
    signals, labels = load_records(config, label_map, **({} if target_fs is None else {"target_fs": target_fs}))
    train_idx, val_idx, test_idx = split_indices(labels, config.seed, split)
    device = torch.device(config.device)
    mk = lambda idx, name: SignalOnlyDataset(idx, labels, signals, augment=augment, max_len=max_len, split=name, device=device,
                                             with_lengths=use_lengths)
    gen = torch.Generator().manual_seed(config.seed)
    return (DeviceSignalLoader(mk(train_idx, "train"), batch_size, shuffle=True, generator=gen),
            DeviceSignalLoader(mk(val_idx, "val"), batch_size), DeviceSignalLoader(mk(test_idx, "test"), batch_size))


# --------------------------------------------------------------------------------------------
# training                                                  reference: train_physionet.py:267-451
# --------------------------------------------------------------------------------------------
def evaluate(model, loader, num_classes=2, predictor=None):
    """Softmax probabilities of the split -> accuracy / F1 / AUC (binary: class-1 probability thresholded at 0.5,
    train_physionet.py:359-379; more classes: argmax, macro F1, one-vs-rest AUC, train_physionet_multi.py:312-330)."""
    model.eval()
    forward = model if predictor is None else predictor
    if getattr(loader.dataset, "lengths", None) is not None:   # the loader yields (signals, lengths) as the inputs
        y_true, y_prob, _, _ = T.predict(lambda inputs: forward(inputs[0].unsqueeze(1), inputs[1]), loader)
    else:
        y_true, y_prob, _, _ = T.predict(forward, loader, lambda x: x.unsqueeze(1))
    if num_classes == 2:
        return T.binary_metrics(y_true, y_prob[:, 1], (y_prob[:, 1] >= 0.5).astype(int))
    from sklearn.metrics import f1_score
    y_pred = np.argmax(y_prob, axis=1)
    return {"accuracy": float((y_true == y_pred).mean()),
            "f1": float(f1_score(y_true, y_pred, average="macro", zero_division=0)),
            "auc": T.auc_or_nan(y_true, y_prob, multi_class="ovr")}


def main(config=Config, num_epochs=30, batch_size=8, quiet=False, use_predictor=False, num_classes=2, label_map=LABEL_MAP,
         augment=True, split=SPLIT, model="resnet", max_len=MAX_LEN, time_attention=False, use_lengths=False,
         rollout_samples=0, target_fs=None):
    """``model``: ``"resnet"`` (the reference's choice) or ``"transformer"`` (its commented alternative, :276); ``max_len``:
    the length every record is padded or cut to.
    ``use_predictor``: run the validation and test passes through an ``ecgmm.inference.Predictor`` (the BatchNorm-folded
    plan of the ResNet1D_SE; for ``model="transformer"`` the four-launches-per-layer plan of :class:`ECGTransformer1D`, with
    either ``time_attention`` and with ``use_lengths``), refreshed after every training epoch and after every checkpoint
    load.  Default off.
    ``time_attention`` or ``config.physionet_time_attention`` (off by default; ``model="transformer"`` only): the encoder
    attends along each record's positions instead of across the batch (:class:`ECGTransformer1D`).
    ``use_lengths`` or ``config.physionet_use_lengths`` (off by default; needs ``time_attention``): the loaders carry
    ``min(len(record), max_len)`` per record and the model gets it, so the zero padding of a short record is neither
    attended to nor averaged (:class:`DeviceSignalLoader` on what the augmentation's roll does at the record's end).
    ``rollout_samples=k`` > 0 (needs ``model="transformer"`` with ``time_attention``): after the test pass, with the weights
    it ended on, ``attention_rollout.npz`` is written into the run directory for the first ``k`` test records:
    ``relevance`` [k, L] (``ecgmm.explain.attention_rollout``), ``lengths`` [k] (``max_len`` without ``use_lengths``),
    ``labels`` [k] and ``probs`` [k, classes].  The default 0 writes nothing.
    ``target_fs`` or ``config.physionet_target_fs`` (default ``None``: records as read): every record whose header names
    another sampling rate is resampled to it on the device before padding (:func:`load_records`).
    -> (history, {"best": metrics, "last": metrics}, checkpoint directory)."""
    time_attention = bool(time_attention or getattr(config, "physionet_time_attention", False))
    use_lengths = bool(use_lengths or getattr(config, "physionet_use_lengths", False))
    rollout_samples = int(rollout_samples)
    target_fs = target_fs if target_fs is not None else getattr(config, "physionet_target_fs", None)
    if rollout_samples < 0:
        raise ValueError(f"rollout_samples={rollout_samples} must be >= 0")
    if rollout_samples and not (model == "transformer" and time_attention):
        raise ValueError("rollout_samples needs model='transformer' and time_attention=True (attention rollout is the "
                         "transformer's map over each record's own positions)")
    if (time_attention or use_lengths) and model == "resnet":
        raise ValueError("time_attention / use_lengths need model='transformer' (the ResNet1D_SE has neither)")
    if use_lengths and not time_attention:
        raise ValueError("use_lengths=True needs time_attention=True (attention across the batch has no per-record length)")
    T.seed_all(config.seed, numpy=True)
    device = torch.device(config.device)
    if not quiet:
        print(f"Using device: {device}")
    train_loader, val_loader, test_loader = get_signalonly_dataloaders(config, batch_size, label_map, augment, split, max_len,
                                                                       **({"use_lengths": True} if use_lengths else {}),
                                                                       **({} if target_fs is None else {"target_fs": target_fs}))
    model = build_model(model, num_classes, config, max_len, **({"time_attention": True} if time_attention else {})).to(device)
    criterion = FocalLoss(alpha=1.0, gamma=2.0)
    optimizer = FusedAdam(model.parameters(), lr=0.001)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=0.001, steps_per_epoch=len(train_loader),
                                                    epochs=num_epochs)
    ckpt_dir = T.run_dir(config.checkpoint_dir)
    predictor = None
    if use_predictor:
        from .inference import Predictor
        predictor = Predictor(model)

    def step(batch, forward=model):
        signals, labels = batch
        if use_lengths:
            signals, lengths = signals
            out = forward(signals.unsqueeze(1), lengths)
        else:
            out = forward(signals.unsqueeze(1))   # [B, L] -> [B, 1, L]
        return criterion(out, labels), out, labels

    def train_pass():
        model.train()
        result = T.run_epoch(train_loader, step, optimizer, scheduler)
        model.eval()
        return result

    def val_pass():   # the accuracy is accumulated over the batches (the reference's `=` at :326 is a bug)
        return T.run_epoch(val_loader, step if predictor is None else lambda batch: step(batch, predictor))

    def on_epoch(h, _extras):
        if not quiet:
            print(f"[{h['epoch']}] train {h['train_loss']:.4f}/{h['train_acc']:.4f}  val {h['val_loss']:.4f}/{h['val_acc']:.4f}")

    # train_physionet.py:335-341: best.pth and best_signal_only_epochN.pth on a lower validation loss; no early stop
    history = T.fit(model, optimizer, train_pass, val_pass, ckpt_dir, num_epochs,
                    best_names=("best.pth", "best_signal_only_epoch{epoch}.pth"), predictor=predictor, on_epoch=on_epoch)
    results = T.test_checkpoints(model, ckpt_dir, ("best", "last"),
                                 lambda: evaluate(model, test_loader, num_classes, predictor=predictor), predictor)
    if not quiet:
        for tag, res in results.items():
            print(f"test[{tag}]: {res}")
    if rollout_samples:
        path = write_attention_rollout(model, test_loader.dataset, rollout_samples, ckpt_dir)
        if not quiet:
            print(f"attention rollout of the first test records -> {path}")
    return history, results, ckpt_dir


def write_attention_rollout(model, dataset, k, out_dir, residual=0.5):
    """``attention_rollout.npz`` in ``out_dir`` for the first ``k`` records of ``dataset`` (a :class:`SignalOnlyDataset`):
    ``relevance`` [k, L], ``lengths`` [k], ``labels`` [k], ``probs`` [k, classes] -> the file's path"""
    from .explain import attention_rollout
    k = min(int(k), len(dataset))
    x = dataset.signals[:k].unsqueeze(1)
    lengths = None if dataset.lengths is None else dataset.lengths[:k]
    relevance = attention_rollout(model, x, lengths, residual=residual)
    was_training = model.training
    model.eval()
    with torch.no_grad():
        logits = model(x) if lengths is None else model(x, lengths)
    model.train(was_training)
    path = os.path.join(out_dir, "attention_rollout.npz")
    np.savez(path, relevance=relevance.cpu().numpy(),
             lengths=(np.full(k, x.shape[2], dtype=np.int32) if lengths is None else dataset.lengths_host[:k].numpy()),
             labels=dataset.labels_host[:k].numpy(), probs=torch.softmax(logits.float(), dim=1).cpu().numpy())
    return path


if __name__ == "__main__":
    main()
