"""PTB-XL single-lead trainer, AFIB vs other rhythms (reference: train_signal_only_ptb.py:18-53, 171-328) -- the script that
produced ``best_ptbxl.pth``.

The reference decodes, decimates and filters every record again at every ``__getitem__`` on CPU workers
(``wfdb.rdsamp(path, channels=[1])`` -> ``[::2]`` -> 200-tap baseline removal -> ``butter(5, 40/125)`` ``filtfilt`` -> crop or
zero-pad to 2476) and draws its batches with ``WeightedRandomSampler(1 / class_count, n)``.  Here each record is read once,
its int16 frames are uploaded as they lie on disk and ONE ``preprocess_i16`` launch per chunk of records produces the rows
(the result is a pure function of the record, so caching it changes nothing); one ``weighted_sample`` launch per epoch draws
the indices on the device and one gather launch per batch collects the rows.  Model, loss, optimizer and schedule are the
reference's: ``ResNet1D_SE`` on ``[B, 1, 2476]``, ``FocalLoss()``, Adam(1e-3), ``OneCycleLR(epochs=30)`` stepped per batch
while 10 epochs run (train_signal_only_ptb.py:254,257: the schedule never leaves its first third; kept).

This module holds the record reader, the labels, the resident dataset, the sampler and the policy values; the loader is
``ecgmm.preprocess.PTBXLLoader`` (shared with ``evaluation_signal``), the epoch loop and the metrics are ``ecgmm.training``'s.

``wfdb`` is replaced by :func:`read_header` / :func:`read_record_i16` / :func:`rdsamp` (format 16, one ``.dat`` per record),
``pandas`` by the ``csv`` module, ``eval`` of the ``scp_codes`` column by ``ast.literal_eval``.  Not carried over: the figures
(confusion matrix, ROC curve); the 100 Hz ``filename_lr`` records; WFDB formats other than 16.
"""
import ast
import csv
import os
import re

import numpy as np
import torch

from . import preprocess as PP
from . import training as T
from .config import Config
from .optim import FusedAdam
from .preprocess import PTBXLLoader   # noqa: F401 -- shared with evaluation_signal; this name is part of this module
from .signal_model import FocalLoss, ResNet1D_SE, find_best_threshold
from .training import split_indices

LENGTH = 2476
SPLIT = (0.4, 0.5)             # train_signal_only_ptb.py:227-228: 60 % train, the remaining 40 % halved
ABNORMAL_RHYTHM_CODES = ["SR", "STACH", "SARRH", "SBRAD", "PACE", "SVARR", "BIGU", "AFLT", "SVTAC", "PSVT", "TRIGU"]   # :190
INVALID_16 = -32768            # format 16's invalid-sample code; wfdb turns it into NaN


# --------------------------------------------------------------------------------------------
# WFDB format 16 (host)                                            replaces wfdb.rdsamp, :43
# --------------------------------------------------------------------------------------------
_GAIN = re.compile(r"^([0-9.eE+-]+)?(?:\((-?\d+)\))?(?:/(.*))?$")


def read_header(path):
    """``path`` without extension -> dict of the ``.hea`` fields.  Record line ``name nsig fs nsamp``; per signal
    ``file format gain(baseline)/units adc_res adc_zero init_value checksum block_size description``.  Defaults as WFDB's:
    gain 200 when absent or 0, baseline = ADC zero when not in parentheses.  Refused: multi-segment records, any format other
    than 16 (samples per frame, skew and byte offsets are format modifiers and refused with it), signals in several files."""
    with open(path + ".hea") as f:
        lines = [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("#")]
    if not lines:
        raise ValueError(f"{path}.hea: empty header")
    rec = lines[0].split()
    if len(rec) < 4:
        raise ValueError(f"{path}.hea: the record line needs name, signals, frequency and samples: {lines[0]!r}")
    if "/" in rec[0]:
        raise ValueError(f"{path}.hea: multi-segment records are not supported")
    nsig, nsamp = int(rec[1]), int(rec[3])
    fs = float(rec[2].split("/")[0].split("(")[0])
    if nsig < 1 or nsamp < 1 or len(lines) < 1 + nsig:
        raise ValueError(f"{path}.hea: {nsig} signals of {nsamp} samples declared, {len(lines) - 1} signal lines found")
    h = dict(record_name=rec[0], n_sig=nsig, fs=fs, sig_len=nsamp, file_name=None, gain=np.empty(nsig), units=[],
             baseline=np.empty(nsig, dtype=np.int64), adc_res=[], adc_zero=[], init_value=[], checksum=[], sig_name=[])
    for i, ln in enumerate(lines[1:1 + nsig]):
        fld = ln.split()
        if len(fld) < 2:
            raise ValueError(f"{path}.hea: signal line {i} has no format: {ln!r}")
        if fld[1] != "16":
            raise ValueError(f"{path}.hea: signal {i} has format {fld[1]!r}; only plain format 16 is supported")
        if h["file_name"] is None:
            h["file_name"] = fld[0]
        elif fld[0] != h["file_name"]:
            raise ValueError(f"{path}.hea: signals in several files ({h['file_name']}, {fld[0]}) are not supported")
        gain, base, units = 200.0, None, "mV"
        if len(fld) > 2:
            m = _GAIN.match(fld[2])
            if m is None:
                raise ValueError(f"{path}.hea: cannot parse the gain field {fld[2]!r}")
            gain = float(m.group(1) or 0) or 200.0
            base = None if m.group(2) is None else int(m.group(2))
            units = m.group(3) or "mV"
        ints = []
        for v in fld[3:8]:     # ADC resolution, ADC zero, initial value, checksum, block size: optional, in this order
            if not re.fullmatch(r"[+-]?\d+", v):
                break
            ints.append(int(v))
        adc_res, adc_zero, init, cks = (ints + [None] * 4)[:4]
        h["gain"][i] = gain
        h["baseline"][i] = (adc_zero or 0) if base is None else base
        h["units"].append(units)
        h["adc_res"].append(adc_res or 0)
        h["adc_zero"].append(adc_zero or 0)
        h["init_value"].append(init)
        h["checksum"].append(cks)
        h["sig_name"].append(" ".join(fld[3 + len(ints):]))
    return h


def read_record_i16(path, verify=True):
    """-> (int16 frames [sig_len, n_sig] exactly as the ``.dat`` holds them, header dict).  ``verify``: every signal's first
    sample and 16-bit checksum (the sum of its samples modulo 2^16) must equal the header's, where the header gives them."""
    h = read_header(path)
    dat = os.path.join(os.path.dirname(path), h["file_name"])
    want = h["sig_len"] * h["n_sig"]
    d = np.fromfile(dat, dtype="<i2")
    if d.size != want:
        raise ValueError(f"{dat}: {d.size} samples, the header declares {h['sig_len']} x {h['n_sig']}")
    d = d.reshape(h["sig_len"], h["n_sig"]).astype(np.int16, copy=False)
    if verify:
        sums = d.sum(axis=0, dtype=np.int64)
        for i in range(h["n_sig"]):
            if h["init_value"][i] is not None and int(d[0, i]) != h["init_value"][i]:
                raise ValueError(f"{dat}: signal {i} starts with {int(d[0, i])}, the header says {h['init_value'][i]}")
            if h["checksum"][i] is not None and (int(sums[i]) - h["checksum"][i]) % 65536 != 0:
                raise ValueError(f"{dat}: signal {i} checksum {int(sums[i]) % 65536} != header {h['checksum'][i] % 65536}")
    return d, h


def rdsamp(path, channels=None, verify=True):
    """``wfdb.rdsamp``: (float64 ``p_signal`` [sig_len, len(channels)] = ``(d - baseline) / gain`` with the invalid-sample
    code as NaN, fields dict).  Host use and tests; the trainer decodes on the device."""
    d, h = read_record_i16(path, verify)
    ch = list(range(h["n_sig"])) if channels is None else [int(c) for c in channels]
    if any(c < 0 or c >= h["n_sig"] for c in ch):
        raise ValueError(f"{path}: channels {ch} outside the record's {h['n_sig']} signals")
    p = (d[:, ch].astype(np.float64) - h["baseline"][ch]) / h["gain"][ch]
    p[d[:, ch] == INVALID_16] = np.nan
    fields = dict(fs=h["fs"], sig_len=h["sig_len"], n_sig=len(ch), units=[h["units"][c] for c in ch],
                  sig_name=[h["sig_name"][c] for c in ch])
    return p, fields


# --------------------------------------------------------------------------------------------
# labels, table, split                                             reference: :183-235
# --------------------------------------------------------------------------------------------
def label_ecg(scp_codes):
    """train_signal_only_ptb.py:193-204.  1: AFIB at 100; else 0: one of the 11 rhythm codes at 100; else 2 (dropped);
    anything malformed 2.  The reference writes ``float(d['AFIB'] == 100.0)`` (the parenthesis closes after the comparison):
    the truth value of that float is the comparison's, so the label is the same and the comparison is kept as it stands."""
    try:
        scp_dict = ast.literal_eval(scp_codes) if isinstance(scp_codes, str) else scp_codes
        if ("AFIB" in scp_dict) and float(scp_dict["AFIB"] == 100.0):
            return 1
        elif any(code in scp_dict and float(scp_dict[code]) == 100.0 for code in ABNORMAL_RHYTHM_CODES):
            return 0
        else:
            return 2
    except Exception:   # noqa: BLE001 -- as the reference: malformed or unrecognized
        return 2


def synthetic_records(config=Config):
    """Generated 12-lead int16 records (5000 frames at 500 Hz, gain 1000 / mV, baseline 0) in place of the data: a beat
    train whose regularity depends on the class, baseline wander and noise.  -> (list of record dicts, int64 labels)."""
    n = config.synthetic_train_size + config.synthetic_val_size + config.synthetic_test_size
    rng = np.random.RandomState(config.seed)
    t = np.arange(5000) / 500.0
    lead_gain = np.linspace(0.6, 1.4, 12)
    records, labels = [], []
    for i in range(n):
        lab = int(i % 4 == 0)      # AFIB is the minority class, as in PTB-XL
        phase = 2 * np.pi * (1.6 if lab else 1.1) * t + (0.35 if lab else 0.0) * np.cumsum(rng.randn(5000)) * 0.15
        beat = np.exp(8.0 * (np.cos(phase) - 1.0))
        x = 0.9 * beat + 0.1 * np.sin(2 * np.pi * 0.3 * t + rng.rand() * 6.28)
        mv = x[:, None] * lead_gain[None, :] + 0.02 * rng.randn(5000, 12)
        records.append(dict(frames=np.round(mv * 1000.0).astype(np.int16), gain=np.full(12, 1000.0),
                            baseline=np.zeros(12, dtype=np.int64)))
        labels.append(lab)
    return records, np.array(labels, dtype=np.int64)


def load_ptbxl(config=Config):
    """``ptbxl_database.csv`` -> (record paths from ``filename_hr`` under ``ptbxl_dir``, int64 labels), the rows labelled 2
    dropped (:183-224).  ``Config.synthetic``: :func:`synthetic_records`."""
    if getattr(config, "synthetic", False):
        return synthetic_records(config)
    records, labels = [], []
    with open(config.ptbxl_database, newline="") as f:
        for row in csv.DictReader(f):
            lab = label_ecg(row.get("scp_codes"))
            if lab != 2:
                records.append(os.path.join(config.ptbxl_dir, row["filename_hr"]))
                labels.append(lab)
    return records, np.array(labels, dtype=np.int64)


def class_weights(y_train):
    """train_signal_only_ptb.py:231-233: 1 / (size of the sample's class) per training sample, float64."""
    y_train = np.asarray(y_train)
    classes, inverse, counts = np.unique(y_train, return_inverse=True, return_counts=True)
    return (1.0 / counts)[inverse]


# --------------------------------------------------------------------------------------------
# dataset, sampler, loader (device resident)
# --------------------------------------------------------------------------------------------
def _load(record):
    """a record path or an in-memory record dict -> (int16 frames [T, nsig], gain [nsig], baseline [nsig])"""
    if isinstance(record, dict):
        return record["frames"], np.asarray(record["gain"], dtype=np.float64), np.asarray(record["baseline"])
    d, h = read_record_i16(os.fspath(record))
    return d, h["gain"], h["baseline"]


class PTBXLSignalDataset:
    """One split, resident on the device as ``signals`` [n, len(leads), length] fp32 (train_signal_only_ptb.py:31-53;
    ``leads=range(12)`` is its commented 12-lead variant, :55-87).  Every record is read once; records of one shape are
    uploaded as int16 frames in chunks of ``chunk`` and pre-processed by one ``preprocess_i16`` launch per chunk.  Records of
    another length go in their own launches, so a short one is filtered at its own length and then zero-padded (:50-52)."""

    augment = False

    def __init__(self, records, labels, length=LENGTH, leads=(1,), device=None, chunk=512, step=2):
        device = torch.device(device or Config.device)
        if device.type != "cuda":
            raise RuntimeError(f"PTBXLSignalDataset: device is {device}; the HIP library is the only compute path "
                               "(no CPU fallback) -- use a ROCm device")
        self.records, self.length, self.leads = list(records), int(length), tuple(int(c) for c in leads)
        self.labels_host = torch.as_tensor(np.asarray(labels), dtype=torch.long)
        if len(self.records) != self.labels_host.numel():
            raise ValueError("PTBXLSignalDataset: one label per record")
        n, nc = len(self.records), len(self.leads)
        self.signals = torch.empty(n, nc, self.length, dtype=torch.float32, device=device)
        self.labels = self.labels_host.to(device)
        pending = {}     # (T, nsig) -> [(position, frames, gain, baseline)]

        def flush(items):
            pos = torch.as_tensor([it[0] for it in items], dtype=torch.long, device=device)
            raw = torch.from_numpy(np.stack([it[1] for it in items])).to(device)
            gain = np.stack([it[2][list(self.leads)] for it in items])
            base = np.stack([it[3][list(self.leads)] for it in items])
            self.signals[pos] = PP.preprocess_i16(raw, self.leads, gain, base, step=step, out_len=self.length)

        for i, rec in enumerate(self.records):
            d, gain, base = _load(rec)
            if max(self.leads) >= d.shape[1] or min(self.leads) < 0:
                raise ValueError(f"record {i}: leads {self.leads} outside its {d.shape[1]} signals")
            group = pending.setdefault(d.shape, [])
            group.append((i, np.ascontiguousarray(d, dtype=np.int16), gain, base))
            if len(group) >= chunk:
                flush(group)
                group.clear()
        for group in pending.values():
            if group:
                flush(group)

    def __len__(self):
        return self.labels_host.numel()

    def __getitem__(self, idx):
        return self.signals[idx], self.labels[idx]


class DeviceWeightedSampler:
    """``WeightedRandomSampler(weights, num_samples, replacement=True)`` on the device: the float64 prefix sum of the weights
    is built and uploaded once, :meth:`sample` draws one epoch's indices in one launch from the Philox stream of
    ``ecgmm.hip.functional`` (``manual_seed``).  Negative, non-finite or all-zero weights are refused, as torch refuses them."""

    def __init__(self, weights, num_samples, device=None):
        self.num_samples = int(num_samples)
        if self.num_samples < 1:
            raise ValueError(f"DeviceWeightedSampler: num_samples must be positive, got {num_samples}")
        self.cdf_host, self.last_positive = PP.weight_cdf(weights)
        self.device = torch.device(device or Config.device)
        self._cdf = None

    def __len__(self):
        return self.num_samples

    def sample(self, seed_offset=None, return_uniforms=False):
        if self._cdf is None:
            if self.device.type != "cuda":
                raise RuntimeError(f"DeviceWeightedSampler: device is {self.device}; the HIP library is the only compute "
                                   "path (no CPU fallback)")
            self._cdf = torch.from_numpy(self.cdf_host).to(self.device)
        return PP.weighted_sample(self._cdf, self.last_positive, self.num_samples, seed_offset, return_uniforms)


def get_ptbxl_dataloaders(config=Config, batch_size=16, length=LENGTH, leads=(1,), split=SPLIT):
    """train (weighted sampler) / val / test loaders, train_signal_only_ptb.py:183-243."""
    records, labels = load_ptbxl(config)
    train_idx, val_idx, test_idx = split_indices(labels, config.seed, split)
    device = torch.device(config.device)
    mk = lambda idx: PTBXLSignalDataset([records[i] for i in idx], labels[idx], length=length, leads=leads, device=device)
    train_ds = mk(train_idx)
    weights = class_weights(labels[train_idx])
    sampler = DeviceWeightedSampler(weights, len(weights), device=device)
    return (PTBXLLoader(train_ds, batch_size, sampler=sampler), PTBXLLoader(mk(val_idx), batch_size),
            PTBXLLoader(mk(test_idx), batch_size))


# --------------------------------------------------------------------------------------------
# training                                                          reference: :247-328
# --------------------------------------------------------------------------------------------
def make_scheduler(optimizer, steps_per_epoch, schedule_epochs=30):
    """train_signal_only_ptb.py:254: the cycle is sized for 30 epochs whatever the number of epochs that run (:257 runs 10,
    so the learning rate is still rising when training stops).  Kept as the reference has it."""
    return torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=0.001, steps_per_epoch=steps_per_epoch, epochs=schedule_epochs)


def main(config=Config, num_epochs=10, schedule_epochs=30, batch_size=16, quiet=False, use_predictor=False, length=LENGTH,
         leads=(1,), split=SPLIT):
    """``use_predictor``: validation and test run through an ``ecgmm.inference.Predictor`` (BatchNorm-folded inference
    plan), refreshed after every training epoch and after the checkpoint load.  Default off.
    -> (history, test metrics with the classification report as text, checkpoint directory)."""
    from sklearn.metrics import classification_report
    T.seed_all(config.seed, numpy=True)
    device = torch.device(config.device)
    ckpt_dir = T.run_dir(config.checkpoint_dir, "signal")
    train_loader, val_loader, test_loader = get_ptbxl_dataloaders(config, batch_size, length, leads, split)
    if not quiet:
        print(f"Train: {len(train_loader.dataset)} | Val: {len(val_loader.dataset)} | Test: {len(test_loader.dataset)}")
    model = ResNet1D_SE(input_channels=len(leads), compute_dtype=getattr(config, "compute_dtype", "bf16")).to(device)
    criterion = FocalLoss()
    optimizer = FusedAdam(model.parameters(), lr=0.001)
    scheduler = make_scheduler(optimizer, len(train_loader), schedule_epochs)
    predictor = None
    if use_predictor:
        from .inference import Predictor
        predictor = Predictor(model)
    forward = model if predictor is None else predictor

    def step(batch):
        signals, labels = batch
        out = model(signals)
        return criterion(out, labels), out, labels

    def train_pass():   # the reference reports no training accuracy: one host read per step, the loss
        model.train()
        result = T.run_epoch(train_loader, step, optimizer, scheduler, count_correct=False)
        model.eval()
        return result

    def val_pass():
        y_true, y_prob, _, val_loss = T.predict(forward, val_loader, criterion=criterion)
        return val_loss, None, {"val_auc": T.auc_or_nan(y_true, y_prob[:, 1])}

    def on_epoch(h, extras):
        h.update(extras)
        if not quiet:
            print(f"Epoch [{h['epoch']}] | Train Loss: {h['train_loss']:.4f} | Val Loss: {h['val_loss']:.4f} | "
                  f"Val AUC: {h['val_auc']:.4f}")

    # :289-291: best.pth on a lower validation loss, nothing else is saved
    history = T.fit(model, optimizer, train_pass, val_pass, ckpt_dir, num_epochs, save_last=None, predictor=predictor,
                    on_epoch=on_epoch)
    # best.pth is absent only when no validation loss was below inf (NaN): then there are no results
    scored = T.test_checkpoints(model, ckpt_dir, ("best",), lambda: T.predict(forward, test_loader), predictor)
    results = {}
    if scored:
        y_true, y_prob = scored["best"][0], scored["best"][1][:, 1]
        best_t = float(find_best_threshold(y_true, y_prob))
        y_pred = (y_prob >= best_t).astype(int)
        results = dict(threshold=best_t, **T.binary_metrics(y_true, y_prob, y_pred),
                       report=classification_report(y_true, y_pred, labels=[0, 1], target_names=["Normal", "AF"],
                                                    zero_division=0))
        if not quiet:
            print(f"Best threshold: {best_t:.2f}")
            print(f"Final Test Accuracy: {results['accuracy']:.4f}\nFinal Test F1-Score : {results['f1']:.4f}\n"
                  f"Final Test ROC AUC  : {results['auc']:.4f}")
            print("\n=== Classification Report ===\n" + results["report"])
    return history, results, ckpt_dir


if __name__ == "__main__":
    main()
