"""Evaluation of a PTB-XL-trained ``ResNet1D_SE`` on the digitized ECG signals (reference: evaluation_signal.py:20-90,
164-202): labels ∩ ``ecg_csv``, 'Borderline' dropped, a per-column ``StandardScaler`` fitted on the evaluated set itself,
the PTB-XL pre-processing (baseline removal, ``butter(5, 40/125)`` ``filtfilt``, crop or zero-pad to 2476), batch 8, and
AUC / F1 / accuracy at the F1-best threshold.

The scaler and the filter run in the existing ``ecgmm_signal_preprocess`` launch (``sc_mean`` / ``sc_scale`` are its
operands), once for the whole set instead of per sample.  Not carried over: the figures."""
import numpy as np
import torch

from . import preprocess as PP
from . import training as T
from .config import Config
from .hip.functional import _require_cuda
from .signal_model import ResNet1D_SE, find_best_threshold
from .train_signal_only_ptb import LENGTH

LABEL_MAP = {"Normal": 0, "Abnormal": 1}      # evaluation_signal.py:76


def preprocess_signal(raw_signal, scaler_mean=None, scaler_scale=None, length=LENGTH):
    """evaluation_signal.py:31-39 per row of a CUDA float tensor [..., L] (assumed at 250 Hz, as the reference assumes):
    remove_baseline_drift -> lowpass_filter(cutoff=40, fs=250, order=5) -> ``[:length]`` or zero padding up to ``length``."""
    _require_cuda(raw_signal, "preprocess_signal")
    y = PP.preprocess_signal(raw_signal, window_size=200, cutoff=40, fs=250, order=5, scaler_mean=scaler_mean,
                             scaler_scale=scaler_scale)
    Ln = y.shape[-1]
    if Ln > length:
        return y[..., :length].contiguous()
    return torch.nn.functional.pad(y, (0, length - Ln))


class DigitizedECGDataset:
    """evaluation_signal.py:42-68, resident on the device: ``signals`` [n, 1, 2476] fp32 in the order of ``labels_df``."""

    augment = False

    def __init__(self, indices, labels_df, ecg_signals, ecg_scaler=None, device=None):
        device = torch.device(device or Config.device)
        self.labels_df = labels_df[labels_df["index"].isin(indices)].reset_index(drop=True)
        self.ecg_signals = ecg_signals.loc[ecg_signals.index.isin(indices)]
        self.ecg_scaler = ecg_scaler
        rows = self.ecg_signals.loc[self.labels_df["index"]].values.astype(np.float32)
        mean = None if ecg_scaler is None else ecg_scaler.mean_
        scale = None if ecg_scaler is None else ecg_scaler.scale_
        x = torch.from_numpy(np.ascontiguousarray(rows))
        self.signals = preprocess_signal(x.to(device), mean, scale).unsqueeze(1)
        self.labels_host = torch.as_tensor(self.labels_df["label"].values.astype(np.int64))
        self.labels = self.labels_host.to(device)

    def __len__(self):
        return self.labels_host.numel()

    def __getitem__(self, idx):
        return self.signals[idx], self.labels[idx]


def get_digitized_test_loader(config=Config):
    """evaluation_signal.py:71-90.  Deviation: the reference passes ``labels_df.index.tolist()`` -- the positions 0 .. m-1 of
    the m filtered rows -- as ``indices``, and its dataset keeps a record only if its ``index`` VALUE is among them (:44-45), so
    it silently drops every record whose index is m or more.  Here the common indices themselves are passed: every record that
    has both a label and a signal is evaluated."""
    import pandas as pd
    from sklearn.preprocessing import StandardScaler
    from .dataset import _read_table
    labels_df = _read_table(config.label_file)
    ecg_signals = pd.read_csv(config.ecg_csv, index_col=0)
    labels_df = labels_df[labels_df["label"] != "Borderline"].copy()
    labels_df["label"] = labels_df["label"].map(LABEL_MAP)
    labels_df["index"] = labels_df["index"].astype(int)
    ecg_signals.index = ecg_signals.index.astype(int)
    common = sorted(set(labels_df["index"]) & set(ecg_signals.index))
    labels_df = labels_df[labels_df["index"].isin(common)].reset_index(drop=True)
    ecg_signals = ecg_signals.loc[ecg_signals.index.isin(common)]
    ecg_scaler = StandardScaler().fit(ecg_signals)
    test_ds = DigitizedECGDataset(common, labels_df, ecg_signals, ecg_scaler, device=config.device)
    return PP.PTBXLLoader(test_ds, batch_size=8)


def main(model_path, config=Config, quiet=False, use_predictor=False):
    """-> dict(threshold, auc, f1, accuracy, report) of the checkpoint ``model_path`` (a ``ResNet1D_SE()`` state dict)."""
    from sklearn.metrics import classification_report, f1_score, roc_auc_score
    device = torch.device(config.device)
    test_loader = get_digitized_test_loader(config)
    model = ResNet1D_SE(compute_dtype=getattr(config, "compute_dtype", "bf16")).to(device)
    model.load_state_dict(torch.load(model_path, map_location=device))
    model.eval()
    fwd = model
    if use_predictor:
        from .inference import Predictor
        fwd = Predictor(model)
    y_true, y_prob, _, _ = T.predict(fwd, test_loader)
    y_prob = y_prob[:, 1]
    best_t = float(find_best_threshold(y_true, y_prob))
    y_pred = (y_prob >= best_t).astype(int)
    res = dict(threshold=best_t, auc=float(roc_auc_score(y_true, y_prob)), f1=float(f1_score(y_true, y_pred)),
               accuracy=float((y_true == y_pred).mean()),
               report=classification_report(y_true, y_pred, labels=[0, 1], target_names=["Normal", "Abnormal"],
                                            zero_division=0))
    if not quiet:
        print(f"\nBest Threshold: {best_t:.2f}")
        print(f"Test AUC: {res['auc']:.4f} | F1: {res['f1']:.4f} | ACC: {res['accuracy']:.4f}")
        print("\n=== Classification Report ===\n" + res["report"])
    return res


if __name__ == "__main__":
    import sys
    main(sys.argv[1])
