"""PhysioNet-2017 single-lead trainer, three classes N / AF / O (reference: train_physionet_multi.py:20-110, 208-334).

Differences from ``train_physionet``: label map with ``O -> 2``, ``ResNet1D_SE(num_classes=3)``, no augmentation, a
70 / 10 / 20 split (train_physionet_multi.py:91-96), macro F1 and one-vs-rest AUC.  Everything else is shared by import."""
import numpy as np

from . import train_physionet as TP
from .config import Config
from .train_physionet import (DeviceSignalLoader, SignalOnlyDataset, bandpass_filter, evaluate,  # noqa: F401
                              pad_sequences, preprocess_signal, read_record, z_score_normalize)

LABEL_MAP = {"N": 0, "AF": 1, "O": 2}      # train_physionet_multi.py:71
# train_physionet_multi.py:91-96: test_size=0.3, then two thirds of the held-out part become the test split
SPLIT = (0.3, 2 / 3)


def find_best_threshold(y_true, y_prob, num_classes=3):
    """train_physionet_multi.py:208-218 as written: the prediction is the argmax whatever the threshold, so the macro F1 is
    the same at every threshold and the first one (0.1) is kept when that F1 is positive, 0.5 otherwise."""
    from sklearn.metrics import f1_score
    best_f1, best_t = 0, [0.5] * num_classes
    for t in np.arange(0.1, 0.9, 0.05):
        y_pred = np.argmax(y_prob, axis=1)
        f1 = f1_score(y_true, y_pred, average="macro")
        if f1 > best_f1:
            best_f1, best_t = f1, [t] * num_classes
    return best_t


def get_signalonly_dataloaders(config=Config, batch_size=8, target_fs=None):
    return TP.get_signalonly_dataloaders(config, batch_size, label_map=LABEL_MAP, augment=False, split=SPLIT,
                                         **({} if target_fs is None else {"target_fs": target_fs}))


def main(config=Config, num_epochs=30, batch_size=8, quiet=False, use_predictor=False, target_fs=None):
    """``target_fs`` (or ``config.physionet_target_fs``): ``train_physionet.load_records``."""
    return TP.main(config, num_epochs, batch_size, quiet, use_predictor, num_classes=3, label_map=LABEL_MAP, augment=False,
                   split=SPLIT, **({} if target_fs is None else {"target_fs": target_fs}))


if __name__ == "__main__":
    main()
