"""PhysioNet-2017 single-lead path, host side: filter design against scipy, padding, the record reader, labels and
splits, argument refusals, the C-ABI table.  No GPU."""
import os

import numpy as np
import pytest
import scipy.signal
import torch
from scipy.io import savemat

from ecgmm import preprocess as PP
from ecgmm import train_physionet as TP
from ecgmm import train_physionet_multi as TM
from ecgmm.config import Config
from ecgmm.hip import lib as L


def _rel(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    return np.max(np.abs(got - ref) / np.where(ref != 0, np.abs(ref), 1.0))


@pytest.mark.parametrize("order,low,high", [(4, 16 / 150, 149 / 150), (1, 0.1, 0.4), (2, 0.05, 0.5), (3, 0.3, 0.9),
                                            (4, 0.02, 0.25)])
def test_butter_bandpass_matches_scipy(order, low, high):
    b_ref, a_ref = scipy.signal.butter(order, [low, high], "band")
    b, a = PP.butter_bandpass(order, low, high)
    assert len(b) == len(a) == 2 * order + 1 and a[0] == 1.0
    assert _rel(b, b_ref) <= 1e-10 and _rel(a, a_ref) <= 1e-10   # relative on every coefficient; exact zeros stay zeros


def test_butter_bandpass_refuses_bad_band():
    for low, high in ((0.0, 0.5), (0.5, 0.5), (0.6, 0.4), (0.2, 1.0)):
        with pytest.raises(ValueError):
            PP.butter_bandpass(4, low, high)


def test_lfilter_zi_of_the_nine_coefficient_filter():
    b, a = scipy.signal.butter(4, [16 / 150, 149 / 150], "band")
    assert len(a) == 9
    assert np.max(np.abs(np.roots(a))) < 0.993   # the pole radius the fp64 direct form has to carry
    assert _rel(PP.lfilter_zi(b, a), scipy.signal.lfilter_zi(b, a)) <= 1e-9


def _pad_ref(seqs, maxlen):
    out = np.zeros((len(seqs), maxlen), dtype=np.float32)
    for i, s in enumerate(seqs):
        k = min(len(s), maxlen)
        out[i, :k] = np.asarray(s[:k], dtype=np.float32)
    return out


def test_pad_sequences_post_post():
    rng = np.random.RandomState(3)
    seqs = [rng.randn(n) for n in (5, 12, 20, 1, 12)]            # shorter, equal and longer than maxlen
    got = TP.pad_sequences(seqs, maxlen=12, dtype="float32", padding="post", truncating="post")
    assert got.dtype == np.float32 and np.array_equal(got, _pad_ref(seqs, 12))
    with pytest.raises(NotImplementedError):
        TP.pad_sequences(seqs, maxlen=12, padding="pre")
    with pytest.raises(NotImplementedError):
        TP.pad_sequences(seqs, maxlen=12, truncating="pre")


def _write_record(dirname, name, val, gain_field, adc_zero=0):
    savemat(os.path.join(dirname, name + ".mat"), {"val": np.asarray(val, dtype=np.int16).reshape(1, -1)})
    with open(os.path.join(dirname, name + ".hea"), "w") as f:
        f.write(f"{name} 1 300 {len(val)} 2013-01-01 00:00:00\n")
        f.write(f"{name}.mat 16+24 {gain_field} 16 {adc_zero} {int(val[0])} 0 0 ECG\n")


def test_read_record_mat_and_header(tmp_path):
    rng = np.random.RandomState(5)
    val = rng.randint(-3000, 3000, size=2714)
    _write_record(tmp_path, "A00001", val, "1000/mV")
    p = TP.read_record(str(tmp_path / "A00001"))
    assert p.shape == (2714, 1) and p.dtype == np.float64
    assert np.array_equal(p[:, 0], val.astype(np.float64) / 1000.0)
    _write_record(tmp_path, "A00002", val, "250.5(-12)/mV")     # gain with an explicit baseline
    assert np.array_equal(TP.read_record(str(tmp_path / "A00002"))[:, 0], (val.astype(np.float64) + 12) / 250.5)
    _write_record(tmp_path, "A00003", val, "400/mV", adc_zero=100)   # no baseline in the gain field: the ADC zero
    assert np.array_equal(TP.read_record(str(tmp_path / "A00003"))[:, 0], (val.astype(np.float64) - 100) / 400.0)
    np.save(tmp_path / "A00004.npy", val.astype(np.float64) / 7)
    assert np.array_equal(TP.read_record(str(tmp_path / "A00004"))[:, 0], val.astype(np.float64) / 7)
    assert np.array_equal(TP.read_record(str(tmp_path / "A00004.npy"))[:, 0], val.astype(np.float64) / 7)
    with pytest.raises(Exception):
        TP.read_record(str(tmp_path / "A09999"))


def test_label_maps_and_noise_filter(tmp_path):
    ref = tmp_path / "REFERENCE.csv"
    ref.write_text("A1,N\nA2,AF\nA3,~\nA4,O\nA5,N\nA6,~\n")
    assert TP.read_labels(str(ref)) == [("A1", 0), ("A2", 1), ("A4", 1), ("A5", 0)]
    assert TP.read_labels(str(ref), TM.LABEL_MAP) == [("A1", 0), ("A2", 1), ("A4", 2), ("A5", 0)]
    assert TP.LABEL_MAP == {"N": 0, "AF": 1, "O": 1} and TM.LABEL_MAP == {"N": 0, "AF": 1, "O": 2}


def test_load_records_skips_what_does_not_load(tmp_path):
    (tmp_path / "training2017").mkdir()
    val = np.arange(100)
    _write_record(tmp_path / "training2017", "A1", val, "1000/mV")
    _write_record(tmp_path / "training2017", "A4", 2 * val, "1000/mV")
    (tmp_path / "REFERENCE.csv").write_text("A1,N\nA2,AF\nA3,~\nA4,O\n")     # A2 has no files
    cfg = type("Cfg", (Config,), {"synthetic": False, "physionet_dir": str(tmp_path),
                                  "physionet_data_dir": str(tmp_path / "training2017"),
                                  "physionet_label_file": str(tmp_path / "REFERENCE.csv")})
    sig, lab = TP.load_records(cfg, TM.LABEL_MAP)
    assert lab.tolist() == [0, 2] and len(sig) == 2 and np.array_equal(sig[1], 2 * val / 1000.0)


@pytest.mark.parametrize("split,sizes", [(TP.SPLIT, (160, 20, 20)), (TM.SPLIT, (140, 20, 40))])
def test_stratified_split_sizes_and_determinism(split, sizes):
    from sklearn.model_selection import train_test_split
    labels = np.array([0] * 120 + [1] * 30 + [2] * 50)
    tr, va, te = TP.split_indices(labels, Config.seed, split)
    assert (len(tr), len(va), len(te)) == sizes
    assert sorted(np.concatenate([tr, va, te]).tolist()) == list(range(200))
    tr2, va2, te2 = TP.split_indices(labels, Config.seed, split)
    assert np.array_equal(tr, tr2) and np.array_equal(va, va2) and np.array_equal(te, te2)
    assert not np.array_equal(tr, TP.split_indices(labels, Config.seed + 1, split)[0])
    # the reference's two calls, restated
    idx = np.arange(200)
    r_tr, r_tmp, _, r_y = train_test_split(idx, labels, test_size=split[0], stratify=labels, random_state=Config.seed)
    r_va, r_te = train_test_split(r_tmp, test_size=split[1], stratify=r_y, random_state=Config.seed)
    assert np.array_equal(tr, r_tr) and np.array_equal(va, r_va) and np.array_equal(te, r_te)
    for part in (tr, va, te):    # stratified: class shares within one sample of 60 / 15 / 25 %
        share = np.bincount(labels[part], minlength=3) / len(part)
        assert np.all(np.abs(share - np.array([0.6, 0.15, 0.25])) <= 1.0 / len(part) + 1e-12)


def test_synthetic_records_are_variable_length_and_deterministic():
    cfg = type("Cfg", (Config,), {"synthetic": True, "synthetic_train_size": 20, "synthetic_val_size": 5,
                                  "synthetic_test_size": 5})
    sig, lab = TP.load_records(cfg, TM.LABEL_MAP)
    sig2, lab2 = TP.load_records(cfg, TM.LABEL_MAP)
    assert len(sig) == 30 and set(lab.tolist()) == {0, 1, 2} and np.array_equal(lab, lab2)
    assert all(2000 <= len(s) <= 18000 for s in sig) and len({len(s) for s in sig}) > 10
    assert all(np.array_equal(x, y) for x, y in zip(sig, sig2))
    assert set(TP.load_records(cfg, TP.LABEL_MAP)[1].tolist()) == {0, 1}


def test_preprocess_signal_refusals():
    x = torch.zeros(2, 3000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TP.preprocess_signal(x)
    with pytest.raises(NotImplementedError, match="resample_signal"):
        TP.preprocess_signal(x, orig_fs=500, target_fs=300)
    for fn in (TP.z_score_normalize, TP.bandpass_filter, TP.augment_signal):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TP.gather_augment(x, torch.zeros(1, dtype=torch.int64))


def test_find_best_threshold_as_the_reference_wrote_it():
    y_true = np.array([0, 1, 2, 2, 1, 0])
    y_prob = np.eye(3)[[0, 1, 2, 1, 1, 0]] * 0.8 + 0.1
    t = TM.find_best_threshold(y_true, y_prob, num_classes=3)
    assert len(t) == 3 and np.allclose(t, 0.1)       # argmax ignores the threshold: the first one wins
    assert TM.find_best_threshold(np.array([0, 0]), np.array([[0.1, 0.9, 0.0]] * 2)) == [0.5] * 3   # F1 0: the default


def test_new_entry_points_are_declared_bound_and_exported():
    import ctypes
    for name in ("ecgmm_signal_filter_zscore", "ecgmm_signal_gather_augment"):
        assert name in L.SIGNATURES
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.lib().ecgmm_version() == 100
    # argument checks run on the host, before any launch
    lib = L.lib()
    one = (ctypes.c_double * 2)(1.0, 0.0)
    assert lib.ecgmm_signal_filter_zscore(None, None, 1, 3000, one, one, one, 9, 1, 1e-8, None) != 0
    assert b"order" in lib.ecgmm_last_error()
    dummy = ctypes.c_void_p(16)
    assert lib.ecgmm_signal_filter_zscore(dummy, dummy, 1, 25000, one, one, one, 1, 1, 1e-8, None) != 0
    assert b"LDS" in lib.ecgmm_last_error()
    assert lib.ecgmm_signal_gather_augment(dummy, 4, 3000, dummy, 8, dummy, None, 1, 0.5, 0.01, 0.8, 1.2, 10, -10, 1, 0,
                                           None) != 0
    assert b"shift" in lib.ecgmm_last_error()
