"""PTB-XL trainer, host side (no GPU): the WFDB format-16 reader, labels, split, class weights, sampler and argument refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ecgmm import train_signal_only_ptb as TS
from ecgmm.config import Config
from ecgmm.hip import lib as L
from ecgmm.train_physionet import split_indices

from . import ptbxl_util as U


def test_reader_round_trip_twelve_signals(tmp_path):
    d, gain, base = U.make_frames(1, 1, 1000, 12)
    path = str(tmp_path / "rec" / "00001_hr")
    U.write_record(path, d[0], gain[0], base[0])
    h = TS.read_header(path)
    assert (h["n_sig"], h["sig_len"], h["fs"], h["file_name"]) == (12, 1000, 500.0, "00001_hr.dat")
    assert np.array_equal(h["gain"], gain[0]) and np.array_equal(h["baseline"], base[0]) and (base[0] != 0).all()
    assert h["sig_name"] == U.LEADS and h["units"] == ["mV"] * 12
    frames, _ = TS.read_record_i16(path)
    assert frames.dtype == np.int16 and frames.shape == (1000, 12) and np.array_equal(frames, d[0])
    p, fields = TS.rdsamp(path)
    assert p.dtype == np.float64 and np.array_equal(p, (d[0].astype(np.float64) - base[0]) / gain[0])
    assert fields["fs"] == 500.0 and fields["sig_len"] == 1000 and fields["n_sig"] == 12


def test_rdsamp_one_channel_is_the_formula(tmp_path):
    d, gain, base = U.make_frames(2, 1, 600, 12)
    d[0, 5, 1] = -32768
    path = str(tmp_path / "r")
    U.write_record(path, d[0], gain[0], base[0])
    p, fields = TS.rdsamp(path, channels=[1])
    want = (d[0, :, 1].astype(np.float64) - base[0, 1]) / gain[0, 1]
    assert p.shape == (600, 1) and fields["sig_name"] == ["II"]
    assert np.isnan(p[5, 0]) and np.array_equal(np.delete(p[:, 0], 5), np.delete(want, 5))   # the invalid-sample code -> NaN
    with pytest.raises(ValueError, match="channels"):
        TS.rdsamp(path, channels=[12])


def test_header_defaults(tmp_path):
    d = (np.arange(40, dtype=np.int16) - 20).reshape(20, 2)
    d.astype("<i2").tofile(str(tmp_path / "r.dat"))
    (tmp_path / "r.hea").write_text("r 2 250 20\nr.dat 16\nr.dat 16 0(5)/uV 12 7\n")
    h = TS.read_header(str(tmp_path / "r"))
    assert list(h["gain"]) == [200.0, 200.0] and list(h["baseline"]) == [0, 5] and h["units"] == ["mV", "uV"]
    (tmp_path / "r.hea").write_text("r 2 250 20\nr.dat 16 100\nr.dat 16 50/mV 12 7\n")
    assert list(TS.read_header(str(tmp_path / "r"))["baseline"]) == [0, 7]                     # baseline = ADC zero
    p, _ = TS.rdsamp(str(tmp_path / "r"))
    assert np.array_equal(p[:, 1], (d[:, 1] - 7) / 50.0)


def test_reader_refusals(tmp_path):
    d, gain, base = U.make_frames(3, 1, 300, 3)
    ok = str(tmp_path / "ok")
    U.write_record(ok, d[0], gain[0], base[0])
    TS.read_record_i16(ok)
    sums = [int(d[0, :, c].astype(np.int64).sum() % 65536) for c in range(3)]
    bad = str(tmp_path / "badsum")
    U.write_record(bad, d[0], gain[0], base[0], checksum=[sums[0], (sums[1] + 1) % 65536, sums[2]])
    with pytest.raises(ValueError, match="checksum"):
        TS.read_record_i16(bad)
    assert np.array_equal(TS.read_record_i16(bad, verify=False)[0], d[0])
    signed = str(tmp_path / "signed")                           # the WFDB library writes the checksum as a signed 16-bit number
    U.write_record(signed, d[0], gain[0], base[0], checksum=[s - 65536 if s >= 32768 else s for s in sums])
    TS.read_record_i16(signed)
    bad = str(tmp_path / "badinit")
    U.write_record(bad, d[0], gain[0], base[0], init=[int(d[0, 0, 0]), int(d[0, 0, 1]), int(d[0, 0, 2]) + 1])
    with pytest.raises(ValueError, match="starts with"):
        TS.read_record_i16(bad)
    for fmt in ("212", "80", "16x2", "16:1", "16+24", "24"):
        bad = str(tmp_path / "fmt")
        U.write_record(bad, d[0], gain[0], base[0], fmt=fmt)
        with pytest.raises(ValueError, match="format"):
            TS.read_header(bad)
    (tmp_path / "seg.hea").write_text("seg/3 2 500 1000\n")
    with pytest.raises(ValueError, match="multi-segment"):
        TS.read_header(str(tmp_path / "seg"))
    (tmp_path / "two.hea").write_text("two 2 500 10\na.dat 16 200\nb.dat 16 200\n")
    with pytest.raises(ValueError, match="several files"):
        TS.read_header(str(tmp_path / "two"))
    short = str(tmp_path / "short")
    U.write_record(short, d[0], gain[0], base[0])
    d[0, :200].astype("<i2").tofile(short + ".dat")
    with pytest.raises(ValueError, match="declares"):
        TS.read_record_i16(short)


@pytest.mark.parametrize("scp,want", [({"AFIB": 100.0}, 1), ({"AFIB": 100.0, "SR": 100.0}, 1), ({"AFIB": 50.0, "SR": 100.0}, 0),
                                      ({"AFIB": 0.0, "STACH": 100.0}, 0), ({"NORM": 100.0}, 2), ("garbage", 2), (None, 2),
                                      ("{'AFIB': 100.0}", 1), ({"SR": "x"}, 2), (float("nan"), 2), ({"TRIGU": 100}, 0)])
def test_label_ecg(scp, want):
    assert TS.label_ecg(scp) == want


def test_load_ptbxl_reads_the_table(tmp_path):
    kept = U.write_tree(str(tmp_path), n=12)
    cfg = type("C", (Config,), {"synthetic": False, "ptbxl_dir": str(tmp_path),
                                "ptbxl_database": str(tmp_path / "ptbxl_database.csv")})
    records, labels = TS.load_ptbxl(cfg)
    assert len(records) == 12 and labels.dtype == np.int64 and labels.tolist() == [k[3] for k in kept]
    assert records[0] == os.path.join(str(tmp_path), "records500/00000/00001_hr")
    assert np.array_equal(TS.read_record_i16(records[7])[0], kept[7][0]) and kept[7][0].shape == (3000, 12)
    assert Config.ptbxl_dir == "./data/ptb_xl" and Config.ptbxl_database == os.path.join("./data/ptb_xl", "ptbxl_database.csv")


def test_synthetic_records():
    cfg = type("S", (Config,), {"synthetic": True, "synthetic_train_size": 10, "synthetic_val_size": 3, "synthetic_test_size": 3})
    records, labels = TS.load_ptbxl(cfg)
    assert len(records) == 16 and set(labels.tolist()) == {0, 1}
    assert all(r["frames"].dtype == np.int16 and r["frames"].shape == (5000, 12) for r in records)


def test_split_is_the_reference_split():
    from sklearn.model_selection import train_test_split
    labels = np.array(([1] + [0] * 4) * 40)
    records = [f"./data/ptb_xl/records500/{i:05d}_hr" for i in range(len(labels))]
    tr, va, te = split_indices(labels, 42, TS.SPLIT)
    assert (len(tr), len(va), len(te)) == (120, 40, 40)
    X_train, X_temp, y_train, y_temp = train_test_split(records, labels, test_size=0.4, stratify=labels, random_state=42)
    X_val, X_test, y_val, y_test = train_test_split(X_temp, y_temp, test_size=0.5, stratify=y_temp, random_state=42)
    assert [records[i] for i in tr] == X_train and [records[i] for i in va] == X_val and [records[i] for i in te] == X_test
    assert np.array_equal(labels[tr], y_train) and np.array_equal(labels[te], y_test)


def test_class_weights_as_the_reference():
    y_train = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0])
    class_sample_count = np.array([len(np.where(y_train == t)[0]) for t in np.unique(y_train)])
    weight = 1. / class_sample_count
    samples_weight = np.array([weight[t] for t in y_train])
    got = TS.class_weights(y_train)
    assert got.dtype == np.float64 and np.array_equal(got, samples_weight)
    assert abs(got[y_train == 1].sum() - got[y_train == 0].sum()) < 1e-12        # the classes are drawn equally often


@pytest.mark.parametrize("weights", [[0.5, -0.1, 0.2], [0.5, float("nan"), 0.2], [0.5, float("inf")], [0.0, 0.0, 0.0], []])
def test_sampler_refuses_what_torch_refuses(weights):
    with pytest.raises(ValueError, match="weight"):
        TS.DeviceWeightedSampler(weights, 4)


def test_sampler_host_side():
    s = TS.DeviceWeightedSampler(torch.tensor([0.0, 0.25, 0.0, 0.5, 0.0, 0.0]), 7, device="cpu")
    assert len(s) == 7 and s.last_positive == 3 and np.array_equal(s.cdf_host, [0.0, 0.25, 0.25, 0.75, 0.75, 0.75])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.sample()
    with pytest.raises(ValueError, match="num_samples"):
        TS.DeviceWeightedSampler([1.0], 0)


class _Rows:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_scheduler_spans_thirty_epochs_of_the_weighted_loader():
    n = 203
    loader = TS.PTBXLLoader(_Rows(n), 16, sampler=TS.DeviceWeightedSampler(np.ones(n), n, device="cpu"))
    assert len(loader) == 13
    assert len(TS.PTBXLLoader(_Rows(n), 16, sampler=TS.DeviceWeightedSampler(np.ones(n), 40, device="cpu"))) == 3
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = TS.make_scheduler(opt, len(loader))
    assert sched.total_steps == 30 * len(loader)
    with pytest.raises(ValueError, match="mutually exclusive"):
        TS.PTBXLLoader(_Rows(n), 16, shuffle=True, sampler=TS.DeviceWeightedSampler(np.ones(n), n, device="cpu"))


def test_dataset_refuses_the_cpu():
    d, gain, base = U.make_frames(4, 1, 600, 12)
    rec = dict(frames=d[0], gain=gain[0], baseline=base[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TS.PTBXLSignalDataset([rec], [0], device="cpu")
    from ecgmm import preprocess as PP
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.preprocess_i16(torch.zeros(1, 600, 12, dtype=torch.int16), [1], gain[:, :1], base[:, :1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.weighted_sample(torch.ones(3, dtype=torch.float64), 2, 4)


def test_entry_points_check_their_arguments_before_any_launch():
    """every refusal returns before the first HIP call, so it can be exercised without a device (the pointers are never read)"""
    lib = L.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    b5 = (C.c_double * 6)(*([0.1] * 6))
    a5 = (C.c_double * 6)(1.0, *([0.1] * 5))
    zi = (C.c_double * 5)()
    ch = lambda *v: (C.c_int * len(v))(*v)

    def pre(R=1, T=5000, nsig=12, chan=ch(1), nc=1, step=2, out_len=2476, window=200, a=a5, order=5):
        return lib.ecgmm_signal_preprocess_i16(p, R, T, nsig, chan, nc, p, p, step, p, out_len, window, b5, a, zi, order, None)

    for kw, word in ((dict(chan=ch(12)), b"channel"), (dict(chan=ch(0, -1), nc=2), b"channel"), (dict(T=398), b"window"),
                     (dict(T=30, window=1), b"3*(order+1)"), (dict(T=9934, step=1), b"LDS"), (dict(T=2 * 9934, step=2), b"LDS"),
                     (dict(out_len=0), b"out_len"), (dict(step=0), b"step"), (dict(nc=17), b"nc"), (dict(order=8), b"order"),
                     (dict(a=(C.c_double * 6)(2.0, *([0.1] * 5))), b"a[0]")):
        assert pre(**kw) == 1, kw                                        # ECGMM_ERR_SHAPE
        assert word in lib.ecgmm_last_error(), (kw, lib.ecgmm_last_error())
    ws = lambda n=10, last=9, count=5: lib.ecgmm_weighted_sample(p, n, last, p, None, count, 1, 0, None)
    for kw in (dict(n=0), dict(last=10), dict(last=-1), dict(count=0), dict(count=2 ** 31)):
        assert ws(**kw) == 1, kw
    assert lib.ecgmm_weighted_sample(None, 10, 9, p, None, 5, 1, 0, None) == 1
