"""Variable-length sequences without a GPU: the semantics the kernels are built to (a per-row masked hold equals torch's packed
LSTM, float64), HF.check_lengths, the refusals, and the length-aware spectrogram loader on CPU tensors."""
import numpy as np
import pytest
import torch

from ecgmm import train_physionet2 as T2
from ecgmm.crnn import CRNN
from ecgmm.hip import functional as HF
from ecgmm.hip import nn as HN
from ecgmm.spectrogram import stft_frames

from . import f64check as F64
from . import lstm_varlen_ref as V


@pytest.mark.parametrize("case,lengths", V.VARLEN_CASES, ids=V.VARLEN_IDS)
def test_masked_hold_is_torchs_packed_lstm(case, lengths):
    """Pins the SEMANTICS, not the kernels: it compares two restatements in tests/lstm_varlen_ref.py and calls no project code
    (so it also passes where the feature is missing; tests/test_lstm_varlen_gpu.py holds the kernels to packed_run).  Every
    tensor of the step-by-step masked hold within 1e-12 of torch's packed LSTM in float64, the padding of x and of the
    cotangent of y filled with values of size 1e3; y and dx exactly 0 at padded positions in both."""
    bf = case[6]
    ins = F64.lstm_inputs(case)
    ins = (ins[0], V.refill_padding(ins[1], lengths, bf, 1), ins[2], ins[3], V.refill_padding(ins[4], lengths, bf, 2)) + ins[5:]
    ref = V.packed_run(ins, lengths, torch.float64)
    got = V.masked_hold_run(ins, lengths, torch.float64)
    assert sorted(ref) == sorted(got)
    for k in ref:
        err = (got[k] - ref[k]).abs().max().item()
        assert err <= 1e-12, (k, err)
    pad = V.pad_mask(lengths, case[1], bf)
    for out in (ref, got):
        assert not out["y"][pad].any() and not out["dx"][pad].any()


def test_check_lengths_accepts_lists_and_cpu_integer_tensors():
    for src in ([3, 1, 5], (3, 1, 5), np.array([3, 1, 5]), torch.tensor([3, 1, 5]), torch.tensor([3, 1, 5], dtype=torch.int32)):
        out = HF.check_lengths(src, 3, 5)
        assert out.dtype == torch.int32 and out.tolist() == [3, 1, 5] and out.device.type == "cpu"


@pytest.mark.parametrize("lengths,B,T,word", [
    ([3, 2], 3, 5, "shape"), ([[3, 2, 1]], 3, 5, "shape"), (torch.tensor([3.0, 2.0, 1.0]), 3, 5, "integer"),
    ([3, 0, 1], 3, 5, r"lengths\[1\] = 0"), ([3, 2, 6], 3, 5, r"lengths\[2\] = 6"), (torch.tensor([-1, 2, 6]), 3, 5, r"lengths\[0\] = -1"),
])
def test_check_lengths_refusals_name_the_fault(lengths, B, T, word):
    with pytest.raises(ValueError, match=word):
        HF.check_lengths(lengths, B, T)


def test_packed_sequence_is_still_refused_and_points_to_lengths():
    m = HN.LSTM(8, 16, batch_first=True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(torch.zeros(2, 3, 8), [3, 2], batch_first=True)
    with pytest.raises(TypeError, match="PackedSequence") as e:
        m(packed)
    assert "lengths=" in str(e.value)


def test_cpu_tensors_are_refused_with_lengths_too():
    m = HN.LSTM(8, 16, batch_first=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 8), lengths=[3, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.lstm(torch.zeros(2, 3, 8), None, list(m.parameters()), 16, batch_first=True, lengths=[3, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.seq_mean(torch.zeros(2, 3, 8), lengths=[3, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CRNN()(torch.zeros(2, 1, 33, 16), [16, 9])


# ----------------------------------------------------------------------------------------------------------------------
# the loader, on CPU tensors
# ----------------------------------------------------------------------------------------------------------------------
def _dataset(with_frames, n=23, seed=5):
    rng = np.random.RandomState(seed)
    signals = [np.zeros(int(rng.randint(2700, 18300)), dtype=np.float32) for _ in range(n)]
    frames = T2.spectrogram_frames(signals)
    spec = torch.arange(n, dtype=torch.float32)[:, None, None, None].expand(n, 1, 33, int(frames.max())).contiguous()
    labels = rng.randint(0, 2, n)
    idx = rng.permutation(n)[:19]
    return signals, frames, spec, labels, idx, T2.SpectrogramDataset(idx, labels, spec, frames if with_frames else None)


def test_spectrogram_frames_are_stft_frames_of_each_record():
    signals, frames, *_ = _dataset(True)
    assert frames.dtype == np.int64 and frames.tolist() == [stft_frames(len(s)) for s in signals]
    assert frames.max() == stft_frames(max(len(s) for s in signals))


@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_with_frames_yields_sorted_batches_of_the_same_rows(shuffle):
    _, frames, spec, labels, idx, ds = _dataset(True)
    mk = lambda d, **kw: T2.DeviceSpectrogramLoader(d, 8, shuffle=shuffle, generator=torch.Generator().manual_seed(3), **kw)
    loader, plain = mk(ds), mk(ds, sort_by_length=False)
    assert loader.sort_by_length and len(loader) == 3
    seen = []
    for ((x, fr), y), ((xu, fru), yu) in zip(loader, plain):
        assert fr.dtype == torch.int32 and x.shape[0] == fr.shape[0] == y.shape[0]
        rows = x[:, 0, 0, 0].long()                      # the spectrogram of record i is filled with i
        assert torch.equal(fr.long(), torch.as_tensor(frames)[rows]) and torch.equal(y, torch.as_tensor(labels)[rows])
        assert bool((fr[1:] <= fr[:-1]).all()), fr
        # the same rows as the unsorted batch, in a stable descending order of it
        ru = xu[:, 0, 0, 0].long()
        assert sorted(ru.tolist()) == sorted(rows.tolist())
        assert torch.equal(rows, ru[torch.sort(fru, descending=True, stable=True).indices])
        seen += rows.tolist()
    assert sorted(seen) == sorted(idx.tolist())
    assert torch.equal(loader.last_order, plain.last_order)


def test_loader_without_frames_is_todays():
    _, _, spec, labels, idx, ds = _dataset(False)
    loader = T2.DeviceSpectrogramLoader(ds, 8)
    assert not loader.sort_by_length
    rows = []
    for x, y in loader:
        assert isinstance(x, torch.Tensor) and x.dim() == 4
        rows += x[:, 0, 0, 0].long().tolist()
    assert rows == idx.tolist()
    with pytest.raises(ValueError, match="frames"):
        T2.DeviceSpectrogramLoader(ds, 8, sort_by_length=True)


def test_dataset_refuses_frames_that_do_not_fit():
    _, frames, spec, labels, idx, _ = _dataset(True)
    with pytest.raises(ValueError, match="frames"):
        T2.SpectrogramDataset(idx, labels, spec, frames[:-1])
    with pytest.raises(ValueError, match="frames"):
        T2.SpectrogramDataset(idx, labels, spec, frames + 1)
