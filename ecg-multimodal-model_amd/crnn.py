"""The spectrogram CRNN of the reference's train_physionet2.py:55-96 on the HIP kernels: three 5x5 ConvBlocks (one launch
plan, csrc/plan_crnn.hip), a 3-layer bidirectional LSTM, the mean over time and a two-layer classifier.  Parameter names,
shapes, registration order and initialisation are torch's, so ``state_dict``s move in both directions with the reference's
``CRNN``."""
import torch
import torch.nn as nn

from .hip import functional as HF
from .hip import nn as HN
from .hip.encoders import dtype_code
from .signal_model import FocalLoss  # noqa: F401  (train_physionet2.py:103-117; re-exported)


class ConvBlock(nn.Module):
    """Conv2d(k=5, pad=2) -> BatchNorm2d -> ReLU -> MaxPool2d(2) (train_physionet2.py:55-65); executed only by its parent's
    plan, like the encoders' layers."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.block = nn.Sequential(HN.Conv2d(in_channels, out_channels, 5, padding=2), HN.BatchNorm2d(out_channels),
                                   nn.ReLU(), nn.MaxPool2d(2))

    def forward(self, x):
        raise RuntimeError("ConvBlock is executed by its parent CRNN's fused launch plan; call the CRNN, not the block")


class CRNN(nn.Module):
    def __init__(self, input_channels=1, num_classes=2, compute_dtype="fp32", lstm_dtype=None):
        """``compute_dtype``: the three ConvBlocks.  ``lstm_dtype``: the BiLSTM's recurrent products, ``None`` = ``"fp32"``
        whatever ``compute_dtype`` is (``"bf16"``: :class:`ecgmm.hip.nn.LSTM` with ``compute_dtype="bf16"``)."""
        super().__init__()
        if input_channels != 1:
            raise ValueError(f"CRNN: input_channels={input_channels} is not supported: the first convolution's kernel takes "
                             "the one-channel log-spectrogram (train_physionet2.py:70 with its default)")
        self.compute_dtype = compute_dtype
        self._dtype = dtype_code(compute_dtype)
        self.conv1 = ConvBlock(input_channels, 32)
        self.conv2 = ConvBlock(32, 64)
        self.conv3 = ConvBlock(64, 128)
        self.flatten = nn.Flatten(start_dim=2)
        self.lstm_dtype = "fp32" if lstm_dtype is None else str(lstm_dtype).lower()
        self.bilstm = HN.LSTM(512, 200, 3, batch_first=True, bidirectional=True, compute_dtype=self.lstm_dtype)
        self.classifier = HN.Sequential(HN.Linear(400, 64), nn.ReLU(), nn.Dropout(0.3), HN.Linear(64, num_classes))

    def _front_tables(self):
        params, buffers = [], []
        for blk in (self.conv1, self.conv2, self.conv3):
            conv, bn = blk.block[0], blk.block[1]
            params += [conv.weight, conv.bias, bn.weight, bn.bias]
            buffers += [bn.running_mean, bn.running_var, bn.num_batches_tracked]
        return params, buffers

    def forward(self, x, lengths=None):
        """``x [B, 1, F, T]``.  ``lengths``: the valid spectrogram frames of each record (``x`` zero-padded behind them).
        The LSTM and the mean over time then take ``clamp(lengths // 8, 1, T // 8)`` steps per record -- three floor pools
        give exactly ``// 8`` -- so the recurrence neither runs through the padding nor averages it in.  The convolution
        front end and its BatchNorm statistics stay as they are, padding included: that is the reference's arithmetic.
        An ``x`` that requires a gradient gets it, in training and in eval mode (``explain.spectrogram_gradients``)."""
        return self._tail(self._front(x), lengths, x.shape[3])[0]

    def _front(self, x):
        """conv1..conv3 + permute + Flatten as one launch plan: ``x [B, 1, F, T]`` -> ``seq [B, T // 8, 512]`` fp32"""
        if not x.is_cuda:
            raise RuntimeError(f"CRNN: tensor is on {x.device}; the HIP library is the only compute path (no CPU fallback) "
                               "-- move the model and inputs to a ROCm device")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"CRNN expects a log-spectrogram [B,1,F,T], got {tuple(x.shape)}")
        F = x.shape[2]
        if 128 * (F // 8) != self.bilstm.input_size:
            raise ValueError(f"CRNN: F={F} frequency bins give {128 * (F // 8)} features per time step after three 2x2 "
                             f"pools, but the LSTM takes {self.bilstm.input_size} (F must be 32..39)")
        if x.shape[3] < 8:
            raise ValueError(f"CRNN: T={x.shape[3]} time bins; three 2x2 pools need at least 8")
        params, buffers = self._front_tables()
        bn = self.conv1.block[1]
        return HF.crnn_front(x, params, buffers, self.training, bn.momentum, bn.eps, self._dtype)

    def _tail(self, seq, lengths, frames):
        """Everything behind the front end: BiLSTM, mean over time, classifier on ``seq [B, T // 8, 512]`` of a spectrogram
        of ``frames`` = T columns -> (logits, the int32 live steps per record or None).  ``forward`` ends in it, and
        ``explain.spectrogram_grad_cam`` starts a graph at ``seq`` with it."""
        if lengths is None:
            out, _ = self.bilstm(seq)
            return self.classifier(HF.seq_mean(out)), None
        steps = seq.shape[1]
        lengths = HF.check_lengths(lengths, seq.shape[0], frames).to(seq.device)
        lengths = torch.clamp(lengths // 8, 1, steps).to(torch.int32)
        out, _ = self.bilstm(seq, lengths=lengths)
        return self.classifier(HF.seq_mean(out, lengths)), lengths
