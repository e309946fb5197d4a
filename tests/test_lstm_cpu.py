"""ecgmm.hip.nn.LSTM without a GPU: torch's parameter layout and initialisation, the refusals, the workspace queries."""
import ctypes as C
import math

import pytest
import torch

from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip import nn as HN


@pytest.mark.parametrize("layers,bi", [(1, False), (2, True), (3, True)])
def test_parameter_names_shapes_and_order_are_torchs(layers, bi):
    ours = HN.LSTM(12, 10, layers, batch_first=True, bidirectional=bi)
    ref = torch.nn.LSTM(12, 10, layers, batch_first=True, bidirectional=bi)
    assert [(n, tuple(p.shape)) for n, p in ours.named_parameters()] == [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    ref.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(ref.state_dict(), strict=True)
    for (n, p), (_, q) in zip(ours.named_parameters(), ref.named_parameters()):
        assert torch.equal(p, q), n


def test_init_is_uniform_within_one_over_sqrt_h():
    torch.manual_seed(0)
    m = HN.LSTM(8, 25, 2, bidirectional=True)
    bound = 1 / math.sqrt(25)
    for n, p in m.named_parameters():
        assert p.abs().max().item() <= bound, n
        assert p.min().item() < p.max().item(), n
        assert p.abs().max().item() > 0.5 * bound, n


@pytest.mark.parametrize("kw,name", [({"dropout": 0.3}, "dropout"), ({"proj_size": 4}, "proj_size"), ({"bias": False}, "bias")])
def test_unsupported_constructor_arguments_are_named(kw, name):
    with pytest.raises(ValueError, match=name):
        HN.LSTM(8, 16, **kw)


def test_packed_sequence_and_unbatched_input_are_refused():
    m = HN.LSTM(8, 16, batch_first=True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(torch.zeros(2, 3, 8), [3, 2], batch_first=True)
    with pytest.raises(TypeError, match="PackedSequence"):
        m(packed)
    with pytest.raises(ValueError, match="unbatched"):
        m(torch.zeros(3, 8))


def test_cpu_tensors_are_refused():
    m = HN.LSTM(8, 16, batch_first=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.lstm(torch.zeros(2, 3, 8), None, list(m.parameters()), 16, batch_first=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.seq_mean(torch.zeros(2, 3, 8))


def _ws(B=8, T=70, In=512, H=200, layers=3, bi=1, bf=1, save=1):
    d = L.LSTMDesc(B, T, In, H, layers, bi, bf, save)
    lib = L.lib()
    return lib.ecgmm_lstm_fwd_workspace(C.byref(d)), lib.ecgmm_lstm_bwd_workspace(C.byref(d))


def test_workspace_queries_run_without_a_gpu():
    f, b = _ws()
    assert f > 8 * 70 * (4 * 200 + 200) * 4 * 6 and b > 8 * 70 * 800 * 4 * 2   # gates + c of 6 layer-directions; dgates of 2
    f2, b2 = _ws(B=16)
    f3, b3 = _ws(T=71)
    assert f2 > f and b2 > b and f3 > f and b3 > b
    f0, _ = _ws(save=0)
    assert 0 < f0 < f


def test_bad_descriptors_return_zero_with_a_message():
    lib = L.lib()
    assert _ws(H=385) == (0, 0)
    assert b"cap of 384" in lib.ecgmm_last_error()
    assert _ws(H=384)[0] > 0 and _ws(H=256)[0] > 0
    assert _ws(layers=0) == (0, 0)
    assert b"layers" in lib.ecgmm_last_error()
    assert _ws(B=0) == (0, 0)


def test_grad_wanted_follows_what_the_backward_pass_was_asked_for():
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            ctx.w = w
            return x * w.detach()

        @staticmethod
        def backward(ctx, dy):
            seen.append(HF._grad_wanted(ctx.w))
            return dy, None

    w = torch.nn.Parameter(torch.ones(3))
    x = torch.ones(3, requires_grad=True)
    torch.autograd.grad(Probe.apply(x, w).sum(), x)
    Probe.apply(x, w).sum().backward()
    Probe.apply(x, w).sum().backward(inputs=[x])
    assert seen == [False, True, False]
