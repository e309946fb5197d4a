"""The attention maps and attention rollout without a GPU: the float64 restatement of tests/attn_maps_ref.py against torch's
own float64 ``multi_head_attention_forward(need_weights=True)``, the vector recursion of the rollout against the explicit
matrix product, the bounds against the fp32 rounding of the exact answer and against three named slips, the refusals, and the
new symbols in the header and the ctypes table."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip import nn as HN
from oracle import fill

from . import attn_bounds as AB
from . import attn_maps_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N, HEADS, HD = 21, 3, 4, 16
LENGTHS = [21, 16, 5]


def _qkv(salt=300, scale=1.0):
    return fill.hash_tensor((S * N, 3 * HEADS * HD), salt, scale)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("lengths", [None, LENGTHS])
def test_restatement_is_torchs_float64_attention_weights(lengths, average, bf):
    qkv = _qkv()
    m = MR.Maps(qkv, None, S, N, HEADS, bf, lengths)
    want = MR.torch_weights(qkv, lengths, S, N, HEADS, bf, average)
    got = m.weights(not average)
    live = m.live if average else m.live[:, None, :]
    err = ((got - want).abs() * live[..., None]).max()                     # the live query rows
    print("lengths %s average %s bf %s: max |restatement - torch f64| = %.3g" % (lengths, average, bf, float(err)))
    assert float(err) <= 1e-15
    if lengths is not None:      # our padded query rows and key columns are exact zeros; torch's padded key columns too
        assert bool((got * ~live[..., None] == 0).all()) and bool((got * ~live[..., None, :] == 0).all())
        assert bool((want * ~live[..., None, :] == 0).all())
    rows = got.sum(-1)
    assert float(((rows - 1.0).abs() * live).max()) <= 1e-14


@pytest.mark.parametrize("lengths", [None, LENGTHS])
@pytest.mark.parametrize("a", [0.5, 0.0, 0.25])
def test_vector_recursion_is_the_explicit_matrix_product(lengths, a):
    layers = [MR.Maps(_qkv(310 + i), None, S, N, HEADS, True, lengths) for i in range(3)]
    lens = torch.tensor(layers[0].lens, dtype=torch.float64)
    v0 = layers[0].live / lens[:, None]
    v = v0
    for m in reversed(layers):
        v = m.rollout_step(v, a)
    want = MR.rollout_by_matrices([m.matrix(a) for m in layers], v0)
    assert float((v - want).abs().max()) <= 1e-15
    assert float((v.sum(-1) - 1.0).abs().max()) <= 1e-14 and bool((v >= 0).all())
    assert bool((v[~layers[0].live] == 0).all())


def test_bounds_accept_the_fp32_rounding_and_reject_the_named_slips():
    qkv = _qkv()
    exact = MR.Maps(qkv, None, S, N, HEADS, True, LENGTHS)
    lse32 = exact.lse.float()                                  # a stored lse: the exact one rounded to fp32
    m = MR.Maps(qkv, lse32, S, N, HEADS, True, LENGTHS)
    v = fill.hash_tensor((N, S), 320, 1.0)
    v[~m.live] = float("nan")
    a = 0.5
    ok = {"per head": AB.ratio((m.P.float().double() - m.P).abs(), m.weights_bound(True)),
          "average": AB.ratio((m.average().float().double() - m.average()).abs(), m.weights_bound(False)),
          "rollout": AB.ratio((m.rollout_step(v, a).float().double() - m.rollout_step(v, a)).abs(), m.rollout_bound(v, a)),
          "row sums": AB.ratio((m.P.float().double().sum(-1) - m.live[:, None, :].double()).abs(), m.rowsum_bound(True)),
          "mass": AB.ratio((m.rollout_step(v, a).float().double().sum(-1) - m._v(v).sum(-1)).abs(), m.mass_bound(v, a))}
    print(ok)
    assert max(ok.values()) <= 1.0, ok
    # a row normalised with another head's lse
    other = MR.Maps(qkv, lse32.roll(1, dims=1), S, N, HEADS, True, LENGTHS)
    slips = {"another head's lse": AB.ratio((other.P - m.P).abs(), m.weights_bound(True)),
             "another head's lse, row sums": AB.ratio((other.P.sum(-1) - m.live[:, None, :].double()).abs(), m.rowsum_bound(True)),
             # the average over the wrong head count
             "wrong head count": AB.ratio((m.P.sum(1) / (HEADS + 1) - m.average()).abs(), m.weights_bound(False)),
             # a rollout step with the map transposed
             "transposed map": AB.ratio((a * m._v(v) + (1 - a) * torch.einsum("nj,nij->ni", m._v(v), m.average()) -
                                         m.rollout_step(v, a)).abs(), m.rollout_bound(v, a))}
    print(slips)
    for name, r in slips.items():
        assert r > 10.0, "the bound does not see: %s (%.3g)" % (name, r)


def test_head_average_restated_in_fp32_is_ordered():
    w = torch.rand(2, 3, 4, 4, generator=torch.Generator().manual_seed(1))
    got = MR.head_average_fp32(w)
    want = ((w[:, 0] + w[:, 1]) + w[:, 2]) * torch.tensor(np.float32(1.0) / np.float32(3.0))
    assert torch.equal(got, want) and got.dtype == torch.float32


def test_refusals():
    from ecgmm import explain
    from ecgmm.config import Config
    from ecgmm.train_physionet import ECGTransformer1D, main
    qkv, lse, v = torch.zeros(6, 192), torch.zeros(2 * 4 * 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.attention_weights(qkv, lse, 3, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.attention_rollout_step(qkv, lse, v, 3, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.multi_head_attention(qkv, 3, 2, 4, return_lse=True)
    for bad in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError, match="residual"):
            HF.attention_rollout_step(qkv, lse, v, 3, 2, 4, residual=bad)
        with pytest.raises(ValueError, match="residual"):
            explain.attention_rollout(ECGTransformer1D(seq_len=16, d_model=64, dim_feedforward=128, time_attention=True),
                                      torch.zeros(2, 1, 16), residual=bad)
    kw = dict(seq_len=16, d_model=64, dim_feedforward=128)
    with pytest.raises(ValueError, match="time_attention"):
        explain.attention_rollout(ECGTransformer1D(**kw), torch.zeros(2, 1, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain.attention_rollout(ECGTransformer1D(time_attention=True, **kw), torch.zeros(2, 1, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain.attention_maps(ECGTransformer1D(**kw), torch.zeros(2, 1, 16))
    for bad in (dict(model="resnet"), dict(model="transformer"), dict(model="resnet", time_attention=True)):
        with pytest.raises(ValueError, match="rollout_samples|time_attention"):
            main(Config, num_epochs=1, quiet=True, rollout_samples=2, **bad)
    with pytest.raises(ValueError, match="rollout_samples"):
        main(Config, num_epochs=1, quiet=True, model="transformer", time_attention=True, rollout_samples=-1)
    # the torch-named keyword stays refused: the forward never forms the weights
    mha = HN.MultiheadAttention(64, 4)
    with pytest.raises(ValueError, match="need_weights"):
        mha(torch.zeros(3, 2, 64), need_weights=True)


def test_c_entry_points_refuse_before_any_launch():
    """no GPU is needed for a refusal: the descriptor, the null operands and the residual are checked on the host"""
    lib = L.lib()
    buf = torch.zeros(64)                                        # 16-byte aligned host memory that is never touched
    p = C.c_void_p(buf.data_ptr())
    assert buf.data_ptr() % 16 == 0
    d = L.MHADesc(3, 2, 4, 16, 0, 0.0)
    for bad in (1.0, -0.25, float("nan")):
        assert lib.ecgmm_mha_rollout_step(C.byref(d), p, p, None, p, C.c_void_p(buf.data_ptr() + 64), bad, None) == 1
        assert b"residual" in lib.ecgmm_last_error()
    assert lib.ecgmm_mha_rollout_step(C.byref(d), p, p, None, p, p, 0.5, None) == 1           # in place
    assert lib.ecgmm_mha_rollout_step(C.byref(d), p, None, None, p, p, 0.5, None) == 1
    assert lib.ecgmm_mha_weights(C.byref(d), p, p, None, None, 0, None) == 1
    assert lib.ecgmm_mha_weights(C.byref(d), p, p, None, p, 2, None) == 1
    assert b"per_head" in lib.ecgmm_last_error()
    for bad in (L.MHADesc(0, 2, 4, 16, 0, 0.0), L.MHADesc(3, 2, 4, 24, 0, 0.0), L.MHADesc(3, 2, 4, 16, 2, 0.0)):
        assert lib.ecgmm_mha_weights(C.byref(bad), p, p, None, p, 0, None) == 1
        assert lib.ecgmm_mha_rollout_step(C.byref(bad), p, p, None, p, p, 0.5, None) == 1
    assert not bool(buf.any())


WEIGHTS = ("int ecgmm_mha_weights(const ecgmm_mha_desc* d, const float* qkv, const float* lse, const int32_t* lengths, "
           "float* weights, int per_head, void* stream);")
STEP = ("int ecgmm_mha_rollout_step(const ecgmm_mha_desc* d, const float* qkv, const float* lse, const int32_t* lengths, "
        "const float* v_in, float* v_out, float residual, void* stream);")


def test_entry_points_declared_bound_and_exported():
    full = open(os.path.join(ROOT, "include", "ecgmm.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", full, flags=re.S))
    assert WEIGHTS in flat and STEP in flat
    for name in ("ecgmm_mha_weights", "ecgmm_mha_rollout_step"):      # each cites the reference lines it serves
        before = full[:full.index("int " + name + "(")]
        last = before[before.rindex("/*"):]
        assert "train_physionet.py:219-220, 236" in last and "multimodal_paper_modal_balance.py:133-140" in last, name
    h = C.CDLL(L.LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    d = C.POINTER(L.MHADesc)
    want = {"ecgmm_mha_weights": (i32, [d, vp, vp, vp, vp, i32, vp]),
            "ecgmm_mha_rollout_step": (i32, [d, vp, vp, vp, vp, vp, f32, vp])}
    for name, (res, args) in want.items():
        assert hasattr(h, name), name + " is not exported"
        got = L.SIGNATURES[name]
        assert got[0] is res and list(got[1]) == args, name
    assert L.lib().ecgmm_version() == 100


def test_python_layers_take_a_sink():
    from ecgmm import explain
    from ecgmm.train_physionet import ECGTransformer1D, main
    p = inspect.signature(HF.multi_head_attention).parameters
    assert p["return_lse"].default is False and p["return_lse"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (HN.TransformerEncoderLayer, HN.TransformerEncoder):
        q = inspect.signature(cls.forward).parameters["attention_sink"]
        assert q.kind is inspect.Parameter.KEYWORD_ONLY and q.default is None, cls.__name__
    q = inspect.signature(HN.MultiheadAttention.attention_weights).parameters
    assert q["lengths"].kind is inspect.Parameter.KEYWORD_ONLY and q["average_attn_weights"].default is True
    assert inspect.signature(ECGTransformer1D.forward).parameters["attention_sink"].default is None
    assert inspect.signature(main).parameters["rollout_samples"].default == 0
    assert inspect.signature(explain.attention_maps).parameters["average"].default is True
    assert inspect.signature(explain.attention_rollout).parameters["residual"].default == 0.5
    assert inspect.signature(HF.attention_weights).parameters["average"].default is True
    assert inspect.signature(HF.attention_rollout_step).parameters["residual"].default == 0.5
