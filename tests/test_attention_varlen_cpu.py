"""CPU-side checks of lengths in the attention path: the two _varlen entry points are declared, bound and exported with the
documented signatures; the Python layers carry a ``lengths`` parameter; ``ECGTransformer1D(time_attention=True)`` keeps the
default's state_dict and loads the reference's golden; what must be refused is refused; and the float64 reference of the GPU
tests (tests/attn_varlen_ref.py: every element alone, trimmed) agrees with torch's own ``key_padding_mask``."""
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

from . import attn_varlen_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("int ecgmm_mha_forward_varlen(const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, float* out, "
       "float* lse, uint64_t seed, uint64_t offset, void* stream);")
BWD = ("int ecgmm_mha_backward_varlen(const ecgmm_mha_desc* d, const float* qkv, const int32_t* lengths, const float* out, "
       "const float* lse, const float* dout, float* dqkv, void* ws, size_t ws_bytes, uint64_t seed, uint64_t offset, "
       "void* stream);")


def test_varlen_entry_points_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecgmm.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    assert FWD in flat and BWD in flat
    h = C.CDLL(L.LIB_PATH)
    vp, u64, sz, i32 = C.c_void_p, C.c_uint64, C.c_size_t, C.c_int32
    d = C.POINTER(L.MHADesc)
    want = {"ecgmm_mha_forward_varlen": (i32, [d, vp, vp, vp, vp, u64, u64, vp]),
            "ecgmm_mha_backward_varlen": (i32, [d, vp, vp, vp, vp, vp, vp, vp, sz, u64, u64, vp])}
    for name, (res, args) in want.items():
        assert hasattr(h, name), name + " is not exported"
        got = L.SIGNATURES[name]
        assert got[0] is res and list(got[1]) == args, name
    full = open(os.path.join(ROOT, "include", "ecgmm.h")).read()
    assert "No attention or key-padding mask." not in full


def test_python_layers_take_lengths():
    from ecgmm.train_physionet import ECGTransformer1D, build_model, main
    p = inspect.signature(HF.multi_head_attention).parameters
    assert list(p)[-1] == "lengths" and p["lengths"].default is None
    for cls in (HN.MultiheadAttention, HN.TransformerEncoderLayer, HN.TransformerEncoder):
        q = inspect.signature(cls.forward).parameters["lengths"]
        assert q.kind is inspect.Parameter.KEYWORD_ONLY and q.default is None, cls.__name__
    assert inspect.signature(ECGTransformer1D.forward).parameters["lengths"].default is None
    assert inspect.signature(ECGTransformer1D.__init__).parameters["time_attention"].default is False
    assert inspect.signature(build_model).parameters["time_attention"].default is False
    m = inspect.signature(main).parameters
    assert m["time_attention"].default is False and m["use_lengths"].default is False
    from ecgmm.config import Config
    assert Config.physionet_time_attention is False and Config.physionet_use_lengths is False


def test_time_attention_keeps_the_state_dict_and_loads_the_golden(golden_dir):
    from ecgmm.train_physionet import ECGTransformer1D
    kw = dict(seq_len=48, d_model=64, nhead=4, num_layers=2, dim_feedforward=128)
    a, b = ECGTransformer1D(**kw), ECGTransformer1D(time_attention=True, **kw)
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    z = np.load(os.path.join(golden_dir, "g11_transformer.npz"))
    assert [str(k) for k in z["keys"]] == list(b.state_dict())
    b.load_state_dict({str(k): torch.from_numpy(z["sd/" + str(k)]) for k in z["keys"]}, strict=True)
    assert all(layer.self_attn.batch_first for layer in b.transformer_encoder.layers)
    assert not any(layer.self_attn.batch_first for layer in a.transformer_encoder.layers)
    assert b.time_attention and not a.time_attention


def test_refusals():
    from ecgmm.config import Config
    from ecgmm.train_physionet import ECGTransformer1D, build_model, main
    kw = dict(seq_len=16, d_model=64, dim_feedforward=128)
    x = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="time_attention"):
        ECGTransformer1D(**kw)(x, lengths=[16, 3])
    timed = ECGTransformer1D(time_attention=True, **kw)
    for bad, word in (([16, 3, 2], "shape"), (torch.tensor([16.0, 3.0]), "dtype"), ([0, 16], "outside"), ([16, 17], "outside")):
        with pytest.raises(ValueError, match=word):
            timed(x, lengths=bad)
    qkv = torch.zeros(6, 192)
    for bad, word in (([3], "shape"), (torch.tensor([1.5, 2.0]), "dtype"), ([0, 3], "outside"), ([3, 4], "outside")):
        with pytest.raises(ValueError, match=word):
            HF.multi_head_attention(qkv, 3, 2, 4, lengths=bad)
    s = torch.zeros(3, 2, 64)                                  # [S, N, E]: one length per n, at most S
    layer, mha = HN.TransformerEncoderLayer(64, 4, 128), HN.MultiheadAttention(64, 4)
    for mod in (layer, mha, HN.TransformerEncoder(layer, 2)):
        with pytest.raises(ValueError, match="shape"):
            mod(s, lengths=[3, 3, 3])
        with pytest.raises(ValueError, match="outside"):
            mod(s, lengths=[4, 1])
    with pytest.raises(ValueError, match="outside"):          # batch_first: N = dimension 0, S = dimension 1
        HN.MultiheadAttention(64, 4, batch_first=True)(s, lengths=[2, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mha(s, lengths=[3, 1])
    # the torch-named arguments stay refused
    with pytest.raises(ValueError, match="key_padding_mask"):
        mha(s, key_padding_mask=torch.zeros(2, 3, dtype=torch.bool), lengths=[3, 1])
    with pytest.raises(ValueError, match="src_key_padding_mask"):
        layer(s, src_key_padding_mask=torch.zeros(2, 3, dtype=torch.bool))
    for kwargs in (dict(time_attention=True), dict(use_lengths=True), dict(time_attention=True, use_lengths=True)):
        with pytest.raises(ValueError, match="transformer"):
            main(Config, num_epochs=1, quiet=True, model="resnet", **kwargs)
    with pytest.raises(ValueError, match="time_attention"):
        main(Config, num_epochs=1, quiet=True, model="transformer", use_lengths=True)
    with pytest.raises(ValueError, match="transformer"):
        build_model("resnet", time_attention=True)


CASES = [(19, 4, 4, 16, False, [19, 7, 1, 16]), (19, 4, 4, 16, True, [19, 7, 1, 16]), (33, 3, 2, 32, True, [17, 33, 32]),
         (5, 5, 2, 16, False, [5, 1, 4, 2, 3])]


@pytest.mark.parametrize("S,N,heads,hd,bf,lengths", CASES, ids=["S%d_N%d_h%d_d%d_bf%d" % c[:5] for c in CASES])
def test_row_alone_reference_agrees_with_torch_key_padding_mask(S, N, heads, hd, bf, lengths):
    E = heads * hd
    qkv = fill.hash_tensor((S * N, 3 * E), 905, 1.0)
    dout = fill.hash_tensor((S * N, E), 906, 1.0)
    live = VR.live_rows(lengths, S, N, bf)
    assert 0 < int(live.sum()) < S * N
    fs = VR.forward_alone(qkv, lengths, S, N, heads, bf)
    out, lse = VR.scatter_forward(fs, lengths, S, N, heads, bf)
    bs = VR.backward_alone(qkv, out, lse, dout, lengths, S, N, heads, bf)
    dqkv = VR.scatter_backward(bs, lengths, S, N, bf)
    t_out, t_dqkv = VR.torch_masked(qkv, dout, lengths, S, N, heads, bf)
    e_out = float((out - t_out)[live].abs().max())
    e_dqkv = float((dqkv - t_dqkv)[live].abs().max())
    print("row-alone reference against torch float64: out %.3g  dqkv %.3g" % (e_out, e_dqkv))
    assert e_out <= 1e-12 and e_dqkv <= 1e-12
    # the padding of the scattered reference is zero, and torch's gradient there is zero too (dout zeroed, never a key)
    assert float(out[~live].abs().max()) == 0 and float(dqkv[~live].abs().max()) == 0 and float(lse.abs().min()) == 0
    assert float(t_dqkv[~live].abs().max()) == 0
    # the mask matters: the unmasked reference on the same rows is another function
    from . import attn_ref as AR
    assert float((AR.Forward(qkv, S, N, heads, bf).out_rows - out)[live].abs().max()) > 1e-3


def test_reference_clamps_and_skips_empty_elements():
    S, N, heads, hd = 9, 4, 2, 16
    qkv = fill.hash_tensor((S * N, 3 * heads * hd), 907, 1.0)
    lengths = [S + 3, -2, 0, 4]
    assert VR.clamp(lengths, S) == [9, 0, 0, 4]
    fs = VR.forward_alone(qkv, lengths, S, N, heads, True)
    assert fs[1] is None and fs[2] is None and fs[0].S == 9 and fs[3].S == 4
    out, lse = VR.scatter_forward(fs, lengths, S, N, heads, True)
    assert float(out[S:3 * S].abs().max()) == 0 and float(lse[1:3].abs().max()) == 0
    # with a keep mask of the padded launch, sliced
    keep = (fill.hash_tensor((N, heads, S, S), 908, 1.0) > -0.25).to(torch.uint8)
    fk = VR.forward_alone(qkv, lengths, S, N, heads, True, keep, 0.25)
    assert torch.equal(fk[3].keep[0], keep[3, :, :4, :4].double())
