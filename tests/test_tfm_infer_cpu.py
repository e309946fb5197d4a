"""CPU-side checks of the transformer's fused layer tails and inference plan (csrc/transformer_infer.hip, csrc/plan_infer.hip,
ecgmm.inference.Predictor(ECGTransformer1D)): the float64 bounds of tests/tfm_infer_bounds.py accept torch's fp32 evaluation
and reject named slips; ABI agreement, size queries, the workspace cap and argument validation without a device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from ecgmm.hip import lib as L

from . import tfm_infer_bounds as TB
from . import tfm_infer_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ecgmm_linear_res_ln", "ecgmm_ffn_res_ln", "ecgmm_transformer_infer_prepared_bytes", "ecgmm_transformer_infer_prepare",
       "ecgmm_transformer_infer_workspace", "ecgmm_transformer_infer")
EPS = 1e-5

# (R, K, E, input scale) / (R, E, ff, input scale)
LINEAR = [(1, 16, 16, 1.0), (17, 64, 64, 1.0), (33, 128, 128, 1.0), (65, 256, 128, 1.0), (33, 256, 256, 1.0),
          (33, 2048, 128, 1.0), (16, 128, 128, 30.0)]
FFN = [(17, 64, 128, 1.0), (33, 128, 256, 1.0), (16, 128, 2048, 1.0), (5, 16, 16, 1.0), (33, 256, 1024, 1.0)]


def _err():
    return L.lib().ecgmm_last_error().decode()


def _linear(c, slip=None):
    f = TR.linear_res_ln(c["a"], c["w"], c["b"], c["res"], c["gamma"], c["beta"], EPS)
    bound, r = TB.linear_res_ln(f)
    return TB.ratio((TR.linear_candidate(c, EPS, slip).double() - f.n.y).abs(), bound), r


def _ffn(c, slip=None):
    f = TR.ffn_res_ln(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["gamma"], c["beta"], EPS)
    bound, r = TB.ffn_res_ln(f)
    return TB.ratio((TR.ffn_candidate(c, EPS, slip).double() - f.n.y).abs(), bound), r


# ---- the bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,E,scale", LINEAR)
def test_linear_bound_accepts_torch_fp32(R, K, E, scale):
    ratio, r = _linear(TR.linear_case(R, K, E, scale, seed=R + K))
    print("linear_res_ln R%d K%d E%d x%g: torch fp32 / bound %.3g, r %.3g" % (R, K, E, scale, ratio, r))
    assert r < TB.R_MAX and ratio <= 1.0


@pytest.mark.parametrize("R,E,ff,scale", FFN)
def test_ffn_bound_accepts_torch_fp32(R, E, ff, scale):
    ratio, r = _ffn(TR.ffn_case(R, E, ff, scale, seed=R + ff))
    print("ffn_res_ln R%d E%d ff%d x%g: torch fp32 / bound %.3g, r %.3g" % (R, E, ff, scale, ratio, r))
    assert r < TB.R_MAX and ratio <= 1.0


@pytest.mark.parametrize("small_var", [False, True])
def test_bounds_accept_torch_fp32_on_small_variance_rows(small_var):
    for ratio, r in (_linear(TR.linear_case(33, 128, 128, seed=5, small_var=small_var)),
                     _ffn(TR.ffn_case(33, 128, 256, seed=5, small_var=small_var))):
        assert r < TB.R_MAX and ratio <= 1.0, (ratio, r)


@pytest.mark.parametrize("slip", ["no_residual", "no_bias", "half_stats", "bf16_prenorm"])
@pytest.mark.parametrize("R,K,E", [(17, 64, 64), (33, 128, 128), (65, 256, 128)])
def test_linear_bound_rejects_the_slip(slip, R, K, E):
    ratio, r = _linear(TR.linear_case(R, K, E, seed=R + K), slip)
    print("linear_res_ln %s R%d K%d E%d: ratio %.3g" % (slip, R, K, E, ratio))
    assert r < TB.R_MAX and ratio > 1.0


@pytest.mark.parametrize("slip", ["no_residual", "no_bias", "no_relu", "half_stats", "bf16_prenorm"])
@pytest.mark.parametrize("R,E,ff", [(17, 64, 128), (33, 128, 256)])
def test_ffn_bound_rejects_the_slip(slip, R, E, ff):
    ratio, r = _ffn(TR.ffn_case(R, E, ff, seed=R + ff), slip)
    print("ffn_res_ln %s R%d E%d ff%d: ratio %.3g" % (slip, R, E, ff, ratio))
    assert r < TB.R_MAX and ratio > 1.0


def test_bounds_reject_a_missing_eps_on_small_variance_rows():
    a, r = _linear(TR.linear_case(33, 128, 128, seed=5, small_var=True), "no_eps")
    b, r2 = _ffn(TR.ffn_case(33, 128, 256, seed=5, small_var=True), "no_eps")
    print("no_eps: linear_res_ln ratio %.3g, ffn_res_ln ratio %.3g" % (a, b))
    assert max(r, r2) < TB.R_MAX and a > 1.0 and b > 1.0


# ---- the C ABI without a device -------------------------------------------------------------------------------------------
def desc(B=8, L_=3000, cin=1, E=128, heads=4, ff=256, layers=2, classes=2, bf=1, eps=1e-5):
    return L.TransformerInferDesc(B, L_, cin, E, heads, ff, layers, classes, bf, eps)


def test_new_symbols_in_header_table_and_library():
    src = open(os.path.join(ROOT, "include", "ecgmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ecgmm_[a-z0-9_]+)\s*\(", src))
    h = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared, name + " not declared in include/ecgmm.h"
        assert name in L.SIGNATURES, name + " not in the ctypes table"
        assert hasattr(h, name), name + " not exported"
    assert L.lib().ecgmm_version() == 100


def _cap(B, L_, E, heads, classes, buffers=8):
    R = B * L_
    return 4 * R * (6 * E + heads) + 4 * B * (E + 64 + classes) + 256 * buffers


@pytest.mark.parametrize("B,L_,E,heads,ff,classes", [(8, 3000, 128, 4, 256, 2), (32, 750, 64, 4, 128, 2), (1, 1, 16, 1, 16, 1),
                                                      (3, 40, 64, 4, 128, 5), (5, 17, 256, 8, 2048, 3), (2, 9, 48, 3, 4096, 2)])
def test_workspace_depends_neither_on_layers_nor_on_ff_and_stays_within_the_cap(B, L_, E, heads, ff, classes):
    lib = L.lib()
    q = lambda **kw: lib.ecgmm_transformer_infer_workspace(C.byref(desc(B, L_, 1, E, heads, ff, 2, classes, **kw)))
    ws = q()
    assert ws > 0, _err()
    d1, d6 = desc(B, L_, 1, E, heads, ff, 1, classes), desc(B, L_, 1, E, heads, ff, 6, classes)
    assert lib.ecgmm_transformer_infer_workspace(C.byref(d1)) == lib.ecgmm_transformer_infer_workspace(C.byref(d6)) == ws
    lo, hi = desc(B, L_, 1, E, heads, 128, 2, classes), desc(B, L_, 1, E, heads, 2048, 2, classes)
    assert lib.ecgmm_transformer_infer_workspace(C.byref(lo)) == lib.ecgmm_transformer_infer_workspace(C.byref(hi)) == ws
    assert q(bf=0) == ws
    assert ws <= _cap(B, L_, E, heads, classes)
    # no [R, ff] tensor: at ff = 2048 that alone would exceed what is there beyond x, qkv, the attention output and the next x
    assert ws < 4 * B * L_ * 2048


def test_prepared_bytes_hold_every_parameter_and_ignore_the_batch():
    lib = L.lib()
    E, ff, layers, classes, Ln = 128, 256, 2, 2, 3000
    nb = lib.ecgmm_transformer_infer_prepared_bytes(C.byref(desc()))
    per_layer = 3 * E * E + 3 * E + E * E + E + ff * E + ff + E * ff + E + 4 * E
    floats = E * 3 + E + Ln * E + layers * per_layer + 64 * E + 64 + classes * 64 + classes
    assert 4 * floats <= nb <= 4 * floats + 256 * (3 + 12 * layers + 4 + 1)
    assert lib.ecgmm_transformer_infer_prepared_bytes(C.byref(desc(B=0))) == nb
    assert lib.ecgmm_transformer_infer_prepared_bytes(C.byref(desc(layers=3))) > nb


def test_bad_descriptors_zero_the_queries_and_name_the_limit():
    lib = L.lib()
    for kw, word in ((dict(E=272), "E=272"), (dict(E=24, heads=1), "E=24"), (dict(ff=40), "ff=40"), (dict(ff=4112), "ff=4112"),
                     (dict(E=512, heads=16), "<= 256"), (dict(heads=3), "heads=3"), (dict(E=256, heads=4), "16 or 32"),
                     (dict(layers=0), "layers=0"), (dict(classes=0), "classes=0"), (dict(cin=13), "input_dim=13"),
                     (dict(bf=2), "batch_first=2"), (dict(eps=-1.0), "eps"), (dict(L_=0), "L=0")):
        assert lib.ecgmm_transformer_infer_workspace(C.byref(desc(**kw))) == 0 and word in _err(), (kw, _err())
        assert lib.ecgmm_transformer_infer_prepared_bytes(C.byref(desc(**kw))) == 0 and word in _err(), (kw, _err())
    assert lib.ecgmm_transformer_infer_workspace(C.byref(desc(B=0))) == 0 and "B=0" in _err()
    assert lib.ecgmm_transformer_infer_workspace(C.byref(desc(B=65535, L_=1 << 20))) == 0 and "too large" in _err()
    assert lib.ecgmm_transformer_infer_workspace(None) == 0 and lib.ecgmm_transformer_infer_prepared_bytes(None) == 0


def test_null_and_short_buffers_are_errors_not_traps():
    lib = L.lib()
    d = desc(2, 40, 1, 64, 4, 128, 2, 2)
    one = C.create_string_buffer(64)
    p1 = C.cast(one, C.c_void_p)
    n = 3 + 12 * 2 + 4
    tab = (C.c_void_p * n)(*[p1] * n)
    assert lib.ecgmm_transformer_infer_prepare(C.byref(d), None, p1, 64, None) == 1 and "null" in _err()
    assert lib.ecgmm_transformer_infer_prepare(C.byref(d), tab, None, 0, None) == 3 and "blob" in _err()
    assert lib.ecgmm_transformer_infer_prepare(C.byref(d), tab, p1, 64, None) == 3 and "blob" in _err()
    tab[7] = None
    assert lib.ecgmm_transformer_infer_prepare(C.byref(d), tab, p1, 1 << 40, None) == 1 and "parameter 7" in _err()
    assert lib.ecgmm_transformer_infer(C.byref(d), None, None, p1, 64, p1, p1, 64, None) == 1 and "null" in _err()
    assert lib.ecgmm_transformer_infer(C.byref(d), p1, None, p1, 64, p1, p1, 64, None) == 3 and "blob" in _err()
    assert lib.ecgmm_transformer_infer(C.byref(d), p1, None, p1, 1 << 40, p1, p1, 64, None) == 3 and "workspace" in _err()
    across = desc(2, 40, 1, 64, 4, 128, 2, 2, bf=0)
    assert lib.ecgmm_transformer_infer(C.byref(across), p1, p1, p1, 1 << 40, p1, p1, 1 << 40, None) == 1 and "batch_first" in _err()
    assert lib.ecgmm_transformer_infer(C.byref(desc(E=272)), p1, None, p1, 1 << 40, p1, p1, 1 << 40, None) == 1 and "E=272" in _err()


def test_the_two_ops_refuse_bad_shapes_null_pointers_and_aliasing():
    lib = L.lib()
    buf = C.create_string_buffer(256)
    base = (C.addressof(buf) + 15) // 16 * 16
    p, q, odd = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 4)
    lin = lambda a=p, w=p, b=p, res=p, g=p, be=p, out=q, R=4, K=64, E=64, eps=1e-5: \
        lib.ecgmm_linear_res_ln(a, w, b, res, g, be, out, R, K, E, eps, None)
    ffn = lambda x=p, w1=p, b1=p, w2=p, b2=p, g=p, be=p, out=q, R=4, E=64, ff=128, eps=1e-5: \
        lib.ecgmm_ffn_res_ln(x, w1, b1, w2, b2, g, be, out, R, E, ff, eps, None)
    for fn, kname in ((lin, "K"), (ffn, "ff")):
        assert fn(E=272) == 1 and "E=272" in _err() and "<= 256" in _err()
        assert fn(E=24) == 1 and "E=24" in _err() and "multiple of 16" in _err()
        assert fn(E=0) == 1 and fn(R=0) == 1 and "R=0" in _err()
        assert fn(**{kname: 40}) == 1 and kname + "=40" in _err() and "multiple of 16" in _err()
        assert fn(**{kname: 4112}) == 1 and kname + "=4112" in _err() and "<= 4096" in _err()
        assert fn(eps=-1.0) == 1 and "eps" in _err()
        assert fn(out=None) == 1 and "null" in _err()
        assert fn(g=None) == 1 and "null" in _err()
        assert fn(out=odd) == 1 and "aligned" in _err()
    assert lin(a=None) == 1 and "null" in _err() and ffn(w2=None) == 1 and "null" in _err()
    # in place is not offered: equal pointers are refused
    assert lin(res=q) == 1 and "alias" in _err()
    assert lin(a=q) == 1 and "alias" in _err()
    assert ffn(x=q) == 1 and "alias" in _err()


# ---- Python ---------------------------------------------------------------------------------------------------------------
def test_predictor_refuses_a_cpu_model_and_unsupported_widths():
    from ecgmm.inference import Predictor
    from ecgmm.train_physionet import ECGTransformer1D
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(ECGTransformer1D(seq_len=16, d_model=64, nhead=4, num_layers=1, dim_feedforward=128))
    with pytest.raises(ValueError, match="d_model=512.*256"):
        Predictor(ECGTransformer1D(seq_len=16, d_model=512, nhead=16, num_layers=1, dim_feedforward=128))
    with pytest.raises(ValueError, match="dim_feedforward=40.*multiple of 16"):
        Predictor(ECGTransformer1D(seq_len=16, d_model=64, nhead=4, num_layers=1, dim_feedforward=40))
    with pytest.raises(ValueError, match="dim_feedforward=4112.*4096"):
        Predictor(ECGTransformer1D(seq_len=16, d_model=64, nhead=4, num_layers=1, dim_feedforward=4112))
    with pytest.raises(TypeError, match="unsupported model.*ECGTransformer1D"):
        Predictor(torch.nn.Linear(2, 2))
    assert "ECGTransformer1D" in Predictor.__doc__


def test_the_fused_ops_are_forward_only_and_need_a_device():
    from ecgmm.hip import functional as HF
    c = TR.linear_case(4, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.linear_res_ln(c["a"], c["w"], c["b"], c["res"], c["gamma"], c["beta"])
    a = c["a"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        HF.linear_res_ln(a, c["w"], c["b"], c["res"], c["gamma"], c["beta"])
    f = TR.ffn_case(4, 16, 16)
    w1 = f["w1"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        HF.ffn_res_ln(f["x"], w1, f["b1"], f["w2"], f["b2"], f["gamma"], f["beta"])
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.ffn_res_ln(f["x"], w1, f["b1"], f["w2"], f["b2"], f["gamma"], f["beta"])


def test_train_physionet_keeps_its_default_signature():
    from ecgmm import train_physionet as TP
    p = inspect.signature(TP.main).parameters
    want = dict(num_epochs=30, batch_size=8, quiet=False, use_predictor=False, num_classes=2, augment=True, model="resnet",
                max_len=TP.MAX_LEN, time_attention=False, use_lengths=False, rollout_samples=0, target_fs=None)
    for k, v in want.items():
        assert p[k].default == v or p[k].default is v, k
    assert inspect.signature(TP.evaluate).parameters["predictor"].default is None
    assert "needs model='resnet'" not in inspect.getsource(TP.main)
