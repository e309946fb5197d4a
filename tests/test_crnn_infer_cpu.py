"""CPU-side checks of the CRNN front end's inference plan (csrc/plan_infer.hip, ecgmm.inference.Predictor(CRNN)): ABI
agreement, size queries and argument validation without a device."""
import ctypes as C
import os
import re

import pytest

from ecgmm.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ecgmm_relu_maxpool2", "ecgmm_conv5_in1_relu_pool2", "ecgmm_fold_conv5_bn", "ecgmm_crnn_front_infer_prepared_bytes",
       "ecgmm_crnn_front_infer_prepare", "ecgmm_crnn_front_infer_workspace", "ecgmm_crnn_front_infer")
DTYPES = [L.BF16, L.F32]


def _err():
    return L.lib().ecgmm_last_error().decode()


def desc(B, F, T, dt):
    return L.CRNNFrontDesc(B, F, T, dt, 0, 0.1, 1e-5)


def test_new_symbols_in_header_table_and_library():
    src = open(os.path.join(ROOT, "include", "ecgmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ecgmm_[a-z0-9_]+)\s*\(", src))
    h = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared, name + " not declared in include/ecgmm.h"
        assert name in L.SIGNATURES, name + " not in the ctypes table"
        assert hasattr(h, name), name + " not exported"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp32"])
def test_size_queries_need_no_device(dt):
    lib = L.lib()
    es = 2 if dt == L.BF16 else 4
    blob = lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(desc(8, 33, 280, dt)))
    # folded fp32 w1, packed w2 / w3 in the compute dtype, three fp32 biases
    assert blob >= 32 * 25 * 4 + (64 * 32 + 128 * 64) * 25 * es + (32 + 64 + 128) * 4
    # the blob does not depend on B, F or T
    assert lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(desc(0, 0, 0, dt))) == blob
    ws = lib.ecgmm_crnn_front_infer_workspace(C.byref(desc(8, 33, 280, dt)))
    # pooled-1 [8,16,140,32], y2 [8,16,140,64], pooled-2 [8,8,70,64], y3 [8,8,70,128]
    assert ws >= (8 * 16 * 140 * (32 + 64) + 8 * 8 * 70 * (64 + 128)) * es
    # ... and nothing of the training plan's: no [B,F,T,32] tensor, no argmax bytes, no statistics rows
    fwd = lib.ecgmm_crnn_front_fwd_workspace(C.byref(desc(8, 33, 280, dt)))
    assert 0 < ws <= fwd - 8 * 33 * 280 * 32 * es


def test_bad_descriptors_zero_the_queries():
    lib = L.lib()
    for bad in (7, -1):
        assert lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(desc(8, 33, 280, bad))) == 0 and "dtype" in _err()
        assert lib.ecgmm_crnn_front_infer_workspace(C.byref(desc(8, 33, 280, bad))) == 0 and "dtype" in _err()
    assert lib.ecgmm_crnn_front_infer_workspace(C.byref(desc(8, 7, 280, L.F32))) == 0 and "F = 7" in _err()
    assert lib.ecgmm_crnn_front_infer_workspace(C.byref(desc(8, 33, 7, L.F32))) == 0 and "T = 7" in _err()
    assert lib.ecgmm_crnn_front_infer_workspace(C.byref(desc(0, 33, 280, L.F32))) == 0
    assert lib.ecgmm_crnn_front_infer_workspace(C.byref(desc(1 << 20, 64, 1 << 12, L.F32))) == 0 and "too large" in _err()
    assert lib.ecgmm_crnn_front_infer_prepared_bytes(None) == 0
    # the blob never looks at the shape
    assert lib.ecgmm_crnn_front_infer_prepared_bytes(C.byref(desc(8, 7, 7, L.F32))) > 0


def test_null_and_short_buffers_are_errors_not_traps():
    lib = L.lib()
    d = desc(2, 33, 40, L.F32)
    one = C.create_string_buffer(64)
    p1 = C.cast(one, C.c_void_p)
    tab, buf = (C.c_void_p * 12)(*[p1] * 12), (C.c_void_p * 9)(*[p1] * 9)
    assert lib.ecgmm_crnn_front_infer_prepare(C.byref(d), None, None, p1, 64, None) == 1 and "null" in _err()
    assert lib.ecgmm_crnn_front_infer_prepare(C.byref(d), tab, buf, None, 0, None) == 3 and "blob" in _err()
    assert lib.ecgmm_crnn_front_infer_prepare(C.byref(d), tab, buf, p1, 64, None) == 3 and "blob" in _err()
    tab[5] = None
    assert lib.ecgmm_crnn_front_infer_prepare(C.byref(d), tab, buf, p1, 1 << 40, None) == 1 and "parameter 5" in _err()
    assert lib.ecgmm_crnn_front_infer(C.byref(d), None, p1, 64, p1, p1, 64, None) == 1 and "null" in _err()
    assert lib.ecgmm_crnn_front_infer(C.byref(d), p1, p1, 64, p1, p1, 64, None) == 3 and "blob" in _err()
    assert lib.ecgmm_crnn_front_infer(C.byref(d), p1, p1, 1 << 40, p1, p1, 64, None) == 3 and "workspace" in _err()
    assert lib.ecgmm_crnn_front_infer(C.byref(desc(2, 33, 40, 5)), p1, p1, 64, p1, p1, 64, None) == 2 and "dtype" in _err()
    # per-op entries
    assert lib.ecgmm_relu_maxpool2(3, p1, p1, 2, 8, 8, 64, 0, None) == 2 and "dtype" in _err()
    assert lib.ecgmm_relu_maxpool2(L.F32, None, p1, 2, 8, 8, 64, 0, None) == 1 and "null" in _err()
    assert lib.ecgmm_relu_maxpool2(L.F32, p1, None, 2, 8, 8, 64, 1, None) == 1 and "null" in _err()
    assert lib.ecgmm_relu_maxpool2(L.F32, p1, p1, 2, 1, 8, 64, 0, None) == 1 and "H=1" in _err()
    assert lib.ecgmm_relu_maxpool2(L.F32, p1, p1, 2, 8, 1, 64, 0, None) == 1 and "W=1" in _err()
    assert lib.ecgmm_relu_maxpool2(L.BF16, p1, p1, 2, 8, 8, 12, 0, None) == 1 and "C=12" in _err()
    assert lib.ecgmm_conv5_in1_relu_pool2(9, p1, p1, p1, p1, 2, 8, 8, None) == 2 and "dtype" in _err()
    assert lib.ecgmm_conv5_in1_relu_pool2(L.F32, None, p1, p1, p1, 2, 8, 8, None) == 1 and "null" in _err()
    assert lib.ecgmm_conv5_in1_relu_pool2(L.F32, p1, p1, None, None, 2, 8, 8, None) == 1 and "null" in _err()
    assert lib.ecgmm_conv5_in1_relu_pool2(L.F32, p1, p1, p1, p1, 2, 1, 8, None) == 1 and "2x2" in _err()
    assert lib.ecgmm_conv5_in1_relu_pool2(L.F32, p1, p1, p1, p1, 2, 8, 1, None) == 1 and "2x2" in _err()
    assert lib.ecgmm_fold_conv5_bn(3, 0, p1, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 64, 32, None) == 2 and "dtype" in _err()
    assert lib.ecgmm_fold_conv5_bn(L.F32, 2, p1, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 32, 1, None) == 1 and "layout" in _err()
    assert lib.ecgmm_fold_conv5_bn(L.F32, 1, None, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 32, 1, None) == 1
    assert lib.ecgmm_fold_conv5_bn(L.F32, 1, p1, None, p1, None, p1, p1, 1e-5, p1, p1, None, 32, 1, None) == 1


def test_predictor_of_a_cpu_crnn_raises_the_cpu_tensor_error():
    """the CRNN is a served model: what is refused is the device, not the class"""
    from ecgmm.crnn import CRNN
    from ecgmm.inference import Predictor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(CRNN())


def test_train_physionet2_keeps_its_default_signatures():
    import inspect

    from ecgmm import train_physionet2 as T2
    assert inspect.signature(T2.evaluate).parameters["predictor"].default is None
    assert inspect.signature(T2.main).parameters["use_predictor"].default is False
