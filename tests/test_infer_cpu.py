"""CPU-side checks of the inference plans: ABI agreement, argument validation without a device, and the test helper's
own fold formula against torch."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from ecgmm.hip import lib as L

from .infer_ref import fold_ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ecgmm_resnet18_infer_prepared_bytes", "ecgmm_resnet18_infer_prepare", "ecgmm_resnet18_infer_workspace",
       "ecgmm_resnet18_infer", "ecgmm_resnet1d_infer_prepared_bytes", "ecgmm_resnet1d_infer_prepare",
       "ecgmm_resnet1d_infer_workspace", "ecgmm_resnet1d_infer", "ecgmm_infer_down_side", "ecgmm_conv_fwd_fused",
       "ecgmm_fold_conv_bn", "ecgmm_relu_maxpool", "ecgmm_gate_res_relu")
SIZE_FNS = ("fwd_workspace", "bwd_workspace", "infer_workspace", "infer_prepared_bytes")


def test_new_symbols_in_header_table_and_library():
    src = open(os.path.join(ROOT, "include", "ecgmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ecgmm_[a-z0-9_]+)\s*\(", src))
    h = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared, name + " not declared in include/ecgmm.h"
        assert name in L.SIGNATURES, name + " not in the ctypes table"
        assert hasattr(h, name), name + " not exported"


def _err():
    return L.lib().ecgmm_last_error().decode()


def test_size_queries_and_bad_descriptors_need_no_device():
    lib = L.lib()
    d = L.ResNet18Desc(8, 224, 224, 256, L.BF16, 0, 0.1, 1e-5)
    blob, ws = lib.ecgmm_resnet18_infer_prepared_bytes(C.byref(d)), lib.ecgmm_resnet18_infer_workspace(C.byref(d))
    assert blob > 11_000_000 * 2 and ws > 8 * 112 * 112 * 64 * 2
    # the blob does not depend on the batch or the image size
    d2 = L.ResNet18Desc(0, 0, 0, 256, L.BF16, 0, 0.1, 1e-5)
    assert lib.ecgmm_resnet18_infer_prepared_bytes(C.byref(d2)) == blob
    s = L.ResNet1DDesc(8, 1, 5000, 256, L.F32, 0, 0.1, 1e-5, 0.0, 0, 0)
    assert lib.ecgmm_resnet1d_infer_prepared_bytes(C.byref(s)) > 0
    assert lib.ecgmm_resnet1d_infer_workspace(C.byref(s)) > 8 * 2500 * 64 * 4
    bad = L.ResNet18Desc(8, 224, 224, 256, 7, 0, 0.1, 1e-5)
    assert lib.ecgmm_resnet18_infer_workspace(C.byref(bad)) == 0 and "dtype" in _err()
    assert lib.ecgmm_resnet18_infer_prepared_bytes(C.byref(bad)) == 0 and "dtype" in _err()
    bad1 = L.ResNet1DDesc(8, 1, 5000, 256, 9, 0, 0.1, 1e-5, 0.0, 0, 0)
    assert lib.ecgmm_resnet1d_infer_workspace(C.byref(bad1)) == 0 and "dtype" in _err()
    small = L.ResNet18Desc(8, 16, 16, 256, L.BF16, 0, 0.1, 1e-5)
    assert lib.ecgmm_resnet18_infer_workspace(C.byref(small)) == 0 and "bad input" in _err()
    # Exact sizes [fwd_workspace, bwd_workspace, infer_workspace, infer_prepared_bytes].  The integers are what the library
    # returned before the network descriptions moved into csrc/net_desc.h (a build of that commit, queried on the CPU): the
    # training and inference plans now share one description, and no size may move.  A too-small input zeroes the three
    # workspaces but not the blob, which never looks at the shape; a bad dtype or cin zeroes all four.
    # (rows the ECGMM_STEM_RECOMPUTE switch cannot touch; the bf16 ResNet18 rows are in the test below)
    for d, want in ((L.ResNet18Desc(1, 32, 32, 2, L.F32, 0, 0.1, 1e-5), [90274816, 14307328, 83968, 44702720]),
                    (L.ResNet18Desc(8, 31, 224, 2, L.F32, 1, 0.1, 1e-5), [0, 0, 0, 44702720]),
                    (L.ResNet18Desc(8, 224, 224, 2, 7, 1, 0.1, 1e-5), [0, 0, 0, 0])):
        assert [getattr(lib, "ecgmm_resnet18_" + f)(C.byref(d)) for f in SIZE_FNS] == want
    for d, want in ((L.ResNet1DDesc(512, 12, 5000, 256, L.BF16, 1, 0.1, 1e-5, 0.3, 0, 0),
                     [1459741696, 1041141760, 329940992, 1063936]),
                    (L.ResNet1DDesc(8, 1, 63, 2, L.F32, 1, 0.1, 1e-5, 0.3, 0, 0), [0, 0, 0, 1862400]),
                    (L.ResNet1DDesc(8, 25, 5000, 2, L.F32, 1, 0.1, 1e-5, 0.3, 0, 0), [0, 0, 0, 0])):
        assert [getattr(lib, "ecgmm_resnet1d_" + f)(C.byref(d)) for f in SIZE_FNS] == want


_CHILD = """
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from ecgmm.hip import lib as L
lib = L.lib()
fns = ("fwd_workspace", "bwd_workspace", "infer_workspace", "infer_prepared_bytes")
out = []
for N, H, W, od in ((256, 224, 224, 256), (8, 250, 2500, 2)):
    d = L.ResNet18Desc(N, H, W, od, L.BF16, 1, 0.1, 1e-5)
    out.append([getattr(lib, "ecgmm_resnet18_" + f)(C.byref(d)) for f in fns])
print(json.dumps(out))
"""


@pytest.mark.parametrize("recompute, want", [
    (None, [[2320534528, 2084395008, 514326528, 22884096], [943228416, 898026496, 200336384, 22363136]]),
    ("1", [[1864535040, 1262476032, 514326528, 22884096], [765107712, 578191104, 200336384, 22363136]]),
])
def test_bf16_resnet18_sizes_with_and_without_stem_recompute(recompute, want):
    """The bf16 training-plan sizes depend on ECGMM_STEM_RECOMPUTE, which is read once per process: each setting gets a
    child process of its own (no device needed).  Integers from the same build as the rows above."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "ECGMM_STEM_RECOMPUTE"}
    if recompute is not None:
        env["ECGMM_STEM_RECOMPUTE"] = recompute
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == want


def test_null_and_short_buffers_are_errors_not_traps():
    lib = L.lib()
    d = L.ResNet18Desc(2, 64, 64, 16, L.F32, 0, 0.1, 1e-5)
    s = L.ResNet1DDesc(2, 1, 1000, 4, L.F32, 0, 0.1, 1e-5, 0.0, 0, 0)
    one = C.create_string_buffer(64)
    p1 = C.cast(one, C.c_void_p)
    # null tables / null blob / short blob
    assert lib.ecgmm_resnet18_infer_prepare(C.byref(d), None, None, p1, 64, None) == 1 and "null" in _err()
    tab18 = (C.c_void_p * 62)(*[p1] * 62)
    buf18 = (C.c_void_p * 60)(*[p1] * 60)
    assert lib.ecgmm_resnet18_infer_prepare(C.byref(d), tab18, buf18, None, 0, None) == 3 and "blob" in _err()
    assert lib.ecgmm_resnet18_infer_prepare(C.byref(d), tab18, buf18, p1, 64, None) == 3 and "blob" in _err()
    tab18[5] = None
    assert lib.ecgmm_resnet18_infer_prepare(C.byref(d), tab18, buf18, p1, 1 << 40, None) == 1 and "parameter 5" in _err()
    tab1 = (C.c_void_p * 52)(*[p1] * 52)
    buf1 = (C.c_void_p * 27)(*[p1] * 27)
    assert lib.ecgmm_resnet1d_infer_prepare(C.byref(s), tab1, buf1, p1, 64, None) == 3 and "blob" in _err()
    # infer: null input, short blob, short workspace
    assert lib.ecgmm_resnet18_infer(C.byref(d), None, p1, 64, p1, p1, 64, None) == 1 and "null" in _err()
    assert lib.ecgmm_resnet18_infer(C.byref(d), p1, p1, 64, p1, p1, 64, None) == 3 and "blob" in _err()
    assert lib.ecgmm_resnet18_infer(C.byref(d), p1, p1, 1 << 40, p1, p1, 64, None) == 3 and "workspace" in _err()
    assert lib.ecgmm_resnet1d_infer(C.byref(s), p1, p1, 1 << 40, p1, None, 0, None) == 3 and "workspace" in _err()
    assert lib.ecgmm_resnet1d_infer(C.byref(s), p1, None, 0, p1, p1, 64, None) == 3 and "blob" in _err()
    bad = L.ResNet1DDesc(2, 1, 1000, 4, 5, 0, 0.1, 1e-5, 0.0, 0, 0)
    assert lib.ecgmm_resnet1d_infer(C.byref(bad), p1, p1, 64, p1, p1, 64, None) == 2 and "dtype" in _err()
    # per-op entries
    c = L.ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 1)
    assert lib.ecgmm_conv_fwd_fused(L.BF16, C.byref(c), None, p1, None, None, p1, 1, None) == 1 and "null" in _err()
    assert lib.ecgmm_conv_fwd_fused(4, C.byref(c), p1, p1, None, None, p1, 1, None) == 2 and "dtype" in _err()
    assert lib.ecgmm_conv_fwd_fused(L.BF16, C.byref(c), p1, p1, None, None, p1, 2, None) == 1 and "act" in _err()
    assert lib.ecgmm_conv_fwd_fused(L.BF16, None, p1, p1, None, None, p1, 1, None) == 1
    assert lib.ecgmm_fold_conv_bn(3, 0, p1, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 64, 64, 9, None) == 2 and "dtype" in _err()
    assert lib.ecgmm_fold_conv_bn(L.F32, 0, None, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 64, 64, 9, None) == 1
    assert lib.ecgmm_fold_conv_bn(L.F32, 0, p1, None, None, p1, p1, p1, 1e-5, p1, p1, None, 64, 64, 9, None) == 1
    assert lib.ecgmm_fold_conv_bn(L.F32, 0, p1, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 64, 64, 25, None) == 1 and "taps" in _err()
    assert lib.ecgmm_fold_conv_bn(L.F32, 1, p1, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 32, 3, 7, None) == 1 and "stem" in _err()
    assert lib.ecgmm_fold_conv_bn(L.F32, 2, p1, None, p1, p1, p1, p1, 1e-5, p1, p1, None, 64, 3, 7, None) == 1 and "layout" in _err()
    assert lib.ecgmm_relu_maxpool(L.BF16, None, p1, 2, 8, 8, 64, None) == 1 and "null" in _err()
    assert lib.ecgmm_relu_maxpool(L.BF16, p1, p1, 2, 8, 8, 12, None) == 1 and "C=12" in _err()
    assert lib.ecgmm_relu_maxpool(6, p1, p1, 2, 8, 8, 64, None) == 2
    assert lib.ecgmm_gate_res_relu(L.BF16, p1, p1, None, p1, 64, 64, 8, None) == 1 and "null" in _err()
    assert lib.ecgmm_gate_res_relu(L.BF16, p1, p1, p1, p1, 65, 64, 8, None) == 1 and "rows" in _err()


def test_predictor_refuses_cpu_model_and_unknown_models():
    from ecgmm.image_encoder import ResNet18
    from ecgmm.inference import Predictor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(ResNet18(num_classes=4, compute_dtype="fp32"))
    with pytest.raises(TypeError, match="unsupported model"):
        Predictor(torch.nn.Linear(2, 2))


def test_every_registered_plan_prepares_through_the_one_base_procedure(monkeypatch):
    """Every plan class ``Predictor`` knows derives from ``PreparedPlan`` and gets its blob from THAT class's prepare step.
    With the step recording its calls, the device requirement waived (so CPU parameters do) and the library itself out of
    reach, constructing each kind of predictor still works: no plan has a size-query-and-allocate sequence of its own."""
    from ecgmm import inference as INF
    from ecgmm.config import Config
    from ecgmm.crnn import CRNN
    from ecgmm.hip.prepared import PreparedPlan
    from ecgmm.image_encoder import ResNet18
    from ecgmm.multimodal import ECGMultimodalModel as TabVariant
    from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel, ResNet1D_SE
    from ecgmm.tabnet import ClinicalTabNetEncoder
    from ecgmm.train_physionet import ECGTransformer1D

    cfg = type("Cfg", (Config,), {"compute_dtype": "fp32", "clinical_input_dim": 24})
    models = {ClinicalTabNetEncoder: [ClinicalTabNetEncoder(2, 32)], CRNN: [CRNN(compute_dtype="fp32")],
              ECGTransformer1D: [ECGTransformer1D(seq_len=16, d_model=64, nhead=4, num_layers=2, dim_feedforward=128)],
              ECGMultimodalModel: [ECGMultimodalModel(cfg), TabVariant(cfg)],
              ResNet18: [ResNet18(num_classes=4, compute_dtype="fp32")], ResNet1D_SE: [ResNet1D_SE(1, 4, compute_dtype="fp32")]}
    assert {kind for kind, _ in INF.PLANS} == set(models), "a registered plan has no model in this test"
    calls, handed_out = [], []

    def prepare(cls, desc, tables, device):
        calls.append((cls, [len(t) for t in tables]))
        handed_out.append(torch.zeros(16, dtype=torch.uint8))
        return handed_out[-1]

    def no_library():
        raise AssertionError("a plan reached the library outside PreparedPlan.prepare")

    monkeypatch.setattr(PreparedPlan, "prepare", classmethod(prepare))
    monkeypatch.setattr(PreparedPlan, "check_params", staticmethod(lambda tensors, what, fp32=None: None))
    monkeypatch.setattr(L, "lib", no_library)
    for kind, plan in INF.PLANS:
        assert issubclass(plan, PreparedPlan), plan.__name__
        assert "prepare" not in vars(plan) and "run" not in vars(plan), plan.__name__ + " overrides a base procedure"
        for model in models[kind]:
            del calls[:], handed_out[:]
            predict = INF.Predictor(model.eval())
            assert type(predict.encoder) is plan
            parts = [p for p in (predict.image, predict.signal, predict.clinical) if p is not None] or [predict.encoder]
            assert len(calls) == len(parts) and all(issubclass(c, PreparedPlan) for c, _ in calls)
            assert [id(p.blob) for p in parts] == [id(b) for b in handed_out], "a blob that the base did not prepare"
            predict.refresh()
            assert len(calls) == 2 * len(parts)
            assert [id(p.blob) for p in parts] == [id(b) for b in handed_out[len(parts):]], "refresh() kept an old blob"


def test_train_evaluate_keeps_its_default_signature():
    import inspect

    from ecgmm import train
    assert inspect.signature(train.evaluate).parameters["predictor"].default is None
    assert inspect.signature(train.run_epoch).parameters["predictor"].default is None
    assert inspect.signature(train.main).parameters["use_predictor"].default is False


@pytest.mark.parametrize("with_bias", [False, True])
def test_fold_formula_of_the_helper_matches_torch_float64(with_bias):
    """guards the reference the GPU tests compare the fold kernel with"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 9, 9, generator=g, dtype=torch.float64)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64)
    cb = torch.randn(7, generator=g, dtype=torch.float64) if with_bias else None
    gamma = torch.randn(7, generator=g, dtype=torch.float64)
    gamma[1], gamma[2] = 0.0, -1e-6                        # zero, tiny negative
    beta = torch.randn(7, generator=g, dtype=torch.float64)
    rm = torch.randn(7, generator=g, dtype=torch.float64)
    rv = torch.rand(7, generator=g, dtype=torch.float64) * 3 + 0.01
    rv[3] = 4000.0
    want = F.batch_norm(F.conv2d(x, w, cb, stride=2, padding=1), rm, rv, gamma, beta, training=False, eps=1e-5)
    wf, bf, _ = fold_ref64(w, cb, gamma, beta, rm, rv, 1e-5)
    got = F.conv2d(x, wf, bf, stride=2, padding=1)
    assert (got - want).abs().max() < 1e-12 * max(1.0, float(want.abs().max()))
