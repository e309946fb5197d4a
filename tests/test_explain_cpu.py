"""CPU-side checks of the explanation surface: the new ABI entries are declared, bound and exported, and the explain
functions refuse CPU tensors like every other product module (there is no torch-CPU path)."""
import ctypes
import os

import pytest
import torch

from ecgmm import explain
from ecgmm.config import Config
from ecgmm.hip import lib as L
from ecgmm.image_encoder import ResNet18
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel

NEW = ("ecgmm_stem_bwd_data", "ecgmm_resnet18_backward_dx", "ecgmm_resnet1d_backward_dx", "ecgmm_resnet18_gradcam",
       "ecgmm_resnet1d_gradcam", "ecgmm_bn_eval_bwd", "ecgmm_bn_small_eval_bwd", "ecgmm_gradcam")


def test_new_entry_points_are_declared_bound_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ecgmm.h")).read()
    h = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name + "(" in header and name in L.SIGNATURES and hasattr(h, name), name
    assert L.lib().ecgmm_version() == 100


def test_gradcam_op_refusals_launch_nothing():
    """ecgmm_gradcam checks its arguments before its first launch: every refusal answers without a GPU"""
    lib = L.lib()
    p = ctypes.c_void_p(256)             # never dereferenced: each call below is refused first
    for args, msg in (((L.F32, None, p, p, p, 2, 7, 7, 512, 224, 224), b"null"), ((L.BF16, p, p, p, None, 2, 7, 7, 512, 224, 224), b"null"),
                      ((L.F32, p, p, p, p, 2, 0, 7, 512, 224, 224), b"bad shape"), ((L.F32, p, p, p, p, 2, 7, 7, 512, 224, 0), b"bad shape"),
                      ((L.F32, p, p, p, p, 1, 46341, 46341, 8, 4, 4), b"too large"), ((L.F32, p, p, p, p, 1, 2, 2, 8, 65536, 32768), b"too large")):
        assert lib.ecgmm_gradcam(*args, None) != 0 and msg in lib.ecgmm_last_error(), args


def test_explain_refuses_cpu_tensors():
    cfg = type("C16", (Config,), {"clinical_input_dim": 16})
    m = ECGMultimodalModel(cfg).train()
    args = (torch.zeros(2, 3, 64, 64), torch.zeros(2, 500), torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain.input_gradients(m, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain.grad_cam(m, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        explain.encoder_grad_cam(ResNet18(num_classes=2), args[0])
    assert m.training and all(p.requires_grad for p in m.parameters())   # the refusal leaves the model as it was
    with pytest.raises(ValueError, match="output must be"):
        explain._logits((None,) * 6, "nope")


def test_overlay_draws_uint8_pictures():
    heat, mixed = explain.overlay(torch.rand(3, 8, 12), torch.linspace(0, 1, 96).reshape(8, 12))
    assert heat.shape == mixed.shape == (8, 12, 3) and str(heat.dtype) == "uint8"
    assert heat[0, 0, 2] > heat[0, 0, 0] and heat[-1, -1, 0] > heat[-1, -1, 2]   # cold corner blue, hot corner red
