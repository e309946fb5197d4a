"""CPU-side checks of the CRNN saliency feature (ecgmm/explain.py: spectrogram_gradients / spectrogram_grad_cam;
csrc/crnn_front.hip: ecgmm_conv5_in1_bwd_data; csrc/plan_crnn.hip: ecgmm_crnn_front_backward_dx; csrc/gradcam.hip:
ecgmm_crnn_gradcam).

tests/crnn_saliency_ref.py -- the float64 restatement the GPU tests hold the kernels to -- is itself held here to textbook
Grad-CAM (Selvaraju et al. 2017) taken with a forward hook on the last ConvBlock of tests/crnn_ref.CRNN().double().eval() and
autograd, at B = 3, F = 33, T = 40, to 1e-12: on the whole record, on records with live steps (textbook Grad-CAM of the live
part of the activation alone -- the padding only rescales the channel weights of a record by Tp / steps, which the
normalisation removes -- with NaN behind the steps in what the restatement is fed), and on an all-zero map.

Every refusal of the three new entry points comes back as an error code with a message before anything is launched, and the
workspace / tile queries run without a GPU; the Python entry points refuse CPU tensors, a model that is no CRNN and a
negative ``saliency_samples``."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from ecgmm.hip import lib as L

from . import crnn_ref as R
from . import crnn_saliency_ref as S

B, FQ, T = 3, 33, 40
TP, FP, CH = T // 8, FQ // 8, 128
TOL = 1e-12


def err():
    return L.lib().ecgmm_last_error()


def textbook(A, dA, steps=None):
    """Grad-CAM from the activation A and the gradient dA [B][C][Fp][Tp] of the chosen logit: per record, on its live part
    A[..., :steps] alone: a_c = mean of dA_c, relu(sum_c a_c A_c), / max (all zero when the maximum is 0); zero behind
    the live part; bilinear upsample to (FQ, T) with align_corners=False"""
    maps = []
    for b in range(A.shape[0]):
        n = A.shape[3] if steps is None else int(steps[b])
        a = dA[b, :, :, :n].mean((1, 2))
        m = torch.relu((a[:, None, None] * A[b, :, :, :n]).sum(0))
        if m.max() > 0:
            m = m / m.max()
        maps.append(F.pad(m, (0, A.shape[3] - n)))
    return F.interpolate(torch.stack(maps)[:, None], size=(FQ, T), mode="bilinear", align_corners=False)[:, 0]


def to_seq(A):
    return A.permute(0, 3, 1, 2).flatten(2)


@pytest.fixture(scope="module")
def hooked():
    """the reference model in float64 eval mode, its last activation and d (predicted logit) / d activation, whole records
    and records of [5, 1, 3] live steps (packed LSTM, mean over each record's own steps)"""
    torch.manual_seed(0)
    ref = R.CRNN().double().eval()
    torch.manual_seed(1)
    x = torch.randn(B, 1, FQ, T, dtype=torch.float64)
    out = {}
    for name, steps in (("whole", None), ("steps", torch.tensor([5, 1, 3]))):
        feats = []
        h = ref.conv3.register_forward_hook(lambda _m, _i, o: feats.append(o))
        try:
            seq = ref.front(x)
        finally:
            h.remove()
        A = feats[0]
        if steps is None:
            y, _ = ref.bilstm(seq)
            logits = ref.classifier(y.mean(dim=1))
        else:
            yp, _ = ref.bilstm(pack_padded_sequence(seq, steps, batch_first=True, enforce_sorted=False))
            y, _ = pad_packed_sequence(yp, batch_first=True, total_length=TP)
            logits = ref.classifier(y.sum(1) / steps.double()[:, None])
        (dA,) = torch.autograd.grad(logits.gather(1, logits.argmax(1, keepdim=True)).sum(), A)
        out[name] = (A.detach(), dA, steps)
    return out


def test_restatement_is_textbook_grad_cam(hooked):
    A, dA, _ = hooked["whole"]
    assert tuple(A.shape) == (B, CH, FP, TP) and float(dA.abs().max()) > 0
    want = textbook(A, dA)
    got = S.gradcam_ref(to_seq(A), to_seq(dA), None, None, CH, FQ, T)
    assert 0.5 < float(want.max()) <= 1.0 and float((got - want).abs().max()) <= TOL
    # frames: the same map with the columns behind them zeroed
    frames = torch.tensor([40, 33, 17])
    cut = S.gradcam_ref(to_seq(A), to_seq(dA), None, frames, CH, FQ, T)
    for b, n in enumerate(frames.tolist()):
        assert torch.equal(cut[b, :, :n], got[b, :, :n]) and bool((cut[b, :, n:] == 0).all())


def test_restatement_with_steps_is_textbook_on_the_live_part(hooked):
    A, dA, steps = hooked["steps"]
    for b, n in enumerate(steps.tolist()):   # the packed LSTM leaves exact zeros behind a record's steps
        assert bool((dA[b, :, :, n:] == 0).all()) and float(dA[b, :, :, :n].abs().max()) > 0
    want = textbook(A, dA, steps)
    seq, dseq = to_seq(A).clone(), to_seq(dA).clone()
    for b, n in enumerate(steps.tolist()):
        seq[b, n:], dseq[b, n:] = float("nan"), float("nan")
    got = S.gradcam_ref(seq, dseq, steps, None, CH, FQ, T)
    assert bool(torch.isfinite(got).all()) and float((got - want).abs().max()) <= TOL
    # and the bound the GPU tests use is finite and small on such inputs
    e = S.gradcam_bound(seq, dseq, steps, None, CH, FQ, T)
    assert bool(torch.isfinite(e).all()) and float(e.max()) < 1e-3


def test_restatement_all_zero_map(hooked):
    A, dA, _ = hooked["whole"]
    assert float(A.min()) >= 0                     # behind a ReLU and a max-pool
    want = textbook(A, -dA.abs())
    got = S.gradcam_ref(to_seq(A), to_seq(-dA.abs()), None, None, CH, FQ, T)
    assert bool((want == 0).all()) and bool((got == 0).all())
    # one record all zero, the others not
    mixed = dA.clone()
    mixed[1] = -dA[1].abs()
    got = S.gradcam_ref(to_seq(A), to_seq(mixed), None, None, CH, FQ, T)
    assert float((got - textbook(A, mixed)).abs().max()) <= TOL and bool((got[1] == 0).all()) and float(got[0].max()) > 0


# ---- the C ABI ----
def _p():
    one = C.c_float(0)
    return one, C.cast(C.pointer(one), C.c_void_p)


def test_conv5_in1_bwd_data_refusals_and_tile_query():
    lib = L.lib()
    _keep, p = _p()
    assert lib.ecgmm_conv5_in1_bwd_data(7, p, p, p, 1, 8, 8, None) == 2 and b"dtype" in err()
    assert lib.ecgmm_conv5_in1_bwd_data(L.F32, p, p, p, 1, 0, 8, None) == 1 and b"bad input" in err()
    assert lib.ecgmm_conv5_in1_bwd_data(L.BF16, p, p, p, 0, 8, 8, None) == 1 and b"bad input" in err()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.ecgmm_conv5_in1_bwd_data(L.F32, *args, 1, 8, 8, None) == 1 and b"null" in err()
    strip, step, rows = C.c_int(0), C.c_int(0), C.c_int(0)
    for H in (1, 2, 33, 100):
        lib.ecgmm_conv5_in1_bwd_data_tile(H, C.byref(strip), C.byref(step), C.byref(rows))
        assert strip.value >= 1 and step.value >= 1 and rows.value >= 1 and rows.value % step.value == 0
    lib.ecgmm_conv5_in1_bwd_data_tile(33, None, None, None)


def test_crnn_front_backward_dx_refusals():
    lib = L.lib()
    _keep, p = _p()
    tab = (C.c_void_p * 12)(*[p.value] * 12)
    d = L.CRNNFrontDesc(2, 33, 40, L.F32, 0, 0.1, 1e-5)
    assert lib.ecgmm_crnn_front_backward_dx(C.byref(d), p, p, tab, None, p, p, 16, p, None) == 3 and b"workspace" in err()
    assert lib.ecgmm_crnn_front_backward_dx(C.byref(d), p, p, tab, None, p, None, 1 << 40, p, None) == 3
    assert lib.ecgmm_crnn_front_backward_dx(C.byref(d), None, p, tab, None, p, p, 1 << 30, p, None) == 1 and b"null" in err()
    nullw = (C.c_void_p * 12)(*([None] + [p.value] * 11))
    assert lib.ecgmm_crnn_front_backward_dx(C.byref(d), p, p, nullw, None, p, p, 1 << 30, p, None) == 1
    assert b"null parameter 0" in err()
    for bad in (L.CRNNFrontDesc(2, 6, 40, L.F32, 0, 0.1, 1e-5), L.CRNNFrontDesc(2, 33, 7, L.F32, 0, 0.1, 1e-5),
                L.CRNNFrontDesc(0, 33, 40, L.F32, 0, 0.1, 1e-5)):
        assert lib.ecgmm_crnn_front_backward_dx(C.byref(bad), p, p, tab, None, p, p, 1 << 30, p, None) == 1
    bad = L.CRNNFrontDesc(2, 33, 40, 7, 0, 0.1, 1e-5)
    assert lib.ecgmm_crnn_front_backward_dx(C.byref(bad), p, p, tab, None, p, p, 1 << 30, p, None) == 2 and b"dtype" in err()


def test_crnn_gradcam_refusals_and_workspace_query():
    lib = L.lib()
    _keep, p = _p()
    sizes = [lib.ecgmm_crnn_gradcam_workspace(b, 71, 4, 128) for b in (1, 2, 8, 64, 256)]
    assert sizes[0] >= (128 + 4 * 71) * 4 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    for shape in ((0, 5, 4, 128), (2, 0, 4, 128), (2, 5, 0, 128), (2, 5, 4, 0)):
        assert lib.ecgmm_crnn_gradcam_workspace(*shape) == 0 and b"bad shape" in err()
    ok = dict(B=2, Tp=5, C=128, Fp=4, F=33, T=40)
    call = lambda seq, dseq, cam, ws, nb, **kw: lib.ecgmm_crnn_gradcam(
        seq, dseq, None, None, ws, nb, cam, *[{**ok, **kw}[k] for k in ("B", "Tp", "C", "Fp", "F", "T")], None)
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert call(*args, p, 1 << 30) == 1 and b"null" in err()
    for k in ok:
        assert call(p, p, p, p, 1 << 30, **{k: 0}) == 1 and b"bad shape" in err(), k
    assert call(p, p, p, p, 16) == 3 and b"workspace" in err()
    assert call(p, p, p, None, 1 << 40) == 3 and b"workspace" in err()


# ---- Python ----
def test_python_refusals():
    from ecgmm import explain as X
    from ecgmm import train_physionet2 as T2
    from ecgmm.crnn import CRNN
    net = CRNN()
    x = torch.zeros(2, 1, 33, 40)
    for fn in (X.spectrogram_gradients, X.spectrogram_grad_cam):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(net, x)
        with pytest.raises(ValueError, match="needs a CRNN"):
            fn(torch.nn.Linear(4, 2), x)
    assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())
    with pytest.raises(ValueError, match="saliency_samples=-1"):
        T2.main(saliency_samples=-1)
    cfg = type("Neg", (T2.Config,), {"physionet2_saliency_samples": -3})
    with pytest.raises(ValueError, match="saliency_samples=-3"):
        T2.main(cfg)
