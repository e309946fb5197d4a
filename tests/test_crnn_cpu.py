"""CPU-side checks of the CRNN front end's per-op entry points (csrc/crnn_front.hip; train_physionet2.py:55-65, 87-93): the
workspace queries run without a GPU, are positive and monotone in the batch, and every refusal comes back as an error code
with a message before anything is launched.  ecgmm_conv_bwd_weight goes on refusing a 5x5 descriptor: the 25-tap weight
gradient has its own entry point."""
import ctypes as C

from ecgmm.hip import lib as L


def desc5(N=2, H=16, W=37, Cin=32, Cout=64, **kw):
    f = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, R=5, S=5, stride=1, pad_h=2, pad_w=2)
    f.update(kw)
    return L.ConvDesc(*[f[k] for k in ("N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad_h", "pad_w")])


def err():
    return L.lib().ecgmm_last_error()


def test_conv_bwd_weight_still_refuses_25_taps():
    lib = L.lib()
    d = desc5(1, 8, 8, 64, 64)
    one = C.c_float(0)
    ws = C.cast(C.pointer(one), C.c_void_p)   # (its workspace-present check comes first; the shape check before any launch)
    assert lib.ecgmm_conv_bwd_weight(L.BF16, C.byref(d), None, None, None, 0, ws, 1 << 30, None) == 1
    assert lib.ecgmm_conv_bwd_weight(L.F32, C.byref(d), None, None, None, 0, ws, 1 << 30, None) == 1


def test_workspace_queries_positive_and_monotone_in_batch():
    lib = L.lib()
    for dt in (L.F32, L.BF16):
        sizes = [lib.ecgmm_conv5_bwd_weight_workspace(dt, C.byref(desc5(N=n))) for n in (1, 2, 8, 64, 256)]
        assert sizes[0] >= 64 * 32 * 25 * 4 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    sizes = [lib.ecgmm_conv5_in1_bwd_weight_workspace(n, 33, 70) for n in (1, 2, 8, 64, 256)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    rows = [lib.ecgmm_conv5_in1_stats_rows(n, 33, 70) for n in (1, 2, 8, 64)]
    assert rows[0] >= 1 and rows == sorted(rows) and rows[-1] > rows[0]
    assert lib.ecgmm_pool2_bn_bwd_workspace(2, 9, 11, 32) > 0
    assert lib.ecgmm_pool2_bn_bwd_workspace(2, 9, 11, 128) > lib.ecgmm_pool2_bn_bwd_workspace(2, 9, 11, 32)


def test_conv5_bwd_weight_refusals():
    lib = L.lib()
    bad = [(desc5(R=3, S=3, pad_h=1, pad_w=1), b"5x5"), (desc5(stride=2), b"5x5"), (desc5(pad_h=1), b"5x5"),
           (desc5(Cin=48), b"multiples of 32"), (desc5(Cout=16), b"multiples of 32"), (desc5(N=0), b"multiples of 32")]
    for d, word in bad:
        assert lib.ecgmm_conv5_bwd_weight_workspace(L.BF16, C.byref(d)) == 0 and word in err()
        assert lib.ecgmm_conv5_bwd_weight(L.BF16, C.byref(d), None, None, None, 0, None, 0, None) == 1 and word in err()
    assert lib.ecgmm_conv5_bwd_weight_workspace(7, C.byref(desc5())) == 0 and b"dtype" in err()
    assert lib.ecgmm_conv5_bwd_weight(7, C.byref(desc5()), None, None, None, 0, None, 0, None) == 2 and b"dtype" in err()
    # the checks come in front of any launch: null operands, then a short workspace
    assert lib.ecgmm_conv5_bwd_weight(L.F32, C.byref(desc5()), None, None, None, 0, None, 0, None) == 1 and b"null" in err()
    one = C.c_float(0)
    p = C.cast(C.pointer(one), C.c_void_p)
    assert lib.ecgmm_conv5_bwd_weight(L.F32, C.byref(desc5()), p, p, p, 0, p, 4, None) == 3 and b"workspace" in err()
    assert lib.ecgmm_conv5_bwd_weight(L.F32, C.byref(desc5()), p, p, p, 0, None, 1 << 40, None) == 3


def test_conv5_in1_refusals():
    lib = L.lib()
    one = C.c_float(0)
    p = C.cast(C.pointer(one), C.c_void_p)
    assert lib.ecgmm_conv5_in1_fwd(7, p, p, None, p, None, 1, 8, 8, None) == 2 and b"dtype" in err()
    assert lib.ecgmm_conv5_in1_fwd(L.F32, p, p, None, p, None, 1, 0, 8, None) == 1 and b"bad input" in err()
    assert lib.ecgmm_conv5_in1_fwd(L.F32, None, p, None, p, None, 1, 8, 8, None) == 1 and b"null" in err()
    assert lib.ecgmm_conv5_in1_bwd_weight_workspace(0, 8, 8) == 0
    assert lib.ecgmm_conv5_in1_bwd_weight(L.BF16, p, p, p, p, 0, p, 4, 2, 9, 11, None) == 3 and b"workspace" in err()
    assert lib.ecgmm_conv5_in1_bwd_weight(L.BF16, None, p, p, p, 0, p, 1 << 30, 2, 9, 11, None) == 1


def test_pool2_refusals():
    lib = L.lib()
    one = C.c_float(0)
    p = C.cast(C.pointer(one), C.c_void_p)
    for N, H, W, Cn in ((2, 1, 8, 32), (2, 8, 1, 32), (2, 8, 8, 48), (2, 8, 8, 16), (2, 8, 8, 512), (0, 8, 8, 32)):
        assert lib.ecgmm_bnrelu_maxpool2(L.F32, p, p, p, None, N, H, W, Cn, 0, None) == 1 and b"bnrelu_maxpool2" in err()
        assert lib.ecgmm_pool2_bn_bwd_workspace(N, H, W, Cn) == 0
        assert lib.ecgmm_pool2_bn_bwd(L.F32, p, p, p, p, 1, None, None, p, None, N, H, W, Cn, 0, p, 1 << 30, None) == 1
    assert lib.ecgmm_bnrelu_maxpool2(7, p, p, p, None, 2, 8, 8, 32, 0, None) == 2 and b"dtype" in err()
    assert lib.ecgmm_bnrelu_maxpool2(L.F32, None, p, p, None, 2, 8, 8, 32, 0, None) == 1 and b"null" in err()
    assert lib.ecgmm_pool2_bn_bwd(L.F32, p, p, p, p, 1, None, None, p, None, 2, 8, 8, 32, 0, p, 4, None) == 3
    assert b"workspace" in err()


# ---- the launch plan and the module (csrc/plan_crnn.hip, ecgmm/crnn.py) ----
def test_crnn_state_dict_matches_the_reference_restatement():
    import torch
    from ecgmm.crnn import CRNN, ConvBlock
    from . import crnn_ref as R
    mine, ref = CRNN(), R.CRNN()
    a, b = mine.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    assert "conv1.block.0.weight" in a and "conv1.block.1.running_mean" in a
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    mine.load_state_dict(b, strict=True)
    ref.load_state_dict(mine.state_dict(), strict=True)
    assert isinstance(mine.conv2, ConvBlock)


def test_crnn_refusals():
    import pytest
    import torch
    from ecgmm.crnn import CRNN, FocalLoss  # noqa: F401
    with pytest.raises(ValueError, match="input_channels"):
        CRNN(input_channels=3)
    with pytest.raises(ValueError, match="bf16"):
        CRNN(compute_dtype="fp8")
    net = CRNN()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(2, 1, 33, 40))
    with pytest.raises(RuntimeError, match="launch plan"):
        net.conv1(torch.zeros(2, 1, 33, 40))


def test_crnn_front_workspace_queries_and_desc_refusals():
    lib = L.lib()
    q = lambda B, F=33, T=573, dt=L.F32: (lib.ecgmm_crnn_front_fwd_workspace(C.byref(L.CRNNFrontDesc(B, F, T, dt, 1, 0.1, 1e-5))),
                                          lib.ecgmm_crnn_front_bwd_workspace(C.byref(L.CRNNFrontDesc(B, F, T, dt, 1, 0.1, 1e-5))))
    sizes = [q(b) for b in (1, 2, 8, 64, 256)]
    assert all(f > 0 and b > 0 for f, b in sizes) and sizes == sorted(sizes)
    assert sizes[-1][0] > sizes[0][0] and sizes[-1][1] > sizes[0][1]
    assert q(4, dt=L.BF16)[0] < q(4)[0]
    assert q(2, F=7) == (0, 0) and b"F = 7" in err()
    assert q(2, T=7) == (0, 0) and b"T = 7" in err()
    assert q(2, dt=7) == (0, 0) and b"dtype" in err()
    assert q(0) == (0, 0)
    one = C.c_float(0)
    p = C.cast(C.pointer(one), C.c_void_p)
    tab = (C.c_void_p * 12)(*[p.value] * 12)
    d = L.CRNNFrontDesc(2, 33, 40, L.F32, 1, 0.1, 1e-5)
    assert lib.ecgmm_crnn_front_forward(C.byref(d), p, tab, tab, p, p, 16, None) == 3 and b"workspace" in err()
    assert lib.ecgmm_crnn_front_backward(C.byref(d), p, p, tab, tab, p, p, 16, None) == 3 and b"workspace" in err()
    bad = L.CRNNFrontDesc(2, 6, 40, L.F32, 1, 0.1, 1e-5)
    assert lib.ecgmm_crnn_front_forward(C.byref(bad), p, tab, tab, p, p, 1 << 30, None) == 1
