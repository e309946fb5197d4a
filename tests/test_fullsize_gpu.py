"""BASELINE full sizes (batch 256, 3x224x224 + 5000 + 16, bf16) are too big for the CPU oracle to
follow in seconds, so they are checked through size-independent properties: run-to-run bitwise
determinism (no float atomics anywhere on the path), BatchNorm output statistics, linearity of the
conv kernels, agreement of the concurrent-stream schedule with the serialized one, loss descent."""
import ctypes as C

import pytest
import torch

from ecgmm.config import Config
from ecgmm.hip import functional as HF
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.multimodal_paper_modal_balance import ECGMultimodalModel
from ecgmm.optim import FusedAdam
from ecgmm.parallel import flatten

from .util import switch_get, switches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 256


def _model(seed=42, overlap=True):
    cfg = type("FullCfg", (Config,), {})
    cfg.compute_dtype, cfg.clinical_input_dim, cfg.overlap_encoders = "bf16", 16, overlap
    torch.manual_seed(seed)
    HF.manual_seed(seed)
    m = ECGMultimodalModel(cfg).to(DEV).train()
    return m


def _batch():
    g = torch.Generator().manual_seed(7)
    return (torch.randn(B, 3, 224, 224, generator=g).clamp_(-1, 1).to(DEV), torch.randn(B, 5000, generator=g).to(DEV),
            torch.randn(B, 16, generator=g).to(DEV), torch.randint(0, 2, (B,), generator=g).to(DEV))


def _one_step(model, batch):
    img, sig, clin, lab = batch
    out = model(img, sig, clin)
    loss = HF.cross_entropy(out[3], lab) + 0.1 * out[4]
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), out[3].detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()
                                                   if p.grad is not None}


def test_full_size_step_is_bitwise_deterministic_and_schedule_independent():
    batch = _batch()
    runs = []
    for overlap, side in ((True, 1), (True, 1), (False, 0)):
        L.check(L.lib().ecgmm_side_wgrad(side))
        m = _model(overlap=overlap)
        HF.manual_seed(123)                       # same dropout masks in every run
        runs.append(_one_step(m, batch))
        del m
    L.check(L.lib().ecgmm_side_wgrad(switch_get(L.lib(), "ECGMM_SIDE_WGRAD")))   # back to what the process started with
    (l0, y0, g0), (l1, y1, g1), (l2, y2, g2) = runs
    assert l0 == l1 == l2 and torch.equal(y0, y1) and torch.equal(y0, y2)
    for k in g0:                                  # run to run: identical bits
        assert torch.equal(g0[k], g1[k]), k
    # Concurrent streams vs one stream: the forward, every activation gradient and every per-channel gradient are
    # identical bits (pure scheduling).  The split-K weight gradients are launched NARROW (half the CUs, half the splits)
    # when they run on the side stream and full-width when they have the GPU to themselves (conv_wgrad.hip,
    # pick_nsplit): same products, another fp32 summation order.
    for k in g0:
        if g0[k].ndim >= 2:
            assert (g0[k] - g2[k]).norm() <= 1e-5 * g2[k].norm() + 1e-12, k
        else:
            assert torch.equal(g0[k], g2[k]), k
    assert all(torch.isfinite(v).all() for v in g0.values())


def test_full_size_training_descends_and_updates_running_stats():
    m = _model()
    flatten(m)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    batch = _batch()
    img, sig, clin, lab = batch
    losses = []
    for _ in range(6):
        opt.zero_grad()
        out = m(img, sig, clin)
        loss = HF.cross_entropy(out[3], lab) + 0.1 * out[4]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] and all(l == l for l in losses)
    assert int(m.image_encoder.bn1.num_batches_tracked) == 6
    assert int(m.signal_encoder.layer3.bn2.num_batches_tracked) == 6
    assert float(m.image_encoder.layer4[1].bn2.running_var.min()) > 0
    w = out[5].cpu()
    assert abs(float(w.sum()) - 1.0) < 1e-5 and out[3].shape == (B, 2)


def test_conv_kernels_are_linear_at_full_size():
    """conv(x1 + x2) == conv(x1) + conv(x2) up to bf16 output rounding, layer1 shape at batch 256."""
    lib = L.lib()
    N, H, W, Cn = B, 56, 56, 64
    d = L.ConvDesc(N, H, W, Cn, Cn, 3, 3, 1, 1, 1)
    g = torch.Generator(device=DEV).manual_seed(3)
    x1 = (torch.randn(N * H * W * Cn, device=DEV, generator=g)).to(torch.bfloat16)
    x2 = (torch.randn(N * H * W * Cn, device=DEV, generator=g)).to(torch.bfloat16)
    w = (torch.randn(Cn * Cn * 9, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    xs = (x1.float() + x2.float()).to(torch.bfloat16)
    ys = []
    for x in (x1, x2, xs):
        y = torch.empty(N * H * W * Cn, device=DEV, dtype=torch.bfloat16)
        L.check(lib.ecgmm_conv_fwd(L.BF16, C.byref(d), ptr(x), ptr(w), None, ptr(y), None, 0, stream()))
        ys.append(y.float())
    torch.cuda.synchronize()
    # xs itself is rounded to bf16, so compare against that rounding budget
    err = (ys[2] - (ys[0] + ys[1])).abs()
    scale = ys[2].abs().mean()
    assert float(err.mean() / scale) < 2e-2
    # and BatchNorm partial sums from the epilogue reproduce the column sums of what was stored
    rows = lib.ecgmm_conv_stats_rows(N * H * W)
    stats = torch.zeros(rows + 64, 2, Cn, device=DEV)
    y = torch.empty(N * H * W * Cn, device=DEV, dtype=torch.bfloat16)
    L.check(lib.ecgmm_conv_fwd(L.BF16, C.byref(d), ptr(xs), ptr(w), None, ptr(y), ptr(stats), 0, stream()))
    torch.cuda.synchronize()
    col = y.float().view(-1, Cn)
    # (stats come from the fp32 accumulators, col from the bf16-stored values: sqrt(N) * 2^-9 * |y| of slack)
    assert torch.allclose(stats[:rows, 0].sum(0), col.sum(0), rtol=2e-3, atol=20.0)
    assert torch.allclose(stats[:rows, 1].sum(0), (col * col).sum(0), rtol=5e-3)



def test_pingpong_conv_loop_is_race_free_under_concurrent_load():
    """The ping-pong K loop of the 128-channel 3x3 tiles (conv_halo_kernel<..., PP>: waves 4-7 one barrier behind waves 0-3,
    LDS-DMA fills retired by counted vmcnt) is a synchronisation structure of its own: screen it for timing-dependent races.
    Layers 2-4 at batch 256, forward and input gradient, 12 launches each while another stream streams 1 GB copies through the
    chip: every launch must reproduce the lock-step kernel's output bit for bit."""
    lib = L.lib()
    side = torch.cuda.Stream()
    big_a = torch.empty(256 << 20, device=DEV, dtype=torch.uint8)
    big_b = torch.empty_like(big_a)
    g = torch.Generator(device=DEV).manual_seed(5)
    with switches(lib, ECGMM_HALO_PP=1):   # (run() sets it; the value from before the test comes back on exit)
        for (H, W, Cn) in ((28, 28, 128), (14, 14, 256), (7, 7, 512)):
            d = L.ConvDesc(B, H, W, Cn, Cn, 3, 3, 1, 1, 1)
            n = B * H * W * Cn
            x = torch.randn(n, device=DEV, generator=g).to(torch.bfloat16)
            w = (torch.randn(Cn * Cn * 9, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
            for fn in (lib.ecgmm_conv_fwd, lib.ecgmm_conv_bwd_data):
                def run(pp):
                    lib.ecgmm_conv_halo_pingpong(pp)
                    y = torch.empty(n, device=DEV, dtype=torch.bfloat16)
                    if fn is lib.ecgmm_conv_fwd:
                        L.check(fn(L.BF16, C.byref(d), ptr(x), ptr(w), None, ptr(y), None, 0, stream()))
                    else:
                        L.check(fn(L.BF16, C.byref(d), ptr(x), ptr(w), None, ptr(y), stream()))
                    return y
                ref = run(0)
                torch.cuda.synchronize()
                for it in range(12):
                    with torch.cuda.stream(side):
                        big_b.copy_(big_a, non_blocking=True)
                        big_a.copy_(big_b, non_blocking=True)
                    y = run(1)
                    torch.cuda.synchronize()
                    assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), (H, Cn, fn.__name__, it)


def test_stream_form_of_the_layer1_tiles_is_race_free_under_concurrent_load():
    """The stream form of the 64 -> 64 channel 3x3 tiles (conv_halo_kernel<64, 9, ., NCS1, 8, false, ST>: the K loop runs on across
    tile boundaries, the previous tile's stores and the next tile's halo / weights all retire through counted vmcnt waits) is a
    synchronisation structure of its own.  Layer 1 at batch 256 (12.25 tiles per workgroup), forward with per-workgroup statistics
    rows and input gradient without and with the residual addend (conv_halo_kernel<64, 9, 2, ..., ST, AD>), 12 launches each while
    another stream streams 1 GB copies through the chip: every launch must reproduce the tile-at-a-time kernel's output AND
    statistics rows bit for bit."""
    lib = L.lib()
    side = torch.cuda.Stream()
    big_a = torch.empty(256 << 20, device=DEV, dtype=torch.uint8)
    big_b = torch.empty_like(big_a)
    g = torch.Generator(device=DEV).manual_seed(6)
    d = L.ConvDesc(B, 56, 56, 64, 64, 3, 3, 1, 1, 1)
    n = B * 56 * 56 * 64
    x = torch.randn(n, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(64 * 64 * 9, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    add = torch.randn(n, device=DEV, generator=g).to(torch.bfloat16)      # residual addend of a block's conv1 input gradient
    with switches(lib, ECGMM_HALO_STREAM=1):   # (run() sets it; the value from before the test comes back on exit)
        for kind in ("fwd", "dgrad", "dgrad+addend"):
            def run(on):
                lib.ecgmm_conv_halo_stream(on)
                y = torch.empty(n, device=DEV, dtype=torch.bfloat16)
                st = torch.zeros(512 * 2 * 64, device=DEV)
                rows = C.c_int(0)
                if kind == "fwd":
                    L.check(lib.ecgmm_conv_fwd_wgrows(L.BF16, C.byref(d), ptr(x), ptr(w), None, ptr(y), ptr(st), C.byref(rows), 0, stream()))
                else:
                    L.check(lib.ecgmm_conv_bwd_data(L.BF16, C.byref(d), ptr(x), ptr(w), ptr(add) if kind == "dgrad+addend" else None,
                                                    ptr(y), stream()))
                return y, st
            ref, ref_st = run(0)
            torch.cuda.synchronize()
            for it in range(12):
                with torch.cuda.stream(side):
                    big_b.copy_(big_a, non_blocking=True)
                    big_a.copy_(big_b, non_blocking=True)
                y, st = run(1)
                torch.cuda.synchronize()
                assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), (kind, it)
                assert torch.equal(st, ref_st), (kind, it)
