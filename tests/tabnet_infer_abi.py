"""The C entry points of csrc/tabnet_infer.hip through ctypes, shared by tests/test_tabnet_infer_ops_gpu.py and
tests/test_tabnet_infer_gpu.py.

The blob is 0xFF-prefilled, handed over with exactly the size the library reports and followed by sentinels; every output is a
0xFF-prefilled view between sentinel zones (tests/lstm_abi.Arena); every run ends by checking the sentinels and that every
element of a requested output was written.  `unpack` reads the folded layers back out of a blob (the layout of the comment in
csrc/tabnet_infer.hip), padding included."""
import ctypes as C
from types import SimpleNamespace as NS

import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import tabnet_infer_ref as R
from .lstm_abi import DEV, Arena, guarded_bytes, tail_touched

OPTIONAL = ("m_explain", "masks", "row_entropy")


def _ff_fill(t):
    t.view(torch.int32).fill_(-1)     # 0xFF in every byte (a NaN pattern)


def desc(c, bn_eps=R.BN_EPS):
    return L.TabNetInferDesc(c.D, c.n_d, c.n_a, c.n_steps, c.n_shared, c.n_independent, c.out_dim, c.gamma, c.epsilon, bn_eps)


def prepare(c, params):
    """ecgmm_tabnet_infer_prepare on the device tensors `params` (tabnet_infer_ref.param_table order) -> (blob, bytes)"""
    lib = L.lib()
    d = desc(c)
    nb = lib.ecgmm_tabnet_infer_prepared_bytes(C.byref(d))
    assert nb > 0 and nb % 256 == 0, lib.ecgmm_last_error()
    blob = guarded_bytes(nb)
    _ff_fill(blob[:nb // 4])
    tab = (C.c_void_p * len(params))(*[t.data_ptr() for t in params])
    L.check(lib.ecgmm_tabnet_infer_prepare(C.byref(d), tab, ptr(blob), nb, stream()), "tabnet infer prepare")
    torch.cuda.synchronize()
    assert not tail_touched(blob), "written past the end of the prepared blob"
    assert bool(torch.isfinite(blob[:nb // 4]).all()), "a float of the blob was not written (or is not finite)"
    return blob, nb


def to_dev(model):
    return [t.detach().to(DEV).contiguous() for t in R.param_table(model)]


def unpack(c, blob, nb):
    """the folded layers of a blob, on the CPU: NS(bn0=(scale [64], shift [64]), ft[f][l] = (W' [2W, Kp], b' [pad64(2W)]),
    att[s] = (W' [Dp, n_a], b' [64]), final [out_dim, n_d])"""
    b = blob.detach().cpu()
    W, Dp = c.n_d + c.n_a, (c.D + 15) // 16 * 16
    pad64 = lambda n: (n + 63) // 64 * 64
    layers = c.n_shared + c.n_independent
    off = 128
    ft = []
    for f in range(c.n_steps + 1):
        row = []
        for l in range(layers):
            Kp = Dp if l == 0 else W
            w = b[off:off + 2 * W * Kp].view(2 * W, Kp)
            off += 2 * W * Kp
            row.append((w, b[off:off + pad64(2 * W)]))
            off += pad64(2 * W)
        ft.append(row)
    att = []
    for s in range(c.n_steps):
        w = b[off:off + Dp * c.n_a].view(Dp, c.n_a)
        off += Dp * c.n_a
        att.append((w, b[off:off + 64]))
        off += 64
    final = b[off:off + c.out_dim * c.n_d].view(c.out_dim, c.n_d)
    off += c.out_dim * c.n_d
    assert 4 * off == nb, "the layout walk of the blob ends at %d bytes, the library reports %d" % (4 * off, nb)
    return NS(bn0=(b[:64], b[64:128]), ft=ft, att=att, final=final, floats=off)


def forward(c, blob, nb, x, want=OPTIONAL):
    """ecgmm_tabnet_infer on x (device, [B, D]) -> {out, m_explain, masks, row_entropy} (the unrequested ones None)"""
    B = x.shape[0]
    shapes = {"out": (B, c.out_dim)}
    if "m_explain" in want:
        shapes["m_explain"] = (B, c.D)
    if "masks" in want:
        shapes["masks"] = (c.n_steps, B, c.D)
    if "row_entropy" in want:
        shapes["row_entropy"] = (B,)
    ar = Arena(shapes)
    for v in ar.views.values():
        _ff_fill(v)
    v = ar.views
    L.check(L.lib().ecgmm_tabnet_infer(C.byref(desc(c)), ptr(x), B, ptr(blob), nb, ptr(v["out"]), ptr(v.get("m_explain")),
                                       ptr(v.get("masks")), ptr(v.get("row_entropy")), stream()), "tabnet infer")
    torch.cuda.synchronize()
    assert not ar.touched(), "tabnet infer wrote outside an output, next to: %s" % ar.touched()
    assert not tail_touched(blob), "tabnet infer wrote past the end of the blob"
    got = {k: None for k in ("out",) + OPTIONAL}
    for k, t in v.items():
        assert bool(torch.isfinite(t).all()), "%s: an element was not written (or is not finite)" % k
        got[k] = t.clone()
    return got
