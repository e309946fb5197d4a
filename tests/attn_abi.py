"""The C entry points of csrc/attention.hip through ctypes, for tests/test_attention_ops_gpu.py: outputs are NaN-filled views
between sentinel zones (tests/tabnet_abi.call), the backward workspace is NaN-filled, exactly as large as the library asks
and followed by sentinels, the keep mask lies between sentinel bytes."""
import ctypes as C

import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from .lstm_abi import DEV, guarded_bytes, tail_touched
from .tabnet_abi import call, dev

MASK_GUARD = 256


def desc(S, N, heads, head_dim, batch_first, p=0.0):
    return L.MHADesc(S, N, heads, head_dim, int(batch_first), float(p))


def forward(qkv, S, N, heads, batch_first, p=0.0, seed=0, offset=0, expect=0):
    """-> {"out": [rows, E], "lse": [N, heads, S]} (cpu)"""
    E = qkv.shape[1] // 3
    d = desc(S, N, heads, E // heads, batch_first, p)
    q = dev(qkv)
    return call("ecgmm_mha_forward", {"out": (S * N, E), "lse": (N, heads, S)},
                lambda v: (C.byref(d), ptr(q), ptr(v["out"]), ptr(v["lse"]), seed, offset), expect=expect)


def backward(qkv, out, lse, dout, S, N, heads, batch_first, p=0.0, seed=0, offset=0):
    """-> dqkv [rows, 3E] (cpu)"""
    E = qkv.shape[1] // 3
    d = desc(S, N, heads, E // heads, batch_first, p)
    nb = L.lib().ecgmm_mha_bwd_workspace(C.byref(d))
    assert nb > 0 and nb % 4 == 0
    ws = guarded_bytes(nb)
    q, o, l, g = dev(qkv), dev(out), dev(lse), dev(dout)
    r = call("ecgmm_mha_backward", {"dqkv": (S * N, 3 * E)},
             lambda v: (C.byref(d), ptr(q), ptr(o), ptr(l), ptr(g), ptr(v["dqkv"]), ptr(ws), nb, seed, offset))
    assert not tail_touched(ws), "mha_backward wrote past its workspace"
    return r["dqkv"]


def keep_mask(S, N, heads, head_dim, batch_first, p, seed, offset):
    """-> uint8 [N, heads, S, S] (cpu); every byte must be written as 0 or 1 and none next to the mask"""
    d = desc(S, N, heads, head_dim, batch_first, p)
    n = N * heads * S * S
    buf = torch.full((n + 2 * MASK_GUARD,), 77, dtype=torch.uint8, device=DEV)
    L.check(L.lib().ecgmm_mha_keep_mask(C.byref(d), ptr(buf[MASK_GUARD:]), seed, offset, stream()), "mha_keep_mask")
    torch.cuda.synchronize()
    assert bool((buf[:MASK_GUARD] == 77).all()) and bool((buf[-MASK_GUARD:] == 77).all()), "written next to the mask"
    m = buf[MASK_GUARD:MASK_GUARD + n].cpu()
    assert bool((m <= 1).all()), "a mask byte was not written"
    return m.reshape(N, heads, S, S)


def embed_fwd(x, w, b, pos):
    B, Cin, Ln = x.shape
    D = w.shape[0]
    x_, w_, b_, p_ = dev(x), dev(w), dev(b), dev(pos)
    return call("ecgmm_embed1d_fwd", {"y": (B, Ln, D)},
                lambda v: (ptr(x_), ptr(w_), ptr(b_), ptr(p_), ptr(v["y"]), B, Cin, Ln, D))["y"]


def embed_bwd(x, w, dy, pos_len, null=()):
    """-> {"dw", "db", "dpos", "dx"} (cpu) without the names in `null`"""
    B, Cin, Ln = x.shape
    D = w.shape[0]
    nb = L.lib().ecgmm_embed1d_bwd_workspace(B, Cin, Ln, D)
    assert nb > 0 and nb % 4 == 0
    ws = guarded_bytes(nb)
    x_, w_, g_ = dev(x), dev(w), dev(dy)
    outs = {"dw": (D, Cin, 3), "db": (D,), "dpos": (pos_len, D), "dx": (B, Cin, Ln)}
    outs = {k: s for k, s in outs.items() if k not in null}
    r = call("ecgmm_embed1d_bwd", outs,
             lambda v: (ptr(x_), ptr(w_), ptr(g_), ptr(v.get("dw")), ptr(v.get("db")), ptr(v.get("dpos")), ptr(v.get("dx")),
                        B, Cin, Ln, D, pos_len, ptr(ws), nb))
    assert not tail_touched(ws), "embed1d_bwd wrote past its workspace"
    return r
