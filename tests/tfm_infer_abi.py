"""The C entry points of csrc/transformer_infer.hip and of the transformer's inference plan through ctypes, shared by
tests/test_tfm_infer_ops_gpu.py and tests/test_tfm_infer_gpu.py.

Every output is a view between sentinel zones (tests/lstm_abi.Arena) prefilled with 0xFF bytes, the plan's workspace is
0xFF-filled, handed over with exactly the size the library reports and followed by sentinels; every run ends by checking the
sentinels.  `per_op_forward` is the plan's forward rebuilt from the per-op entry points in separate buffers; it counts its
calls."""
import ctypes as C

import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from .lstm_abi import DEV, Arena, guarded_bytes, tail_touched

LAYER_KEYS = ("in_w", "in_b", "out_w", "out_b", "w1", "b1", "w2", "b2", "g1", "be1", "g2", "be2")


def _ff_fill(t):
    t.view(torch.int32).fill_(-1)     # 0xFF in every byte (a NaN pattern)


def _out(R, E):
    ar = Arena({"out": (R, E)})
    _ff_fill(ar.views["out"])
    return ar


def _done(ar, what):
    torch.cuda.synchronize()
    assert not ar.touched(), "%s wrote outside its output, next to: %s" % (what, ar.touched())
    out = ar.views["out"]
    assert bool(torch.isfinite(out).all()), what + ": an element of the output was not written (or is not finite)"
    return out.clone()


def linear_res_ln(c, R=None, rows=None, eps=1e-5):
    """c: device operands of a tfm_infer_ref.linear_case; the first R rows, or the rows `rows` (a slice)"""
    a, res = c["a"], c["res"]
    if rows is not None:
        a, res = a[rows].contiguous(), res[rows].contiguous()
    elif R is not None:
        a, res = a[:R], res[:R]
    ar = _out(a.shape[0], c["w"].shape[0])
    L.check(L.lib().ecgmm_linear_res_ln(ptr(a), ptr(c["w"]), ptr(c["b"]), ptr(res), ptr(c["gamma"]), ptr(c["beta"]),
                                        ptr(ar.views["out"]), a.shape[0], a.shape[1], c["w"].shape[0], eps, stream()),
            "linear_res_ln")
    return _done(ar, "linear_res_ln")


def ffn_res_ln(c, R=None, rows=None, eps=1e-5):
    x = c["x"]
    if rows is not None:
        x = x[rows].contiguous()
    elif R is not None:
        x = x[:R]
    ar = _out(x.shape[0], x.shape[1])
    L.check(L.lib().ecgmm_ffn_res_ln(ptr(x), ptr(c["w1"]), ptr(c["b1"]), ptr(c["w2"]), ptr(c["b2"]), ptr(c["gamma"]),
                                     ptr(c["beta"]), ptr(ar.views["out"]), x.shape[0], x.shape[1], c["w1"].shape[0], eps,
                                     stream()), "ffn_res_ln")
    return _done(ar, "ffn_res_ln")


def to_dev(c):
    return {k: v.to(DEV).contiguous() for k, v in c.items()}


# ---- the plan -------------------------------------------------------------------------------------------------------------
def plan_params(B, Ln, cin, E, heads, ff, layers, classes, seed=0):
    """seeded parameters of an ECGTransformer1D on the device, as a dict: conv_w, conv_b, pos [Ln, E], layers [dict of
    LAYER_KEYS], cw1, cb1, cw2, cb2"""
    g = torch.Generator().manual_seed(3000 + seed)
    rn = lambda *s, k=1.0: (k * torch.randn(*s, generator=g)).to(DEV)
    p = dict(conv_w=rn(E, cin, 3, k=0.5), conv_b=rn(E, k=0.1), pos=rn(Ln, E, k=0.5), layers=[])
    for _ in range(layers):
        p["layers"].append(dict(in_w=rn(3 * E, E, k=E ** -0.5), in_b=rn(3 * E, k=0.1), out_w=rn(E, E, k=E ** -0.5),
                                out_b=rn(E, k=0.1), w1=rn(ff, E, k=E ** -0.5), b1=rn(ff, k=0.1), w2=rn(E, ff, k=ff ** -0.5),
                                b2=rn(E, k=0.1), g1=1.0 + rn(E, k=0.1), be1=rn(E, k=0.1), g2=1.0 + rn(E, k=0.1),
                                be2=rn(E, k=0.1)))
    p.update(cw1=rn(64, E, k=E ** -0.5), cb1=rn(64, k=0.1), cw2=rn(classes, 64, k=0.125), cb2=rn(classes, k=0.1))
    return p


def param_table(p):
    t = [p["conv_w"], p["conv_b"], p["pos"]]
    for k in p["layers"]:
        t += [k[n] for n in LAYER_KEYS]
    return t + [p["cw1"], p["cb1"], p["cw2"], p["cb2"]]


def plan_forward(p, x, lengths, heads, batch_first, eps=1e-5):
    """ecgmm_transformer_infer on a blob prepared from `p`; x [B, cin, Ln] and lengths (int32 [B] or None) on the device"""
    lib = L.lib()
    B, cin, Ln = x.shape
    E, ff, classes = p["conv_w"].shape[0], p["layers"][0]["w1"].shape[0], p["cw2"].shape[0]
    d = L.TransformerInferDesc(B, Ln, cin, E, heads, ff, len(p["layers"]), classes, int(batch_first), eps)
    nb = lib.ecgmm_transformer_infer_prepared_bytes(C.byref(d))
    assert nb > 0 and nb % 4 == 0, lib.ecgmm_last_error()
    blob = guarded_bytes(nb)
    _ff_fill(blob[:nb // 4])
    tab = param_table(p)
    L.check(lib.ecgmm_transformer_infer_prepare(C.byref(d), (C.c_void_p * len(tab))(*[t.data_ptr() for t in tab]), ptr(blob), nb,
                                                stream()), "transformer infer prepare")
    nw = lib.ecgmm_transformer_infer_workspace(C.byref(d))
    assert nw > 0 and nw % 4 == 0, lib.ecgmm_last_error()
    ws = guarded_bytes(nw)
    _ff_fill(ws[:nw // 4])
    ar = _out(B, classes)
    L.check(lib.ecgmm_transformer_infer(C.byref(d), ptr(x), ptr(lengths), ptr(blob), nb, ptr(ar.views["out"]), ptr(ws), nw,
                                        stream()), "transformer infer")
    out = _done(ar, "transformer infer")
    assert not tail_touched(blob), "written past the end of the prepared blob"
    assert not tail_touched(ws), "written past the end of the workspace"
    return out


class Calls:
    """a counting front of the library: `calls.fn(...)` checks the return code and counts the call under its name"""

    def __init__(self):
        self.count = {}

    def __getattr__(self, name):
        fn = getattr(L.lib(), name)

        def call(*a):
            self.count[name] = self.count.get(name, 0) + 1
            L.check(fn(*a), name)
        return call

    @property
    def total(self):
        return sum(self.count.values())


def per_op_forward(p, x, lengths, heads, batch_first, eps=1e-5):
    """the same forward from the per-op entry points, every result in a buffer of its own -> (logits, Calls)"""
    B, cin, Ln = x.shape
    E, ff, classes = p["conv_w"].shape[0], p["layers"][0]["w1"].shape[0], p["cw2"].shape[0]
    R = B * Ln
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    lib = Calls()
    if lengths is not None:   # exactly ECGTransformer1D.forward's plumbing
        live = torch.arange(Ln, device=DEV)[None, None, :] < lengths[:, None, None]
        x = x.masked_fill(~live, 0.0).contiguous()
    cur = new(R, E)
    lib.ecgmm_embed1d_fwd(ptr(x), ptr(p["conv_w"]), ptr(p["conv_b"]), ptr(p["pos"]), ptr(cur), B, cin, Ln, E, stream())
    md = L.MHADesc(Ln if batch_first else B, B if batch_first else Ln, heads, E // heads, int(batch_first), 0.0)
    per_layer = []
    for k in p["layers"]:
        before = lib.total
        qkv, att, lse, mid, nxt = new(R, 3 * E), new(R, E), new(R * heads), new(R, E), new(R, E)
        lib.ecgmm_linear_fwd(ptr(cur), ptr(k["in_w"]), ptr(k["in_b"]), ptr(qkv), R, E, 3 * E, L.ACT_NONE, stream())
        if lengths is None:
            lib.ecgmm_mha_forward(C.byref(md), ptr(qkv), ptr(att), ptr(lse), 0, 0, stream())
        else:
            lib.ecgmm_mha_forward_varlen(C.byref(md), ptr(qkv), ptr(lengths), ptr(att), ptr(lse), 0, 0, stream())
        lib.ecgmm_linear_res_ln(ptr(att), ptr(k["out_w"]), ptr(k["out_b"]), ptr(cur), ptr(k["g1"]), ptr(k["be1"]), ptr(mid), R, E,
                                E, eps, stream())
        lib.ecgmm_ffn_res_ln(ptr(mid), ptr(k["w1"]), ptr(k["b1"]), ptr(k["w2"]), ptr(k["b2"]), ptr(k["g2"]), ptr(k["be2"]),
                             ptr(nxt), R, E, ff, eps, stream())
        cur = nxt
        per_layer.append(lib.total - before)
    pooled, h1, logits = new(B, E), new(B, 64), new(B, classes)
    if lengths is None:
        lib.ecgmm_avgpool(L.F32, ptr(cur), ptr(pooled), B, Ln, E, None, stream())
    else:
        lib.ecgmm_seq_mean_varlen_fwd(ptr(cur), ptr(lengths), ptr(pooled), B, Ln, E, stream())
    lib.ecgmm_linear_fwd(ptr(pooled), ptr(p["cw1"]), ptr(p["cb1"]), ptr(h1), B, E, 64, L.ACT_RELU, stream())
    lib.ecgmm_linear_fwd(ptr(h1), ptr(p["cw2"]), ptr(p["cb2"]), ptr(logits), B, 64, classes, L.ACT_NONE, stream())
    torch.cuda.synchronize()
    lib.per_layer = per_layer
    return logits, lib
