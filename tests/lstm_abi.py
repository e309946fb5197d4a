"""ecgmm_lstm_forward / ecgmm_lstm_backward through ctypes, shared by tests/test_lstm_gpu.py and tests/test_lstm_f64_gpu.py.

Every output is a NaN-filled view into one arena with a zone of GUARD sentinel floats before and after it; the forward
workspace and the backward scratch are NaN-filled, handed over with exactly the size the library reports, and followed by
GUARD sentinel floats.  Every run ends by checking every sentinel, so each caller also tests that nothing is written outside
the outputs."""
import ctypes as C

import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

DEV = "cuda:0"
GUARD = 256                 # floats: 1 KiB
SENTINEL = -12345.671875    # exact in fp32
NAN = float("nan")


class Arena:
    """views [guard | view | pad to 256 B | guard | view | ...] of one allocation; the views start 256-byte aligned"""

    def __init__(self, shapes):
        self.spans, off = {}, GUARD
        for name, shape in shapes.items():
            n = 1
            for s in shape:
                n *= s
            self.spans[name] = (off, n, tuple(shape))
            off = (off + n + 63) // 64 * 64 + GUARD
        self.buf = torch.full((off,), SENTINEL, device=DEV, dtype=torch.float32)
        self.views = {}
        for name, (o, n, shape) in self.spans.items():
            self.buf[o:o + n] = NAN
            self.views[name] = self.buf[o:o + n].view(shape)

    def touched(self):
        """names of the views next to which a sentinel changed"""
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for o, n, _ in self.spans.values():
            mask[o:o + n] = False
        bad = mask & (self.buf != SENTINEL)
        if not bool(bad.any()):
            return []
        idx = bad.nonzero().reshape(-1).tolist()
        return ["%s%+d" % min(((name, i - o) for name, (o, n, _) in self.spans.items()), key=lambda p: abs(p[1])) for i in idx[:8]]


def guarded_bytes(nbytes):
    """NaN-filled buffer of nbytes (a multiple of 4) followed by GUARD sentinels"""
    n = nbytes // 4
    t = torch.full((n + GUARD,), NAN, device=DEV, dtype=torch.float32)
    t[n:] = SENTINEL
    return t


def tail_touched(t):
    return bool((t[-GUARD:] != SENTINEL).any())


def table(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def misaligned(t):
    """a copy of t whose data_ptr() is 4 mod 16: one float into a larger allocation"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def run(case, ins, use=("y", "h", "c"), save=1, backward=True, null=(), misalign_whh=False):
    """The C entry points on the inputs `ins` = (torch module, x, h0, c0, gy, gh, gc) of `case` = (B, T, In, H, layers,
    bidirectional, batch_first, states given).  use: the cotangents handed to the backward (the others are null pointers).
    null: optional pointers passed as null: "hn", "cn", "dx", "dh0", "dc0", "grads" (the whole table) or ("grad", i) (entry i
    of the table).  misalign_whh: every W_hh is one float into a larger allocation.  Returns {name: tensor} of what was
    requested, named as f64check.lstm_run names them."""
    B, T, In, H, layers, bi, bf, given = case
    mod, x, h0, c0, gy, gh, gc = ins
    lib = L.lib()
    names = [n for n, _ in mod.named_parameters()]
    params = [p.detach().to(DEV).contiguous() for p in mod.parameters()]
    if misalign_whh:
        params = [misaligned(p) if "weight_hh" in n else p for n, p in zip(names, params)]
    dv = lambda t: None if t is None else t.to(DEV).contiguous()
    x, h0, c0, gy, gh, gc = (dv(t) for t in (x, h0, c0, gy, gh, gc))
    d = L.LSTMDesc(B, T, In, H, layers, int(bi), int(bf), int(save))
    nf = lib.ecgmm_lstm_fwd_workspace(C.byref(d))
    assert nf > 0 and nf % 4 == 0, lib.ecgmm_last_error()
    shapes = {}
    for k, t in (("y", gy), ("hn", gh), ("cn", gc)):
        if k not in null:
            shapes[k] = t.shape
    if backward:
        if "dx" not in null:
            shapes["dx"] = x.shape
        if given:
            for k, t in (("dh0", h0), ("dc0", c0)):
                if k not in null:
                    shapes[k] = t.shape
        if "grads" not in null:
            for i, (n, p) in enumerate(zip(names, params)):
                if ("grad", i) not in null:
                    shapes["d" + n] = p.shape
    ar = Arena(shapes)
    v = ar.views
    ws = guarded_bytes(nf)
    L.check(lib.ecgmm_lstm_forward(C.byref(d), ptr(x), table(params), ptr(h0), ptr(c0), ptr(v["y"]), ptr(v.get("hn")),
                                   ptr(v.get("cn")), ptr(ws), nf, stream()), "lstm_forward")
    sc = None
    if backward:
        nb = lib.ecgmm_lstm_bwd_workspace(C.byref(d))
        assert nb > 0 and nb % 4 == 0, lib.ecgmm_last_error()
        sc = guarded_bytes(nb)
        grads = None if "grads" in null else table([v.get("d" + n) for n in names])
        L.check(lib.ecgmm_lstm_backward(C.byref(d), ptr(x), table(params), ptr(h0), ptr(c0), ptr(gy if "y" in use else None),
                                        ptr(gh if "h" in use else None), ptr(gc if "c" in use else None), ptr(ws),
                                        ptr(v.get("dx")), grads, ptr(v.get("dh0")), ptr(v.get("dc0")), ptr(sc), nb, stream()),
                "lstm_backward")
    torch.cuda.synchronize()
    assert not ar.touched(), "written outside an output, next to: %s" % ar.touched()
    assert not tail_touched(ws), "written past the end of the forward workspace"
    assert sc is None or not tail_touched(sc), "written past the end of the backward scratch"
    for k, t in v.items():
        assert bool(torch.isfinite(t).all()), "%s: NaN / inf left in an output" % k
    return dict(v)
