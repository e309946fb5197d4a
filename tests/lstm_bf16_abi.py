"""ecgmm_lstm_forward_dt / ecgmm_lstm_backward_dt through ctypes, with the arena, sentinels and NaN prefills of
tests/lstm_abi.py, plus the saved tensors that ecgmm_lstm_ws_view locates (for single-layer calls: dgates of each direction)."""
import ctypes as C

import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from .lstm_abi import DEV, Arena, guarded_bytes, misaligned, table, tail_touched


def view(d, dtype, which, layer, direction, buf):
    """the float view of a saved tensor inside the workspace / scratch tensor `buf`"""
    off, nb = C.c_size_t(), C.c_size_t()
    L.check(L.lib().ecgmm_lstm_ws_view(C.byref(d), dtype, which.encode(), layer, direction, C.byref(off), C.byref(nb)), "ws_view")
    assert off.value % 4 == 0 and nb.value % 4 == 0
    return buf[off.value // 4:(off.value + nb.value) // 4]


def run(case, ins, dtype=L.BF16, lengths=None, use=("y", "h", "c"), save=1, backward=True, null=(), misalign_whh=False,
        x_override=None):
    """as lstm_abi.run, through the _dt entry points.  lengths: a list (device int32 is made here) or None.  Returns
    {name: tensor}; single-layer backward calls also return "dgates0" / "dgates1" ([rows of x][4H], clones)."""
    B, T, In, H, layers, bi, bf, given = case
    mod, x, h0, c0, gy, gh, gc = ins
    lib = L.lib()
    names = [n for n, _ in mod.named_parameters()]
    params = [p.detach().to(DEV).contiguous() for p in mod.parameters()]
    if misalign_whh:
        params = [misaligned(p) if "weight_hh" in n else p for n, p in zip(names, params)]
    dv = lambda t: None if t is None else t.to(DEV).contiguous()
    x, h0, c0, gy, gh, gc = (dv(t) for t in (x if x_override is None else x_override, h0, c0, gy, gh, gc))
    ln = None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32, device=DEV)
    d = L.LSTMDesc(B, T, In, H, layers, int(bi), int(bf), int(save))
    nf = lib.ecgmm_lstm_fwd_workspace_dt(C.byref(d), dtype)
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
    L.check(lib.ecgmm_lstm_forward_dt(C.byref(d), dtype, ptr(x), ptr(ln), table(params), ptr(h0), ptr(c0), ptr(v["y"]),
                                      ptr(v.get("hn")), ptr(v.get("cn")), ptr(ws), nf, stream()), "lstm_forward_dt")
    sc = None
    res = dict(v)
    if backward:
        nb = lib.ecgmm_lstm_bwd_workspace_dt(C.byref(d), dtype)
        assert nb > 0 and nb % 4 == 0, lib.ecgmm_last_error()
        sc = guarded_bytes(nb)
        grads = None if "grads" in null else table([v.get("d" + n) for n in names])
        L.check(lib.ecgmm_lstm_backward_dt(C.byref(d), dtype, ptr(x), ptr(ln), table(params), ptr(h0), ptr(c0),
                                           ptr(gy if "y" in use else None), ptr(gh if "h" in use else None),
                                           ptr(gc if "c" in use else None), ptr(ws), ptr(v.get("dx")), grads,
                                           ptr(v.get("dh0")), ptr(v.get("dc0")), ptr(sc), nb, stream()), "lstm_backward_dt")
        if layers == 1:
            for k in range(2 if bi else 1):
                res["dgates%d" % k] = view(d, dtype, "dgates", 0, k, sc).clone().view(x.shape[0], x.shape[1], 4 * H)
    torch.cuda.synchronize()
    assert not ar.touched(), "written outside an output, next to: %s" % ar.touched()
    assert not tail_touched(ws), "written past the end of the forward workspace"
    assert sc is None or not tail_touched(sc), "written past the end of the backward scratch"
    for k, t in res.items():
        assert bool(torch.isfinite(t).all()), "%s: NaN / inf left in an output" % k
    if save:
        res["_ws"], res["_desc"] = ws, d
    return res
