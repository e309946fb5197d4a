"""The C entry points of csrc/tabnet.hip and ecgmm_bn_small_eval_bwd through ctypes, for tests/test_tabnet_f64_gpu.py.

Every output is a NaN-filled view into one arena (tests/lstm_abi.Arena) with a zone of sentinel floats before and after it;
call() checks every sentinel after the call and asserts that every output is finite, so each caller also tests that nothing
is written outside the outputs and that every element of them is written.  An output that a call accumulates into is
prefilled; a null optional pointer is an output that is simply not named.  A refused call (expect = an ECGMM_ERR_* code)
must leave every output as it was."""
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from .lstm_abi import DEV, Arena

ERR_SHAPE = 1


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def call(fn, outs, args, prefill=None, expect=0, what=None):
    """fn: the entry point's name; outs {name: shape}; args(v) -> the argument list without the stream, v = {name: view}
    (v.get(name) is None for an output left out: a null pointer); prefill {name: tensor}.  Returns {name: cpu tensor}."""
    lib = L.lib()
    ar = Arena(outs)
    v = ar.views
    for k, t in (prefill or {}).items():
        v[k].copy_(t)
    before = ar.buf.clone()
    rc = getattr(lib, fn)(*args(v), stream())
    torch.cuda.synchronize()
    assert not ar.touched(), "%s wrote outside an output, next to: %s" % (fn, ar.touched())
    if expect:
        assert rc == expect, "%s: code %d, expected %d" % (fn, rc, expect)
        same = (ar.buf == before) | (torch.isnan(ar.buf) & torch.isnan(before))
        assert bool(same.all()), "%s: a refused call wrote to its outputs" % fn
        return None
    L.check(rc, what or fn)
    for k, t in v.items():
        assert bool(torch.isfinite(t).all()), "%s %s: NaN / inf left in an output" % (fn, k)
    return {k: t.cpu() for k, t in v.items()}


def counter(value):
    """an int64 cell between two sentinel cells (nbt): (tensor, pointer to the middle)"""
    t = torch.tensor([-777, value, -777], dtype=torch.int64, device=DEV)
    return t, ptr(t[1:])


def counter_value(t):
    assert int(t[0]) == -777 and int(t[2]) == -777, "written next to nbt"
    return int(t[1])


def glu(z, dout=None):
    N, D = z.shape[0], z.shape[1] // 2
    z_ = dev(z)
    out = call("ecgmm_glu_fwd", {"out": (N, D)}, lambda v: (ptr(z_), ptr(v["out"]), N, D))
    if dout is not None:
        g = dev(dout)
        out.update(call("ecgmm_glu_bwd", {"dz": (N, 2 * D)}, lambda v: (ptr(z_), ptr(g), ptr(v["dz"]), N, D)))
    return out


def sparsemax(x, dp=None, expect=0, D=None):
    N = x.shape[0]
    D = x.shape[1] if D is None else D
    x_ = dev(x)
    out = call("ecgmm_sparsemax_fwd", {"p": tuple(x.shape)}, lambda v: (ptr(x_), ptr(v["p"]), N, D), expect=expect)
    if expect:
        g = dev(torch.ones_like(x))
        call("ecgmm_sparsemax_bwd", {"dx": tuple(x.shape)}, lambda v: (ptr(x_), ptr(g), ptr(v["dx"]), N, D), expect=expect)
        return None
    if dp is not None:
        p_, g = dev(out["p"]), dev(dp)
        out.update(call("ecgmm_sparsemax_bwd", {"dx": tuple(x.shape)}, lambda v: (ptr(p_), ptr(g), ptr(v["dx"]), N, D)))
    return out


def entropy(M, eps, g=None):
    N, D = M.shape
    M_ = dev(M)
    out = call("ecgmm_entropy_fwd", {"out": (1,)}, lambda v: (ptr(M_), ptr(v["out"]), N, D, eps))
    if g is not None:
        g_ = dev(g)
        out.update(call("ecgmm_entropy_bwd", {"dM": (N, D)}, lambda v: (ptr(M_), ptr(g_), ptr(v["dM"]), N, D, eps)))
    return out


def ew(op, a, b, s):
    a_, b_ = dev(a), dev(b)
    return call("ecgmm_ew", {"out": tuple(a.shape)}, lambda v: (op, ptr(a_), ptr(b_), ptr(v["out"]), a.numel(), s))["out"]


def split(x, nd, relu):
    N, D = x.shape
    x_ = dev(x)
    return call("ecgmm_split_cols", {"d": (N, nd), "a": (N, D - nd)},
                lambda v: (ptr(x_), ptr(v["d"]), ptr(v["a"]), N, D, nd, relu))


def split_bwd(d, gd, ga, D, nd, relu):
    N = d.shape[0]
    d_, gd_, ga_ = dev(d), dev(gd), dev(ga)
    return call("ecgmm_split_cols_bwd", {"gx": (N, D)}, lambda v: (ptr(d_), ptr(gd_), ptr(ga_), ptr(v["gx"]), N, D, nd, relu))["gx"]


def bn_fwd(x, gamma, beta, rm0, rv0, nbt0, training, momentum, eps, expect=0):
    """rm0 / rv0 / nbt0 None: null pointers.  Returns y, save and (where given) rm, rv, nbt after the call"""
    N, C = x.shape
    x_, g_, b_ = dev(x), dev(gamma), dev(beta)
    outs = {"y": (N, C), "save": (2, C)}
    pre = {}
    if rm0 is not None:
        outs["rm"], outs["rv"] = (C,), (C,)
        pre = {"rm": rm0, "rv": rv0}
    cnt, cp = (None, None) if nbt0 is None else counter(nbt0)
    out = call("ecgmm_bn_small_fwd", outs,
               lambda v: (ptr(x_), ptr(g_), ptr(b_), ptr(v.get("rm")), ptr(v.get("rv")), cp, ptr(v["y"]), ptr(v["save"]), N, C,
                          int(training), momentum, eps), prefill=pre, expect=expect)
    if cnt is not None:
        n = counter_value(cnt)
        if expect:
            assert n == nbt0, "a refused call changed nbt"
        else:
            out["nbt"] = n
    return out


def bn_bwd(x, dy, gamma, save, training, accumulate, dg0=None, db0=None, null=()):
    """training: ecgmm_bn_small_bwd, else ecgmm_bn_small_eval_bwd (null: any of "dx", "dgamma", "dbeta").  accumulate = 0 leaves
    the NaN prefill in dgamma / dbeta: the kernel must overwrite it"""
    N, C = x.shape
    x_, dy_, g_, s_ = dev(x), dev(dy), dev(gamma), dev(save)
    outs = {k: s for k, s in (("dx", (N, C)), ("dgamma", (C,)), ("dbeta", (C,))) if k not in null}
    pre = {k: t for k, t in (("dgamma", dg0), ("dbeta", db0)) if accumulate and k not in null}
    fn = "ecgmm_bn_small_bwd" if training else "ecgmm_bn_small_eval_bwd"
    return call(fn, outs, lambda v: (ptr(x_), ptr(dy_), ptr(g_), ptr(s_), ptr(v.get("dx")), ptr(v.get("dgamma")),
                                     ptr(v.get("dbeta")), N, C, int(accumulate)), prefill=pre)
