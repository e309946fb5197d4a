"""The TabNet row kernels, the small BatchNorm and Ghost-BatchNorm against float64, op by op, and the whole encoder stage by
stage from its own stored tensors (bounds and input families: the TabNet section of tests/f64check.py; the C entry points go
through tests/tabnet_abi.py, whose every call checks the sentinels around every output and that every output is finite).

Each test prints the worst ratio to its derived bound; nothing here is calibrated against the kernels.  The ratios measured
on the MI355X are recorded in DESIGN.md (f3 TabNet, "Checks")."""
import pytest
import torch

from ecgmm import tabnet as G
from ecgmm.hip import functional as HF
from ecgmm.hip import nn as hnn
from oracle import fill

from . import f64check as F64
from . import tabnet_abi as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


def say(what, **ratios):
    print("[tabnet f64] %-40s %s" % (what, "  ".join("%s %.3g" % kv for kv in ratios.items())))


# ---------------------------------------------------------------------------------------------------------------------
# the row kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", F64.SPMAX_D)
@pytest.mark.parametrize("family", F64.SPMAX_FAMILIES)
def test_sparsemax_forward_backward(family, D):
    worst = {"p": 0.0, "row_sum": 0.0, "dx": 0.0}
    for N in F64.TAB_ROWS:
        x = F64.sparsemax_rows(N, D, family)
        dp = fill.hash_tensor((N, D), 81)
        out = A.sparsemax(x, dp)
        r = F64.check_sparsemax(x, out["p"], "sparsemax %s N=%d D=%d" % (family, N, D))
        rb = F64.check_sparsemax_bwd(out["p"], dp, out["dx"], "sparsemax bwd %s N=%d D=%d" % (family, N, D))
        worst = {"p": max(worst["p"], r.ratio), "row_sum": max(worst["row_sum"], r.row_sum), "dx": max(worst["dx"], rb.ratio)}
    say("sparsemax %s D=%d" % (family, D), **worst)


@pytest.mark.parametrize("D", [65, 0])
def test_sparsemax_refuses_a_width_outside_1_to_64(D):
    x = fill.hash_tensor((7, max(D, 1)), 82)
    A.sparsemax(x, expect=A.ERR_SHAPE, D=D)


@pytest.mark.parametrize("extreme", [False, True], ids=["hash", "pm100"])
@pytest.mark.parametrize("D", F64.GLU_D)
def test_glu_forward_backward(D, extreme):
    worst, seen = {}, 0.0
    for N in F64.TAB_ROWS:
        z, dout = F64.glu_inputs(N, D, extreme)
        out = A.glu(z, dout)
        res = F64.check_glu(z, out["out"], dout, out["dz"], "glu N=%d D=%d" % (N, D))
        if extreme:     # the gate is 0 or 1 within the bound where expf overflowed / underflowed, and nothing is NaN
            s, b = out["dz"][:, :D].double() / dout.double(), z[:, D:]       # the gate as the kernel applied it (one rounding off)
            lim = (F64.K_SIG + 2) * F64.U
            assert bool(((s - 1).abs()[b >= 100] <= lim).all()) and bool((s.abs()[b <= -100] <= lim).all())
        for k, r in res.items():
            worst[k] = max(worst.get(k, 0.0), r.ratio)
            seen = max(seen, r.kappa_seen)
    say("glu D=%d %s" % (D, "pm100" if extreme else "hash"), sigmoid_err_seen_u=seen, **worst)


@pytest.mark.parametrize("D", [2, 5, 64])
def test_entropy_forward_backward(D):
    worst, seen = {}, 0.0
    for N in F64.TAB_ROWS:
        M, g = F64.entropy_inputs(N, D)
        out = A.entropy(M, F64.ENT_EPS, g)
        res = F64.check_entropy(M, out["out"], F64.ENT_EPS, g, out["dM"], "entropy N=%d D=%d" % (N, D))
        for k, r in res.items():
            worst[k] = max(worst.get(k, 0.0), r.ratio)
        seen = max(seen, res["dM"].kappa_seen)
    say("entropy D=%d" % D, bwd_err_seen_u=seen, **worst)


def test_entropy_of_an_all_zero_mask_is_exactly_zero():
    M = torch.zeros(257, 5)
    out = A.entropy(M, F64.ENT_EPS)
    assert float(out["out"]) == 0.0


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("op", list(F64.EW_OPS))
def test_ew_every_op(op, n):
    a, b, s = F64.ew_inputs(n)
    b = b if F64.EW_ARITY[op] == 2 else None
    r = F64.check_ew(op, a, b, s, A.ew(F64.EW_OPS[op], a, b, s), "ew %s n=%d" % (op, n))
    say("ew %s n=%d" % (op, n), ratio=r.ratio)


@pytest.mark.parametrize("op", ["PRIOR", "RSUB"])
def test_ew_grid_stride_second_trip(op):
    """n = 4096 * 256 + 257: the grid is capped at 4096 blocks, so the last 257 elements are a second trip of the loop"""
    n = F64.EW_GRID_CAP + 257
    a, b, s = F64.ew_inputs(n)
    b = b if F64.EW_ARITY[op] == 2 else None
    r = F64.check_ew(op, a, b, s, A.ew(F64.EW_OPS[op], a, b, s), "ew %s n=%d" % (op, n))
    say("ew %s second trip" % op, ratio=r.ratio)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N,D,nd", F64.SPLIT_CASES)
def test_split_cols_and_its_backward_are_exact(N, D, nd, relu):
    x, gd, ga = F64.split_inputs(N, D, nd)
    out = A.split(x, nd, relu)
    d_ref, a_ref = F64.split_ref(x, nd, relu)
    assert torch.equal(out["d"], d_ref) and torch.equal(out["a"], a_ref)
    for use_d, use_a in ((True, True), (False, True), (True, False)):
        gx = A.split_bwd(out["d"], gd if use_d else None, ga if use_a else None, D, nd, relu)
        assert torch.equal(gx, F64.split_bwd_ref(out["d"], gd if use_d else None, ga if use_a else None, D, nd, relu)), (use_d, use_a)


# ---------------------------------------------------------------------------------------------------------------------
# bn_small
# ---------------------------------------------------------------------------------------------------------------------
def _bn_case(N, C, training, momentum=0.02, null=(), mean_ratio=None, accumulate=0):
    d = F64.bn_small_inputs(N, C, mean_ratio)
    gamma = None if "gamma" in null else d["gamma"]
    beta = None if "beta" in null else d["beta"]
    rm0, rv0 = (None, None) if "running" in null else (d["rm0"], d["rv0"])
    nbt0 = None if "nbt" in null else 5
    name = "bn_small N=%d C=%d %s" % (N, C, "train" if training else "eval")
    f = A.bn_fwd(d["x"], gamma, beta, rm0, rv0, nbt0, training, momentum, EPS)
    res, _ = F64.check_bn_small_fwd(d["x"], gamma, beta, rm0, rv0, nbt0, momentum, EPS, training, f["y"], f["save"], f.get("rm"),
                                    f.get("rv"), f.get("nbt"), name)
    b = A.bn_bwd(d["x"], d["dy"], gamma, f["save"], training, accumulate, d["dg0"], d["db0"])
    res2 = F64.check_bn_small_bwd(d["x"], d["dy"], gamma, f["save"], training, b["dx"], b["dgamma"], b["dbeta"],
                                  d["dg0"] if accumulate else None, d["db0"] if accumulate else None, name)
    out = {k: r.ratio for k, r in res.items()}
    out.update({k: r.ratio for k, r in res2.items()})
    return out


@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("C", F64.BN_SMALL_C)
def test_bn_small_forward_backward(C, training):
    worst = {}
    for N in F64.BN_SMALL_N:
        for momentum in (0.01, 0.02):
            for accumulate in (0, 1):
                for k, v in _bn_case(N, C, training, momentum=momentum, accumulate=accumulate).items():
                    worst[k] = max(worst.get(k, 0.0), v)
    say("bn_small C=%d %s" % (C, "train" if training else "eval"), **worst)


@pytest.mark.parametrize("null", ["gamma", "beta", "running", "nbt"])
def test_bn_small_null_optional_pointers(null):
    worst = {}
    for N, C, acc in ((257, 3, 0), (65, 64, 1)):
        for training in ((1,) if null == "running" else (1, 0)):
            for k, v in _bn_case(N, C, training, null=(null,), accumulate=acc).items():
                worst[k] = max(worst.get(k, 0.0), v)
    say("bn_small null %s" % null, **worst)


@pytest.mark.parametrize("N,C", [(128, 2), (513, 64)])
def test_bn_small_at_a_mean_of_1000_standard_deviations(N, C):
    worst = {}
    for training in (1, 0):
        for k, v in _bn_case(N, C, training, mean_ratio=1e3).items():
            worst[k] = max(worst.get(k, 0.0), v)
    say("bn_small mean/std=1e3 N=%d C=%d" % (N, C), **worst)


@pytest.mark.parametrize("null", ["dx", "dgamma", "dbeta", "dgamma+dbeta"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_bn_small_eval_backward_null_outputs(null, accumulate):
    N, C = 257, 3
    d = F64.bn_small_inputs(N, C)
    f = A.bn_fwd(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, 0, 0.02, EPS)
    b = A.bn_bwd(d["x"], d["dy"], d["gamma"], f["save"], 0, accumulate, d["dg0"], d["db0"], null=tuple(null.split("+")))
    assert set(b) == {"dx", "dgamma", "dbeta"} - set(null.split("+"))
    res = F64.check_bn_small_bwd(d["x"], d["dy"], d["gamma"], f["save"], 0, b.get("dx"), b.get("dgamma"), b.get("dbeta"),
                                 d["dg0"] if accumulate else None, d["db0"] if accumulate else None, "bn_small eval bwd")
    say("bn_small eval bwd null %s acc=%d" % (null, accumulate), **{k: r.ratio for k, r in res.items()})


def test_bn_small_refuses_one_row_in_training():
    """torch raises there (one value per channel); the running statistics, nbt, y and save stay as they were"""
    d = F64.bn_small_inputs(1, 3)
    A.bn_fwd(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, 1, 0.02, EPS, expect=A.ERR_SHAPE)
    f = A.bn_fwd(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, 0, 0.02, EPS)          # eval: one row is fine
    F64.check_bn_small_fwd(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, 0.02, EPS, 0, f["y"], f["save"], f["rm"], f["rv"],
                           f["nbt"], "bn_small N=1 eval")


# ---------------------------------------------------------------------------------------------------------------------
# Ghost BatchNorm (the autograd function and the GBN module)
# ---------------------------------------------------------------------------------------------------------------------
def _ghost(B, vbs, C, training, momentum=0.02):
    d = F64.bn_small_inputs(B, C)
    gbn = G.GBN(C, vbs, momentum).to(DEV)
    bn = gbn.bn
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rm0"]); bn.running_var.copy_(d["rv0"])
        bn.num_batches_tracked.fill_(5)
    gbn.train(bool(training))
    x = d["x"].to(DEV).requires_grad_(True)
    y = gbn(x)
    save = y.grad_fn.saved_tensors[1].cpu()
    y.backward(d["dy"].to(DEV))
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu()
    return F64.check_ghost_bn(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, momentum, bn.eps, vbs, training, c(y), save,
                              c(bn.running_mean), c(bn.running_var), int(bn.num_batches_tracked), d["dy"], c(x.grad),
                              c(bn.weight.grad), c(bn.bias.grad), "ghost bn B=%d vbs=%d" % (B, vbs))


@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("B,vbs", F64.GHOST_CASES)
def test_ghost_batchnorm_per_chunk(B, vbs, training):
    worst = {}
    for C in (3, 64):
        for k, v in _ghost(B, vbs, C, training).items():
            worst[k] = max(worst.get(k, 0.0), v)
    say("ghost bn B=%d vbs=%d %s" % (B, vbs, "train" if training else "eval"), **worst)


def test_ghost_batchnorm_raises_on_a_one_row_slice_in_training():
    """B = 257 at vbs = 16: 17 chunks of 16 rows and a last one of a single row; torch's BatchNorm1d raises there"""
    assert F64.ghost_slices(257, 16)[-1] == (256, 257)
    gbn = G.GBN(3, 16).to(DEV).train()
    with pytest.raises((ValueError, RuntimeError)):
        gbn(fill.hash_tensor((257, 3), 83).to(DEV))
    gbn.eval()
    assert gbn(fill.hash_tensor((257, 3), 83).to(DEV)).shape == (257, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the encoder, stage by stage, from its stored tensors
# ---------------------------------------------------------------------------------------------------------------------
FN_INPUTS = {"_Mul": (0, 1), "_AddScale": (0, 1), "_Scale": (0,), "_PriorUpdate": (0, 1), "_GLU": (0,), "_Sparsemax": (0,),
             "_Split": (0,), "_Entropy": (0,), "_GhostBN": (0,)}


class Recorder:
    """Records every stage of a forward (each autograd function of ecgmm/tabnet.py and every Linear module): the input it
    read, the output it stored and, through Tensor.register_hook, the gradient arriving at the output and the stage's OWN
    input gradient (each input goes in as a fresh view, so its hook sees this stage's gradient and not the sum over every
    reader of the tensor)."""

    def __init__(self, model, monkeypatch):
        self.calls = []
        for name, idx in FN_INPUTS.items():
            monkeypatch.setattr(G, name, self._proxy(name, getattr(G, name), idx))
        self.handles = []
        for m in set(model.modules()):
            if isinstance(m, hnn.Linear):
                self.handles.append(m.register_forward_pre_hook(lambda mod, args: (self._fresh(args[0]),)))
                self.handles.append(m.register_forward_hook(self._linear))

    @staticmethod
    def _fresh(t):
        return t.view_as(t) if torch.is_tensor(t) and t.requires_grad else t

    def _entry(self, kind, args, ins, outs, **more):
        e = dict(kind=kind, args=args, ins=ins, outs=outs, gin={}, gout={}, **more)

        def keep(where, i):
            def hook(g):
                if g is not None:      # (an output nobody reads gets an undefined gradient)
                    where[i] = g.detach().clone()
            return hook
        for i, t in ins.items():
            if torch.is_tensor(t) and t.requires_grad:
                t.register_hook(keep(e["gin"], i))
        for i, t in enumerate(outs):
            if t.requires_grad:
                t.register_hook(keep(e["gout"], i))
        self.calls.append(e)
        return e

    def _proxy(self, name, fn, idx):
        rec = self

        class Proxy:
            @staticmethod
            def apply(*args):
                args = list(args)
                for i in idx:
                    args[i] = rec._fresh(args[i])
                more = {}
                if name == "_GhostBN":
                    more["before"] = [t.detach().clone() for t in args[3:6]]
                out = fn.apply(*args)
                outs = out if isinstance(out, tuple) else (out,)
                if name == "_GhostBN":
                    more["after"] = [t.detach().clone() for t in args[3:6]]
                    more["save"] = out.grad_fn.saved_tensors[1].detach().clone()
                rec._entry(name, args, {i: args[i] for i in idx}, outs, **more)
                return out
        return Proxy

    def _linear(self, mod, args, out):
        self._entry("linear", args, {0: args[0]}, (out,), module=mod)

    def close(self):
        for h in self.handles:
            h.remove()


def c64(t):
    return None if t is None else t.detach().cpu()


def check_stage(e, worst):
    """one recorded stage against float64 of that stage on its own stored input; worst {checker: ratio} is updated"""
    k = e["kind"]
    ins = {i: c64(t) if torch.is_tensor(t) else t for i, t in e["ins"].items()}
    outs = [c64(t) for t in e["outs"]]
    gin, gout = {i: c64(t) for i, t in e["gin"].items()}, {i: c64(t) for i, t in e["gout"].items()}
    g = gout.get(0)

    def up(key, r):
        worst[key] = max(worst.get(key, 0.0), r if isinstance(r, float) else r.ratio)

    def ew(tag, op, a, b, s, got):
        up(tag, F64.check_ew(op, a, b, s, got, "%s %s" % (k, tag)))

    if k == "linear":
        w = c64(e["module"].weight)
        ref = F64.linear_ref(ins[0], w, None, g)
        up("linear y", F64.check_dot(outs[0], *ref["y"][:3], name="linear y"))
        if g is not None and 0 in gin:
            up("linear dx", F64.check_dot(gin[0], *ref["dx"][:3], name="linear dx"))
    elif k == "_Mul":
        ew("mul", "MUL", ins[0], ins[1], 0.0, outs[0])
        if g is not None:
            if 0 in gin:
                ew("mul bwd", "MUL", g, ins[1], 0.0, gin[0])
            if 1 in gin:
                ew("mul bwd", "MUL", g, ins[0], 0.0, gin[1])
    elif k == "_AddScale":
        s = e["args"][2]
        ew("add_scale", "ADD_SCALE", ins[0], ins[1], s, outs[0])
        for i in gin:
            if s == 1.0:
                assert torch.equal(gin[i], g)
            else:
                ew("add_scale bwd", "SCALE", g, None, s, gin[i])
    elif k == "_Scale":
        s = e["args"][1]
        ew("scale", "SCALE", ins[0], None, s, outs[0])
        if 0 in gin:
            ew("scale bwd", "SCALE", g, None, s, gin[0])
    elif k == "_PriorUpdate":
        gamma = e["args"][2]
        if ins[1] is None:
            ew("prior", "RSUB", ins[0], None, gamma, outs[0])
            if 0 in gin:
                ew("prior bwd", "SCALE", g, None, -1.0, gin[0])
        else:
            ew("prior", "PRIOR", ins[0], ins[1], gamma, outs[0])
            if 0 in gin:
                ew("prior bwd", "NEG_MUL", g, ins[1], 0.0, gin[0])
            if 1 in gin:
                ew("prior bwd", "PRIOR", ins[0], g, gamma, gin[1])
    elif k == "_Split":
        nd, relu = e["args"][1], e["args"][2]
        d_ref, a_ref = F64.split_ref(ins[0], nd, relu)
        assert torch.equal(outs[0], d_ref) and torch.equal(outs[1], a_ref), "split"
        if 0 in gin:
            assert torch.equal(gin[0], F64.split_bwd_ref(outs[0], gout.get(0), gout.get(1), ins[0].shape[1], nd, relu)), "split bwd"
        up("split", 0.0)
    elif k == "_GLU":
        dz = gin.get(0) if g is not None else None
        for key, r in F64.check_glu(ins[0], outs[0], g if dz is not None else None, dz, "glu").items():
            up("glu " + key, r)
    elif k == "_Sparsemax":
        r = F64.check_sparsemax(ins[0], outs[0])
        up("sparsemax", r)
        up("sparsemax row sum", r.row_sum)
        if g is not None and 0 in gin:
            up("sparsemax bwd", F64.check_sparsemax_bwd(outs[0], g, gin[0]))
    elif k == "_Entropy":
        dM = gin.get(0) if g is not None else None
        for key, r in F64.check_entropy(ins[0], outs[0], e["args"][1], g if dM is not None else None, dM).items():
            up("entropy " + key, r)
    elif k == "_GhostBN":
        gamma, beta = e["args"][1], e["args"][2]
        training, mom, eps, vbs = e["args"][6:10]
        b4, af = [c64(t) for t in e["before"]], [c64(t) for t in e["after"]]
        have = g is not None        # (the raw input of initial_bn needs no gradient in training: dgamma / dbeta alone)
        res = F64.check_ghost_bn(ins[0], c64(gamma), c64(beta), b4[0], b4[1], int(b4[2]), mom, eps, vbs, int(training), outs[0],
                                 c64(e["save"]), af[0], af[1], int(af[2]), g, gin.get(0) if have else None,
                                 c64(gamma.grad) if have else None, c64(beta.grad) if have else None, "gbn")
        for key, r in res.items():
            up("gbn " + key, r)
    else:
        raise AssertionError(k)


def check_weights(rec, worst, expect_missing_uses=0):
    """every Linear's weight gradient = the float64 sum over the uses the backward reached of dy_i^T x_i (K = uses * B)"""
    by_mod = {}
    for e in rec.calls:
        if e["kind"] == "linear":
            by_mod.setdefault(e["module"], []).append(e)
    for mod, uses in by_mod.items():
        pairs = [(c64(e["ins"][0]), c64(e["gout"][0])) for e in uses if 0 in e["gout"]]
        if isinstance(mod, G.SharedLinear):
            assert len(uses) - len(pairs) == expect_missing_uses, (len(uses), len(pairs))
            assert mod._pending == mod._seen == 0 or expect_missing_uses, "use counts left behind"
        if not pairs:
            continue
        ref, Aabs, K = F64.shared_dw_ref(pairs)
        key = "shared dw" if isinstance(mod, G.SharedLinear) else "linear dw"
        r = F64.check_dot(c64(mod.weight.grad), ref, Aabs, K, name="%s (%d uses)" % (key, len(pairs)))
        worst[key] = max(worst.get(key, 0.0), r.ratio)


def run_sequences(model, B, monkeypatch, out_dim):
    model = model.to(DEV).train()
    with torch.no_grad():
        for n_, b in model.named_buffers():
            if n_.endswith("running_mean"):
                b.copy_(0.1 * fill.hash_tensor(tuple(b.shape), 3).to(DEV))
    rec = Recorder(model, monkeypatch)
    x = fill.hash_tensor((B, model.tabnet.encoder.input_dim), 17, 1.5).to(DEV)
    w = fill.hash_tensor((B, out_dim), 18).to(DEV)
    results = {}

    def forward(xin):
        rec.calls.clear()
        out, ml = model(xin)
        return out, ml, (G._Mul.apply(out, w)).sum() + 0.3 * ml

    def check(tag, missing=0):
        torch.cuda.synchronize()
        worst = {}
        for e in rec.calls:
            check_stage(e, worst)
        check_weights(rec, worst, missing)
        results[tag] = worst
        say(tag + " B=%d" % B, **worst)
        assert all(v <= 1.0 for v in worst.values()), worst

    shared = any(isinstance(m, G.SharedLinear) for m in model.modules())
    # 1. a forward that is never back-propagated, then a full step
    forward(x)
    _, _, loss = forward(x)
    loss.backward()
    check("after an unused forward")
    # 2. M_loss alone: the last step's feature transformer gets no gradient, so one use of each shared weight is missing
    HF.release_grads(model)
    _, ml, _ = forward(x)
    ml.backward()
    check("M_loss alone", missing=1 if shared else 0)
    # ... and the full step after it starts its sums afresh
    HF.release_grads(model)
    _, _, loss = forward(x)
    loss.backward()
    check("full step after M_loss alone")
    # 3. eval mode, the input requires a gradient: BatchNorm is differentiated through its running statistics
    HF.release_grads(model)
    model.eval()
    xg = x.clone().requires_grad_(True)
    _, _, loss = forward(xg)
    loss.backward()
    check("eval, input gradient")
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    rec.close()
    return results


@pytest.mark.parametrize("B", [40, 130, 257, 300])
def test_clinical_encoder_stage_by_stage(B, monkeypatch):
    torch.manual_seed(1)
    run_sequences(G.ClinicalTabNetEncoder(2), B, monkeypatch, 32)


class _Wrap(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.tabnet = net

    def forward(self, x):
        return self.tabnet(x)


@pytest.mark.parametrize("name,kw,B", [
    ("in5_d8_a8_steps4", dict(input_dim=5, output_dim=6, n_d=8, n_a=8, n_steps=4), 130),
    ("no_shared", dict(input_dim=5, output_dim=6, n_d=8, n_a=8, n_steps=3, n_shared=0), 130),
    ("no_independent", dict(input_dim=5, output_dim=6, n_d=8, n_a=8, n_steps=3, n_independent=0), 130),
    ("vbs16_b50", dict(input_dim=5, output_dim=6, n_d=8, n_a=8, n_steps=3, virtual_batch_size=16), 50),
], ids=lambda v: v if isinstance(v, str) else "")
def test_tabnet_variants_stage_by_stage(name, kw, B, monkeypatch):
    torch.manual_seed(2)
    run_sequences(_Wrap(G.TabNetNoEmbeddings(**kw)), B, monkeypatch, kw["output_dim"])
