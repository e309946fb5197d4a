"""Either encoder's inference forward as a chain of the per-op C entry points, and its check against float64.

The inference plans (csrc/plan_infer.hip) run every op through the same internal call as a public per-op entry point:
ecgmm_fold_conv_bn (the fold of a BatchNorm into the convolution in front of it), ecgmm_stem_fwd_wgrows (bf16) / ecgmm_stem_fwd
(fp32) with no statistics rows, ecgmm_relu_maxpool, ecgmm_conv_fwd_fused, ecgmm_avgpool, ecgmm_se_mlp_fwd (or the two
ecgmm_linear_fwd of se_mlp_forward, csrc/plan_common.h, where ECGMM_SE_MLP_FUSED is off), ecgmm_gate_res_relu and
ecgmm_linear_fwd.  `Chain` builds the network from those calls alone.  What it does NOT share with the plan is everything
the plan adds: the prepared blob and its layout, the rotating block buffers that alias the dead stem output, which tensor is
handed on as addend or next input, the in-place gate pass and the side stream.  Here every tensor, folded weights included,
lives in its own NaN-prefilled allocation with NaN guard elements behind it, nothing is written in place and everything is kept.

`check_chain` then holds every tensor of the chain to the float64 evaluation of the ONE op that wrote it on that op's STORED
inputs (bounds of tests/f64check.py and tests/infer_ref.py), so a plan whose features equal the chain's bit for bit
(tests/test_infer_chain_gpu.py) is checked op by op as well.

The parameters and BatchNorm buffers are hash-filled (oracle/fill.py); the BatchNorms of BN_EXTREME get the fills of
tests/test_infer_gpu.py::_bn_case: negative, zero and tiny gammas, a running variance of 3e4 and one far below eps."""
import ctypes as C

import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from oracle import fill, ref_models as O

from . import f64check as F
from . import plan_replay as PR
from .lstm_abi import Arena, table
from .test_conv_edges_f64_gpu import _chk
from .test_conv_layers_f64_gpu import Geo, poisoned
from .test_infer_gpu import _bn_case
from .util import DEV, TDT, switch_get

OUT_DIM = {"r18": 16, "r1d": 5}
PREFIX = {"r18": "ecgmm_resnet18_infer", "r1d": "ecgmm_resnet1d_infer"}
BN_EXTREME = {"r18": ("bn1", "layer2.0.bn2", "layer3.0.downsample.1"), "r1d": ("initial.1", "layer2.bn1", "layer3.downsample.1")}
EPS = 1e-5


def ff(t):
    """0xFF bytes: NaN in fp32 and in bf16"""
    t.view(torch.int32).fill_(-1)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def build_model(kind, cin):
    if kind == "r18":
        model = fill.hash_fill_module(O.ResNet18(num_classes=OUT_DIM[kind]), "chain18.")
    else:
        model = fill.hash_fill_module(O.ResNet1D_SE(cin, OUT_DIM[kind]), "chain1d.")
    sd = model.state_dict()
    with torch.no_grad():
        for j, bn in enumerate(BN_EXTREME[kind]):
            gamma, beta, rm, rv, _ = _bn_case(sd[bn + ".weight"].numel(), 7 + j, False)
            for key, v in ((".weight", gamma), (".bias", beta), (".running_mean", rm), (".running_var", rv)):
                sd[bn + key].copy_(v)
    return model.eval()


class Chain:
    """kind "r18": ResNet18 on shape (N, 3, H, W);  kind "r1d": ResNet1D_SE on shape (N, cin, L).
    .W: the folded weights (compute dtype, packed) and biases (fp32) by name / (name, block), as ecgmm_fold_conv_bn wrote them;
    .T: every activation of the last run() by name / (name, block), flat, as stored;  .feat: the features [N][out_dim]."""

    def __init__(self, kind, shape, dt):
        self.kind, self.shape, self.dt, self.bf16, self.lib = kind, tuple(shape), dt, dt == L.BF16, L.lib()
        if kind == "r18":
            N, cin, H, W = shape
            self.x = fill.hash_tensor(shape, 821).to(DEV)
        else:
            (N, cin, W), H = shape, 1
            self.x = fill.hash_tensor(shape, 823, 1.7).to(DEV)
        self.N, self.cin = N, cin
        self.net = PR.Net(kind, N, cin, H, W, self.bf16, training=False, eps=EPS)
        model = build_model(kind, cin)
        self.names = [n for n, _ in model.named_parameters()]
        self.P = {n: p.detach().to(DEV).contiguous() for n, p in model.named_parameters()}
        self.bnames = [n for n, _ in model.named_buffers()]
        self.B = {n: b.detach().clone().to(DEV) for n, b in model.named_buffers()}
        assert len(self.names) == (L.RESNET18_NPARAMS if kind == "r18" else L.RESNET1D_NPARAMS)
        assert len(self.bnames) == (L.RESNET18_NBUFFERS if kind == "r18" else L.RESNET1D_NBUFFERS)
        self.se_fused = bool(switch_get(self.lib, "ECGMM_SE_MLP_FUSED"))
        self._guarded = []
        self.W = {}
        self.fold()
        self.T, self.feat = self.run()

    def desc(self, N=None):
        net = self.net
        if self.kind == "r18":
            return L.ResNet18Desc(N or self.N, net.H, net.W, OUT_DIM[self.kind], self.dt, 0, 0.1, EPS)
        return L.ResNet1DDesc(N or self.N, self.cin, net.W, OUT_DIM[self.kind], self.dt, 0, 0.1, EPS, 0.0, 0, 0)

    # ---- buffers
    def new(self, store, key, n, dtype):
        """n NaN elements for one kernel to fill, with NaN guard elements behind them (checked by guards())"""
        buf = poisoned(n, dtype)
        self._guarded.append((key, buf, n))
        store[key] = buf[:n]
        return buf

    def guards(self):
        torch.cuda.synchronize()
        for key, buf, n in self._guarded:
            assert torch.isnan(buf[n:].float()).all(), "%s: written past its last element" % (key,)

    # ---- the fold: one ecgmm_fold_conv_bn per convolution
    def _fold(self, key, layout, wname, bname, bn):
        w = PR.w4(self.P[wname])
        cout, cin = w.shape[0], w.shape[1]
        if layout == 1:
            rs, n = w.shape[2], self.lib.ecgmm_stem_packed_elems(cin, w.shape[2])
        else:
            rs, n = w.shape[2] * w.shape[3], w.numel()
        wkey, bkey = (("w" + key[0], key[1]), ("b" + key[0], key[1])) if isinstance(key, tuple) else ("w" + key, "b" + key)
        wout, bout = self.new(self.W, wkey, n, TDT[self.dt]), self.new(self.W, bkey, cout, torch.float32)
        cb = None if bname is None else self.P[bname]
        L.check(self.lib.ecgmm_fold_conv_bn(self.dt, layout, ptr(self.P[wname]), ptr(cb), ptr(self.P[bn + ".weight"]),
                                            ptr(self.P[bn + ".bias"]), ptr(self.B[bn + ".running_mean"]),
                                            ptr(self.B[bn + ".running_var"]), EPS, ptr(wout), ptr(bout), None, cout, cin, rs,
                                            stream()), "fold %s" % (key,))

    def fold(self):
        net = self.net
        self._fold("stem", 1, net.stem_w, net.stem_b, net.stem_bn)
        for k in net.blocks:
            nm = net.names(k)
            self._fold(("1", k.i), 0, nm["c1"], nm["b1"], nm["bn1"])
            self._fold(("2", k.i), 0, nm["c2"], nm["b2"], nm["bn2"])
            if k.down:
                self._fold(("d", k.i), 0, nm["cd"], nm["bd"], nm["bnd"])
        self.guards()

    # ---- per-op calls
    def _conv(self, T, key, g, x, w, b, addend, act):
        y = self.new(T, key, g.M * g.Cout, TDT[self.dt])
        L.check(self.lib.ecgmm_conv_fwd_fused(self.dt, C.byref(g.d), ptr(x), ptr(w), ptr(b), ptr(addend), ptr(y), act, stream()),
                "conv_fwd_fused %s" % (key,))
        return y

    def _avgpool(self, T, key, x, R, Cn):
        out = self.new(T, key, self.N * Cn, torch.float32)
        L.check(self.lib.ecgmm_avgpool(self.dt, ptr(x), ptr(out), self.N, R, Cn, None, stream()), "avgpool %s" % (key,))
        return out

    def _linear(self, T, key, x, w, b, In, Out, act):
        y = self.new(T, key, self.N * Out, torch.float32)
        L.check(self.lib.ecgmm_linear_fwd(ptr(x), ptr(w), ptr(b), ptr(y), self.N, In, Out, act, stream()), "linear_fwd %s" % (key,))
        return y

    def geoms(self, k):
        N, kh, ph = self.N, self.net.kh, self.net.pad[0]
        return (Geo(N, k.hin, k.win, k.cin, k.cout, kh, 3, k.stride, ph, 1), Geo(N, k.hout, k.wout, k.cout, k.cout, kh, 3, 1, ph, 1),
                Geo(N, k.hin, k.win, k.cin, k.cout, 1, 1, k.stride, 0, 0))

    def run(self):
        """the whole forward into fresh tensors -> (T, feat)"""
        net, lib, dt, N, W, P = self.net, self.lib, self.dt, self.N, self.W, self.P
        T = {}
        y0 = self.new(T, "y0", N * net.H1 * net.W1 * 64, TDT[dt])
        stem = lib.ecgmm_stem_fwd_wgrows if self.bf16 else lib.ecgmm_stem_fwd
        L.check(stem(dt, ptr(self.x), ptr(W["wstem"]), ptr(W["bstem"]), ptr(y0), None, N, self.cin, net.H, net.W, net.stem_r, stream()),
                "stem")
        cur = self.new(T, "p0", N * net.H2 * net.W2 * 64, TDT[dt])
        L.check(lib.ecgmm_relu_maxpool(dt, ptr(y0), ptr(cur), N, net.H1, net.W1, 64, stream()), "relu_maxpool")
        for k in net.blocks:
            i, nm = k.i, net.names(k)
            g1, g2, gd = self.geoms(k)
            a1 = self._conv(T, ("a1", i), g1, cur, W[("w1", i)], W[("b1", i)], None, L.ACT_RELU)
            if not net.se:
                res = self._conv(T, ("yd", i), gd, cur, W[("wd", i)], W[("bd", i)], None, L.ACT_NONE) if k.down else cur
                cur = self._conv(T, ("out", i), g2, a1, W[("w2", i)], W[("b2", i)], res, L.ACT_RELU)
                continue
            y2 = self._conv(T, ("y2", i), g2, a1, W[("w2", i)], W[("b2", i)], None, L.ACT_NONE)
            R = k.hout * k.wout
            m = self._avgpool(T, ("m", i), y2, R, k.cout)
            sw = [P[n] for n in nm["se"]]
            if self.se_fused:
                h, g = self.new(T, ("h", i), N * k.cr, torch.float32), self.new(T, ("g", i), N * k.cout, torch.float32)
                L.check(lib.ecgmm_se_mlp_fwd(ptr(m), ptr(sw[0]), ptr(sw[1]), ptr(sw[2]), ptr(sw[3]), ptr(h), ptr(g), N, k.cout, k.cr,
                                             stream()), "se_mlp_fwd %d" % i)
            else:
                h = self._linear(T, ("h", i), m, sw[0], sw[1], k.cout, k.cr, L.ACT_RELU)
                g = self._linear(T, ("g", i), h, sw[2], sw[3], k.cr, k.cout, L.ACT_SIGMOID)
            res = self._conv(T, ("yd", i), gd, cur, W[("wd", i)], W[("bd", i)], None, L.ACT_NONE) if k.down else cur
            out = self.new(T, ("out", i), N * R * k.cout, TDT[dt])
            L.check(lib.ecgmm_gate_res_relu(dt, ptr(y2), ptr(g), ptr(res), ptr(out), N * R, k.cout, R, stream()), "gate_res_relu %d" % i)
            cur = out
        last = net.blocks[-1]
        pooled = self._avgpool(T, "pooled", cur, last.hout * last.wout, last.cout)
        if net.kind == "r18":
            feat = self._linear(T, "feat", pooled, P["fc.weight"], P["fc.bias"], 512, OUT_DIM["r18"], L.ACT_NONE)
        else:
            h1 = self._linear(T, "h1", pooled, P["classifier.1.weight"], P["classifier.1.bias"], 256, 64, L.ACT_RELU)
            feat = self._linear(T, "feat", h1, P["classifier.4.weight"], P["classifier.4.bias"], 64, OUT_DIM["r1d"], L.ACT_NONE)
        self.guards()
        return T, T["feat"].view(N, -1).clone()

    # ---- the plan
    def plan(self, N=None, blob=None):
        """ecgmm_*_infer_prepare + ecgmm_*_infer on the first N samples: blob, workspace and features are views of one Arena,
        each exactly the size the library reports, between sentinel zones, all 0xFF bytes before the calls -> features.
        blob: a blob an earlier call prepared (left in .blob), used as it is instead of preparing one"""
        N = N or self.N
        lib, d, pre = self.lib, self.desc(N), PREFIX[self.kind]
        nblob = getattr(lib, pre + "_prepared_bytes")(C.byref(d))
        nws = getattr(lib, pre + "_workspace")(C.byref(d))
        assert nblob > 0 and nws > 0 and nblob % 4 == 0 and nws % 4 == 0, lib.ecgmm_last_error()
        shapes = {"ws": (nws // 4,), "feat": (N, OUT_DIM[self.kind])}
        if blob is None:
            shapes["blob"] = (nblob // 4,)
        ar = Arena(shapes)
        for v in ar.views.values():
            ff(v)
        x = self.x[:N].contiguous()
        if blob is None:
            blob = ar.views["blob"]
            params, buffers = table([self.P[n] for n in self.names]), table([self.B[n] for n in self.bnames])
            L.check(getattr(lib, pre + "_prepare")(C.byref(d), params, buffers, ptr(blob), nblob, stream()), "prepare")
        assert blob.numel() * 4 == nblob
        before = blob.clone()
        L.check(getattr(lib, pre)(C.byref(d), ptr(x), ptr(blob), nblob, ptr(ar.views["feat"]), ptr(ar.views["ws"]), nws, stream()),
                "infer")
        torch.cuda.synchronize()
        assert not ar.touched(), "the plan wrote outside blob / workspace / features, next to: %s" % ar.touched()
        assert same_bits(before, blob), "the forward wrote into its blob"
        self.blob = blob
        return ar.views["feat"].clone()


# ======================================================================================================================
# every chain tensor against float64 of the one op that wrote it
# ======================================================================================================================
def _unpack(w, cout, cin, kh, kw):
    """forward pack [Cout][taps][Cin] -> OIHW float64"""
    return w.view(cout, kh, kw, cin).permute(0, 3, 1, 2).double()


def check_chain(ch, T=None, rep=None):
    T = ch.T if T is None else T
    rep = rep or PR.Rep()
    net, dt, bf, N, W, P = ch.net, ch.dt, ch.bf16, ch.N, ch.W, ch.P
    act = lambda t, Cn, H, Wd: t.view(N, H, Wd, Cn).permute(0, 3, 1, 2).double()
    ng = ch.cin * net.stem_r
    full = W["wstem"].view(64, -1, 8).double()
    assert bool((full[:, ng:] == 0).all()) and bool((full[:, :, 7] == 0).all()), "stem pack padding not zero"
    w0 = full[:, :ng, :7].reshape(64, ch.cin, net.stem_r, 7)
    x4 = PR.rnd(ch.x.view(N, ch.cin, net.H, net.W), bf)
    ref = F.conv_ref64(x4, w0, None, stride=2, padding=net.stem_pad, bias=W["bstem"])
    rep("stem", _chk(dt, act(T["y0"], 64, net.H1, net.W1), ref.y, ref.ay, ng * 7, "stem y0"))
    rep("relu_maxpool", F.check_relu_maxpool(T["p0"], T["y0"], N, net.H1, net.W1, 64, bf, "relu_maxpool p0"))
    cur = act(T["p0"], 64, net.H2, net.W2)
    cur_rows = T["p0"].view(-1, 64)
    for k in net.blocks:
        i, nm, tag = k.i, net.names(k), "blk%d " % k.i
        taps = net.kh * 3
        shp = (k.cout, k.hout, k.wout)
        M, R = N * k.hout * k.wout, k.hout * k.wout
        w1, w2 = _unpack(W[("w1", i)], k.cout, k.cin, net.kh, 3), _unpack(W[("w2", i)], k.cout, k.cout, net.kh, 3)
        r1 = F.conv_ref64(cur, w1, None, stride=k.stride, padding=net.pad, bias=W[("b1", i)])
        a1 = act(T[("a1", i)], *shp)
        rep("conv", _chk(dt, a1, r1.y, r1.ay, k.cin * taps, tag + "a1", relu=True))
        res, res_rows = cur, cur_rows
        if k.down:
            rd = F.conv_ref64(cur, _unpack(W[("wd", i)], k.cout, k.cin, 1, 1), None, stride=k.stride, padding=(0, 0), bias=W[("bd", i)])
            res, res_rows = act(T[("yd", i)], *shp), T[("yd", i)].view(M, k.cout)
            rep("conv", _chk(dt, res, rd.y, rd.ay, k.cin, tag + "yd"))
        r2 = F.conv_ref64(a1, w2, None, stride=1, padding=net.pad, bias=W[("b2", i)])
        out = act(T[("out", i)], *shp)
        if not net.se:
            rep("conv", _chk(dt, out, r2.y + res, r2.ay + res.abs(), k.cout * taps, tag + "out", relu=True))
        else:
            y2 = T[("y2", i)]
            rep("conv", _chk(dt, act(y2, *shp), r2.y, r2.ay, k.cout * taps, tag + "y2"))
            m, h, g = T[("m", i)].view(N, k.cout), T[("h", i)].view(N, k.cr), T[("g", i)].view(N, k.cout)
            rep("avgpool", F.check_avgpool(m, y2.view(N, R, k.cout), name=tag + "se avgpool m"))
            sw = [P[n] for n in nm["se"]]
            rep("se_mlp", F.check_se_mlp(F.se_mlp_stages(m, sw[0], sw[1], sw[2], sw[3], h, g), {"h": h, "g": g}, tag + "se"))
            rep("gate_res_relu", F.check_gate_res_relu(T[("out", i)].view(M, k.cout), y2.view(M, k.cout), g, res_rows, R, bf, tag + "out"))
        cur, cur_rows = out, T[("out", i)].view(M, k.cout)
    last = net.blocks[-1]
    pooled = T["pooled"].view(N, last.cout)
    rep("avgpool", F.check_avgpool(pooled, cur_rows.view(N, last.hout * last.wout, last.cout), name="avgpool pooled"))
    feat = T["feat"].view(N, -1)
    if net.kind == "r18":
        ref, A, K, _ = F.linear_ref(pooled, P["fc.weight"], P["fc.bias"])["y"]
        rep("linear", F.check_dot(feat, ref, A, K, "fc feat"))
        return rep
    h1 = T["h1"].view(N, 64)
    ref, A, K, _ = F.linear_ref(pooled, P["classifier.1.weight"], P["classifier.1.bias"], act="relu")["y"]
    rep("linear", F.check_dot(h1, ref, A, K, "classifier h1"))
    ref, A, K, _ = F.linear_ref(h1, P["classifier.4.weight"], P["classifier.4.bias"])["y"]
    rep("linear", F.check_dot(feat, ref, A, K, "classifier feat"))
    return rep
