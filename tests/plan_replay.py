"""Replay of the two encoder launch plans (csrc/plan_resnet18.hip, csrc/plan_resnet1d.hip) op by op against float64.

A plan run leaves every intermediate tensor in its workspaces.  Given those tensors by name (what ecgmm_resnet18_ws_view /
ecgmm_resnet1d_ws_view expose, converted by the caller to float64: activations NCHW -- [N, C, 1, L] for the signal encoder --,
coef* [4][C], packed weights OIHW, bits / dmask as bool, idx0 as int64), the parameters, the BatchNorm buffers before and after,
the input and dfeat, this module walks the network in the plan's order and checks every stored tensor against the float64
evaluation of THAT ONE OP on the STORED inputs, with the checkers and constants of tests/f64check.py.  Every comparison
therefore has a one-op error bound, and a failure names the op: "blk5 out", "blk3 bn2 bwd dy", "blk6 dw2", ...

What this module knows of a plan is only the network (torch's named_parameters() / state-dict names, conv arithmetic) and which
buffer a stage reads and writes (X[st & 1], dy[st & 1], ...): that is the thing under test.  Nothing here imports the HIP
library (like tests/f64check.py), so tests/test_plan_replay_cpu.py can prove the checker on dicts built with plain torch.

Bounds by dtype:
  bf16 plan: conv outputs / input gradients check_bf16 (KAPPA), weight gradients check_dw (EPS_DW, TAU_DW), statistics within
             KAPPA per element + SIGMA on the sums, carried through coef_ref.
  fp32 plan: the convolutions are fp32 dot products (f32 MFMA): check_dot with K = the reduction length (the any-order bound
             g_k(K + 2) * A); statistics within that per element + g_k(M) on the sums (M summands in any order).
  BatchNorm-backward sums: K_sum = M, the any-order worst case (no launch arithmetic is mirrored here); the merged SE form
             sums over the R rows of a sample first and then over the N samples: R + N + 8 <= M + 8 roundings, same bound.
"""
import torch

from . import f64check as F


def rnd(t, bf16):
    """the value a bf16 plan reads an fp32 operand as"""
    return t.float().to(torch.bfloat16).double() if bf16 else t.double()


def cl(t):
    """NCHW -> channels-last [N][H][W][C]"""
    return t.permute(0, 2, 3, 1)


def rows(t):
    """NCHW -> [M][C]"""
    return cl(t).reshape(-1, t.shape[1])


def act(flat, N, C, H, W):
    """the first N*H*W*C elements of a channels-last buffer as NCHW"""
    return flat.reshape(-1)[:N * H * W * C].view(N, H, W, C).permute(0, 3, 1, 2)


def w4(w):
    """conv weight as OIHW (Conv1d weights [O][I][K] -> [O][I][1][K])"""
    return w if w.dim() == 4 else w.unsqueeze(2)


class Blk:
    def __init__(self, i, pre, cin, cout, stride, hin, win, kh):
        self.i, self.pre, self.cin, self.cout, self.stride, self.hin, self.win = i, pre, cin, cout, stride, hin, win
        self.down = stride != 1 or cin != cout
        self.hout = (hin + 2 * (kh // 2) - kh) // stride + 1
        self.wout = (win + 2 - 3) // stride + 1
        self.cr = cout // 16


class Net:
    """kind "r18": ResNet18 on [N, 3, H, W];  kind "r1d": ResNet1D_SE on [N, cin, L] (H = 1, W = L).
    fused2: the blocks whose bn2 reduction was fused into the next block's conv1 input gradient (ResNet18 with
    ECGMM_BN_FUSE_MIN_M below their pixel count): their dcur arrives masked and dz is never written.
    What the plan was started with is the caller's to say (this module does not import the library):
    bits: the forward stored the ReLU mask of every `out` as bits (None: a ResNet18 bf16 training plan does, ECGMM_RELU_BITS
    on); stem_fused: the training stem backward ran as one pool + BatchNorm pass (ECGMM_STEM_FUSE on), else as max-pool
    backward into big0 and a BatchNorm backward from there, as the eval form always does."""

    def __init__(self, kind, N, cin, H, W, bf16, training=True, eps=1e-5, momentum=0.1, dropout_p=0.0, fused2=(), bits=None,
                 stem_fused=True):
        self.kind, self.N, self.cin, self.H, self.W, self.bf16, self.training = kind, N, cin, H, W, bf16, training
        self.eps, self.momentum, self.dropout_p, self.fused2 = eps, momentum, dropout_p, set(fused2)
        self.stem_fused = bool(stem_fused)
        self.se = kind == "r1d"
        self.kh = 3 if kind == "r18" else 1
        self.pad = (self.kh // 2, 1)
        self.stem_r = 7 if kind == "r18" else 1
        self.stem_pad = (self.stem_r // 2, 3)
        self.H1 = (H + 2 * self.stem_pad[0] - self.stem_r) // 2 + 1
        self.W1 = (W + 6 - 7) // 2 + 1
        self.H2, self.W2 = (self.H1 - 1) // 2 + 1, (self.W1 - 1) // 2 + 1
        if kind == "r18":
            self.stem_w, self.stem_b, self.stem_bn = "conv1.weight", None, "bn1"
            spec = [("layer%d.%d." % (l + 1, b), 64 << l, 2 if (b == 0 and l > 0) else 1) for l in range(4) for b in range(2)]
            self.bits = bool(bf16 and training) if bits is None else bool(bits)
            self.feat_c = 512
        else:
            self.stem_w, self.stem_b, self.stem_bn = "initial.0.weight", "initial.0.bias", "initial.1"
            spec = [("layer%d." % (i + 1), 64 << i, 1 if i == 0 else 2) for i in range(3)]
            self.bits = False
            self.feat_c = 256
        self.blocks, c, h, w = [], 64, self.H2, self.W2
        for i, (pre, cout, stride) in enumerate(spec):
            k = Blk(i, pre, c, cout, stride, h, w, self.kh)
            self.blocks.append(k)
            c, h, w = cout, k.hout, k.wout
        self.max_act = max([N * self.H2 * self.W2 * 64] + [N * k.hout * k.wout * k.cout for k in self.blocks])
        self.n_stages = len(self.blocks) + 2
        self.dual = kind == "r18"           # two dy / dy1 / dyd buffers, used alternately

    def names(self, k):
        """parameter / buffer names of block k: conv weights, conv biases (None for ResNet18), BatchNorm prefixes"""
        p = k.pre
        b = (lambda s: p + s) if self.se else (lambda s: None)
        return dict(c1=p + "conv1.weight", b1=b("conv1.bias"), bn1=p + "bn1", c2=p + "conv2.weight", b2=b("conv2.bias"),
                    bn2=p + "bn2", cd=p + "downsample.0.weight", bd=b("downsample.0.bias"), bnd=p + "downsample.1",
                    se=[p + "se.fc.%s" % s for s in ("0.weight", "0.bias", "2.weight", "2.bias")])


class Rep:
    """worst ratio per op class, for the docstring figures (print with show()), and which branch of the replay the stored
    data selected (paths: "blk3 din" -> "folded" / "dtmp", "stem bwd" -> "one pass" / "two passes")"""

    def __init__(self):
        self.worst = {}
        self.paths = {}

    def __call__(self, cls, r):
        for v in (r.values() if isinstance(r, dict) else [r]):
            ratio = v.ratio if hasattr(v, "ratio") else float(v)
            self.worst[cls] = max(self.worst.get(cls, 0.0), ratio)
        return r

    def show(self, what):
        print("REPLAY %s: " % what + ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items())))


def _chk_conv(net, got, ref, A, K, name):
    assert torch.isfinite(got).all(), name + ": non-finite values"
    if net.bf16:
        return F.check_bf16(got, ref, A, name=name)
    return F.check_dot(got, ref, A, K, name)


def _chk_dw(net, got, ref, A, K, name):
    got = w4(got.double())
    assert torch.isfinite(got).all(), name + ": non-finite weight gradient"
    if net.bf16:
        return F.check_dw(got, ref, A, name=name)
    return F.check_dot(got, ref, A, K, name)


def _chk_coef(net, ref, K, coef, bn, P, B0, B1, name):
    """coef [4][C] and the running statistics from the float64 statistics of the conv output `ref` (a ConvRef of the stored
    operands): the plan's rows are sums of the kernel's fp32 accumulators, so each summand may be off by the conv bound"""
    g, b = P[bn + ".weight"], P[bn + ".bias"]
    rm0, rv0 = B0[bn + ".running_mean"], B0[bn + ".running_var"]
    rm1, rv1 = B1[bn + ".running_mean"], B1[bn + ".running_var"]
    n0, n1 = int(B0[bn + ".num_batches_tracked"]), int(B1[bn + ".num_batches_tracked"])
    if not net.training:
        assert torch.equal(rm0, rm1) and torch.equal(rv0, rv1) and n0 == n1, name + ": eval mode changed the running statistics"
        return F.check_coef(coef, F.eval_coef_ref(g, b, rm0, rv0, net.eps), name=name)
    assert n1 == n0 + 1, "%s: num_batches_tracked %d -> %d" % (name, n0, n1)
    y = ref.y
    M = y.numel() // y.shape[1]
    a = (F.KAPPA if net.bf16 else F.g_k(K + 2)) * ref.ay
    s1g, s2g = (F.SIGMA, F.SIGMA) if net.bf16 else (F.g_k(M), F.g_k(M + 1))
    dims = (0, 2, 3)
    ds1 = a.sum(dims) + s1g * y.abs().sum(dims)
    ds2 = (2 * y.abs() * a + a * a).sum(dims) + s2g * (y * y).sum(dims)
    cref = F.coef_ref(y.sum(dims), (y * y).sum(dims), M, g, b, net.eps, rm0, rv0, net.momentum, ds1, ds2)
    return F.check_coef(coef, cref, rm1, rv1, name=name)


def _bn_bwd(net, dout, y, coef, gamma, dgamma, dbeta, dy, name, dz_out=None, dbias=None, maskref=None, gate=None, addc=None):
    M = y.shape[0]
    for t, what in ((dgamma, "dgamma"), (dbeta, "dbeta"), (dy, "dy")):
        assert torch.isfinite(t.double()).all(), "%s %s: non-finite values" % (name, what)
    if net.training:
        return F.check_bn_bwd(dout, y, coef, gamma, net.bf16, M, dgamma, dbeta, dy, dz_out, dbias, M, maskref, gate, addc, name)
    return F.check_bn_eval_bwd(dout, y, coef, net.bf16, M, dgamma, dbeta, dy, dz_out, dbias, M, maskref, gate, addc, name)


# ======================================================================================================================
# forward
# ======================================================================================================================
def replay_forward(net, T, P, B0, B1, x, feat, rep=None):
    """T: the forward workspace by name (global tensors by name, per-block ones by (name, block)); P: parameters by name;
    B0 / B1: the BatchNorm buffers before / after the call; x: the input [N, cin, H, W]; feat: the plan's output."""
    rep = rep or Rep()
    bf, N = net.bf16, net.N
    xr = rnd(x, bf)
    w0 = rnd(w4(P[net.stem_w]), bf)
    ref = F.conv_ref64(xr, w0, None, stride=2, padding=net.stem_pad, bias=None if net.stem_b is None else P[net.stem_b])
    rep("conv", _chk_conv(net, T["y0"], ref.y, ref.ay, net.cin * net.stem_r * 7, "stem conv y0"))
    rep("coef", _chk_coef(net, ref, net.cin * net.stem_r * 7, T["coef0"], net.stem_bn, P, B0, B1, "stem coef0"))
    c0 = T["coef0"]
    rep("maxpool", F.check_pool_fwd(cl(T["p0"]), cl(T["idx0"]), cl(T["y0"]), c0[0], c0[1], bf, name="stem maxpool p0"))
    cur = T["p0"]
    for k in net.blocks:
        i, nm = k.i, net.names(k)
        tag = "blk%d " % i
        taps = net.kh * 3
        wr = {"w1": rnd(w4(P[nm["c1"]]), bf), "w2": rnd(w4(P[nm["c2"]]), bf)}
        if k.down:
            wr["wd"] = rnd(w4(P[nm["cd"]]), bf)
        for key, want in wr.items():
            for pack in "fd":
                got = T[(key + pack, i)]
                assert got.shape == want.shape and torch.equal(got, want), \
                    "%spack %s: %d elements differ from the rounded parameter" % (tag, key + pack, int((got != want).sum()))
        rep("pack", 0.0)
        M = N * k.hout * k.wout
        r1 = F.conv_ref64(cur, wr["w1"], None, stride=k.stride, padding=net.pad, bias=None if nm["b1"] is None else P[nm["b1"]])
        rep("conv", _chk_conv(net, T[("y1", i)], r1.y, r1.ay, k.cin * taps, tag + "conv1 y1"))
        rep("coef", _chk_coef(net, r1, k.cin * taps, T[("coef1", i)], nm["bn1"], P, B0, B1, tag + "coef1"))
        c1, c2 = T[("coef1", i)], T[("coef2", i)]
        want, A = F.bn_act_ref(rows(T[("y1", i)]), c1[0], c1[1], relu=True)
        rep("bn_act", F.check_stored(rows(T[("a1", i)]), want, A, F.K_ACT, bf, tag + "a1"))
        r2 = F.conv_ref64(T[("a1", i)], wr["w2"], None, stride=1, padding=net.pad, bias=None if nm["b2"] is None else P[nm["b2"]])
        rep("conv", _chk_conv(net, T[("y2", i)], r2.y, r2.ay, k.cout * taps, tag + "conv2 y2"))
        rep("coef", _chk_coef(net, r2, k.cout * taps, c2, nm["bn2"], P, B0, B1, tag + "coef2"))
        gate = None
        if net.se:
            R = k.hout * k.wout
            y2r = cl(T[("y2", i)]).reshape(N, R, k.cout)
            rep("avgpool", F.check_avgpool(T[("m", i)], y2r, c2[0], c2[1], tag + "se avgpool m"))
            sw = [P[n] for n in nm["se"]]
            st = F.se_mlp_stages(T[("m", i)], sw[0], sw[1], sw[2], sw[3], T[("h", i)], T[("g", i)])
            rep("se_mlp", F.check_se_mlp(st, {"h": T[("h", i)], "g": T[("g", i)]}, tag + "se"))
            gate = F.per_row(T[("g", i)], R, M)
        if k.down:
            rd = F.conv_ref64(cur, wr["wd"], None, stride=k.stride, padding=(0, 0), bias=None if nm["bd"] is None else P[nm["bd"]])
            rep("conv", _chk_conv(net, T[("yd", i)], rd.y, rd.ay, k.cin, tag + "downsample yd"))
            rep("coef", _chk_coef(net, rd, k.cin, T[("coefd", i)], nm["bnd"], P, B0, B1, tag + "coefd"))
            cd = T[("coefd", i)]
            want, A = F.bn_act_ref(rows(T[("y2", i)]), c2[0], c2[1], rows(T[("yd", i)]), cd[0], cd[1], gate, relu=True)
        else:
            want, A = F.bn_act_ref(rows(T[("y2", i)]), c2[0], c2[1], rows(cur), None, None, gate, relu=True)
        rep("bn_act", F.check_stored(rows(T[("out", i)]), want, A, F.K_ACT, bf, tag + "out"))
        if net.bits:
            bad = T[("bits", i)] != (T[("out", i)] > 0)
            assert not bool(bad.any()), "%sbits: %d bits are not the sign of the stored out" % (tag, int(bad.sum()))
            rep("bits", 0.0)
        cur = T[("out", i)]
    last = net.blocks[-1]
    R = last.hout * last.wout
    rep("avgpool", F.check_avgpool(T["pooled"], cl(cur).reshape(N, R, last.cout), name="avgpool pooled"))
    if net.kind == "r18":
        ref, A, K, _ = F.linear_ref(T["pooled"], P["fc.weight"], P["fc.bias"])["y"]
        rep("linear", F.check_dot(feat, ref, A, K, "fc feat"))
        return rep
    ref, A, K, _ = F.linear_ref(T["pooled"], P["classifier.1.weight"], P["classifier.1.bias"], act="relu")["y"]
    rep("linear", F.check_dot(T["h1"], ref, A, K, "classifier h1"))
    hin = T["h1"]
    if net.training and net.dropout_p > 0:
        keep = T["dmask"]
        assert 0 < int(keep.sum()) < keep.numel(), "dropout dmask: keeps %d of %d" % (int(keep.sum()), keep.numel())
        rep("dropout", F.check_dropout(T["hd"], T["h1"], keep, net.dropout_p, "dropout hd"))
        hin = T["hd"]
    ref, A, K, _ = F.linear_ref(hin, P["classifier.4.weight"], P["classifier.4.bias"])["y"]
    rep("linear", F.check_dot(feat, ref, A, K, "classifier feat"))
    return rep


# ======================================================================================================================
# backward, one stage: 0 = head + broadcast, 1 .. nblocks = the blocks from the last to the first, nblocks + 1 = stem
# ======================================================================================================================
def _lin_bwd(rep, x, w, dz, G, wname, bname, dx_got, name, dx_post=None):
    r = F.linear_ref(x, w, None, dz=dz)
    for key, got in (("dw", G[wname]), ("db", G[bname])):
        ref, A, K, _ = r[key]
        assert torch.isfinite(got.double()).all(), "%s %s: non-finite values" % (name, key)
        rep("linear", F.check_dot(got, ref, A, K, "%s %s" % (name, key)))
    ref, A, K, _ = r["dx"]
    if dx_post is not None:
        return dx_post(ref, A, K)
    rep("linear", F.check_dot(dx_got, ref, A, K, name + " dx"))


def replay_backward_stage(net, T, S, G, P, x, dfeat, st, dx=None, rep=None):
    """S: the backward workspace after stage st (activation buffers flat, channels-last, NaN where never written; X / dy / dy1 /
    dyd as lists of buffers); G: the gradient buffers by parameter name after stage st; dx: the input gradient (last stage)."""
    rep = rep or Rep()
    bf, N = net.bf16, net.N
    nb = len(net.blocks)
    if st == 0:
        last = net.blocks[-1]
        R = last.hout * last.wout
        if net.kind == "r18":
            _lin_bwd(rep, T["pooled"], P["fc.weight"], dfeat, G, "fc.weight", "fc.bias", S["dpooled"], "fc bwd")
        else:
            drop = net.training and net.dropout_p > 0
            hin = T["hd"] if drop else T["h1"]

            def through_dropout(ref, A, K):
                if drop:
                    want, Ad = F.dropout_ref(ref, T["dmask"], net.dropout_p, A)
                    bound = F.dot_bound(Ad, K) + F.g_k(F.K_DROPOUT) * (want.abs() + F.dot_bound(Ad, K))
                    ratio = F._ratio((S["dfeat_h"].double() - want).abs(), bound)
                    rr = F.Report("classifier.4 bwd dx through dropout", float(ratio.max()), F._unravel(int(ratio.argmax()), want.shape))
                    print(rr)
                    assert rr.ok, str(rr)
                    rep("dropout", rr)
                else:
                    rep("linear", F.check_dot(S["dfeat_h"], ref, A, K, "classifier.4 bwd dx"))
            _lin_bwd(rep, hin, P["classifier.4.weight"], dfeat, G, "classifier.4.weight", "classifier.4.bias", None,
                     "classifier.4 bwd", through_dropout)
            want = S["dfeat_h"].double() * (T["h1"] > 0)
            assert torch.equal(S["dh1"].double(), want), "classifier relu bwd dh1: %d elements differ" % int((S["dh1"].double() != want).sum())
            _lin_bwd(rep, T["pooled"], P["classifier.1.weight"], S["dh1"], G, "classifier.1.weight", "classifier.1.bias",
                     S["dpooled"], "classifier.1 bwd")
        got = cl(act(S["X"][0], N, last.cout, last.hout, last.wout)).reshape(N, R, last.cout)
        rep("bcast", F.check_bcast(got, S["dpooled"], R, bf, "bcast X[0]"))
        return rep
    if st <= nb:
        i = nb - st
        k, nm = net.blocks[i], net.names(net.blocks[i])
        tag = "blk%d " % i
        taps = net.kh * 3
        pp = (st & 1) if net.dual else 0
        M, R = N * k.hout * k.wout, k.hout * k.wout
        shp = (N, k.cout, k.hout, k.wout)
        inp = T["p0"] if i == 0 else T[("out", i - 1)]
        dcur = act(S["X"][(st - 1) & 1], *shp)
        assert torch.isfinite(dcur).all(), tag + "dcur X[%d]: non-finite values" % ((st - 1) & 1)
        out_i, y2, y1 = T[("out", i)], T[("y2", i)], T[("y1", i)]
        fused2 = i in net.fused2
        gate = addc = None
        if net.se:
            c2 = T[("coef2", i)]
            mask3 = cl(out_i > 0).reshape(N, R, k.cout)
            dg = S["dg"].reshape(-1)[:N * k.cout].view(N, k.cout)
            rep("se_gate", F.check_se_gate_grad(dg, cl(dcur).reshape(N, R, k.cout), mask3, cl(y2).reshape(N, R, k.cout), c2[0], c2[1],
                                                tag + "se gate grad dg"))
            sw = [P[n] for n in nm["se"]]
            ds = S["ds"].reshape(-1)[:N * k.cout].view(N, k.cout)
            dh = S["dh"].reshape(-1)[:N * k.cr].view(N, k.cr)
            dm = S["dm"].reshape(-1)[:N * k.cout].view(N, k.cout)
            stg = F.se_mlp_stages(T[("m", i)], sw[0], sw[1], sw[2], sw[3], T[("h", i)], T[("g", i)], dg, ds, dh, 1.0 / R)
            got = {"ds": ds, "dh": dh, "dm": dm, "dw1": G[nm["se"][0]], "db1": G[nm["se"][1]], "dw2": G[nm["se"][2]], "db2": G[nm["se"][3]]}
            rep("se_mlp", F.check_se_mlp({s: v for s, v in stg.items() if s in got}, got, tag + "se bwd"))
            gate, addc = F.per_row(T[("g", i)], R, M), F.per_row(dm, R, M)
        # bn2: dy, dz, dgamma2, dbeta2
        dy = act(S["dy"][pp], *shp)
        dzb = act(S["dz"], *shp)
        if fused2:
            assert bool(torch.isnan(dzb).all()), tag + "dz: written although the masked gradient arrives in X (fused reduction)"
        G2 = (G[nm["bn2"] + ".weight"], G[nm["bn2"] + ".bias"])
        rep("bn_bwd", _bn_bwd(net, rows(dcur), rows(y2), T[("coef2", i)], P[nm["bn2"] + ".weight"], G2[0], G2[1], rows(dy),
                              tag + "bn2 bwd", dz_out=None if fused2 else rows(dzb), dbias=None if nm["b2"] is None else G[nm["b2"]],
                              maskref=None if fused2 else rows(out_i), gate=gate, addc=addc))
        dzp = dcur if fused2 else dzb
        # conv2: dw2 from the stored a1 and dy, da
        w2 = rnd(w4(P[nm["c2"]]), bf)
        r2 = F.conv_ref64(T[("a1", i)], w2, dy, stride=1, padding=net.pad)
        rep("dw", _chk_dw(net, G[nm["c2"]], r2.dw, r2.adw, M, tag + "dw2"))
        da = act(S["da"], *shp)
        rep("dgrad", _chk_conv(net, da, r2.dx, r2.adx, k.cout * taps, tag + "da"))
        # bn1: the mask is recomputed from y1
        dy1 = act(S["dy1"][pp], *shp)
        rep("bn_bwd", _bn_bwd(net, rows(da), rows(y1), T[("coef1", i)], P[nm["bn1"] + ".weight"], G[nm["bn1"] + ".weight"],
                              G[nm["bn1"] + ".bias"], rows(dy1), tag + "bn1 bwd", dbias=None if nm["b1"] is None else G[nm["b1"]],
                              maskref="y"))
        w1 = rnd(w4(P[nm["c1"]]), bf)
        din = act(S["X"][st & 1], N, k.cin, k.hin, k.win)
        Kx = k.cout * taps
        if k.down:
            dyd = act(S["dyd"][pp], *shp)
            rep("bn_bwd", _bn_bwd(net, rows(dzp), rows(T[("yd", i)]), T[("coefd", i)], P[nm["bnd"] + ".weight"],
                                  G[nm["bnd"] + ".weight"], G[nm["bnd"] + ".bias"], rows(dyd), tag + "bnd bwd",
                                  dbias=None if nm["bd"] is None else G[nm["bd"]]))
            wd = rnd(w4(P[nm["cd"]]), bf)
            rd = F.conv_ref64(inp, wd, dyd, stride=k.stride, padding=(0, 0))
            rep("dw", _chk_dw(net, G[nm["cd"]], rd.dw, rd.adw, M, tag + "dwd"))
            dtmp = act(S["dtmp"], N, k.cin, k.hin, k.win)
            if bool(torch.isnan(dtmp).all()):      # the fold ran: one rounding of the sum of both input gradients
                rep.paths[tag + "din"] = "folded"
                r1 = F.conv_ref64(inp, w1, dy1, stride=k.stride, padding=net.pad)
                want, A, Kx = r1.dx + rd.dx, r1.adx + rd.adx, Kx + k.cout + 1
            else:                                   # two roundings, through dtmp
                rep.paths[tag + "din"] = "dtmp"
                rep("dgrad", _chk_conv(net, dtmp, rd.dx, rd.adx, k.cout, tag + "dtmp"))
                r1 = F.conv_ref64(inp, w1, dy1, stride=k.stride, padding=net.pad, addend=dtmp)
                want, A = r1.dx, r1.adx
        else:
            r1 = F.conv_ref64(inp, w1, dy1, stride=k.stride, padding=net.pad, addend=dzp)
            want, A = r1.dx, r1.adx
            if (i - 1) in net.fused2:               # stored already masked by the previous block's ReLU
                keep = T[("out", i - 1)] > 0
                want, A = want * keep, A * keep
        rep("dw", _chk_dw(net, G[nm["c1"]], r1.dw, r1.adw, M, tag + "dw1"))
        rep("dgrad", _chk_conv(net, din, want, A, Kx, tag + "din X[%d]" % (st & 1)))
        return rep
    # ---- stem
    assert st == nb + 1, "stage %d out of range" % st
    H1, W1, H2, W2 = net.H1, net.W1, net.H2, net.W2
    M, MP = N * H1 * W1, N * H2 * W2
    dp0 = cl(act(S["X"][nb & 1], N, 64, H2, W2))
    assert torch.isfinite(dp0).all(), "stem dp0 X[%d]: non-finite values" % (nb & 1)
    p0, idx0, y0, c0 = cl(T["p0"]), cl(T["idx0"]), cl(T["y0"]), T["coef0"]
    gam = P[net.stem_bn + ".weight"]
    dgam, dbet = G[net.stem_bn + ".weight"], G[net.stem_bn + ".bias"]
    big1n = act(S["big1"], N, 64, H1, W1)
    big1 = cl(big1n)
    assert torch.isfinite(big1).all() and torch.isfinite(dgam).all() and torch.isfinite(dbet).all(), "stem bwd: non-finite values"
    dbias = None if net.stem_b is None else G[net.stem_b]
    big0 = cl(act(S["big0"], N, 64, H1, W1))
    if net.training and net.stem_fused:
        rep.paths["stem bwd"] = "one pass"
        assert bool(torch.isnan(big0).all()), "stem big0: written although the stem backward ran as one pass"
        (s1, s2), (m1, m2) = F.pool_red_ref(dp0, p0, c0)
        rep("stem_bwd", F.check_sum(dbet, s1, m1, MP + 1, "stem pool_bn_bwd dbeta"))
        rep("stem_bwd", F.check_sum(dgam, s2, m2, F.K_POOL_RED + MP + 1, "stem pool_bn_bwd dgamma"))
        dz64, mag = F.pool_bwd_ref(dp0, p0, idx0, H1, W1)
        k1 = gam.double() * c0[3].double()
        want, A = F.pool_dy_ref(dz64, mag, y0, c0, k1, dbet.double() / M, dgam.double() / M)
        rep("stem_bwd", F.check_stored(big1, want, A, F.K_POOL_DY, bf, "stem pool_bn_bwd big1"))
        if dbias is not None:
            s = big1.double().reshape(-1, 64)
            rep("stem_bwd", F.check_sum(dbias, s.sum(0), s.abs().sum(0), M + 1, "stem pool_bn_bwd dbias"))
    else:
        # two passes: the max-pool + ReLU backward into big0, then the BatchNorm backward of the plan's mode from the stored
        # big0 (training: the full form with its two sums; eval: the affine form), the 1-D stem conv's dbias from big1
        rep.paths["stem bwd"] = "two passes"
        assert torch.isfinite(big0).all(), "stem maxpool bwd big0: non-finite values"
        rep("stem_bwd", F.check_pool_bwd(big0, dp0, p0, idx0, bf, "stem maxpool bwd big0"))
        rep("bn_bwd", _bn_bwd(net, big0.reshape(-1, 64), y0.reshape(-1, 64), c0, gam, dgam, dbet, big1.reshape(-1, 64), "stem bn bwd",
                              dbias=dbias))
    xr = rnd(x, bf)
    w0 = rnd(w4(P[net.stem_w]), bf)
    r0 = F.conv_ref64(xr, w0, big1n, stride=2, padding=net.stem_pad)
    rep("dw", _chk_dw(net, G[net.stem_w], r0.dw, r0.adw, M, "stem dw0"))
    if dx is not None:
        # the bound tests/test_input_grad_gpu.py::test_stem_bwd_data_vs_float64 uses
        got = dx.double()
        assert torch.isfinite(got).all(), "stem input gradient: non-finite values"
        if bf:
            v = r0.dx.abs()
            e = torch.frexp(v).exponent
            half32 = torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 25), torch.zeros_like(v))
            ratio = F._ratio((got - r0.dx).abs(), F.KAPPA * r0.adx + half32)
            rr = F.Report("stem input gradient", float(ratio.max()), F._unravel(int(ratio.argmax()), got.shape))
        else:
            e = float((got - r0.dx).norm() / (r0.dx.norm() + 1e-30))
            rr = F.Report("stem input gradient", e / 2e-5, ())
        print(rr)
        assert rr.ok, str(rr)
        assert bool((got[r0.adx == 0] == 0).all()), "stem input gradient: a never-read input element has a gradient"
        rep("stem_dx", rr)
    return rep
