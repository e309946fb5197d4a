"""The two encoder launch plans (csrc/plan_resnet18.hip, csrc/plan_resnet1d.hip) run through the C ABI and replayed op by op
against float64 (tests/plan_replay.py, bounds of tests/f64check.py): every tensor a plan leaves in its workspaces -- found
through ecgmm_resnet18_ws_view / ecgmm_resnet1d_ws_view -- against the float64 evaluation of the one op that wrote it, on the
stored inputs of that op.  Forward, then the backward as one-stage calls with a replay after each stage.

Every output (feat, the input gradient, every parameter gradient) is a view of one tests/lstm_abi.py Arena between sentinel
zones; both workspaces are handed over with exactly the size the library reports and followed by sentinels.  Outputs and
workspaces are filled with 0xFF bytes (NaN in fp32 and in bf16) before the forward and before every backward call -- between
two backward stages every named tensor but the one X buffer that carries the gradient to the next stage -- so a stage that
reads anything else of an earlier stage fails.  The forward workspace must come out of the backward bit for bit as it went in.

Cases: the base shapes (ResNet18 (3, 3, 72, 104) with odd extents into the stride-2 blocks and (2, 3, 96, 160); ResNet1D_SE
(3, 1, 999) and (2, 12, 1000), dropout 0.3 with a fixed seed and offset).  At none of these is a pixel count N * H * W a
multiple of 256, which the halo convolution (and with it the fused BatchNorm-backward reduction) requires, so the switched run
adds one shape per plan where they do run: ResNet18 (2, 3, 128, 128) -- blocks 0 and 2 take the fused reduction (their
successor is a stride-1 block of 2048 / 512 pixels; asserted from the geometry rule and against the library's own answer) --
and ResNet1D_SE (2, 1, 1021) (256 / 128 pooled samples per signal).

Which path the library took is read from the stored data as well (staged() -> Plan.seen, one PATHS line per run): the fused
stem backward leaves big0 all 0xFF, the merged SE pass writes sa1 / sa2 / sa3 / se_rows, a folded downsample gradient leaves
dtmp unwritten, a plan that stores no ReLU bits leaves the bits views alone; each is held to the switches this process was
started with (Net.bits and Net.stem_fused come from ECGMM_RELU_BITS and ECGMM_STEM_FUSE).  The other value of every
start-up-only switch runs these same checks in a child process: tests/startup_legs.py, tests/test_startup_legs_gpu.py.

Measured on the MI355X, worst |err| / bound per op class over every case and run of this file (1 is a bf16 rounding tie: the
stored rounding term alone; 0 is an exact comparison; print them with -s, REPLAY lines):

  op class                         ResNet18 bf16   ResNet18 fp32   ResNet1D_SE bf16   ResNet1D_SE fp32
  conv (y0 y1 y2 yd)               1               0.056           1                  0.37
  coef + running stats (train)     0.25            0.0057          0.25               0.015
  coef (eval)                      0.47            0.47            0.42               0.42
  maxpool p0 / idx0                1               0.33            1                  0.33
  pack (both packs), bits          0               0               0                  0
  bn_act (a1, out)                 1               0.37            1                  0.45
  avgpool (pooled, m)              0.058           0.19            0.029              0.051
  se_mlp (h g ds dh dm dw db)      -               -               0.71               0.64
  linear (fc / classifier)         0.42            0.41            0.43               0.40
  dropout (hd, dfeat_h)            -               -               0.30               0.32
  bcast X[0]                       1               0.48            1                  0.48
  se gate grad dg                  -               -               0.039              0.035
  bn_bwd (dy dz dgamma dbeta db)   1               0.72            1                  0.70
  dw (dw1 dw2 dwd dw0)             0.078           0.13            0.060              0.017
  dgrad (da dtmp X)                1               0.011           1                  0.027
  stem_bwd (big1 dgamma0 dbeta0)   1               0.53            1                  0.33
  stem input gradient              0.38            0.014           0.24               0.0074

No new constant is calibrated: the bounds of the ops without a checker before this file (avgpool, bcast_rows, the SE gate
gradient and its merged form, the dropout scaling) are derived operation counts (tests/f64check.py, last section), and the one
bound that changed -- the tap a bf16 max-pool may name, now within one bf16 ulp of the maximum instead of half -- follows from
the kernel comparing the taps as stored (measured: 1.44 half ulps at the stem of the first case, where the old bound failed).

Run time on the MI355X: the 30 tests of this module take 5.3 s in all (the slowest 0.32 s), beside about 115 s for the
suite before it.
"""
import ctypes as C

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from oracle import fill, ref_models as O

from . import plan_replay as PR
from .lstm_abi import Arena, guarded_bytes, tail_touched, table
from .util import DEV, TDT, switch_get, switches

pytestmark = pytest.mark.gpu
DROP_P, SEED, OFFSET = 0.3, 20240607, 11
OUT_DIM = {"r18": 16, "r1d": 5}
PREFIX = {"r18": "ecgmm_resnet18", "r1d": "ecgmm_resnet1d"}
SHAPES = {"r18": [(3, 3, 72, 104), (2, 3, 96, 160)], "r1d": [(3, 1, 999), (2, 12, 1000)]}
HALO_SHAPES = {"r18": (2, 3, 128, 128), "r1d": (2, 1, 1021)}
SE_MERGED_ONLY = ("sa1", "sa2", "sa3", "se_rows")      # backward-workspace tensors only the merged SE / bn2 pass writes


def ff(t):
    """0xFF bytes: NaN in fp32 and in bf16"""
    t.view(torch.int32).fill_(-1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Plan:
    """one descriptor: model, parameter / buffer tables, arena of outputs, guarded workspaces"""

    def __init__(self, kind, shape, dt, training=True):
        self.kind, self.dt, self.lib = kind, dt, L.lib()
        bf16 = dt == L.BF16
        if kind == "r18":
            N, cin, H, W = shape
            model = fill.hash_fill_module(O.ResNet18(num_classes=OUT_DIM[kind]), "replay18.")
            self.x = fill.hash_tensor(shape, 811).to(DEV)
            self.desc = L.ResNet18Desc(N, H, W, OUT_DIM[kind], dt, int(training), 0.1, 1e-5)
        else:
            N, cin, W = shape
            H = 1
            model = fill.hash_fill_module(O.ResNet1D_SE(cin, OUT_DIM[kind]), "replay1d.")
            self.x = fill.hash_tensor(shape, 813, 1.7).to(DEV)
            self.desc = L.ResNet1DDesc(N, cin, W, OUT_DIM[kind], dt, int(training), 0.1, 1e-5, DROP_P, SEED, OFFSET)
        # what this process was started with (both are read once at start-up): whether the forward stores the ReLU bits and
        # whether the training stem backward is one pass; the replay holds the stored data to either
        on = lambda name: bool(switch_get(self.lib, name))
        self.net = PR.Net(kind, N, cin, H, W, bf16, training, dropout_p=DROP_P if kind == "r1d" else 0.0,
                          bits=bf16 and training and on("ECGMM_RELU_BITS"), stem_fused=on("ECGMM_STEM_FUSE"))
        self.seen = {}
        self.dfeat = fill.hash_tensor((N, OUT_DIM[kind]), 812).to(DEV)
        self.names = [n for n, _ in model.named_parameters()]
        self.P = {n: p.detach().to(DEV).contiguous() for n, p in model.named_parameters()}
        assert len(self.names) == (L.RESNET18_NPARAMS if kind == "r18" else L.RESNET1D_NPARAMS)
        self.bnames = [n for n, _ in model.named_buffers()]
        self.B0 = {n: b.detach().clone().to(DEV) for n, b in model.named_buffers()}
        self.B = {n: b.clone() for n, b in self.B0.items()}
        assert len(self.bnames) == (L.RESNET18_NBUFFERS if kind == "r18" else L.RESNET1D_NBUFFERS)
        pre = PREFIX[kind]
        self.fn = {k: getattr(self.lib, pre + "_" + k) for k in ("fwd_workspace", "bwd_workspace", "forward", "backward_dx", "ws_view")}
        self.nf, self.nb = self.fn["fwd_workspace"](C.byref(self.desc)), self.fn["bwd_workspace"](C.byref(self.desc))
        assert self.nf > 0 and self.nb > 0 and self.nf % 4 == 0 and self.nb % 4 == 0, self.lib.ecgmm_last_error()
        shapes = {"feat": (N, OUT_DIM[kind]), "dx": tuple(self.x.shape)}
        shapes.update({"g:" + n: tuple(self.P[n].shape) for n in self.names})
        self.arena = Arena(shapes)
        self.wf, self.wb = guarded_bytes(self.nf), guarded_bytes(self.nb)

    # ---- calls
    def guards(self, what):
        torch.cuda.synchronize()
        assert not self.arena.touched(), "%s wrote outside an output, next to: %s" % (what, self.arena.touched())
        assert not tail_touched(self.wf), what + " wrote past the end of the forward workspace"
        assert not tail_touched(self.wb), what + " wrote past the end of the backward workspace"

    def forward(self):
        for n in self.bnames:
            self.B[n].copy_(self.B0[n])
        ff(self.wf[:self.nf // 4])
        ff(self.arena.views["feat"])
        L.check(self.fn["forward"](C.byref(self.desc), ptr(self.x), table([self.P[n] for n in self.names]),
                                   table([self.B[n] for n in self.bnames]), ptr(self.arena.views["feat"]), ptr(self.wf), self.nf,
                                   stream()), "forward")
        self.guards("forward")
        return self.arena.views["feat"].clone()

    def fill_backward(self, keep=None):
        """0xFF over every gradient and over the backward workspace.  keep = an X index (between two stages): that buffer carries
        the gradient to the next stage and survives, as do the unnamed scratch rows (the partial rows of a fused
        BatchNorm-backward reduction are written one stage ahead of their reader); every other named tensor is filled"""
        if keep is None:
            ff(self.wb[:self.nb // 4])
        else:
            names = [("X", 1 - keep)] + [(n, 0) for n in ("dz", "da", "dtmp", "big0", "big1", "dpooled")]
            names += [(n, i) for n in ("dy", "dy1", "dyd") for i in ((0, 1) if self.net.dual else (0,))]
            if self.net.se:
                names += [(n, 0) for n in ("dh1", "dfeat_h", "dg", "ds", "dh", "dm") + SE_MERGED_ONLY]
            for n, i in names:
                ff(self.raw(1, n, i))
        for n, v in self.arena.views.items():
            if n != "feat":
                ff(v)

    def backward(self, b, e):
        L.check(self.fn["backward_dx"](C.byref(self.desc), ptr(self.x), ptr(self.dfeat), table([self.P[n] for n in self.names]),
                                       table([self.arena.views["g:" + n] for n in self.names]), ptr(self.wf), ptr(self.wb), self.nb,
                                       b, e, ptr(self.arena.views["dx"]), stream()), "backward [%d, %d)" % (b, e))
        self.guards("backward [%d, %d)" % (b, e))

    # ---- views
    def view(self, backward, name, index):
        off, nbytes = C.c_size_t(), C.c_size_t()
        rc = self.fn["ws_view"](C.byref(self.desc), backward, name.encode(), index, C.byref(off), C.byref(nbytes))
        return rc, off.value, nbytes.value

    def raw(self, backward, name, index=0):
        rc, off, nbytes = self.view(backward, name, index)
        L.check(rc, "ws_view %s[%d]" % (name, index))
        ws, total = (self.wb, self.nb) if backward else (self.wf, self.nf)
        assert off + nbytes <= total
        return ws.view(torch.uint8)[off:off + nbytes]

    def untouched(self, backward, name, index=0):
        """every byte of the view is still the 0xFF it was filled with"""
        return bool((self.raw(backward, name, index) == 0xFF).all())

    def act(self, backward, name, index, Cn, H, W):
        t = self.raw(backward, name, index).view(TDT[self.dt])
        return t.view(self.net.N, H, W, Cn).permute(0, 3, 1, 2).double()

    def f32(self, backward, name, index, *shape):
        return self.raw(backward, name, index).view(torch.float32).view(*shape).clone()

    def read_forward(self):
        net, N = self.net, self.net.N
        T = {"y0": self.act(0, "y0", 0, 64, net.H1, net.W1), "coef0": self.f32(0, "coef0", 0, 4, 64),
             "p0": self.act(0, "p0", 0, 64, net.H2, net.W2),
             "idx0": self.raw(0, "idx0").view(N, net.H2, net.W2, 64).permute(0, 3, 1, 2).long(),
             "pooled": self.f32(0, "pooled", 0, N, net.feat_c)}
        taps = (net.kh, 3)
        for k in net.blocks:
            i = k.i
            for n in ("y1", "a1", "y2", "out") + (("yd",) if k.down else ()):
                T[(n, i)] = self.act(0, n, i, k.cout, k.hout, k.wout)
            for n in ("coef1", "coef2") + (("coefd",) if k.down else ()):
                T[(n, i)] = self.f32(0, n, i, 4, k.cout)
            for key, ci, rs in (("w1", k.cin, taps), ("w2", k.cout, taps)) + ((("wd", k.cin, (1, 1)),) if k.down else ()):
                f = self.raw(0, key + "f", i).view(TDT[self.dt]).view(k.cout, rs[0], rs[1], ci).permute(0, 3, 1, 2).double()
                d = self.raw(0, key + "d", i).view(TDT[self.dt]).view(ci, rs[0], rs[1], k.cout).permute(3, 0, 1, 2).double()
                T[(key + "f", i)], T[(key + "d", i)] = f, d
            if net.bits:
                by = self.raw(0, "bits", i).view(-1, k.cout // 8, 1).to(torch.int32)
                bits = (by >> torch.arange(8, device=DEV, dtype=torch.int32).view(1, 1, 8)) & 1
                T[("bits", i)] = bits.view(N, k.hout, k.wout, k.cout).permute(0, 3, 1, 2).bool()
            if net.se:
                T[("m", i)], T[("h", i)], T[("g", i)] = (self.f32(0, "m", i, N, k.cout), self.f32(0, "h", i, N, k.cr),
                                                         self.f32(0, "g", i, N, k.cout))
        if net.se:
            T["h1"] = self.f32(0, "h1", 0, N, 64)
            if net.training:
                T["hd"], T["dmask"] = self.f32(0, "hd", 0, N, 64), self.raw(0, "dmask").view(N, 64).bool()
        return T

    def read_backward(self):
        net, N = self.net, self.net.N
        flat = lambda n, i=0: self.raw(1, n, i).view(TDT[self.dt]).double()
        two = (lambda n: [flat(n, 0), flat(n, 1)]) if net.dual else (lambda n: [flat(n)])
        S = dict(X=[flat("X", 0), flat("X", 1)], dz=flat("dz"), dy=two("dy"), dy1=two("dy1"), dyd=two("dyd"), da=flat("da"),
                 dtmp=flat("dtmp"), big0=flat("big0"), big1=flat("big1"), dpooled=self.f32(1, "dpooled", 0, N, net.feat_c))
        if net.se:
            S.update(dh1=self.f32(1, "dh1", 0, N, 64), dfeat_h=self.f32(1, "dfeat_h", 0, N, 64))
            S.update({n: self.f32(1, n, 0, -1) for n in ("dg", "ds", "dh", "dm")})
        return S

    def grads(self):
        return {n: self.arena.views["g:" + n].clone() for n in self.names}


def bits_untouched(plan, when):
    """a plan that promised no ReLU bits (eval, or started with ECGMM_RELU_BITS=0) has the views and must leave them alone"""
    net = plan.net
    if net.kind == "r18" and net.bf16 and not net.bits:
        for k in net.blocks:
            assert plan.untouched(0, "bits", k.i), "block %d: bits written %s although the plan stores none" % (k.i, when)
        return True
    return False


def staged(plan, rep):
    """forward + replay, then the backward one stage per call with a replay after each; returns (feat, {grad name: tensor}, dx).
    plan.seen: which workspace tensors each stage left written, byte by byte -- the evidence of the path the library took
    (big0: the two-pass stem; dtmp: the unfolded downsample gradient; sa1..se_rows: the merged SE form; dz; bits)"""
    net = plan.net
    nb = len(net.blocks)
    seen = plan.seen = dict(dz={}, dtmp={}, se_merged={}, big0=None, bits=None)
    feat = plan.forward()
    seen["bits"] = "none after the forward" if bits_untouched(plan, "by the forward") else "written" if net.bits else None
    T = plan.read_forward()
    PR.replay_forward(net, T, plan.P, plan.B0, plan.B, plan.x.view(net.N, net.cin, net.H, net.W), feat, rep)
    before = plan.wf.clone()
    final, dx = {}, None
    plan.fill_backward()
    x4 = plan.x.view(net.N, net.cin, net.H, net.W)
    for st in range(net.n_stages):
        plan.backward(st, st + 1)
        S, G = plan.read_backward(), plan.grads()
        last = st == net.n_stages - 1
        dxs = plan.arena.views["dx"].clone()
        if last:
            dx = dxs
        else:
            assert bool(torch.isnan(dxs).all()), "stage %d wrote the input gradient" % st
        PR.replay_backward_stage(net, T, S, G, plan.P, x4, plan.dfeat, st, dxs.view(x4.shape) if last else None, rep)
        if 1 <= st <= nb:
            k = net.blocks[nb - st]
            seen["dz"][k.i] = not plan.untouched(1, "dz")
            if k.down:
                seen["dtmp"][k.i] = not plan.untouched(1, "dtmp")
            if net.se:
                wrote = [not plan.untouched(1, n) for n in SE_MERGED_ONLY]
                assert all(wrote) or not any(wrote), "block %d: %s written in part: %s" % (k.i, SE_MERGED_ONLY, wrote)
                seen["se_merged"][k.i] = wrote[0]
        elif last:
            seen["big0"] = not plan.untouched(1, "big0")
        for n, g in G.items():
            if bool(torch.isfinite(g).all()):
                assert n not in final, "%s written by two stages" % n
                final[n] = g
            else:
                assert bool(torch.isnan(g).all()), "%s partly written by stage %d" % (n, st)
        plan.fill_backward(keep=st & 1)
    assert sorted(final) == sorted(plan.names), set(plan.names) - set(final)
    assert same_bits(before, plan.wf), "the backward wrote into the forward workspace"
    if bits_untouched(plan, "by the backward"):
        seen["bits"] = "none after the forward, none after the backward"
    # the paths in effect in this process (the environment it was started with), held against the stored data
    lib = plan.lib
    assert seen["big0"] == (not (net.training and switch_get(lib, "ECGMM_STEM_FUSE"))), "stem big0 written: %s" % seen["big0"]
    assert rep.paths["stem bwd"] == ("two passes" if seen["big0"] else "one pass")
    if net.se:
        merged = bool(net.training and switch_get(lib, "ECGMM_SE_MERGE"))
        assert seen["se_merged"] == {k.i: merged for k in net.blocks}, "merged SE pass ran on blocks %s" % seen["se_merged"]
    for k in net.blocks:
        if k.down:      # (with ECGMM_DOWN_FOLD on, which blocks fold is the igemm kernel's decision: the replay follows dtmp)
            assert rep.paths["blk%d din" % k.i] == ("dtmp" if seen["dtmp"][k.i] else "folded")
            assert seen["dtmp"][k.i] or switch_get(lib, "ECGMM_DOWN_FOLD"), "block %d folded with ECGMM_DOWN_FOLD=0" % k.i
        assert seen["dz"][k.i] == (k.i not in net.fused2), "block %d: dz written %s, fused2 %s" % (k.i, seen["dz"][k.i], net.fused2)
    return feat, final, dx, T


def show_paths(plan, what):
    """one PATHS line per run: what the stored data says about the branches taken"""
    s = plan.seen
    on = lambda d: ",".join(str(i) for i in sorted(d) if d[i]) or "-"
    print("PATHS %s: stem big0 %s; dz written on blocks %s; dtmp written on blocks %s of %s; merged SE scratch written on "
          "blocks %s; fused bn2 reductions %s; bits %s" % (what, "written (two passes)" if s["big0"] else "0xFF (one pass)",
                                                           on(s["dz"]), on(s["dtmp"]), sorted(s["dtmp"]), on(s["se_merged"]),
                                                           sorted(plan.net.fused2), s["bits"]))


def fused_blocks(plan, capable_only=False):
    """ResNet18 blocks whose bn2 reduction is fused into the next block's conv1 input gradient (ECGMM_BN_FUSE_MIN_M = 0 in the
    runs that have any; the threshold in effect is part of the rule):
    the rule of plan_resnet18.hip (bf16 training, the next block has no downsample and its conv1 input gradient runs on the
    halo kernel: stride-1 3x3, pixels a multiple of 256, channels of 64 / 128, 256 + 2 (W + 1) halo rows within 384 / 320),
    checked against the library's own answer (ecgmm_conv_bwd_data_bnred_rows) under the switches in effect.  That query says
    what the kernel can do; whether the plan asks it to is the plan's own switch: none with ECGMM_BN_FUSE=0 (capable_only:
    the blocks the kernel could serve, whatever that switch says)"""
    net = plan.net
    if net.kind != "r18" or not net.bf16 or not net.training:
        return set()
    plan_fuses = bool(switch_get(plan.lib, "ECGMM_BN_FUSE"))
    out = set()
    for k in net.blocks[:-1]:
        nx = net.blocks[k.i + 1]
        rule = (not nx.down and (net.N * nx.hin * nx.win) % 256 == 0 and nx.cin % 64 == 0 and (nx.cin == 64 or nx.cin % 128 == 0)
                and 256 + 2 * (nx.win + 1) <= (320 if nx.cin > 64 else 384))
        d = L.ConvDesc(net.N, nx.hin, nx.win, nx.cin, nx.cout, 3, 3, nx.stride, 1, 1)
        assert rule == (plan.lib.ecgmm_conv_bwd_data_bnred_rows(L.BF16, C.byref(d)) > 0), "block %d" % k.i
        if rule and (capable_only or (plan_fuses and net.N * k.hout * k.wout >= switch_get(plan.lib, "ECGMM_BN_FUSE_MIN_M"))):
            out.add(k.i)
    return out


CASES = [(k, s, dt) for k in ("r18", "r1d") for s in SHAPES[k] for dt in (L.BF16, L.F32)]
ids = lambda cases: ["%s-%s-%s" % (k, "x".join(map(str, s)), "bf16" if dt == L.BF16 else "fp32") for k, s, dt in cases]


@pytest.mark.parametrize("kind,shape,dt", CASES, ids=ids(CASES))
def test_plan_replays_against_float64_default_switches(kind, shape, dt):
    """runs 1, 4 and 6: staged backward replayed stage by stage; the whole backward in one call on freshly filled buffers
    gives the same bits; the forward called twice gives the same bits; views of absent tensors are refused"""
    plan = Plan(kind, shape, dt)
    rep = PR.Rep()
    feat, final, dx, _ = staged(plan, rep)
    rep.show("%s %s %s default" % (kind, shape, "bf16" if dt == L.BF16 else "fp32"))
    show_paths(plan, "%s %s %s default" % (kind, shape, "bf16" if dt == L.BF16 else "fp32"))
    # the whole backward in one call
    plan.fill_backward()
    plan.backward(0, plan.net.n_stages)
    whole = plan.grads()
    for n in plan.names:
        assert same_bits(whole[n], final[n]), "%s: one call and staged calls differ" % n
    assert same_bits(plan.arena.views["dx"], dx), "input gradient: one call and staged calls differ"
    # the forward again, into the same workspace
    ws1 = plan.wf.clone()
    feat2 = plan.forward()
    assert same_bits(feat, feat2) and same_bits(ws1, plan.wf), "the second forward differs from the first"
    # absent tensors
    # (the bits views belong to the layout of every bf16 ResNet18 plan, whether or not this process writes them)
    absent = [(0, "yd", 0), (0, "coefd", 0), (0, "nonsense", 0), (1, "X", 2)]
    absent += [] if (kind == "r18" and dt == L.BF16) else [(0, "bits", 0)]
    for bw, name, index in absent:
        assert plan.view(bw, name, index)[0] == 1 and name.encode() in plan.lib.ecgmm_last_error(), (name, index)


SW_CASES = CASES + [(k, HALO_SHAPES[k], L.BF16) for k in ("r18", "r1d")]


@pytest.mark.parametrize("kind,shape,dt", SW_CASES, ids=ids(SW_CASES))
def test_plan_replays_with_halo_ring_and_fused_reductions(kind, shape, dt):
    """run 2: ECGMM_CONV_HALO=2, ECGMM_WGRAD_RING=2, ECGMM_BN_FUSE_MIN_M=0"""
    lib = L.lib()
    with switches(lib, ECGMM_CONV_HALO=2, ECGMM_WGRAD_RING=2, ECGMM_BN_FUSE_MIN_M=0):
        plan = Plan(kind, shape, dt)
        plan.net.fused2 = fused_blocks(plan)
        print("fused bn2 reductions: blocks", sorted(plan.net.fused2))
        if kind == "r18" and shape == HALO_SHAPES["r18"]:
            assert plan.net.fused2 == {0, 2}, plan.net.fused2       # fail if none did: this is the case that is here for them
        elif shape in SHAPES[kind]:
            assert not plan.net.fused2                               # (no pixel count of the base shapes is a multiple of 256)
        rep = PR.Rep()
        staged(plan, rep)
        rep.show("%s %s %s halo+ring+fused" % (kind, shape, "bf16" if dt == L.BF16 else "fp32"))


@pytest.mark.parametrize("kind,shape,dt", CASES, ids=ids(CASES))
def test_plan_replays_with_the_side_streams_off(kind, shape, dt):
    """run 3"""
    lib = L.lib()
    try:
        L.check(lib.ecgmm_side_wgrad(0))
        plan = Plan(kind, shape, dt)
        rep = PR.Rep()
        staged(plan, rep)
        rep.show("%s %s %s side streams off" % (kind, shape, "bf16" if dt == L.BF16 else "fp32"))
    finally:
        L.check(lib.ecgmm_side_wgrad(switch_get(lib, "ECGMM_SIDE_WGRAD")))


EVAL_CASES = [(k, SHAPES[k][0], dt) for k in ("r18", "r1d") for dt in (L.BF16, L.F32)]


@pytest.mark.parametrize("kind,shape,dt", EVAL_CASES, ids=ids(EVAL_CASES))
def test_plan_replays_in_eval_mode(kind, shape, dt):
    """run 5: the affine BatchNorm backward; running statistics untouched (asserted by the replay's coef check); no bits written"""
    plan = Plan(kind, shape, dt, training=False)
    rep = PR.Rep()
    staged(plan, rep)
    rep.show("%s %s %s eval" % (kind, shape, "bf16" if dt == L.BF16 else "fp32"))
    for n in plan.bnames:
        assert torch.equal(plan.B[n], plan.B0[n]), n + " changed in eval mode"
    if kind == "r18" and dt == L.BF16:
        for k in plan.net.blocks:
            assert bool((plan.raw(0, "bits", k.i) == 0xFF).all()), "block %d: bits written in eval mode" % k.i
