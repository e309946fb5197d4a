"""CPU proof of tests/plan_replay.py and of the workspace views.

The replay is given what a correct plan would leave behind -- every stored tensor computed with plain torch in fp32 on the CPU
(and, for the bf16 plan, rounded to bf16 where the plan stores bf16), in the plan's own order and from the stored tensors --
and must accept it with every unsure-mask share under UNSURE_CAP.  Then the same dict is built with one slip of the kind a
launch plan can make (a wrong workspace tensor, a wrong parity, a wrong table index, a corrupted channel) and the replay must
reject it naming the op.  No HIP kernel runs here; the library is loaded only for the view tests (host-only entry points).
"""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as TF

from oracle import fill, ref_models as O

from . import plan_replay as PR

NAN = float("nan")
R18_SHAPE, R1D_SHAPE = (2, 3, 40, 56), (2, 2, 203)
DROP_P = 0.3


def make(kind, bf16, training=True):
    if kind == "r18":
        N, cin, H, W = R18_SHAPE
        model = fill.hash_fill_module(O.ResNet18(num_classes=16), "replay18.")
        net = PR.Net("r18", N, cin, H, W, bf16, training)
        x = fill.hash_tensor((N, cin, H, W), 801)
        dfeat = fill.hash_tensor((N, 16), 802)
    else:
        N, cin, L = R1D_SHAPE
        model = fill.hash_fill_module(O.ResNet1D_SE(cin, 5), "replay1d.")
        net = PR.Net("r1d", N, cin, 1, L, bf16, training, dropout_p=DROP_P)
        x = fill.hash_tensor((N, cin, 1, L), 803, 1.7)
        dfeat = fill.hash_tensor((N, 5), 804)
    return net, model, x, dfeat


# ----------------------------------------------------------------------------------------------------------------------
# the plans restated with plain torch fp32, tensor by tensor; `slip` names the one mistake to make
# ----------------------------------------------------------------------------------------------------------------------
def _w(net, w):
    w = PR.w4(w.float())
    return w.bfloat16().float() if net.bf16 else w


def _conv_bwd(x, w, dy, stride, pad):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    gx, gw = torch.autograd.grad(TF.conv2d(x, w, None, stride, pad), (x, w), dy)
    return gx, gw


def _coef(net, y32, bn, P, B0, B1):
    """coef [4][C] from the fp32 conv output (the plan: from the kernel's fp32 accumulators), running statistics updated"""
    g, b = P[bn + ".weight"], P[bn + ".bias"]
    if net.training:
        M = y32.numel() // y32.shape[1]
        mean = y32.mean((0, 2, 3))
        var = y32.var((0, 2, 3), unbiased=False)
        B1[bn + ".running_mean"] = (1 - net.momentum) * B0[bn + ".running_mean"] + net.momentum * mean
        B1[bn + ".running_var"] = (1 - net.momentum) * B0[bn + ".running_var"] + net.momentum * var * M / max(M - 1, 1)
        B1[bn + ".num_batches_tracked"] = B0[bn + ".num_batches_tracked"] + 1
    else:
        mean, var = B0[bn + ".running_mean"], B0[bn + ".running_var"]
    inv = 1.0 / torch.sqrt(var + net.eps)
    sc = g * inv
    return torch.stack([sc, b - mean * sc, mean, inv])


def _ch(v):
    return v.view(1, -1, 1, 1)


def _maxpool(a):
    """3x3 / 2 / 1 max-pool of a >= 0 (NCHW): value and the earliest tap kh * 3 + kw that holds it"""
    N, Cn, H, W = a.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = torch.full((N, Cn, 2 * OH + 1, 2 * OW + 1), float("-inf"))
    p[:, :, 1:H + 1, 1:W + 1] = a
    best = torch.full((N, Cn, OH, OW), float("-inf"))
    idx = torch.zeros((N, Cn, OH, OW), dtype=torch.int64)
    for t in range(9):
        tap = p[:, :, t // 3:t // 3 + 2 * OH:2, t % 3:t % 3 + 2 * OW:2]
        up = tap > best
        idx[up], best = t, torch.maximum(best, tap)
    return best, idx


def _unpool(dp, pooled, idx, H, W):
    N, Cn, OH, OW = dp.shape
    out = torch.zeros(N, Cn, H + 2, W + 2)
    for t in range(9):
        sel = (idx == t) & (pooled > 0)
        out[:, :, t // 3:t // 3 + 2 * OH:2, t % 3:t % 3 + 2 * OW:2] += torch.where(sel, dp, torch.zeros_like(dp))
    return out[:, :, 1:H + 1, 1:W + 1]


def _bn_bwd(net, dz, y, coef, gamma, dbias=False):
    """(dy, dgamma, dbeta[, dbias]) of one BatchNorm backward in fp32 from dz = the gradient behind the mask / gate"""
    xh = (y - _ch(coef[2])) * _ch(coef[3])
    M = y.numel() // y.shape[1]
    dbeta, dgamma = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    if net.training:
        dy = _ch(gamma * coef[3]) * (dz - _ch(dbeta / M) - xh * _ch(dgamma / M))
    else:
        dy = dz * _ch(coef[0])
    return dy, dgamma, dbeta


def build(net, model, x, dfeat, slip=None, fold=True):
    """-> T, P, B0, B1, feat, snaps: snaps[st] = (S, G, dx) after backward stage st"""
    bf, N = net.bf16, net.N
    st_ = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    P = {n: p.detach().clone() for n, p in model.named_parameters()}
    B0 = {n: b.detach().clone() for n, b in model.named_buffers()}
    B1 = {n: b.clone() for n, b in B0.items()}
    T, W = {}, {}
    xr = st_(x.float())
    bias = (lambda n: None if n is None else P[n])
    # ---- forward
    y0 = TF.conv2d(xr, _w(net, P[net.stem_w]), bias(net.stem_b), 2, net.stem_pad)
    c0 = _coef(net, y0, net.stem_bn, P, B0, B1)
    y0 = st_(y0)
    p0, idx0 = _maxpool(torch.relu(y0 * _ch(c0[0]) + _ch(c0[1])))
    p0 = st_(p0)
    T.update(y0=y0, coef0=c0, p0=p0, idx0=idx0)
    cur = p0
    for k in net.blocks:
        i, nm = k.i, net.names(k)
        w1, w2 = _w(net, P[nm["c1"]]), _w(net, P[nm["c2"]])
        W[i] = dict(w1=w1, w2=w2)
        for key, w in (("w1", w1), ("w2", w2)):
            T[(key + "f", i)], T[(key + "d", i)] = w.clone(), w.clone()
        y1 = TF.conv2d(cur, w1, bias(nm["b1"]), k.stride, net.pad)
        c1 = _coef(net, y1, nm["bn1"], P, B0, B1)
        y1 = st_(y1)
        a1 = st_(torch.relu(y1 * _ch(c1[0]) + _ch(c1[1])))
        y2 = TF.conv2d(a1, w2, bias(nm["b2"]), 1, net.pad)
        c2 = _coef(net, y2, nm["bn2"], P, B0, B1)
        y2 = st_(y2)
        z = y2 * _ch(c2[0]) + _ch(c2[1])
        if net.se:
            s = [P[n] for n in nm["se"]]
            m = y2.mean((2, 3)) * c2[0] + c2[1]
            h = torch.relu(m @ s[0].t() + s[1])
            g = torch.sigmoid(h @ s[2].t() + s[3])
            T[("m", i)], T[("h", i)], T[("g", i)] = m, h, g
            z = z * g.view(N, -1, 1, 1)
        if k.down:
            wd = _w(net, P[nm["cd"]])
            W[i]["wd"] = wd
            T[("wdf", i)], T[("wdd", i)] = wd.clone(), wd.clone()
            yd = TF.conv2d(cur, wd, bias(nm["bd"]), k.stride, (0, 0))
            cd = _coef(net, yd, nm["bnd"], P, B0, B1)
            yd = st_(yd)
            T[("yd", i)], T[("coefd", i)] = yd, cd
            if slip == "coefd_coef2" and i == (2 if net.kind == "r18" else 1):
                z = y2 * _ch(cd[0]) + _ch(cd[1])
                if net.se:
                    z = z * T[("g", i)].view(N, -1, 1, 1)
                res = yd * _ch(c2[0]) + _ch(c2[1])
            else:
                res = yd * _ch(cd[0]) + _ch(cd[1])
        else:
            res = a1 if (slip == "res_a1" and i == (1 if net.kind == "r18" else 0)) else cur
        out = st_(torch.relu(z + res))
        T.update({("y1", i): y1, ("coef1", i): c1, ("a1", i): a1, ("y2", i): y2, ("coef2", i): c2, ("out", i): out})
        if net.bits:
            T[("bits", i)] = out > 0
            if slip == "bits_flip" and i == 3:
                T[("bits", i)].view(-1)[1234] ^= True
        cur = out
    pooled = cur.mean((2, 3))
    T["pooled"] = pooled
    if net.kind == "r18":
        feat = pooled @ P["fc.weight"].t() + P["fc.bias"]
    else:
        h1 = torch.relu(pooled @ P["classifier.1.weight"].t() + P["classifier.1.bias"])
        T["h1"], hin = h1, h1
        if net.training:
            keep = fill.hash_tensor((N, 64), 805) * 0.5 + 0.5 >= DROP_P
            scale = 1.0 / (1.0 - torch.tensor(DROP_P))
            hin = torch.where(keep, h1 * scale, torch.zeros_like(h1))
            T["dmask"], T["hd"] = keep, hin
        feat = hin @ P["classifier.4.weight"].t() + P["classifier.4.bias"]
    # ---- backward
    buf = lambda: torch.full((net.max_act,), NAN)
    two = lambda: [buf(), buf()] if net.dual else [buf()]
    S = dict(X=[buf(), buf()], dz=buf(), dy=two(), dy1=two(), dyd=two(), da=buf(), dtmp=buf(),
             big0=torch.full((N * net.H1 * net.W1 * 64,), NAN), big1=torch.full((N * net.H1 * net.W1 * 64,), NAN))
    G = {n: torch.full_like(p, NAN) for n, p in P.items()}
    snaps = []

    def put(b, t):
        v = PR.cl(t).reshape(-1)
        b[:v.numel()] = v

    def snap(dx=None):
        snaps.append(({k: [b.double().clone() for b in v] if isinstance(v, list) else v.double().clone() for k, v in S.items()},
                      {k: v.clone() for k, v in G.items()}, dx))

    nb = len(net.blocks)
    last = net.blocks[-1]
    # stage 0
    if net.kind == "r18":
        G["fc.weight"], G["fc.bias"] = dfeat.t() @ pooled, dfeat.sum(0)
        dpooled = dfeat @ P["fc.weight"]
    else:
        G["classifier.4.weight"], G["classifier.4.bias"] = dfeat.t() @ hin, dfeat.sum(0)
        dfh = dfeat @ P["classifier.4.weight"]
        if net.training:
            dfh = torch.where(T["dmask"], dfh * scale, torch.zeros_like(dfh))
        dh1 = dfh * (T["h1"] > 0)
        G["classifier.1.weight"], G["classifier.1.bias"] = dh1.t() @ pooled, dh1.sum(0)
        dpooled = dh1 @ P["classifier.1.weight"]
        S["dfeat_h"], S["dh1"] = dfh, dh1
        S.update(dg=torch.full((N * 256,), NAN), ds=torch.full((N * 256,), NAN), dh=torch.full((N * 16,), NAN), dm=torch.full((N * 256,), NAN))
    S["dpooled"] = dpooled
    R = last.hout * last.wout
    dX = st_((dpooled * torch.tensor(1.0 / R, dtype=torch.float32)).view(N, -1, 1, 1).expand(-1, -1, last.hout, last.wout).contiguous())
    put(S["X"][0], dX)
    snap()
    for st in range(1, nb + 1):
        i = nb - st
        k, nm = net.blocks[i], net.names(net.blocks[i])
        pp = (st & 1) if net.dual else 0
        for key in ("dz", "da", "dtmp"):       # per-stage transients
            S[key].fill_(NAN)
        inp = T["p0"] if i == 0 else T[("out", i - 1)]
        dcur = dX
        out_i, y2, y1 = T[("out", i)], T[("y2", i)], T[("y1", i)]
        maskt = out_i
        if slip == "mask_prev" and i == (1 if net.kind == "r18" else 0):
            maskt = inp
        dz = torch.where(maskt > 0, dcur, torch.zeros_like(dcur))
        if slip == "dz_unmasked" and i == nb - 2:
            put(S["dz"], dcur)
        else:
            put(S["dz"], dz)
        d = dz
        if net.se:
            c2 = T[("coef2", i)]
            s = [P[n] for n in nm["se"]]
            g, h, m = T[("g", i)], T[("h", i)], T[("m", i)]
            dzt = torch.where(out_i > 0, dcur, torch.zeros_like(dcur))
            dg = (dzt * (y2 * _ch(c2[0]) + _ch(c2[1]))).sum((2, 3))
            ds = dg * g * (1 - g)
            dh = (ds @ s[2]) * (h > 0)
            dm = dh @ s[0]
            if not (slip == "se_no_1_over_L" and i == 2):
                dm = dm * torch.tensor(1.0 / (k.hout * k.wout), dtype=torch.float32)
            G[nm["se"][2]], G[nm["se"][3]], G[nm["se"][0]], G[nm["se"][1]] = ds.t() @ h, ds.sum(0), dh.t() @ m, dh.sum(0)
            for key, v in (("dg", dg), ("ds", ds), ("dh", dh), ("dm", dm)):
                S[key].fill_(NAN)
                S[key][:v.numel()] = v.reshape(-1)
            d = dz * g.view(N, -1, 1, 1) + dm.view(N, -1, 1, 1)
        dy, dgam, dbet = _bn_bwd(net, d, y2, T[("coef2", i)], P[nm["bn2"] + ".weight"])
        dy = st_(dy)
        if slip == "dbeta_index" and i == nb - 1:
            G[nm["bn2"] + ".weight"] = dbet         # dbeta lands on dgamma's entry; the bias entry is never written
        else:
            G[nm["bn2"] + ".weight"], G[nm["bn2"] + ".bias"] = dgam, dbet
        if nm["b2"] is not None:
            G[nm["b2"]] = dy.sum((0, 2, 3))
        put(S["dy"][pp ^ 1] if (slip == "stale_dy" and st == 3) else S["dy"][pp], dy)
        da, G[nm["c2"]] = _conv_bwd(T[("a1", i)], W[i]["w2"], dy, 1, net.pad)
        da = st_(da)
        put(S["da"], da)
        c1 = T[("coef1", i)]
        dz1 = torch.where(y1 * _ch(c1[0]) + _ch(c1[1]) > 0, da, torch.zeros_like(da))
        dy1, G[nm["bn1"] + ".weight"], G[nm["bn1"] + ".bias"] = _bn_bwd(net, dz1, y1, c1, P[nm["bn1"] + ".weight"])
        dy1 = st_(dy1)
        if nm["b1"] is not None:
            G[nm["b1"]] = dy1.sum((0, 2, 3))
        put(S["dy1"][pp], dy1)
        gx1, gw1 = _conv_bwd(inp, W[i]["w1"], dy1, k.stride, net.pad)
        if slip == "dw_channel_zero" and i == 4 % nb:
            gw1[3] = 0
        G[nm["c1"]] = gw1
        if k.down:
            dyd, G[nm["bnd"] + ".weight"], G[nm["bnd"] + ".bias"] = _bn_bwd(net, dz, T[("yd", i)], T[("coefd", i)], P[nm["bnd"] + ".weight"])
            dyd = st_(dyd)
            if nm["bd"] is not None:
                G[nm["bd"]] = dyd.sum((0, 2, 3))
            put(S["dyd"][pp], dyd)
            gxd, G[nm["cd"]] = _conv_bwd(inp, W[i]["wd"], dyd, k.stride, (0, 0))
            if fold:
                dX = st_(gx1 + gxd)
            else:
                dtmp = st_(gxd)
                put(S["dtmp"], dtmp)
                dX = st_(gx1 + dtmp)
        else:
            dX = st_(gx1 + dz)
        for n_ in (nm["c1"], nm["c2"], nm["cd"]):
            if n_ in G and G[n_].dim() != P[n_].dim():
                G[n_] = G[n_].reshape(P[n_].shape)
        put(S["X"][(st & 1) ^ 1] if (slip == "x_parity" and st == 2) else S["X"][st & 1], dX)
        snap()
    # stem
    H1, W1 = net.H1, net.W1
    M = N * H1 * W1
    gam = P[net.stem_bn + ".weight"]
    c0 = T["coef0"]
    if net.training and net.stem_fused:
        g_ = torch.where(p0 > 0, dX, torch.zeros_like(dX))
        dbet = g_.sum((0, 2, 3))
        rsc = torch.where(c0[0] != 0, 1.0 / c0[0], torch.zeros_like(c0[0]))
        dgam = (g_ * (p0 - _ch(c0[1] + c0[2] * c0[0])) * _ch(rsc)).sum((0, 2, 3)) * c0[3]
        dz0 = _unpool(dX, p0, idx0, H1, W1)
        xh = (y0 - _ch(c0[2])) * _ch(c0[3])
        big1 = st_(_ch(gam * c0[3]) * (dz0 - _ch(dbet / M) - xh * _ch(dgam / M)))
    else:
        # two passes (eval, or training without the fused pass): max-pool backward into big0, BatchNorm backward of the mode
        big0 = st_(_unpool(dX, p0, idx0, H1, W1))
        if slip == "big0_tap":                  # the largest element lands one column beside the tap idx0 names
            n_, c_, h_, w_ = PR.F._unravel(int(big0.abs().argmax()), big0.shape)
            w2_ = w_ + 1 if w_ + 1 < W1 else w_ - 1
            big0[n_, c_, h_, w2_] += big0[n_, c_, h_, w_]
            big0[n_, c_, h_, w_] = 0
        put(S["big0"], big0)
        big1, dgam, dbet = _bn_bwd(net, big0, y0, c0, gam)
        if slip == "big1_affine":               # the eval formula behind a training forward
            big1 = big0 * _ch(c0[0])
        big1 = st_(big1)
    G[net.stem_bn + ".weight"], G[net.stem_bn + ".bias"] = dgam, dbet
    if net.stem_b is not None:
        G[net.stem_b] = big1.sum((0, 2, 3))
        if slip == "dbias_short":               # one row (the largest) never added
            r_ = PR.rows(big1)
            G[net.stem_b] = G[net.stem_b] - r_[int(r_.abs().sum(1).argmax())]
    put(S["big1"], big1)
    _, gw0 = _conv_bwd(xr, _w(net, P[net.stem_w]), big1, 2, net.stem_pad)
    G[net.stem_w] = gw0.reshape(P[net.stem_w].shape)
    # (in float64, stored as fp32: the bound of this fp32 output, KAPPA of the kernels' chunked fp32 accumulation, is below what
    #  torch's serial fp32 sum over 64 x 49 terms reaches on some CPUs -- 1.47 x on one machine, 0.74 x on another)
    dx, _ = _conv_bwd(xr.double(), _w(net, P[net.stem_w]).double(), big1.double(), 2, net.stem_pad)
    dx = dx.float()
    snap(dx)
    T = {k: (v if v.dtype in (torch.bool, torch.int64) else v.double()) for k, v in T.items()}
    return T, P, B0, B1, feat, snaps


def replay_all(net, built, x, dfeat, stages=None, forward=True):
    T, P, B0, B1, feat, snaps = built
    rep = PR.Rep()
    if forward:
        PR.replay_forward(net, T, P, B0, B1, x, feat, rep)
    for st in (range(net.n_stages) if stages is None else stages):
        S, G, dx = snaps[st]
        PR.replay_backward_stage(net, T, S, G, P, x, dfeat, st, dx, rep)
    return rep


CASES = [("r18", False), ("r18", True), ("r1d", False), ("r1d", True)]
IDS = ["r18-fp32", "r18-bf16", "r1d-fp32", "r1d-bf16"]


@pytest.mark.parametrize("kind,bf16", CASES, ids=IDS)
def test_replay_accepts_a_plan_restated_in_torch(kind, bf16):
    """(every check_unsure inside the checkers has passed when this returns: the unsure share of every op is under the cap)"""
    net, model, x, dfeat = make(kind, bf16)
    rep = replay_all(net, build(net, model, x, dfeat), x, dfeat)
    rep.show("%s %s torch-cpu" % (kind, "bf16" if bf16 else "fp32"))
    assert max(rep.worst.values()) <= 1.0
    want = {"conv", "coef", "maxpool", "pack", "bn_act", "avgpool", "linear", "bcast", "bn_bwd", "dw", "dgrad", "stem_bwd", "stem_dx"}
    want |= {"se_mlp", "se_gate", "dropout"} if kind == "r1d" else set()
    want |= {"bits"} if (kind == "r18" and bf16) else set()
    assert want <= set(rep.worst), want - set(rep.worst)


@pytest.mark.parametrize("kind,bf16", [("r18", True), ("r1d", False)], ids=["r18-bf16", "r1d-fp32"])
def test_replay_accepts_the_unfolded_downsample_and_eval_mode(kind, bf16):
    net, model, x, dfeat = make(kind, bf16)
    replay_all(net, build(net, model, x, dfeat, fold=False), x, dfeat, stages=[2, 3], forward=False)
    net, model, x, dfeat = make(kind, bf16, training=False)
    rep = replay_all(net, build(net, model, x, dfeat), x, dfeat)
    assert max(rep.worst.values()) <= 1.0


# slip -> (kinds it exists for, forward?, backward stage of (r18, r1d), the op the replay must name)
SLIPS = {
    "res_a1": (("r18", "r1d"), True, None, r"blk[01] out"),
    "coefd_coef2": (("r18", "r1d"), True, None, r"blk[12] out"),
    "mask_prev": (("r18", "r1d"), False, (7, 3), r"blk[01] bn2 bwd"),
    "stale_dy": (("r18",), False, (3, None), r"blk5 bn2 bwd dy"),
    "x_parity": (("r18", "r1d"), False, (2, 2), r"blk\d (dcur|bn2 bwd|se gate grad)"),
    "dbeta_index": (("r18", "r1d"), False, (1, 1), r"blk[27] bn2 bwd dbeta"),
    "dw_channel_zero": (("r18", "r1d"), False, (4, 2), r"blk[41] dw1"),
    "bits_flip": (("r18",), True, None, r"blk3 bits"),
    "se_no_1_over_L": (("r1d",), False, (None, 1), r"blk2 se bwd dm"),
    "dz_unmasked": (("r18", "r1d"), False, (2, 2), r"blk[16] bn2 bwd dz_out"),
}
SLIP_PARAMS = [(s, k, bf) for s, v in SLIPS.items() for k in v[0] for bf in ((True,) if s == "bits_flip" else (False, True))]


@pytest.mark.parametrize("slip,kind,bf16", SLIP_PARAMS, ids=["%s-%s-%s" % (s, k, "bf16" if b else "fp32") for s, k, b in SLIP_PARAMS])
def test_replay_rejects_a_slip_and_names_the_op(slip, kind, bf16):
    _, fwd, stages, pattern = SLIPS[slip]
    net, model, x, dfeat = make(kind, bf16)
    built = build(net, model, x, dfeat, slip=slip)
    with pytest.raises(AssertionError) as e:
        if fwd:
            replay_all(net, built, x, dfeat, stages=[])
        else:
            replay_all(net, built, x, dfeat, stages=[stages[0 if kind == "r18" else 1]], forward=False)
    assert re.search(pattern, str(e.value)), str(e.value)[:400]


# ----------------------------------------------------------------------------------------------------------------------
# the training stem in two passes (a plan started with ECGMM_STEM_FUSE=0) and a plan that stores no ReLU bits
# (ECGMM_RELU_BITS=0): what the caller tells Net
# ----------------------------------------------------------------------------------------------------------------------
def two_pass(kind, bf16):
    net, model, x, dfeat = make(kind, bf16)
    net.stem_fused = False
    return net, model, x, dfeat


@pytest.mark.parametrize("kind,bf16", CASES, ids=IDS)
def test_replay_accepts_the_training_stem_in_two_passes(kind, bf16):
    net, model, x, dfeat = two_pass(kind, bf16)
    stem = [net.n_stages - 1]
    two = build(net, model, x, dfeat)
    rep = replay_all(net, two, x, dfeat, stages=stem, forward=False)
    assert rep.paths == {"stem bwd": "two passes"} and max(rep.worst.values()) <= 1.0
    assert {"stem_bwd", "bn_bwd", "dw", "stem_dx"} <= set(rep.worst)
    # the same dicts told to be the one-pass form: big0 is there although nothing should have written it
    net.stem_fused = True
    with pytest.raises(AssertionError, match="stem big0: written"):
        replay_all(net, two, x, dfeat, stages=stem, forward=False)
    # and the one-pass dicts told to be two passes: big0 was never written
    one = build(net, model, x, dfeat)
    rep = replay_all(net, one, x, dfeat, stages=stem, forward=False)
    assert rep.paths == {"stem bwd": "one pass"}
    net.stem_fused = False
    with pytest.raises(AssertionError, match="stem maxpool bwd big0"):
        replay_all(net, one, x, dfeat, stages=stem, forward=False)


# planted error -> (kinds, the op the replay must name)
STEM_SLIPS = {
    "big0_tap": (("r18", "r1d"), r"stem maxpool bwd big0"),
    "big1_affine": (("r18", "r1d"), r"stem bn bwd dy"),
    "dbias_short": (("r1d",), r"stem bn bwd dbias"),
}
STEM_SLIP_PARAMS = [(s, k, bf) for s, v in STEM_SLIPS.items() for k in v[0] for bf in (False, True)]


@pytest.mark.parametrize("slip,kind,bf16", STEM_SLIP_PARAMS,
                         ids=["%s-%s-%s" % (s, k, "bf16" if b else "fp32") for s, k, b in STEM_SLIP_PARAMS])
def test_replay_rejects_a_slip_in_the_two_pass_training_stem(slip, kind, bf16):
    net, model, x, dfeat = two_pass(kind, bf16)
    built = build(net, model, x, dfeat, slip=slip)
    with pytest.raises(AssertionError) as e:
        replay_all(net, built, x, dfeat, stages=[net.n_stages - 1], forward=False)
    assert re.search(STEM_SLIPS[slip][1], str(e.value)), str(e.value)[:400]


def test_the_downsample_branch_taken_is_reported():
    net, model, x, dfeat = make("r18", True)
    for fold, want in ((True, "folded"), (False, "dtmp")):
        rep = replay_all(net, build(net, model, x, dfeat, fold=fold), x, dfeat, stages=[2, 3], forward=False)
        assert rep.paths == {"blk6 din": want}, rep.paths       # (stage 2 = block 6, layer4.0; block 5 has no downsample)


def test_bits_are_checked_only_where_the_plan_stores_them():
    net, model, x, dfeat = make("r18", True)
    assert net.bits and not make("r18", False)[0].bits and not make("r18", True, training=False)[0].bits
    built = build(net, model, x, dfeat, slip="bits_flip")
    N, cin, H, W = R18_SHAPE
    for bits in (None, True):
        with pytest.raises(AssertionError, match="blk3 bits: 1 bits"):
            replay_all(PR.Net("r18", N, cin, H, W, True, bits=bits), built, x, dfeat, stages=[])
    off = PR.Net("r18", N, cin, H, W, True, bits=False)
    assert not off.bits
    rep = replay_all(off, built, x, dfeat, stages=[])
    assert "bits" not in rep.worst and max(rep.worst.values()) <= 1.0
    # (a plan that stores none has none to hand over either)
    T = {k: v for k, v in built[0].items() if k[0] != "bits"}
    replay_all(off, (T,) + built[1:], x, dfeat, stages=[])


# ----------------------------------------------------------------------------------------------------------------------
# the workspace views (host-only entry points of the built library)
# ----------------------------------------------------------------------------------------------------------------------
def _view(lib, fn, d, backward, name, index):
    off, nbytes = C.c_size_t(), C.c_size_t()
    rc = fn(C.byref(d), backward, name.encode(), index, C.byref(off), C.byref(nbytes))
    return rc, off.value, nbytes.value


def expected_views(net):
    """{(backward, name, index): bytes} the descriptor implies, from the network's own arithmetic"""
    es, N, f = (2 if net.bf16 else 4), net.N, 4
    taps = net.kh * 3
    pool = N * net.H2 * net.W2 * 64
    big = N * net.H1 * net.W1 * 64 * es
    v = {(0, "y0", 0): big, (0, "coef0", 0): 4 * 64 * f, (0, "p0", 0): pool * es, (0, "idx0", 0): pool,
         (0, "pooled", 0): N * net.feat_c * f}
    if net.se:
        v.update({(0, "h1", 0): N * 64 * f, (0, "hd", 0): N * 64 * f, (0, "dmask", 0): N * 64})
    for k in net.blocks:
        osz = N * k.hout * k.wout * k.cout
        w1, w2, wd = k.cout * k.cin * taps * es, k.cout * k.cout * taps * es, k.cout * k.cin * es
        per = dict(w1f=w1, w1d=w1, w2f=w2, w2d=w2, y1=osz * es, a1=osz * es, y2=osz * es, out=osz * es, coef1=4 * k.cout * f, coef2=4 * k.cout * f)
        if k.down:
            per.update(wdf=wd, wdd=wd, yd=osz * es, coefd=4 * k.cout * f)
        if net.kind == "r18" and net.bf16:
            per["bits"] = osz // 8
        if net.se:
            per.update(m=N * k.cout * f, h=N * k.cr * f, g=N * k.cout * f)
        v.update({(0, n, k.i): b for n, b in per.items()})
    actb = net.max_act * es
    for n in ("dz", "da", "dtmp"):
        v[(1, n, 0)] = actb
    for n in ("X",) + (("dy", "dy1", "dyd") if net.dual else ()):
        v[(1, n, 0)] = v[(1, n, 1)] = actb
    if not net.dual:
        v.update({(1, n, 0): actb for n in ("dy", "dy1", "dyd")})
        v.update({(1, "dh1", 0): N * 64 * f, (1, "dfeat_h", 0): N * 64 * f, (1, "dg", 0): N * 256 * f, (1, "ds", 0): N * 256 * f,
                  (1, "dh", 0): N * 16 * f, (1, "dm", 0): N * 256 * f})
        # what only the merged SE / BatchNorm backward pass writes: per-sample sums and its 16 reduction rows [2][256]
        v.update({(1, n, 0): N * 256 * f for n in ("sa1", "sa2", "sa3")})
        v[(1, "se_rows", 0)] = 16 * 2 * 256 * f
    v.update({(1, "big0", 0): big, (1, "big1", 0): big, (1, "dpooled", 0): N * net.feat_c * f})
    return v


def plan_desc(L, net, out_dim=16, seed=7, offset=3):
    dt = L.BF16 if net.bf16 else L.F32
    if net.kind == "r18":
        return L.ResNet18Desc(net.N, net.H, net.W, out_dim, dt, int(net.training), net.momentum, net.eps)
    return L.ResNet1DDesc(net.N, net.cin, net.W, out_dim, dt, int(net.training), net.momentum, net.eps, net.dropout_p, seed, offset)


@pytest.mark.parametrize("kind", ["r18", "r1d"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("training", [0, 1], ids=["eval", "train"])
def test_workspace_views_lie_inside_the_workspace_and_do_not_overlap(kind, bf16, training):
    from ecgmm.hip import lib as L
    lib = L.lib()
    shape = (3, 3, 72, 104) if kind == "r18" else (3, 1, 1, 999)
    net = PR.Net(kind, shape[0], shape[1], shape[2], shape[3], bf16, bool(training), dropout_p=0.3)
    d = plan_desc(L, net)
    pre = "ecgmm_resnet18" if kind == "r18" else "ecgmm_resnet1d"
    fn = getattr(lib, pre + "_ws_view")
    total = [getattr(lib, pre + "_fwd_workspace")(C.byref(d)), getattr(lib, pre + "_bwd_workspace")(C.byref(d))]
    assert total[0] > 0 and total[1] > 0
    want = expected_views(net)
    rc, off, nb = _view(lib, fn, d, 0, "wstem", 0)
    assert rc == 0 and off == 0 and nb > 0
    spans = {0: [(off, off + nb, "wstem")], 1: []}
    for (bw, name, index), nbytes in want.items():
        rc, off, nb = _view(lib, fn, d, bw, name, index)
        assert rc == 0, (name, index, lib.ecgmm_last_error())
        assert nb == nbytes, (name, index, nb, nbytes)
        assert off % 256 == 0 and off + nb <= total[bw], (name, index, off, nb, total[bw])
        spans[bw].append((off, off + nb, "%s[%d]" % (name, index)))
    for bw in (0, 1):
        s = sorted(spans[bw])
        for a, b in zip(s, s[1:]):
            assert a[1] <= b[0], "views %s and %s overlap" % (a[2], b[2])
    # what this descriptor does not have, and what nobody has
    missing = [(0, "yd", 0), (0, "coefd", 0), (0, "wdf", 0), (0, "nonsense", 0), (1, "y1", 0), (0, "y1", len(net.blocks)), (1, "X", 2),
               (0, "y0", 1), (1, "dz", 1)]
    if not (kind == "r18" and bf16):
        missing.append((0, "bits", 0))
    if kind == "r18":
        missing += [(0, "m", 0), (1, "dg", 0), (1, "sa1", 0), (1, "se_rows", 0), (0, "wdd", 1), (0, "yd", 7)]
    for bw, name, index in missing:
        rc, _, _ = _view(lib, fn, d, bw, name, index)
        assert rc == 1 and name.encode() in lib.ecgmm_last_error(), (name, index, rc)


def test_view_of_the_stem_output_is_refused_under_stem_recompute():
    from ecgmm.hip import lib as L
    from .util import switches
    lib = L.lib()
    d = L.ResNet18Desc(4, 64, 64, 16, L.BF16, 1, 0.1, 1e-5)
    fn = lib.ecgmm_resnet18_ws_view
    stored = lib.ecgmm_resnet18_fwd_workspace(C.byref(d))
    assert _view(lib, fn, d, 0, "y0", 0)[0] == 0
    with switches(lib, ECGMM_STEM_RECOMPUTE=1):
        assert lib.ecgmm_resnet18_fwd_workspace(C.byref(d)) < stored       # the recomputing stem is on: no stored conv output
        rc = [_view(lib, fn, d, bw, n, 0)[0] for bw, n in ((0, "y0"), (1, "big0"), (1, "big1"))]
        assert _view(lib, fn, d, 0, "p0", 0)[0] == 0
    assert rc == [1, 1, 1], rc
    assert _view(lib, fn, d, 0, "y0", 0)[0] == 0
