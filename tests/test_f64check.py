"""The float64 conv checker (tests/f64check.py) on the CPU: it accepts the exact answer rounded to bf16 and torch's own fp32
convolution, and it rejects the ways a persistent tiled kernel goes wrong -- a 256-pixel tile zeroed (the last one, one that
spans images), a tile holding its neighbour's output, a 64-channel K slice missing, an image-border row read from the
neighbouring image instead of the zero padding, one element 4 bf16 ulps off, and for the weight gradient one tile's
contribution missing or one split-K chunk counted twice."""
import pytest
import torch
import torch.nn.functional as F

from . import f64check as F64

TILE = 256
N, CIN, COUT, H, W = 16, 128, 64, 12, 12        # 144 pixels per image: tile 1 (pixels 256..511) spans images 1..3


def _bf16(t):
    return t.to(torch.bfloat16).double()


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(11)
    z = torch.randn(N, CIN, H, W, generator=g)
    off = 1.0 + ((torch.arange(N).view(-1, 1) * 37 + torch.arange(CIN).view(1, -1) * 11) % 64).float().view(N, CIN, 1, 1) / 16
    x = _bf16(torch.where(z > 0, z + off, torch.zeros_like(z)))
    w = _bf16(torch.randn(COUT, CIN, 3, 3, generator=g) * (2.0 / (CIN * 9)) ** 0.5)
    dy = _bf16(torch.randn(N, COUT, H, W, generator=g) + torch.linspace(-2, 2, N * COUT).view(N, COUT, 1, 1))
    ref = F64.conv_ref64(x, w, dy, 1, (1, 1), chunk=5)
    return x, w, dy, ref


def _pix(t):
    """NCHW -> [pixels, channels] view in the kernels' channels-last pixel order (a copy)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).clone()


def _unpix(p, like):
    n, c, h, w = like.shape
    return p.view(n, h, w, c).permute(0, 3, 1, 2).contiguous()


def _rejects(out, ref, acc):
    r = F64.bf16_ratio(out, ref, acc)
    return r.ratio > 1.0


def test_reference_matches_a_plain_float64_convolution(case):
    x, w, dy, ref = case
    y = F.conv2d(x, w, padding=1)
    assert torch.equal(ref.y, y)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xr, wr, padding=1).backward(dy)
    assert torch.allclose(ref.dx, xr.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref.dw, wr.grad, rtol=1e-12, atol=1e-10)
    assert torch.equal(ref.ay, F.conv2d(x.abs(), w.abs(), padding=1))
    assert (ref.ay >= ref.y.abs()).all() and (ref.adx >= ref.dx.abs()).all() and (ref.adw >= ref.dw.abs() - 1e-9).all()


def test_half_ulp():
    v = torch.tensor([1.0, 1.99, 2.0, 0.75, 0.0, -3.0], dtype=torch.float64)
    assert F64.half_ulp_bf16(v).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0, 2.0 ** -7]
    # every fp32 -> bf16 rounding stays within it (what a kernel's epilogue does)
    t = torch.randn(100000, generator=torch.Generator().manual_seed(1)) * 100
    assert ((t.to(torch.bfloat16).double() - t.double()).abs() <= F64.half_ulp_bf16(t)).all()
    # ... also below 2^-126, where bf16 is evenly spaced by 2^-133: the binade rule alone (2^(e - 9)) is too small there
    s = torch.rand(100000, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2.0 ** -126
    s32 = s.float()
    assert bool((s32 > 0).any()) and F64.half_ulp_bf16(torch.tensor([2.0 ** -126, 2.0 ** -130, 2.0 ** -140], dtype=torch.float64)).tolist() == [2.0 ** -134] * 3
    err = (s32.to(torch.bfloat16).double() - s32.double()).abs()
    assert (err <= F64.half_ulp_bf16(s32)).all()
    assert (err > torch.ldexp(torch.ones_like(s), torch.frexp(s32.double()).exponent - 9)).any()


def test_accepts_the_exact_answer_rounded_and_torch_fp32(case):
    x, w, dy, ref = case
    F64.check_bf16(_bf16(ref.y), ref.y, ref.ay, name="bf16(ref) y")
    F64.check_bf16(_bf16(ref.dx), ref.dx, ref.adx, name="bf16(ref) dx")
    xf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
    y32 = F.conv2d(xf, wf, padding=1)
    y32.backward(dy.float())
    F64.check_bf16(y32.detach(), ref.y, ref.ay, name="torch fp32 y")
    F64.check_bf16(_bf16(y32.detach()), ref.y, ref.ay, name="bf16(torch fp32) y")
    F64.check_bf16(xf.grad, ref.dx, ref.adx, name="torch fp32 dx")
    F64.check_dw(wf.grad, ref.dw, ref.adw, name="torch fp32 dw")
    F64.check_dw(ref.dw.float(), ref.dw, ref.adw, name="fp32(ref) dw")


def _mutations(x, w, ref):
    """(name, mutated bf16 output y) pairs, each a copy of bf16(ref.y) with one defect"""
    base = _pix(_bf16(ref.y))
    M = base.shape[0]
    ntile = M // TILE
    out = []

    m = base.clone()
    m[(ntile - 1) * TILE:ntile * TILE] = 0
    out.append(("last tile zeroed", m))
    m = base.clone()
    m[TILE:2 * TILE] = 0
    out.append(("tile spanning images zeroed", m))
    m = base.clone()
    m[2 * TILE:3 * TILE] = base[3 * TILE:4 * TILE]
    out.append(("tile holds its neighbour's output", m))
    # one 64-channel K slice (input channels 64..127) missing from one tile
    part = _pix(F.conv2d(x[:, 64:128], w[:, 64:128], padding=1))
    m = base.clone()
    m[4 * TILE:5 * TILE] = _bf16(_pix(ref.y)[4 * TILE:5 * TILE] - part[4 * TILE:5 * TILE])
    out.append(("K slice missing from one tile", m))
    # image 5's top output row read the last row of image 4 instead of the zero padding above it
    n = 5
    xin = torch.cat([x[n - 1:n, :, H - 1:H], x[n:n + 1]], dim=2)           # [1, Cin, H + 1, W]: real row above
    ytop = F.conv2d(xin, w, padding=(0, 1))[:, :, 0]                      # output row 0 of image n
    yt = ref.y.clone()
    yt[n, :, 0] = ytop[0]
    out.append(("image-border row from the neighbouring image", _pix(_bf16(yt))))
    # one element off by 4 bf16 ulps (an element of median magnitude)
    flat = _bf16(ref.y).reshape(-1)
    k = int(torch.argsort(flat.abs())[flat.numel() // 2])
    b16 = flat.to(torch.bfloat16).clone()
    iv = b16.view(torch.int16)
    iv[k] += 4
    out.append(("one element off by 4 ulps", _pix(b16.double().view(ref.y.shape))))
    return out


def test_rejects_each_tile_defect(case):
    x, w, dy, ref = case
    for name, m in _mutations(x, w, ref):
        r = F64.bf16_ratio(_unpix(m, ref.y), ref.y, ref.ay, name=name)
        print(r)
        assert r.ratio > 1.0, "checker accepted: " + name


def test_rejects_an_input_gradient_defect(case):
    x, w, dy, ref = case
    base = _pix(_bf16(ref.dx))
    m = base.clone()
    m[TILE:2 * TILE] = base[2 * TILE:3 * TILE]
    assert _rejects(_unpix(m, ref.dx), ref.dx, ref.adx)
    m = base.clone()
    m[-TILE:] = 0
    assert _rejects(_unpix(m, ref.dx), ref.dx, ref.adx)


def _dw_of_pixels(x, dy, lo, hi):
    """weight gradient contributed by output pixels [lo, hi) (channels-last order)"""
    mask = torch.zeros(dy.shape[0] * dy.shape[2] * dy.shape[3], dtype=torch.float64)
    mask[lo:hi] = 1
    dym = dy * mask.view(dy.shape[0], dy.shape[2], dy.shape[3]).unsqueeze(1)
    wr = torch.zeros(COUT, CIN, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wr, padding=1).backward(dym)
    return wr.grad


def test_rejects_weight_gradient_defects(case):
    x, w, dy, ref = case
    M = N * H * W
    base = ref.dw.float()
    missing = base - _dw_of_pixels(x, dy, 3 * TILE, 4 * TILE).float()
    r = F64.dw_ratio(missing, ref.dw, ref.adw, name="dw: one tile missing")
    print(r, r.rel_l2)
    assert not r.ok and r.rel_l2 > F64.DW_REL_L2
    twice = base + _dw_of_pixels(x, dy, M // 4, M // 2).float()       # split-K chunk 2 of 4 added twice
    r = F64.dw_ratio(twice, ref.dw, ref.adw, name="dw: split-K chunk twice")
    print(r, r.rel_l2)
    assert not r.ok and r.rel_l2 > F64.DW_REL_L2
    # and one chunk of eight: the per-element bound alone catches it
    r = F64.dw_ratio(base + _dw_of_pixels(x, dy, 0, M // 8).float(), ref.dw, ref.adw)
    assert not r.ok


def test_statistics_and_reduction_sums():
    g = torch.Generator().manual_seed(3)
    x = _bf16(torch.randn(4, 64, 8, 8, generator=g).relu())
    w = _bf16(torch.randn(64, 64, 3, 3, generator=g) * 0.05)
    ref = F64.conv_ref64(x, w, None)
    y = ref.y.float()
    rows = torch.stack([_pix(y).view(-1, 64, 64).sum(1), (_pix(y) ** 2).view(-1, 64, 64).sum(1)], 1)   # [4][2][64]
    F64.check_stats(rows, ref)
    bad = rows.clone()
    bad[1] = 0                                    # one workgroup's row lost
    with pytest.raises(AssertionError):
        F64.check_stats(bad, ref)
    # BatchNorm-backward reduction rows
    d = _bf16(torch.randn(4, 64, 8, 8, generator=g))
    coef = torch.stack([torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1,
                        torch.ones(64)])
    yb = _bf16(torch.randn(4, 64, 8, 8, generator=g))
    (s1, s2), _, _ = F64.bnred_ref(d, yb, coef)
    rows = torch.stack([s1, s2]).unsqueeze(0).float()
    F64.check_bnred(rows, d, yb, coef)
    rows[0, 1, 7] += 0.01 * float(s2.abs().max())
    with pytest.raises(AssertionError):
        F64.check_bnred(rows, d, yb, coef)


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm and pooling checkers: the "kernel output" is torch's own fp32 (or bf16-stored) evaluation of the same formulas.
# It passes every bound; each defect below fails.
# ----------------------------------------------------------------------------------------------------------------------
def _bn_emulate(d, bf16, rows, rps=None, mask="y", eps=1e-5):
    """the passes in torch fp32: statistics rows (the M pixel rows split into `rows` chunks), finalize (rows summed in double
    as the kernels do), apply, backward.  Returns a dict of what the kernels would store."""
    y, dout = d["y"], d["dout"]
    M, C = y.shape
    o = dict(M=M, C=C)
    o["rows"] = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in y.chunk(rows)])              # [rows][2][C] fp32
    s1, s2 = o["rows"][:, 0].double().sum(0), o["rows"][:, 1].double().sum(0)
    mean, var = s1 / M, (s2 / M - (s1 / M) ** 2).clamp_min(0)
    inv = (1.0 / (var + F64.f32(eps)).sqrt()).float()
    sc = d["gamma"] * inv
    o["coef"] = torch.stack([sc, d["beta"] - mean.float() * sc, mean.float(), inv])
    unb = var * M / (M - 1) if M > 1 else var
    o["rm"] = (1 - 0.1) * torch.zeros(C) + torch.tensor(0.1) * mean.float()
    o["rv"] = (1 - 0.1) * torch.ones(C) + torch.tensor(0.1) * unb.float()
    gate = F64.per_row(d["gate"], rps, M).float() if rps else None
    addc = F64.per_row(d["addc"], rps, M).float() if rps else None
    o["gate"], o["addc"] = gate, addc
    z = y * o["coef"][0] + o["coef"][1]
    out = (z * gate if rps else z) + (d["res"] * d["rscale"] + d["rshift"])
    o["out"] = F64._b(out.clamp_min(0), bf16)
    m = (z > 0) if mask == "y" else (mask > 0)
    o["masked"] = torch.where(m, dout, torch.zeros_like(dout))
    dz = o["masked"] * gate + addc if rps else o["masked"]
    xh = (y - o["coef"][2]) * o["coef"][3]
    o["dbeta"], o["dgamma"] = dz.sum(0), (dz * xh).sum(0)
    k1, k2, k3 = d["gamma"] * o["coef"][3], o["dbeta"] / M, o["dgamma"] / M
    o["dz"], o["xh"], o["k"] = dz, xh, (k1, k2, k3)
    o["dy_unrounded"] = k1 * (dz - k2 - xh * k3)
    o["dy"] = F64._b(o["dy_unrounded"], bf16)
    o["dbias"] = o["dy"].sum(0)
    return o


def _bwd_ratios(d, o, bf16, rps, **over):
    g = dict(dgamma=o["dgamma"], dbeta=o["dbeta"], dy=o["dy"], dz_out=o["masked"], dbias=o["dbias"])
    g.update(over)
    K = F64.chain_len(o["M"], 1, o["C"], 8 if bf16 else 4, 1024)
    return F64.check_bn_bwd(d["dout"], d["y"], o["coef"], d["gamma"], bf16, K, g["dgamma"], g["dbeta"], g["dy"], g["dz_out"],
                            g["dbias"], K, maskref="y", gate=o["gate"] if rps else None, addc=o["addc"] if rps else None)


BN_CPU = [(777, 16, False, None, 2), (626, 64, True, 313, 5), (626, 64, False, 313, 5), (1, 64, False, None, 1)]


@pytest.mark.parametrize("M,C,bf16,rps,rows", BN_CPU)
def test_bn_pool_checkers_accept_torch_fp32(M, C, bf16, rps, rows):
    d = F64.bn_inputs(M, C, bf16, rps)
    o = _bn_emulate(d, bf16, rows, rps)
    vec = 8 if bf16 else 4
    F64.check_colstats(o["rows"], d["y"], F64.chain_len(M, rows, C, vec, 256))
    s1, s2 = o["rows"][:, 0].double().sum(0), o["rows"][:, 1].double().sum(0)
    ref = F64.coef_ref(s1, s2, M, d["gamma"], d["beta"], 1e-5, torch.zeros(C), torch.ones(C), 0.1)
    F64.check_coef(o["coef"], ref, o["rm"], o["rv"])
    want, A = F64.bn_act_ref(d["y"], o["coef"][0], o["coef"][1], d["res"], d["rscale"], d["rshift"], o["gate"] if rps else None, True)
    F64.check_stored(o["out"], want, A, F64.K_ACT, bf16, "bn_act")
    _bwd_ratios(d, o, bf16, rps)
    if M > 1 and not bf16:
        # F.batch_norm itself (its own summation order), against the bound carried from the statistics' sum bounds
        (t1, t2), (m1, m2) = F64.colstats_ref(d["y"])
        K = F64.chain_len(M, rows, C, vec, 256)
        ref = F64.coef_ref(t1, t2, M, d["gamma"], d["beta"], 1e-5, torch.zeros(C), torch.ones(C), 0.1,
                           F64.g_k(K) * m1, F64.g_k(K + 1) * m2)
        rm, rv = torch.zeros(C), torch.ones(C)
        x4 = d["y"].t().reshape(1, C, M, 1)
        bn = F.batch_norm(x4, rm, rv, d["gamma"], d["beta"], True, 0.1, 1e-5)
        inv = 1.0 / (x4.var(dim=(0, 2, 3), unbiased=False) + 1e-5).sqrt()
        sc = d["gamma"] * inv
        F64.check_coef(torch.stack([sc, d["beta"] - rm / 0.1 * sc, rm / 0.1, inv]), ref, rm, rv, name="F.batch_norm coef")


def test_unsure_share_of_every_input_family_is_under_the_cap():
    """the float64 reference alone: |bn(y)| inside K_AFFINE roundings of zero for at most UNSURE_CAP of the elements.
    (Every family a ReLU mask is recomputed on.  The large-mean sweep, ratios 1 .. 32768, is measured through col_stats and
    bn_finalize only: no mask is taken there, and at |mean| / std in the thousands y * scale + shift cancels so far that
    5e-4 of its elements would be unsure.)"""
    def share(y, sc, sh):
        return F64.check_unsure(F64.affine_mask(y, sc, sh)[1], "inputs")
    for M, C, bf16, ratios in [(1, 64, 0, None), (1, 64, 1, None), (7, 4, 0, None), (7, 8, 1, None), (777, 16, 0, None), (777, 16, 1, None), (626, 64, 0, None),
                               (626, 64, 1, None), (4099, 128, 0, None), (4099, 128, 1, None), (300, 1024, 1, None),
                               (20000, 512, 0, None), (40000, 512, 1, None), (4099, 64, 0, (0, 4, 32, 256))]:
        d = F64.bn_inputs(M, C, bool(bf16), None, ratios)
        (s1, s2), _ = F64.colstats_ref(d["y"])
        v = F64.coef_ref(s1, s2, M, d["gamma"], d["beta"], 1e-5).val
        print((M, C, bf16), share(d["y"], v["scale"].float(), v["shift"].float()))
    for shape in [(2, 64, 1, 1), (1, 64, 2, 2), (3, 64, 1, 41), (2, 64, 7, 1), (2, 64, 9, 7), (1, 128, 12, 10), (2, 64, 364, 364)]:
        for bf16 in ((False, True) if shape[2] < 300 else (False,)):
            p = F64.pool_inputs(shape[0], shape[1], shape[2], shape[3], bf16)
            print(shape, bf16, share(p["y"].reshape(-1, shape[1]), p["scale"], p["shift"]))


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_rejects_each_batchnorm_forward_defect():
    M, C, rows, rps = 626, 64, 5, 313
    d = F64.bn_inputs(M, C, False, rps)
    o = _bn_emulate(d, False, rows, rps)
    K = F64.chain_len(M, rows, C, 4, 256)
    y = d["y"]
    # 1. one pixel row missing from the statistics
    short = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in y[:-1].chunk(rows)])
    assert _fails(lambda: F64.check_colstats(short, y, K))
    # 2. one partial row counted twice
    assert _fails(lambda: F64.check_colstats(torch.cat([o["rows"], o["rows"][1:2]]), y, K))
    s1, s2 = o["rows"][:, 0].double().sum(0), o["rows"][:, 1].double().sum(0)
    ref = F64.coef_ref(s1, s2, M, d["gamma"], d["beta"], 1e-5, torch.zeros(C), torch.ones(C), 0.1)
    assert F64.coef_ratio(o["coef"], ref, o["rm"], o["rv"]).ok
    # 3. eps left out of invstd
    var = (s2 / M - (s1 / M) ** 2)
    c = o["coef"].clone()
    c[3] = (1.0 / var.sqrt()).float()
    r = F64.coef_ratio(c, ref)
    assert not r.ok and r.where[0] == "invstd", r
    # 4. biased variance written to running_var
    r = F64.coef_ratio(o["coef"], ref, o["rm"], 0.9 * torch.ones(C) + 0.1 * var.float())
    assert not r.ok and r.where[0] == "rv", r
    # 5. mean off by one bf16 ulp
    c = o["coef"].clone()
    c[2] += (2 * F64.half_ulp_bf16(c[2])).float()
    r = F64.coef_ratio(c, ref)
    assert not r.ok and r.where[0] == "mean", r
    # 6. the neighbouring sample's gate on the last row of a sample (a row -> sample division off by one), rows_per_sample = 313
    for bf16 in (False, True):
        db = F64.bn_inputs(M, C, bf16, rps)
        ob = _bn_emulate(db, bf16, rows, rps)
        want, A = F64.bn_act_ref(db["y"], ob["coef"][0], ob["coef"][1], db["res"], db["rscale"], db["rshift"], ob["gate"], True)
        assert F64.stored_ratio(ob["out"], want, A, F64.K_ACT, bf16).ok
        z = db["y"][312] * ob["coef"][0] + ob["coef"][1]
        bad = ob["out"].clone()
        bad[312] = F64._b((z * db["gate"][1] + (db["res"][312] * db["rscale"] + db["rshift"])).clamp_min(0), bf16)
        r = F64.stored_ratio(bad, want, A, F64.K_ACT, bf16)
        assert not r.ok and r.where[0] == 312, r


@pytest.mark.parametrize("bf16", [False, True])
def test_rejects_each_batchnorm_backward_defect(bf16):
    M, C, rows, rps = 626, 64, 5, 313
    d = F64.bn_inputs(M, C, bf16, rps)
    o = _bn_emulate(d, bf16, rows, rps)
    assert max(_bwd_ratios(d, o, bf16, rps).values()) <= 1.0
    k1, k2, k3 = o["k"]
    # 6. (backward) the neighbouring sample's gate and additive term on the last row of sample 0
    dz = o["dz"].clone()
    dz[312] = o["masked"][312] * d["gate"][1] + d["addc"][1]
    assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dy=F64._b(k1 * (dz - k2 - o["xh"] * k3), bf16)))
    # 7. one ReLU mask bit flipped on an element that is clearly non-zero
    z = d["y"] * o["coef"][0] + o["coef"][1]
    i = int(torch.argmax((z.abs() * d["dout"].abs()).reshape(-1)))
    r_, c_ = i // C, i % C
    flip = o["masked"].clone()
    flip[r_, c_] = d["dout"][r_, c_] - flip[r_, c_]
    dzf = flip * o["gate"] + o["addc"]
    assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dz_out=flip))
    assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dy=F64._b(k1 * (dzf - k2 - o["xh"] * k3), bf16), dz_out=None))
    assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dbeta=dzf.sum(0), dgamma=(dzf * o["xh"]).sum(0), dy=None, dz_out=None, dbias=None))
    # 8. k3 applied without xhat
    assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dy=F64._b(k1 * (o["dz"] - k2 - k3), bf16), dbias=None))
    if bf16:
        # 9. dy wrong by 4 ulp (an element of median magnitude).  Of the stored bf16 type only: 4 fp32 ulps are 8 u |ref|, and
        # the derived fp32 bound, u |ref| + 2 g_5 A with A >= |ref|, is 11 u |ref| at the least -- the per-element bound cannot
        # resolve a few fp32 ulps, and no constant is tightened to make it (the fp32 dy is pinned by mutations 6 - 8 instead)
        flat = o["dy"].reshape(-1)
        k = int(torch.argsort(flat.abs())[flat.numel() // 2])
        b16 = flat.to(torch.bfloat16).clone()
        b16.view(torch.int16)[k] += 4
        assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dy=b16.float().view(M, C), dbias=None))
        # 10. dbias summed from the unrounded dy instead of the stored dy
        assert _fails(lambda: _bwd_ratios(d, o, bf16, rps, dbias=o["dy_unrounded"].sum(0)))


def _pool_emulate(p, bf16):
    """torch's own pooling of the stored-precision activations: pooled, idx (earliest tap on ties), dz"""
    a = F64._b((p["y"] * p["scale"] + p["shift"]).clamp_min(0), bf16)
    T = F64.pool_taps(a.double(), float("-inf"))
    pooled = T.amax(3)
    idx = (T == pooled.unsqueeze(3)).double().argmax(3).to(torch.uint8)
    N, H, W, C = a.shape
    dz, _ = F64.pool_bwd_ref(p["dp"], pooled, idx, H, W)
    return pooled.float(), idx, F64._b(dz.float(), bf16)


POOL_CPU = [(2, 64, 1, 1), (1, 64, 2, 2), (3, 64, 1, 41), (2, 64, 7, 1), (2, 64, 9, 7), (1, 128, 12, 10)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", POOL_CPU)
def test_pool_checkers_accept_torch(shape, bf16):
    N, C, H, W = shape
    p = F64.pool_inputs(N, C, H, W, bf16)
    pooled, idx, dz = _pool_emulate(p, bf16)
    r = F64.check_pool_fwd(pooled, idx, p["y"], p["scale"], p["shift"], bf16)
    assert r.ties > 0 or H * W == 1                     # all-zero windows: exact ties (a 1x1 image has one tap)
    F64.check_pool_bwd(dz, p["dp"], pooled, idx, bf16)


def test_pool_checker_accepts_taps_that_tie_after_bf16_rounding():
    """Behind a small BatchNorm scale several bf16 conv outputs land in one bf16 cell of the activation: torch's pooling of
    the stored bf16 activation then names the earliest of them, whose float64 value is up to one bf16 ulp below the largest.
    The checker accepts that (tap ratio above 1 of the stored bound, within the doubled tap bound) and still rejects a tap
    two ulps below the maximum and the later of two taps that tie exactly."""
    N, C, H, W = 2, 64, 9, 7
    p = F64.pool_inputs(N, C, H, W, True)
    p["scale"], p["shift"] = 0.11 * p["scale"], 1.0 + 0.05 * p["shift"]
    pooled, idx, _ = _pool_emulate(p, True)
    r = F64.check_pool_fwd(pooled, idx, p["y"], p["scale"], p["shift"], True)
    assert 0.5 < r.parts["tap"] <= 1.0 and r.parts["value"] <= 1.0, r.parts      # beyond the stored bound, within two of them
    a = (p["y"].double() * p["scale"].double() + p["shift"].double()).clamp_min(0)
    T = F64.pool_taps(a, float("-inf"))
    mx = T.amax(3, keepdim=True)
    low = torch.isfinite(T) & (mx - T > 4 * F64.half_ulp_bf16(mx)) & (mx - T < 8 * F64.half_ulp_bf16(mx))
    assert low.any()
    n_, oh, ow, t, c_ = (int(v) for v in low.nonzero()[0])
    bad = idx.clone()
    bad[n_, oh, ow, c_] = t
    r = F64.pool_fwd_ratio(pooled, bad, p["y"], p["scale"], p["shift"], True)
    assert not r.ok and r.parts["tap"] > 2.0, r.parts


@pytest.mark.parametrize("bf16", [False, True])
def test_rejects_each_pooling_defect(bf16):
    N, C, H, W = 2, 64, 9, 7
    p = F64.pool_inputs(N, C, H, W, bf16)
    pooled, idx, dz = _pool_emulate(p, bf16)
    fwd = lambda pl, ix: F64.pool_fwd_ratio(pl, ix, p["y"], p["scale"], p["shift"], bf16)
    assert fwd(pooled, idx).ok
    # 11. arg-max on the later of two tied taps: an interior all-zero window (taps 0 and 1 tie at 0) naming tap 1
    a = (p["y"].double() * p["scale"].double() + p["shift"].double()).clamp_min(0)
    T = F64.pool_taps(a, float("-inf"))
    zero = (T.amax(3) == 0) & torch.isfinite(T[:, :, :, 0]) & torch.isfinite(T[:, :, :, 1])
    assert zero.any()
    w = tuple(int(v) for v in zero.nonzero()[0])
    bad = idx.clone()
    bad[w] = 1
    r = fwd(pooled, bad)
    assert not r.ok and r.parts["late_ties"] == 1 and r.parts["value"] <= 1 and r.parts["tap"] <= 1, r.parts
    # ... and on a border window whose first taps lie outside the image: the earliest is the first tap inside
    assert int(idx[0, 0, 0].min()) >= 4
    bad = idx.clone()
    bad[0, 0, 0] = 0
    assert not fwd(pooled, bad).ok
    # 13. the last window row dropped (H = 9 is odd: window row 4 covers input rows 7, 8)
    bad = pooled.clone()
    bad[:, -1] = 0
    r = fwd(bad, idx)
    assert not r.ok and r.where[1] == pooled.shape[1] - 1, r
    # 12. a window's gradient routed to the same tap of the neighbouring window
    assert F64.pool_bwd_ratio(dz, p["dp"], pooled, idx, bf16).ok
    live = (pooled[:, 1:-1, 1:-1] > 0).nonzero()[0]
    n_, oh, ow, c_ = int(live[0]), int(live[1]) + 1, int(live[2]) + 1, int(live[3])
    t = int(idx[n_, oh, ow, c_])
    h, w_ = 2 * oh - 1 + t // 3, 2 * ow - 1 + t % 3
    bad = dz.clone()
    g = p["dp"][n_, oh, ow, c_]
    bad[n_, h, w_, c_] -= g
    bad[n_, h, w_ + 2, c_] += g
    assert not F64.pool_bwd_ratio(F64._b(bad, bf16), p["dp"], pooled, idx, bf16).ok


@pytest.mark.parametrize("bf16", [False, True])
def test_eval_backward_checker_accepts_torch_fp32(bf16):
    """ecgmm_bn_eval_bwd's formulas in torch fp32 (dy stored as fp32 / bf16), gated with rows_per_sample = 313, against
    bn_eval_dy_ref / K_EVAL_DY and the sum bounds; the scale left out of dy, or the dy sum taken unrounded, is rejected"""
    M, C, rows, rps = 626, 64, 5, 313
    d = F64.bn_inputs(M, C, bf16, rps)
    o = _bn_emulate(d, bf16, rows, rps)
    coef = o["coef"]
    dz32, xh32 = o["dz"], o["xh"]                                  # masked dout * gate + addc, (y - mean) * invstd: fp32
    dy = F64._b(dz32 * coef[0], bf16)
    K = F64.chain_len(M, rows, C, 8 if bf16 else 4, 256)
    mask, unsure = F64.affine_mask(d["y"], coef[0], coef[1])
    F64.check_unsure(unsure, "eval bwd")
    dz, A, masked = F64.bn_dz_ref(d["dout"], mask, o["gate"], o["addc"])
    assert not bool(((o["masked"].double() != masked) & ~unsure).any())
    xh = F64.xhat_ref(d["y"], coef)
    sums, slack, mags = F64.bn_bwd_sums_ref(dz, A, xh, unsure, d["dout"].double() * o["gate"].double())
    F64.check_sum(dz32.sum(0), sums[0], mags[0], F64.K_DZ + K + 1, "eval dbeta", slack[0])
    F64.check_sum((dz32 * xh32).sum(0), sums[1], mags[1], F64.K_DZXHAT + K + 1, "eval dgamma", slack[1])
    want, Ady = F64.bn_eval_dy_ref(dz, A, coef[0])
    F64.check_stored(dy, want, Ady, F64.K_EVAL_DY, bf16, "eval dy", skip=unsure)
    F64.check_sum(dy.sum(0), dy.double().sum(0), dy.double().abs().sum(0), K + 1, "eval dbias")
    assert not F64.stored_ratio(F64._b(dz32, bf16), want, Ady, F64.K_EVAL_DY, bf16, skip=unsure).ok            # dy without the scale
    bad = dy.clone()
    bad[312] = F64._b((o["masked"][312] * d["gate"][1] + d["addc"][1]) * coef[0], bf16)                      # the next sample's gate
    r = F64.stored_ratio(bad, want, Ady, F64.K_EVAL_DY, bf16, skip=unsure)
    assert not r.ok and r.where[0] == 312, r
    if bf16:
        assert _fails(lambda: F64.check_sum((dz32 * coef[0]).sum(0), dy.double().sum(0), dy.double().abs().sum(0), K + 1, "dbias"))


def _stem_bwd_emulate(p, pooled, idx, bf16):
    """ecgmm_pool_bn_bwd in torch fp32, in the kernels' own form: the reduction over windows of g = dp * [pooled > 0] and
    g * (pooled - beta) with beta = shift + mean * scale, scaled by 1 / scale after the sum and by invstd in the finalize;
    dy = k1 * z + (bn * y + an) with bn = -(k1 * k3) * invstd, an = -(k1 * k2) - bn * mean, z the fp32 sum of the routed terms"""
    sc, sh, mu, inv = p["scale"], p["shift"], p["mean"], p["invstd"]
    N, H, W, C = p["y"].shape
    M = N * H * W
    g = torch.where(pooled > 0, p["dp"], torch.zeros_like(p["dp"]))
    beta = sh + mu * sc
    rsc = torch.where(sc != 0, 1.0 / sc, torch.zeros_like(sc))
    dbeta = g.sum((0, 1, 2))
    dgamma = ((g * (pooled - beta)).sum((0, 1, 2)) * rsc * inv)
    k1, k2, k3 = p["gamma"] * inv, dbeta / M, dgamma / M
    bn = -(k1 * k3) * inv
    an = -(k1 * k2) - bn * mu
    z = F64.pool_bwd_ref(p["dp"], pooled, idx, H, W)[0].float()
    unrounded = k1 * z + (bn * p["y"] + an)
    dy = F64._b(unrounded, bf16)
    return dict(dbeta=dbeta, dgamma=dgamma, dy=dy, dbias=dy.sum((0, 1, 2)), k=(k1, bn, an), z=z, M=M, unrounded=unrounded)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", [(2, 64, 9, 7), (1, 128, 12, 10), (3, 64, 1, 41)])
def test_fused_stem_backward_checker_accepts_torch_fp32(shape, bf16):
    """pool_red_ref / K_POOL_RED and pool_dy_ref / K_POOL_DY accept the torch fp32 evaluation of the fused stem backward (dy
    stored as fp32 / bf16), stage by stage through its own stored dbeta / dgamma; they reject the shift left out of beta, the
    mean term left out of `an`, and a window's gradient at the neighbouring pixel"""
    N, C, H, W = shape
    vec = 8 if bf16 else 4
    p = F64.pool_inputs(N, C, H, W, bf16)
    pooled, idx, _ = _pool_emulate(p, bf16)
    e = _stem_bwd_emulate(p, pooled, idx, bf16)
    coef = torch.stack([p["scale"], p["shift"], p["mean"], p["invstd"]])
    MP = pooled.numel() // C
    K = F64.chain_len(MP, 1, C, vec, 1024)
    (s1, s2), (m1, m2) = F64.pool_red_ref(p["dp"], pooled, coef)
    F64.check_sum(e["dbeta"], s1, m1, K + 1, "stem dbeta")
    F64.check_sum(e["dgamma"], s2, m2, F64.K_POOL_RED + K + 1, "stem dgamma")
    dz64, mag = F64.pool_bwd_ref(p["dp"], pooled, idx, H, W)
    k1 = p["gamma"].double() * p["invstd"].double()

    def dy_ratio(dy):
        want, A = F64.pool_dy_ref(dz64, mag, p["y"], coef, k1, e["dbeta"].double() / e["M"], e["dgamma"].double() / e["M"])
        return F64.stored_ratio(dy, want, A, F64.K_POOL_DY, bf16, "stem dy")
    r = dy_ratio(e["dy"])
    print(r)
    assert r.ok, r
    s = e["dy"].double().reshape(-1, C)
    Kb = 4 * (e["M"] // 4 + 1) + 1
    F64.check_sum(e["dbias"], s.sum(0), s.abs().sum(0), Kb, "stem dbias")
    # defects
    g = torch.where(pooled > 0, p["dp"], torch.zeros_like(p["dp"]))
    rsc = 1.0 / p["scale"]
    noshift = (g * (pooled - p["mean"] * p["scale"])).sum((0, 1, 2)) * rsc * p["invstd"]
    assert _fails(lambda: F64.check_sum(noshift, s2, m2, F64.K_POOL_RED + K + 1, "stem dgamma"))
    k1f, bn, an = e["k"]
    assert not dy_ratio(F64._b(k1f * e["z"] + (bn * p["y"] + (an + bn * p["mean"])), bf16)).ok
    zs = torch.roll(e["z"], 1, dims=2)
    assert not dy_ratio(F64._b(k1f * zs + (bn * p["y"] + an), bf16)).ok
    if bf16:
        u = e["unrounded"].double().reshape(-1, C)
        assert _fails(lambda: F64.check_sum(u.sum(0).float(), s.sum(0), s.abs().sum(0), Kb, "stem dbias"))


# ----------------------------------------------------------------------------------------------------------------------
# The dense tails: the dot-product bound, the per-stage SE MLP check and the chain bar accept torch's fp32 and reject each
# defect of the launch geometry they are there for.
# ----------------------------------------------------------------------------------------------------------------------
ACTS = {"none": lambda z: z, "relu": torch.relu, "sigmoid": torch.sigmoid}


def _linear_fp32(B, In, Out, act="none"):
    x, w, b, dz = F64.linear_inputs(B, In, Out)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    z = F.linear(xr, wr, br)
    z.backward(dz)
    return (x, w, b, dz), dict(y=ACTS[act](z.detach()), dx=xr.grad, dw=wr.grad, db=br.grad)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", F64.LINEAR_CASES)
def test_dot_checker_accepts_torch_fp32_linear(shape, act):
    (x, w, b, dz), got = _linear_fp32(*shape, act)
    ref = F64.linear_ref(x, w, b, dz, act)
    for k, (r, A, K, sig) in ref.items():
        F64.check_dot(got[k], r, A, K, "%s %s %s" % (shape, act, k), sigmoid=sig)
    # and without a bias
    r, A, K, sig = F64.linear_ref(x, w, None, None, act)["y"]
    F64.check_dot(ACTS[act](F.linear(x, w)), r, A, K, "%s %s y, no bias" % (shape, act), sigmoid=sig)


def _se_fp32(N, C, CR, rows=None):
    """the SE MLP stage by stage in torch fp32; rows: the batch rows the weight gradients sum over (None = all)"""
    d = F64.se_inputs(N, C, CR)
    m, w1, b1, w2, b2, dg = (d[k] for k in ("m", "w1", "b1", "w2", "b2", "dg"))
    o = {"h": torch.relu(m @ w1.t() + b1)}
    o["g"] = torch.sigmoid(o["h"] @ w2.t() + b2)
    o["ds"] = dg * o["g"] * (1 - o["g"])
    o["dh"] = (o["ds"] @ w2) * (o["h"] > 0).float()
    o["dm"] = (o["dh"] @ w1) * torch.tensor(F64.SE_SCALE, dtype=torch.float32)
    r = slice(None) if rows is None else rows
    o["dw2"], o["db2"] = o["ds"][r].t() @ o["h"][r], o["ds"][r].sum(0)
    o["dw1"], o["db1"] = o["dh"][r].t() @ m[r], o["dh"][r].sum(0)
    st = F64.se_mlp_stages(m, w1, b1, w2, b2, o["h"], o["g"], dg, o["ds"], o["dh"], F64.SE_SCALE)
    return st, o


@pytest.mark.parametrize("shape", F64.SE_CASES)
def test_se_mlp_checker_accepts_an_fp32_restatement(shape):
    st, o = _se_fp32(*shape)
    assert set(st) == {"h", "g", "ds", "dh", "dm", "dw1", "db1", "dw2", "db2"}
    F64.check_se_mlp(st, o, "se_mlp %s" % (shape,))


def test_dot_bound_demands_exactness_where_nothing_is_summed():
    z = torch.zeros(3, 4)
    assert F64.dot_ratio(z, z, z, 16).ok
    assert not F64.dot_ratio(z + 1e-30, z, z, 16).ok
    assert not F64.dot_ratio(z + float("nan"), z, z + 1, 16).ok


@pytest.mark.parametrize("shape", [(272, 672, 128), (48, 80, 16), (16, 16, 16)])
def test_dot_checker_rejects_each_tile_defect_of_a_linear(shape):
    """one 16x16 output tile of y, dx and dw, each with: one 4-wide k group dropped, one counted twice, the neighbour tile's
    values, and (y) the bias missing on one column.  At (16, 16, 16) every output is a single tile and has no neighbour:
    there the tile holds its rows displaced by one 4-row MFMA block, the nearest displacement the kernel's indexing has."""
    B, In, Out = shape
    (x, w, b, dz), got = _linear_fp32(B, In, Out)
    ref = F64.linear_ref(x, w, b, dz)
    # (left operand rows, right operand rows, reduction axis): out[i][j] = sum_k Lop[i][k] * Rop[j][k]
    ops = {"y": (x, w), "dx": (dz, w.t().contiguous()), "dw": (dz.t().contiguous(), x.t().contiguous())}
    for k, (lo, ro) in ops.items():
        r, A, K, _ = ref[k]
        M, N = r.shape
        assert K == lo.shape[1] and F64.dot_ratio(got[k], r, A, K).ok
        m0, n0, k0 = M - 16, N - 16, 4 * ((K // 4) // 2)
        group = lo[m0:m0 + 16, k0:k0 + 4] @ ro[n0:n0 + 16, k0:k0 + 4].t()
        for sign, what in ((-1, "dropped"), (1, "counted twice")):
            bad = got[k].clone()
            bad[m0:m0 + 16, n0:n0 + 16] += sign * group
            rep = F64.dot_ratio(bad, r, A, K)
            assert not rep.ok and m0 <= rep.where[0] < m0 + 16 and n0 <= rep.where[1] < n0 + 16, (k, what, rep)
        bad = got[k].clone()
        if m0 >= 16:
            bad[m0:m0 + 16, n0:n0 + 16] = got[k][m0 - 16:m0, n0:n0 + 16]
        elif n0 >= 16:
            bad[m0:m0 + 16, n0:n0 + 16] = got[k][m0:m0 + 16, n0 - 16:n0]
        else:
            bad[m0:m0 + 16, n0:n0 + 16] = torch.roll(got[k][m0:m0 + 16, n0:n0 + 16], 4, 0)
        assert not F64.dot_ratio(bad, r, A, K).ok, (k, "neighbour tile")
    r, A, K, _ = ref["y"]
    col = Out - 16 + int(b[Out - 16:].abs().argmax())
    bad = got["y"].clone()
    bad[B - 16:, col] -= b[col]
    rep = F64.dot_ratio(bad, r, A, K)
    assert not rep.ok and rep.where[1] == col, rep


@pytest.mark.parametrize("C,CR", [(64, 4), (128, 8)])
def test_se_mlp_checker_rejects_weight_gradient_defects(C, CR):
    """se_mlp_bwd_weights_kernel at N = 67: batch slice 15 (rows 15, 31, 47, 63) missing; the 4x-unrolled trip's rows
    (0..63: every slice makes one) missing, leaving only the tail loop's rows 64..66"""
    N = 67
    st, good = _se_fp32(N, C, CR)
    every = torch.arange(N)
    for what, rows in (("slice 15", every[every % 16 != 15]), ("unrolled trip", every[every >= 64])):
        _, bad = _se_fp32(N, C, CR, rows)
        for k in ("dw1", "db1", "dw2", "db2"):
            assert F64.se_stage_ratio(good[k], st[k], k).ok
            assert not F64.se_stage_ratio(bad[k], st[k], k).ok, (what, k)


def test_chain_bar_rejects_missing_rows_of_the_head_backward():
    """head_rows_bwd_kernel at B = 272 (64 blocks x 4 waves, rows 256..271 are a wave's second row): those rows missing from
    every parameter gradient; one wave's partial (rows 1 and 257) missing from the fold of the row kernel's gradients"""
    B, dims, hidden, nc = 272, (256, 256, 256), 128, 2
    head = F64.head_fill(F64.HeadRef(dims, hidden, nc))
    raws, lab = F64.head_inputs(B, dims, nc)
    ones = torch.ones(B)
    out64, draw64, g64 = F64.head_run(head, raws, lab, "all_heads", torch.float64)
    _, _, g64w = F64.head_run(head, raws, lab, "all_heads", torch.float64, ones)
    out32, draw32, g32 = F64.head_run(head, raws, lab, "all_heads", torch.float32)
    for a, b in zip(g64, g64w):     # the row-weighted loss with unit weights has the gradients of the loss itself
        assert F64.chain_figure(b, a) < 1e-12
    for a, r, o in zip(list(out32[:5]) + draw32 + g32, list(out64[:5]) + draw64 + g64, list(out32[:5]) + draw32 + g32):
        assert F64.chain_ratio(a, r, o).ratio <= 1 / F64.CHAIN_MARGIN + 1e-12
    second = ones.clone()
    second[256:] = 0
    _, _, bad = F64.head_run(head, raws, lab, "all_heads", torch.float32, second)
    for i, name in enumerate(F64.HeadRef.TABLE_NAMES):
        assert not F64.chain_ratio(bad[i], g64[i], g32[i], name).ok, name
    wave = ones.clone()
    wave[1] = wave[257] = 0
    _, _, bad = F64.head_run(head, raws, lab, "all_heads", torch.float32, wave)
    for i, name in enumerate(F64.HeadRef.TABLE_NAMES[:15]):
        assert not F64.chain_ratio(bad[i], g64[i], g32[i], name).ok, name


def test_chain_figure_demands_exactness_of_an_all_zero_tensor():
    z = torch.zeros(5)
    assert F64.chain_figure(z, z) == 0.0 and F64.chain_figure(z + 1e-30, z) == float("inf")
    assert F64.chain_figure(torch.tensor([1.0, float("nan")]), torch.ones(2)) == float("inf")


# ----------------------------------------------------------------------------------------------------------------------
# The LSTM checkers (f64check.py, "The LSTM recurrence")
# ----------------------------------------------------------------------------------------------------------------------
def _old_bar(a, ref):
    """the whole-tensor figure of tests/test_lstm_gpu.py (bar 2e-5)"""
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("case,use", F64.LSTM_CHAIN_CASES, ids=F64.LSTM_CHAIN_IDS)
def test_seq_chain_checker_accepts_torch_fp32_lstm(case, use):
    """torch's own fp32 run sits at 1 / CHAIN_MARGIN of its bar by construction; what this asserts from the float64 reference
    alone is that no slice of any tensor of any case is below LSTM_MIN_RMS, so that none needs skipping"""
    r64, r32 = F64.lstm_refs(case, use)
    w = F64.lstm_chain_check(r32, r64, r32, case[6], F64.LSTM_CHAIN_IDS[F64.LSTM_CHAIN_CASES.index((case, use))])
    assert w.ratio <= 1 / F64.CHAIN_MARGIN + 1e-12
    rms = min(F64.seq_chain_ratio(r32[k], r64[k], r32[k], F64.lstm_slice_dim(k, case[6])).min_rms for k in r64)
    print("smallest slice rms of the float64 reference: %.3g" % rms)
    assert rms >= F64.LSTM_MIN_RMS
    if use == ("h",):       # the decaying-gradient case: the smallest slice is dx[t = 0]
        _, dx_rms = F64.seq_slice_figures(r64["dx"], r64["dx"], 0)
        assert float(dx_rms[0]) == rms and 1e-15 < rms < 5e-15 and float(dx_rms[-1]) > 1e-3


@pytest.mark.parametrize("H", F64.LSTM_STEP_H)
def test_single_step_bound_accepts_torch_fp32_cell(H):
    worst = 0.0
    for B in F64.LSTM_STEP_B:
        for In in F64.LSTM_STEP_IN:
            for bi in (False, True):
                ins = F64.lstm_inputs(F64.lstm_step_case(B, In, H, bi))
                r = F64.lstm_step_check(F64.lstm_run(ins, torch.float32), ins, "torch fp32 H=%d B=%d In=%d D=%d" % (H, B, In, 1 + bi))
                worst = max(worst, r.ratio)
    ins = F64.lstm_inputs(F64.lstm_step_case(17, 24, 132, True), 3.0, 4.0)
    F64.lstm_step_check(F64.lstm_run(ins, torch.float32), ins, "torch fp32 saturated")
    assert worst <= 1.0


def test_single_step_bound_rejects_cell_defects():
    ins = F64.lstm_inputs(F64.lstm_step_case(17, 24, 132, True))
    good = F64.lstm_run(ins, torch.float32)
    assert F64.lstm_step_ratio(good, ins).ok
    for name, mutate in (("tile 8 of y zeroed", lambda o: o["y"][:, 0, 128:132].zero_()),
                         ("rows 15 and 16 of cn swapped", lambda o: o["cn"][0, 15:17].copy_(o["cn"][0, 15:17].flip(0))),
                         ("one element of cn 1e-3 off", lambda o: o["cn"][1, 3, 7].add_(1e-3))):
        bad = {k: v.clone() for k, v in good.items()}
        mutate(bad)
        bad["hn"] = bad["y"][:, 0].reshape(17, 2, 132).transpose(0, 1).contiguous()
        assert not F64.lstm_step_ratio(bad, ins).ok, name
    bad = {k: v.clone() for k, v in good.items()}
    bad["hn"][0, 0, 0] += 1e-6
    assert not F64.lstm_step_ratio(bad, ins).hn_is_y


def _unrolled(ins, dtype, use, cut=None, wrong_c=False):
    """a one-layer, one-direction, batch-first LSTM unrolled by hand in `dtype`, named as F64.lstm_run names its results.
    cut = s: the backward drops the carry (dh, dc) between step s and step s - 1.  wrong_c: the backward's forget-gate
    gradient reads c_{t-2} for c_{t-1} (the forward's values are unchanged: the substitute enters as (f - f) * c)."""
    mod, x, h0, c0, gy, gh, gc = ins
    H, T = mod.hidden_size, x.shape[1]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    w_ih, w_hh, b_ih, b_hh = par = [leaf(getattr(mod, n)) for n in names]
    x, h0, c0 = leaf(x), leaf(h0), leaf(c0)
    h, c, cs, ys = h0[0], c0[0], [c0[0]], []
    for t in range(T):
        if cut == t:
            h, c = h.detach(), c.detach()
        pre = x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        if wrong_c and t >= 1:
            c = f.detach() * c + (f - f.detach()) * cs[t - 1].detach() + i * g
        else:
            c = f * c + i * g
        h = o * torch.tanh(c)
        cs.append(c)
        ys.append(h)
    y = torch.stack(ys, 1)
    loss = 0
    if "y" in use:
        loss = loss + (y * gy.to(dtype)).sum()
    if "h" in use:
        loss = loss + (h * gh[0].to(dtype)).sum()
    if "c" in use:
        loss = loss + (c * gc[0].to(dtype)).sum()
    loss.backward()
    out = {"y": y, "hn": h[None], "cn": c[None], "dx": x.grad, "dh0": h0.grad, "dc0": c0.grad}
    out.update({"d" + n: p.grad for n, p in zip(names, par)})
    return {k: v.detach() for k, v in out.items()}


def _seq_ok(got, r64, r32, key, bf=True):
    return F64.seq_chain_ratio(got[key], r64[key], r32[key], F64.lstm_slice_dim(key, bf), key).ok


def test_seq_chain_checker_rejects_backward_indexing_slips():
    case, use = (5, 9, 12, 37, 1, False, True, True), ("y", "h", "c")
    ins = F64.lstm_inputs(case)
    r64, r32 = F64.lstm_refs(case, use)
    good = _unrolled(ins, torch.float32, use)
    assert F64.chain_figure(_unrolled(ins, torch.float64, use)["dx"], r64["dx"]) < 1e-12     # the restatement is the LSTM
    for k in r64:
        assert _seq_ok(good, r64, r32, k), k
    cut = _unrolled(ins, torch.float32, use, cut=6)        # the carry dropped at step 6: dx of steps 0..5 lacks it
    for k in ("y", "hn", "cn"):
        assert torch.equal(cut[k], good[k])
    assert torch.equal(cut["dx"][:, 6:], good["dx"][:, 6:])
    for k in ("dx", "dh0", "dc0", "dweight_ih_l0", "dweight_hh_l0", "dbias_ih_l0", "dbias_hh_l0"):
        assert not _seq_ok(cut, r64, r32, k), k
    wrong = _unrolled(ins, torch.float32, use, wrong_c=True)
    for k in ("y", "hn", "cn"):
        assert torch.equal(wrong[k], good[k])
    for k in ("dx", "dh0", "dweight_ih_l0", "dweight_hh_l0", "dbias_ih_l0", "dbias_hh_l0"):
        assert not _seq_ok(wrong, r64, r32, k), k


def test_seq_chain_checker_rejects_forward_tile_and_row_slips():
    case, use = F64.LSTM_CHAIN_CASES[1]      # (9, 24, 20, 132), batch-first
    r64, r32 = F64.lstm_refs(case, use)
    y = r32["y"].clone()
    y[:, 7, 16:32] = 0                       # one 16-wide hidden tile of one step zeroed
    assert not F64.seq_chain_ratio(y, r64["y"], r32["y"], 1).ok
    y = r32["y"].clone()
    y[[2, 3], 7] = y[[3, 2], 7]              # two batch rows swapped at one step
    r = F64.seq_chain_ratio(y, r64["y"], r32["y"], 1)
    assert not r.ok and r.where == (7,)
    y = r32["y"].clone()
    y[0, 23, 131] = float("nan")
    assert not F64.seq_chain_ratio(y, r64["y"], r32["y"], 1).ok


def test_per_slice_check_sees_what_the_whole_tensor_bar_does_not():
    """dx of the 70-step case with the loss on h_n only, whose per-step maximum falls by 1.5 - 2 x per step going back:
      - the first 45 steps scaled by 1.5 (wrong by 50 % over two thirds of the sequence): PASSES the old whole-tensor bar
        (2.5e-6 < 2e-5), rejected per slice;
      - the first 60 steps scaled by 1.5: rejected per slice; the old bar sees this one too (2.8e-3): step 59 still carries
        5.5e-3 of the tensor's maximum;
    y of the reverse direction shifted by one step: FAILS the old bar already, and is rejected per slice."""
    case, use = F64.LSTM_CHAIN_CASES[0]
    r64, r32 = F64.lstm_refs(case, use)
    for steps, old_passes in ((45, True), (60, False)):
        dx = r32["dx"].clone()
        dx[:steps] *= 1.5
        old = _old_bar(dx, r64["dx"])
        print("dx[:%d] x 1.5: whole-tensor figure %.3g (bar 2e-5)" % (steps, old))
        assert (old < 2e-5) == old_passes
        r = F64.seq_chain_ratio(dx, r64["dx"], r32["dx"], 0)
        assert not r.ok and r.ratio > 1e4
        with pytest.raises(AssertionError):
            F64.seq_chain_check(dx, r64["dx"], r32["dx"], 0, quiet=True)
    case, use = F64.LSTM_CHAIN_CASES[3]      # (17, 3, 24, 128), bidirectional, time-major
    r64, r32 = F64.lstm_refs(case, use)
    H = case[3]
    y = r32["y"].clone()
    y[:, :, H:] = y[:, :, H:].roll(1, 0)
    old = _old_bar(y, r64["y"])
    print("reverse direction shifted by one step: whole-tensor figure %.3g (bar 2e-5)" % old)
    assert old > 2e-5
    assert not F64.seq_chain_ratio(y, r64["y"], r32["y"], 0).ok


# ----------------------------------------------------------------------------------------------------------------------
# The TabNet checkers: each accepts torch's CPU fp32 evaluation of the kernel's own formula at every shape the GPU tests use
# (sums in double where the kernel sums in double), and rejects the slips a row kernel, a ghost-batch loop or a shared
# weight's accumulation can make.
# ----------------------------------------------------------------------------------------------------------------------
from oracle import fill as _fill, tabnet_ref as _T  # noqa: E402


def _spmax32(x, dk=0):
    """the kernel's sparsemax in fp32 (sorted prefix sums); dk: tau from the support size k + dk (clamped to 1..D)"""
    x = x.float()
    v = x - x.amax(1, keepdim=True)
    srt = v.sort(1, descending=True).values
    cum = srt.cumsum(1)
    ks = torch.arange(1, x.shape[1] + 1, dtype=torch.float32).view(1, -1)
    k = ((1 + ks * srt) > cum).sum(1, keepdim=True)
    k = (k + dk).clamp(1, x.shape[1])
    tau = (cum.gather(1, k - 1) - 1) / k.float()
    return (v - tau).clamp_min(0)


def _spmax_bwd32(p, dp):
    sup = p > 0
    vhat = (dp * sup).sum(1, keepdim=True) / sup.sum(1, keepdim=True).clamp_min(1).float()
    return torch.where(sup, dp - vhat, torch.zeros_like(dp))


@pytest.mark.parametrize("D", F64.SPMAX_D)
@pytest.mark.parametrize("family", F64.SPMAX_FAMILIES)
def test_sparsemax_checker_accepts_torch_fp32(family, D):
    for N in F64.TAB_ROWS:
        x = F64.sparsemax_rows(N, D, family)
        for p in (_spmax32(x), _T.sparsemax(x)):
            F64.check_sparsemax(x, p)
        p = _spmax32(x)
        dp = _fill.hash_tensor((N, D), 81)
        F64.check_sparsemax_bwd(p, dp, _spmax_bwd32(p, dp))


def test_sparsemax_families_reach_their_edges():
    """the tie family puts exact ties on the threshold, the dominant family has leads of exactly 1 and none below it, and
    the hash family reaches every support size"""
    x = F64.sparsemax_rows(257, 5, "ties")
    z = (x - x.amax(1, keepdim=True)).double()
    p, _, k = F64.sparsemax_ref(x)
    zs = z.sort(1, descending=True).values
    tau = (zs.cumsum(1) - 1) / torch.arange(1, 6, dtype=torch.float64)
    on = (zs[:, 1:] == tau[:, :-1]).any(1)          # z_(k+1) == tau_k: an entry exactly on the threshold
    assert int(on.sum()) >= 16
    xs = F64.sparsemax_rows(257, 5, "dominant").double().sort(1, descending=True).values
    assert bool(((xs[:, 0] - xs[:, 1]) == 1).any()) and bool(((xs[:, 0] - xs[:, 1]) >= 1).all())
    assert set(int(v) for v in F64.sparsemax_ref(F64.sparsemax_rows(513, 5, "hash"))[2]) == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("D", [3, 5, 63, 64])
@pytest.mark.parametrize("dk", [-1, 1])
def test_sparsemax_checker_rejects_a_support_size_off_by_one(D, dk):
    x = F64.sparsemax_rows(257, D, "hash")
    assert _fails(lambda: F64.check_sparsemax(x, _spmax32(x, dk)))
    xp = F64.sparsemax_rows(257, D, "prior")
    assert _fails(lambda: F64.check_sparsemax(xp, _spmax32(xp, dk)))


def test_sparsemax_checkers_reject_a_skipped_row_block_and_a_wrong_mean():
    x = F64.sparsemax_rows(513, 5, "hash")
    p = _spmax32(x)
    dp = _fill.hash_tensor((513, 5), 81)
    stale = p.clone()
    stale[256:512] = 0.0
    assert _fails(lambda: F64.check_sparsemax(x, stale))
    dx = _spmax_bwd32(p, dp)
    skipped = dx.clone()
    skipped[256:512] = 0.0
    assert _fails(lambda: F64.check_sparsemax_bwd(p, dp, skipped))
    assert _fails(lambda: F64.check_sparsemax_bwd(p, dp, dp - dp.mean(1, keepdim=True)))        # mean over the row, not the support
    leak = dx.clone()
    leak[p == 0] = 1e-30
    assert _fails(lambda: F64.check_sparsemax_bwd(p, dp, leak))                                 # outside the support: exactly 0


def _glu32(z, dout, swap=False, no_1ms=False):
    D = z.shape[1] // 2
    a, b = (z[:, D:], z[:, :D]) if swap else (z[:, :D], z[:, D:])
    s = 1.0 / (1.0 + torch.exp(-b))
    dzb = dout * a * s if no_1ms else dout * a * s * (1.0 - s)
    return a * s, torch.cat([dout * s, dzb], 1)


@pytest.mark.parametrize("extreme", [False, True])
@pytest.mark.parametrize("D", F64.GLU_D)
def test_glu_checker_accepts_torch_fp32_and_rejects_swapped_halves_and_a_missing_factor(D, extreme):
    for N in F64.TAB_ROWS:
        z, dout = F64.glu_inputs(N, D, extreme)
        out, dz = _glu32(z, dout)
        F64.check_glu(z, out, dout, dz)
        zz = z.clone().requires_grad_(True)
        o2 = zz[:, :D] * torch.sigmoid(zz[:, D:])
        o2.backward(dout)
        F64.check_glu(z, o2.detach(), dout, zz.grad)
        assert _fails(lambda: F64.check_glu(z, _glu32(z, dout, swap=True)[0]))
        if N * D > 4:
            assert _fails(lambda: F64.check_glu(z, out, dout, _glu32(z, dout, no_1ms=True)[1]))
    if extreme:
        nan = out.clone()
        nan[0, 0] = float("nan")
        assert _fails(lambda: F64.check_glu(z, nan))


def _entropy32(M, g, eps=F64.ENT_EPS, div=None):
    N = M.shape[0]
    e = torch.tensor(eps, dtype=torch.float32)
    term = M * torch.log(M + e)
    out = (term.double().sum() / (div or N)).float().reshape(1)
    dM = (g / torch.tensor(float(N))) * (torch.log(M + e) + M / (M + e))
    return out, dM


@pytest.mark.parametrize("D", [2, 5, 64])
def test_entropy_checker_accepts_torch_fp32_and_rejects_a_mean_over_every_element(D):
    for N in F64.TAB_ROWS:
        M, g = F64.entropy_inputs(N, D)
        out, dM = _entropy32(M, g)
        F64.check_entropy(M, out, F64.ENT_EPS, g, dM)
        assert _fails(lambda: F64.check_entropy(M, _entropy32(M, g, div=N * D)[0]))
        assert _fails(lambda: F64.check_entropy(M, None, F64.ENT_EPS, g, dM / D))
    assert float(_entropy32(torch.zeros(7, D), g)[0]) == 0.0
    F64.check_entropy(torch.zeros(7, D), torch.zeros(1))


def _ew32(op, a, b, s):
    s = torch.tensor(s, dtype=torch.float32)
    return {"MUL": lambda: a * b, "ADD_SCALE": lambda: (a + b) * s, "PRIOR": lambda: b * (s - a), "RELU": lambda: a.clamp_min(0),
            "RELU_BWD": lambda: torch.where(a > 0, b, torch.zeros_like(a)), "SCALE": lambda: a * s, "NEG_MUL": lambda: -a * b,
            "ADD": lambda: a + b, "RSUB": lambda: s - a}[op]()


@pytest.mark.parametrize("op", list(F64.EW_OPS))
def test_ew_checker_accepts_torch_fp32_and_rejects_an_unwritten_tail(op):
    for n in (1, 257, F64.EW_GRID_CAP + 257):
        a, b, s = F64.ew_inputs(n)
        out = _ew32(op, a, b if F64.EW_ARITY[op] == 2 else None, s)
        F64.check_ew(op, a, b if F64.EW_ARITY[op] == 2 else None, s, out)
    tail = out.clone()
    tail[F64.EW_GRID_CAP:] = 0.0
    assert _fails(lambda: F64.check_ew(op, a, b if F64.EW_ARITY[op] == 2 else None, s, tail))
    if op in F64.EW_EXACT and op not in ("RELU", "RELU_BWD"):
        off = out.clone()
        off[5] = torch.nextafter(off[5], torch.tensor(float("inf")))
        assert _fails(lambda: F64.check_ew(op, a, b if F64.EW_ARITY[op] == 2 else None, s, off))     # one ulp is not exact


@pytest.mark.parametrize("N,D,nd", F64.SPLIT_CASES)
def test_split_reference_is_the_slice_and_its_mask(N, D, nd):
    x, gd, ga = F64.split_inputs(N, D, nd)
    assert bool((x == 0).any()) or N * D < 8
    for relu in (0, 1):
        d, a = F64.split_ref(x, nd, relu)
        xr = x.clone().requires_grad_(True)
        dd = torch.relu(xr[:, :nd]) if relu else xr[:, :nd]
        (dd * gd).sum().backward()
        assert torch.equal(d, dd.detach()) and torch.equal(a, x[:, nd:])
        assert torch.equal(F64.split_bwd_ref(d, gd, None, D, nd, relu), xr.grad)
        assert torch.equal(F64.split_bwd_ref(d, None, ga, D, nd, relu)[:, nd:], ga)


def _bn32(x, gamma, beta, rm0, rv0, momentum, eps, training, biased=False):
    """the kernel's bn_small forward: statistics in double, stored as fp32, the affine in fp32 -> y, save, rm, rv"""
    N, C = x.shape
    g = torch.ones(C) if gamma is None else gamma
    b = torch.zeros(C) if beta is None else beta
    rm, rv = (None, None) if rm0 is None else (rm0.clone(), rv0.clone())
    if training:
        xd = x.double()
        mean = xd.sum(0) / N
        var = ((xd * xd).sum(0) / N - mean * mean).clamp_min(0)
        if rm is not None:
            mom = torch.tensor(momentum, dtype=torch.float32)
            unb = var if biased or N == 1 else var * N / (N - 1.0)
            rm = (1 - mom) * rm + mom * mean.float()
            rv = (1 - mom) * rv + mom * unb.float()
    else:
        mean, var = rm0.double(), rv0.double()
    inv = (1.0 / (var + float(torch.tensor(eps, dtype=torch.float32))).sqrt()).float()
    m = mean.float()
    return (x - m) * inv * g + b, torch.stack([m, inv]), rm, rv


def _bn_bwd32(x, dy, gamma, save, training, dg0=None, db0=None):
    N, C = x.shape
    g = torch.ones(C) if gamma is None else gamma
    m, inv = save[0], save[1]
    xh = (x - m) * inv
    s1 = dy.double().sum(0).float()
    s2 = (dy.double() * xh.double()).sum(0).float()
    if training:
        dx = (g * inv) * (dy - s1 / N - xh * (s2 / N))
    else:
        dx = dy * (g * inv)
    return dx, (s2 if dg0 is None else dg0 + s2), (s1 if db0 is None else db0 + s1)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("C", F64.BN_SMALL_C)
def test_bn_small_checkers_accept_torch_fp32(C, training):
    for N in F64.BN_SMALL_N:
        for ratio in (None, 1e3):
            for momentum in (0.01, 0.02):
                d = F64.bn_small_inputs(N, C, ratio)
                y, save, rm, rv = _bn32(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], momentum, 1e-5, training)
                F64.check_bn_small_fwd(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, momentum, 1e-5, training, y, save, rm, rv,
                                       5 + training)
                for acc in (0, 1):
                    dg0, db0 = (d["dg0"], d["db0"]) if acc else (None, None)
                    dx, dg, db = _bn_bwd32(d["x"], d["dy"], d["gamma"], save, training, dg0, db0)
                    F64.check_bn_small_bwd(d["x"], d["dy"], d["gamma"], save, training, dx, dg, db, dg0, db0)


def test_bn_small_checkers_reject_their_defects():
    N, C = 65, 3
    d = F64.bn_small_inputs(N, C)
    args = (d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"])
    y, save, rm, rv = _bn32(*args, 0.02, 1e-5, 1)
    fwd = lambda y=y, save=save, rm=rm, rv=rv, nbt=6: F64.check_bn_small_fwd(*args, 5, 0.02, 1e-5, 1, y, save, rm, rv, nbt)
    fwd()
    assert _fails(lambda: fwd(rv=_bn32(*args, 0.02, 1e-5, 1, biased=True)[3]))          # biased variance in the running update
    assert _fails(lambda: fwd(rm=_bn32(*args, 0.01, 1e-5, 1)[2]))                       # the other momentum
    assert _fails(lambda: fwd(nbt=5))
    big = F64.bn_small_inputs(513, C)
    yb, sb, _, _ = _bn32(big["x"], big["gamma"], big["beta"], None, None, 0.02, 1e-5, 1)
    y256, s256, _, _ = _bn32(big["x"][:256], big["gamma"], big["beta"], None, None, 0.02, 1e-5, 1)      # the stride loop not taken
    chk = lambda y, s: F64.check_bn_small_fwd(big["x"], big["gamma"], big["beta"], None, None, None, 0.02, 1e-5, 1, y, s, None, None, None)
    chk(yb, sb)
    assert _fails(lambda: chk(yb, s256))
    dx, dg, db = _bn_bwd32(big["x"], big["dy"], big["gamma"], sb, 1)
    bwd = lambda **kw: F64.check_bn_small_bwd(big["x"], big["dy"], big["gamma"], sb, 1, **kw)
    bwd(dx=dx, dgamma=dg, dbeta=db)
    part = _bn_bwd32(big["x"][:512], big["dy"][:512], big["gamma"], sb, 1)
    assert _fails(lambda: bwd(dgamma=part[1])) and _fails(lambda: bwd(dbeta=part[2]))   # the 513th row missing from the sums
    skipped = dx.clone()
    skipped[256:512] = 0.0
    assert _fails(lambda: bwd(dx=skipped))
    assert _fails(lambda: F64.check_bn_small_bwd(big["x"], big["dy"], big["gamma"], sb, 1, dgamma=dg, dg0=big["dg0"], db0=big["db0"]))
    assert _fails(lambda: F64.check_bn_small_bwd(big["x"], big["dy"], big["gamma"], sb, 0, dx=dx))   # eval has no mean terms


def _ghost32(d, B, vbs, training, momentum=0.02, slices=None, keep_last=False):
    sl = slices or F64.ghost_slices(B, vbs)
    rm, rv = d["rm0"], d["rv0"]
    ys, saves, dxs, dg, db = [], [], [], None, None
    for i0, i1 in sl:
        y, save, rm_, rv_ = _bn32(d["x"][i0:i1], d["gamma"], d["beta"], rm, rv, momentum, 1e-5, training)
        if training:
            rm, rv = rm_, rv_
        dx, dg_, db_ = _bn_bwd32(d["x"][i0:i1], d["dy"][i0:i1], d["gamma"], save, training, None if keep_last else dg,
                                 None if keep_last else db)
        dg, db = dg_, db_
        ys.append(y); saves.append(save); dxs.append(dx)
    return dict(y=torch.cat(ys), save=torch.stack(saves), rm=rm, rv=rv, nbt=5 + (len(sl) if training else 0), dx=torch.cat(dxs),
                dgamma=dg, dbeta=db)


def _ghost_check(d, B, vbs, training, o):
    return F64.check_ghost_bn(d["x"], d["gamma"], d["beta"], d["rm0"], d["rv0"], 5, 0.02, 1e-5, vbs, training, o["y"], o["save"],
                              o["rm"], o["rv"], o["nbt"], d["dy"], o["dx"], o["dgamma"], o["dbeta"])


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("B,vbs", F64.GHOST_CASES)
def test_ghost_bn_checker_accepts_torch_fp32_per_chunk(B, vbs, training):
    for C in (3, 64):
        d = F64.bn_small_inputs(B, C)
        _ghost_check(d, B, vbs, training, _ghost32(d, B, vbs, training))


def test_ghost_slices_are_torch_chunks():
    assert F64.ghost_slices(130, 128) == [(0, 65), (65, 130)] and F64.ghost_slices(257, 16)[-1] == (256, 257)
    assert F64.ghost_slices(300, 128) == [(0, 100), (100, 200), (200, 300)] and F64.ghost_slices(7, None) == [(0, 7)]
    for B in (2, 129, 385, 50):
        for vbs in (128, 16):
            sizes = [c.shape[0] for c in torch.zeros(B, 1).chunk(-(-B // vbs))]
            assert [b - a for a, b in F64.ghost_slices(B, vbs)] == sizes


def test_ghost_bn_checker_rejects_fixed_size_slices_and_a_dropped_virtual_batch():
    B, vbs, C = 130, 128, 3
    d = F64.bn_small_inputs(B, C)
    good = _ghost32(d, B, vbs, 1)
    _ghost_check(d, B, vbs, 1, good)
    assert _fails(lambda: _ghost_check(d, B, vbs, 1, _ghost32(d, B, vbs, 1, slices=[(0, 128), (128, 130)])))    # 128 + 2, not 65 + 65
    last = _ghost32(d, B, vbs, 1, keep_last=True)
    assert _fails(lambda: _ghost_check(d, B, vbs, 1, dict(good, dgamma=last["dgamma"])))                        # only the last slice's dgamma
    assert _fails(lambda: _ghost_check(d, B, vbs, 1, dict(good, dbeta=last["dbeta"])))
    assert _fails(lambda: _ghost_check(d, B, vbs, 1, dict(good, nbt=6)))                                        # one step per slice
    one = _ghost32(d, B, vbs, 1, slices=[(0, 65)])
    assert _fails(lambda: _ghost_check(d, B, vbs, 1, dict(good, rm=one["rm"])))                                 # the second update missing


def test_shared_weight_gradient_check_rejects_a_missing_use():
    B, In, Out = 130, 64, 128
    pairs = [(_fill.hash_tensor((B, In), 90 + i), _fill.hash_tensor((B, Out), 95 + i)) for i in range(4)]
    ref, A, K = F64.shared_dw_ref(pairs)
    assert K == 4 * B
    dw = sum(dy.t() @ x for x, dy in pairs)
    assert F64.dot_ratio(dw, ref, A, K).ok
    for miss in range(4):
        part = sum(dy.t() @ x for i, (x, dy) in enumerate(pairs) if i != miss)
        assert not F64.dot_ratio(part, ref, A, K).ok
    twice = dw + pairs[0][1].t() @ pairs[0][0]
    assert not F64.dot_ratio(twice, ref, A, K).ok


def test_plan_only_checkers_accept_torch_fp32_and_reject_defects():
    """avgpool (plain and through coefficients), bcast_rows, the SE gate gradient and the dropout scaling: torch's fp32
    evaluation passes each derived bound; a dropped row, a dropped shift, a missing 1 / R, an unmasked element and a missing
    1 / (1 - p) are rejected"""
    from oracle import fill
    h = fill.hash_tensor
    N, R, C = 3, 125, 64
    x, sc, sh = h((N, R, C), 90, 2.0), 1 + 0.3 * h((C,), 91), 0.2 * h((C,), 92)
    F64.check_avgpool(x.mean(1), x)
    F64.check_avgpool(x.mean(1) * sc + sh, x, sc, sh)
    ref, A, K = F64.avgpool_ref(x, sc, sh)
    assert K == R + 3
    assert not F64.plain_ratio(x[:, :-1].sum(1) / R * sc + sh, ref, A, K, "row dropped").ok
    assert not F64.plain_ratio(x.mean(1) * sc, ref, A, K, "shift dropped").ok
    for bf16 in (False, True):
        v = h((N, C), 93)
        got = F64._b((v * torch.tensor(1.0 / R)).unsqueeze(1).expand(-1, R, -1), bf16)
        F64.check_bcast(got, v, R, bf16)
        with pytest.raises(AssertionError):
            F64.check_bcast(F64._b(v.unsqueeze(1).expand(-1, R, -1), bf16), v, R, bf16)
    dout, y, mask = h((N, R, C), 94), h((N, R, C), 95, 2.0), h((N, R, C), 96) > -0.3
    dg = (torch.where(mask, dout, torch.zeros_like(dout)) * (y * sc + sh)).sum(1)
    F64.check_se_gate_grad(dg, dout, mask, y, sc, sh)
    ref, A, K = F64.se_gate_grad_ref(dout, mask, y, sc, sh)
    flip = mask.clone()
    flip[1, 7, 5] ^= True
    bad = (torch.where(flip, dout, torch.zeros_like(dout)) * (y * sc + sh)).sum(1)
    assert not F64.plain_ratio(bad, ref, A, K, "one mask element").ok
    xx, keep, p = h((N, 64), 97), h((N, 64), 98) > -0.4, 0.3
    F64.check_dropout(torch.where(keep, xx * (1.0 / (1.0 - torch.tensor(p))), torch.zeros_like(xx)), xx, keep, p)
    with pytest.raises(AssertionError):
        F64.check_dropout(torch.where(keep, xx, torch.zeros_like(xx)), xx, keep, p)


def test_eval_coef_ref_accepts_torch_fp32_and_rejects_a_swapped_statistic():
    from oracle import fill
    h = fill.hash_tensor
    C = 128
    g, b, rm, rv = 1 + 0.1 * h((C,), 101), 0.1 * h((C,), 102), 0.1 * h((C,), 103), 1 + 0.2 * h((C,), 104).abs()
    inv = 1.0 / torch.sqrt(rv + 1e-5)
    coef = torch.stack([g * inv, b - rm * (g * inv), rm, inv])
    ref = F64.eval_coef_ref(g, b, rm, rv, 1e-5)
    assert F64.coef_ratio(coef, ref).ok
    assert not F64.coef_ratio(coef, F64.eval_coef_ref(g, b, rm, rv.flip(0), 1e-5)).ok



# ----------------------------------------------------------------------------------------------------------------------
# The fp32-operand conv checker (f32_ratio, dw_f32_ratio, check_stats_f32) at the largest K tests/test_conv_edges_f64_gpu.py
# uses: 128 channels x 9 taps = 1152 summands for y / dx, 9600 pixels for a weight gradient.  It accepts torch's own CPU
# fp32 conv2d / autograd with the final constants and rejects a zeroed element, a neighbour pixel's value, a dropped
# 16-byte chunk (4 channels) of one tap, a wrong image-border row, and for dw a split counted twice and a split left out.
# ----------------------------------------------------------------------------------------------------------------------
K32 = 128 * 9
DW32_PIXELS = 6 * 40 * 40
DW32_SPLIT = 32              # fp32: 16 pixels a step, 600 steps over min(600, 512) splits: 2 steps = 32 pixels per split


def _fp32_operands(n, cin, cout, h, w, seed):
    """full-mantissa fp32 values: activations >= 0 with exact zeros and a per-image / per-channel offset, signed gradients"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, cin, h, w, generator=g)
    off = 1.0 + ((torch.arange(n).view(-1, 1) * 37 + torch.arange(cin).view(1, -1) * 11) % 64).float().view(n, cin, 1, 1) / 16
    x = torch.where(z > 0, z + off, torch.zeros_like(z))
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    dy = torch.randn(n, cout, h, w, generator=g) + torch.linspace(-2, 2, n * cout).view(n, cout, 1, 1)
    return x, wt, dy


@pytest.fixture(scope="module")
def case32():
    x, w, dy = _fp32_operands(3, 128, 64, 9, 11, 21)
    b = torch.linspace(-1, 1, 64)
    return x, w, dy, b, F64.conv_ref64(x, w, dy, 1, (1, 1), bias=b)


@pytest.fixture(scope="module")
def case32_dw():
    x, w, dy = _fp32_operands(6, 64, 64, 40, 40, 22)
    return x, w, dy, F64.conv_ref64(x, w, dy, 1, (1, 1))


def _torch32(x, w, dy, b=None):
    xf, wf = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xf, wf, b, padding=1)
    y.backward(dy)
    return y.detach(), xf.grad, wf.grad


def test_fp32_conv_checker_accepts_torch_fp32(case32, case32_dw):
    x, w, dy, b, ref = case32
    y32, dx32, _ = _torch32(x, w, dy, b)
    ry = F64.check_f32(y32, ref.y, ref.ay, K32, name="torch fp32 y")
    rdx = F64.check_f32(dx32, ref.dx, ref.adx, 64 * 9, name="torch fp32 dx")
    F64.check_f32(ref.y.float(), ref.y, ref.ay, K32, name="fp32(ref) y")
    p = _pix(y32)                                  # statistics rows as the epilogue forms them: fp32 sums of 64 pixels
    pad = torch.zeros(-p.shape[0] % 64, p.shape[1])
    p = torch.cat([p, pad]).view(-1, 64, p.shape[1])
    rows = torch.stack([p.sum(1), (p * p).sum(1)], 1)
    F64.check_stats_f32(rows, ref, K32, name="torch fp32 stats")
    bad = rows.clone()
    bad[2] = 0
    with pytest.raises(AssertionError):
        F64.check_stats_f32(bad, ref, K32)
    x, w, dy, ref = case32_dw
    _, _, dw32 = _torch32(x, w, dy)
    rdw = F64.check_dw_f32(dw32, ref.dw, ref.adw, DW32_PIXELS, name="torch fp32 dw")
    F64.check_dw_f32(ref.dw.float(), ref.dw, ref.adw, DW32_PIXELS, name="fp32(ref) dw")
    prior = torch.randn(dw32.shape, generator=torch.Generator().manual_seed(24))          # accumulate = 1 onto an independent tensor
    F64.check_dw_f32(prior + dw32, prior.double() + ref.dw, prior.double().abs() + ref.adw, DW32_PIXELS,
                     name="torch fp32 dw, accumulated onto a prior")
    print("torch CPU fp32: y %.3g, dx %.3g of A; dw %.3g of A, %.3g of rms" % (ry.kappa_seen, rdx.kappa_seen, rdw.kappa_seen,
                                                                             rdw.eps_seen))


def test_fp32_conv_checker_demands_exactness_where_nothing_is_summed():
    """1x1 / stride 2: the input gradient of a pixel with an odd row or column has A == 0 and must be exactly 0"""
    x, w, dy = _fp32_operands(2, 16, 8, 9, 9, 23)
    w = w[:, :, :1, :1].contiguous()
    dy = dy[:, :, :5, :5].contiguous()
    ref = F64.conv_ref64(x, w, dy, 2, (0, 0))
    assert (ref.adx[:, :, 1::2] == 0).all() and (ref.adx[:, :, :, 1::2] == 0).all()
    assert F64.f32_ratio(ref.dx.float(), ref.dx, ref.adx, 8).ok
    m = ref.dx.float().clone()
    m[1, 3, 1, 2] = 1e-30
    assert F64.f32_ratio(m, ref.dx, ref.adx, 8).ratio == float("inf")
    m = ref.dx.float().clone()
    m[0, 0, 0, 1] = float("nan")
    assert not F64.f32_ratio(m, ref.dx, ref.adx, 8).ok


def _mutations32(x, w, ref):
    """(name, mutated fp32 output [pixels][channels]) pairs, each a copy of fp32(ref.y) with one defect"""
    base = _pix(ref.y.float())
    n, _, h, wd = ref.y.shape
    out = []
    flat = base.reshape(-1)
    k = int(torch.argsort(flat.abs())[flat.numel() // 2])
    m = base.clone()
    m.view(-1)[k] = 0
    out.append(("one element zeroed", m))
    m = base.clone()
    m[150] = base[151]
    out.append(("a pixel holds its neighbour's value", m))
    # one 16-byte chunk (input channels 4..7) of the centre tap missing from one pixel, where those inputs are not zero
    img, py, px = 1, 4, 5
    assert (x[img, 4:8, py, px] != 0).any()
    part = (x[img, 4:8, py, px].double()[None] * w[:, 4:8, 1, 1].double()).sum(1)
    yt = ref.y.clone()
    yt[img, :, py, px] -= part
    out.append(("a 4-channel chunk of one tap dropped", _pix(yt.float())))
    # image 2's top output row read the last row of image 1 instead of the zero padding above it
    img = 2
    xin = torch.cat([x[img - 1:img, :, h - 1:h], x[img:img + 1]], dim=2).double()
    ytop = F.conv2d(xin, w.double(), padding=(0, 1))[:, :, 0]
    yt = ref.y.clone()
    yt[img, :, 0] += ytop[0] - F.conv2d(x[img:img + 1].double(), w.double(), padding=1)[0, :, 0]
    out.append(("image-border row from the neighbouring image", _pix(yt.float())))
    return out


def test_fp32_conv_checker_rejects_each_defect(case32):
    x, w, dy, b, ref = case32
    for name, m in _mutations32(x, w, ref):
        r = F64.f32_ratio(_unpix(m, ref.y), ref.y, ref.ay, K32, name=name)
        print(r)
        assert r.ratio > 1.0, "checker accepted: " + name
    base = _pix(ref.dx.float())
    m = base.clone()
    m[40] = base[41]
    assert not F64.f32_ratio(_unpix(m, ref.dx), ref.dx, ref.adx, 64 * 9).ok
    m = base.clone()
    m[-1, -4:] = 0                      # the last 16 bytes of the tensor left unwritten (zeros)
    assert not F64.f32_ratio(_unpix(m, ref.dx), ref.dx, ref.adx, 64 * 9).ok
    m[-1, -4:] = float("nan")           # ... or still holding the poison
    assert not F64.f32_ratio(_unpix(m, ref.dx), ref.dx, ref.adx, 64 * 9).ok


def _dw32_of_pixels(x, dy, lo, hi):
    mask = torch.zeros(dy.shape[0] * dy.shape[2] * dy.shape[3], dtype=torch.float64)
    mask[lo:hi] = 1
    dym = dy.double() * mask.view(dy.shape[0], dy.shape[2], dy.shape[3]).unsqueeze(1)
    wr = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, padding=1).backward(dym)
    return wr.grad


def test_fp32_conv_checker_rejects_weight_gradient_split_defects(case32_dw):
    x, w, dy, ref = case32_dw
    split = _dw32_of_pixels(x, dy, 7 * DW32_SPLIT, 8 * DW32_SPLIT)
    for name, m in (("a split counted twice", ref.dw + split), ("a split left out", ref.dw - split),
                    ("the last split left out", ref.dw - _dw32_of_pixels(x, dy, DW32_PIXELS - DW32_SPLIT, DW32_PIXELS))):
        r = F64.dw_f32_ratio(m.float(), ref.dw, ref.adw, DW32_PIXELS, name="dw: " + name)
        print(r)
        assert not r.ok, "checker accepted: " + name
    m = ref.dw.float().clone()
    m[5, 7, 1, 1] = float("nan")
    assert not F64.dw_f32_ratio(m, ref.dw, ref.adw, DW32_PIXELS).ok


# ---- the two passes of the inference plans (csrc/infer_fold.hip): relu_maxpool, gate_res_relu ----
def _pool_emul(y, shift=0, flat_pad=False, clamp=True):
    """relu_maxpool_kernel restated in torch on the stored type: best = 0 (or -inf: no ReLU); best = f > best ? f : best over
    the in-image taps.  shift: the window starts at 2 * o - 1 + shift; flat_pad: no bounds check on the column, so a tap
    outside the row reads its neighbour in memory (the previous row's last pixel, the next row's first)"""
    N, H, W, C = y.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    flat = y.float().reshape(N * H * W, C)
    n = torch.arange(N).view(N, 1, 1)
    oh, ow = torch.arange(OH).view(1, OH, 1), torch.arange(OW).view(1, 1, OW)
    best = torch.full((N, OH, OW, C), 0.0 if clamp else float("-inf"))
    for kh in range(3):
        for kw in range(3):
            h, w = oh * 2 - 1 + shift + kh, ow * 2 - 1 + shift + kw
            inside = (h >= 0) & (h < H) & ((w >= 0) & (w < W) if not flat_pad else torch.ones_like(w, dtype=torch.bool))
            idx = ((n * H + h) * W + w).expand(N, OH, OW)
            inside = (inside & (idx >= 0) & (idx < N * H * W)).expand(N, OH, OW)
            f = flat[idx.clamp(0, N * H * W - 1)]
            take = inside.unsqueeze(3) & (f > best)
            best = torch.where(take, f, best)
    return best.to(y.dtype)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 7, 9, 8), (1, 8, 8, 16), (1, 1, 37, 8), (3, 1, 2, 8), (1, 1, 1, 8), (2, 2, 1, 8)])
def test_relu_maxpool_checker_accepts_the_kernel_restated_in_torch(shape, bf16):
    N, H, W, C = shape
    dt = torch.bfloat16 if bf16 else torch.float32
    y = _fill.hash_tensor(shape, 1201, 2.0).to(dt)
    F64.check_relu_maxpool(_pool_emul(y), y, N, H, W, C, bf16)
    neg = -y.abs()
    neg[0, 0, 0, :4] = -0.0
    out = _pool_emul(neg)
    assert not bool(torch.signbit(out).any()) and not bool(out.any())
    F64.check_relu_maxpool(out, neg, N, H, W, C, bf16, "all negative")
    nan = y.clone()
    nan[0, H // 2, W // 2, 3] = float("nan")
    F64.check_relu_maxpool(_pool_emul(nan), nan, N, H, W, C, bf16, "one NaN tap")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_relu_maxpool_checker_rejects_each_defect(bf16):
    N, H, W, C = 2, 7, 9, 8
    dt = torch.bfloat16 if bf16 else torch.float32
    y = _fill.hash_tensor((N, H, W, C), 1202, 2.0).to(dt)
    good = _pool_emul(y)
    assert F64.relu_maxpool_ratio(good, y, N, H, W, C, bf16).ok
    minus0 = good.clone()
    minus0[good == 0] = -0.0
    assert bool((good == 0).any())
    nan = y.clone()
    nan[1, 3, 4, 2] = float("nan")
    wins = _pool_emul(nan).clone()
    wins[1, 2, 2, 2] = float("nan")
    for name, bad, src in (("window shifted by one", _pool_emul(y, shift=1), y),
                           ("padding read as the neighbour in memory", _pool_emul(y, flat_pad=True), y),
                           ("ReLU omitted", _pool_emul(y, clamp=False), y),
                           ("-0 stored", minus0, y), ("a NaN tap wins", wins, nan),
                           ("every element one ulp up", torch.nextafter(good.float(), torch.tensor(9.0)).to(dt) if not bf16
                            else (good.view(torch.int16) + (good > 0).to(torch.int16)).view(dt), y)):
        r = F64.relu_maxpool_ratio(bad, src, N, H, W, C, bf16, name)
        print(r, r.bad)
        assert not r.ok, "checker accepted: " + name
    with pytest.raises(AssertionError):
        F64.check_relu_maxpool(_pool_emul(y, shift=1), y, N, H, W, C, bf16)


def _gate_case(bf16):
    N, rps, C = 3, 13, 16
    dt = torch.bfloat16 if bf16 else torch.float32
    h = _fill.hash_tensor
    y, res = h((N * rps, C), 1203, 2.0).to(dt), h((N * rps, C), 1204, 1.5).to(dt)
    gate = 0.5 + 0.6 * h((N, C), 1205)
    gate[0, 1], gate[2, 0] = 0.0, -0.75
    return y, gate, res, rps, dt


def _gate_emul(y, gate, res, rps, dt, row_off=0, relu=True, use_res=True, fused=False):
    """gate_res_relu_kernel restated in torch: fp32 arithmetic on the stored operands (fused: the product not rounded),
    rounded once to the stored type.  row_off: the gate row is (r + row_off) // rps"""
    M = y.shape[0]
    row = ((torch.arange(M) + row_off) // rps).clamp(0, gate.shape[0] - 1)
    g = gate[row]
    r = res.float() if use_res else torch.zeros_like(res.float())
    v = (y.double() * g.double() + r.double()).float() if fused else y.float() * g + r
    return (v.clamp_min(0) if relu else v).to(dt)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_gate_res_relu_checker_accepts_torch_and_rejects_each_defect(bf16):
    y, gate, res, rps, dt = _gate_case(bf16)
    for fused in (False, True):
        F64.check_gate_res_relu(_gate_emul(y, gate, res, rps, dt, fused=fused), y, gate, res, rps, bf16)

    def rejected(out):
        try:
            return not F64.gate_res_relu_ratio(out, y, gate, res, rps, bf16).ok
        except AssertionError:      # (a negative value after the ReLU)
            return True
    good = _gate_emul(y, gate, res, rps, dt)
    assert not rejected(good)
    for name, bad in (("gate row of the next sample at the boundary", _gate_emul(y, gate, res, rps, dt, row_off=1)),
                      ("gate row of the previous sample at the boundary", _gate_emul(y, gate, res, rps, dt, row_off=-1)),
                      ("ReLU omitted", _gate_emul(y, gate, res, rps, dt, relu=False)),
                      ("res dropped", _gate_emul(y, gate, res, rps, dt, use_res=False))):
        assert rejected(bad), "checker accepted: " + name
    # only the rows at a rows_per_sample boundary differ in the first two: the checker must see a single row
    one = good.clone()
    one[rps - 1] = _gate_emul(y, gate, res, rps, dt, row_off=1)[rps - 1]
    assert rejected(one), "checker accepted one boundary row gated by its neighbour"
    nan = good.clone()
    nan[5, 3] = float("nan")
    with pytest.raises(AssertionError):
        F64.check_gate_res_relu(nan, y, gate, res, rps, bf16)
