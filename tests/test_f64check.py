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
