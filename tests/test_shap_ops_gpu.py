"""The entry points of csrc/shap.hip through ctypes against tests/shap_ref.py, within the bounds of tests/shap_bounds.py.

Every output is a 0xFF-filled view (NaN for floats) into one byte arena with a zone of sentinel bytes before and after it,
checked after every call; the workspace has exactly the size the library reports and is followed by sentinels.  The gates
of the float64 reference are taken from the device's own stored pre-activations, which are themselves checked against
float64.  Worst measured ratios on the MI355X are recorded in DESIGN.md section 22."""
import numpy as np
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import shap_bounds as Bd
from . import shap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENT, ERR_SHAPE, ERR_WORKSPACE = 1024, 0xA5, 1, 3
DT = {"u8": (torch.uint8, 1), "i32": (torch.int32, 4), "f32": (torch.float32, 4), "f64": (torch.float64, 8)}


class ByteArena:
    """[guard | view | pad to 256 B | guard | view ...] of one uint8 allocation; shapes {name: (dtype key, shape)}"""

    def __init__(self, shapes):
        self.spans, off = {}, GUARD
        for name, (dt, shape) in shapes.items():
            n = int(np.prod(shape)) * DT[dt][1]
            self.spans[name] = (off, n, dt, tuple(shape))
            off = (off + n + 255) // 256 * 256 + GUARD
        self.buf = torch.full((off,), SENT, dtype=torch.uint8, device=DEV)
        self.views = {}
        for name, (o, n, dt, shape) in self.spans.items():
            self.buf[o:o + n] = 0xFF
            self.views[name] = self.buf[o:o + n].view(DT[dt][0]).view(shape)

    def touched(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for o, n, _, _ in self.spans.values():
            mask[o:o + n] = False
        return bool((mask & (self.buf != SENT)).any())


def call(fn, shapes, args, expect=0):
    ar = ByteArena(shapes)
    before = ar.buf.clone()
    rc = getattr(L.lib(), fn)(*args(ar.views), stream())
    torch.cuda.synchronize()
    assert not ar.touched(), fn + " wrote outside an output"
    if expect:
        assert rc == expect, "%s: code %d, expected %d" % (fn, rc, expect)
        assert bool((ar.buf == before).all()), fn + ": a refused call wrote to its outputs"
        return None
    L.check(rc, fn)
    return {k: v.cpu().numpy() for k, v in ar.views.items() if k != "ws"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ws_bytes(B, K, D, H, C):
    n = L.lib().ecgmm_shap_mlp_workspace(B, K, D, H, C)
    assert n > 0
    return n


def gradient(x, bg, ridx, t, w1, b1, w2, var=True, z=True, expect=0, dims=None, ws_short=0):
    B, D = x.shape
    N, (K, H, C) = bg.shape[0], (ridx.shape[1], w1.shape[0], w2.shape[0])
    shapes = {"phi": ("f32", (B, D, C))}
    if var:
        shapes["var"] = ("f32", (B, D, C))
    if z:
        shapes["z"] = ("f32", (B, K, H))
    nb = ws_bytes(B, K, D, H, C)
    shapes["ws"] = ("u8", (nb,))
    t_ = [dev(a) for a in (x, bg, ridx, t, w1, b1, w2)]
    Bc, Nc, Kc, Dc, Hc, Cc = dims or (B, N, K, D, H, C)
    return call("ecgmm_shap_gradient", shapes,
                lambda v: (*(ptr(a) for a in t_), Bc, Nc, Kc, Dc, Hc, Cc, ptr(v["phi"]), ptr(v.get("var")), ptr(v.get("z")),
                           ptr(v["ws"]), nb - ws_short), expect=expect)


def deep(x, bg, w1, b1, w2, z=True, expect=0, dims=None, ws_short=0):
    B, D = x.shape
    N, H, C = bg.shape[0], w1.shape[0], w2.shape[0]
    shapes = {"phi": ("f32", (B, D, C))}
    if z:
        shapes["zx"], shapes["zb"] = ("f32", (B, H)), ("f32", (N, H))
    nb = ws_bytes(B, N, D, H, C)
    shapes["ws"] = ("u8", (nb,))
    t_ = [dev(a) for a in (x, bg, w1, b1, w2)]
    Bc, Nc, Dc, Hc, Cc = dims or (B, N, D, H, C)
    return call("ecgmm_shap_deep", shapes,
                lambda v: (*(ptr(a) for a in t_), Bc, Nc, Dc, Hc, Cc, ptr(v["phi"]), ptr(v.get("zx")), ptr(v.get("zb")),
                           ptr(v["ws"]), nb - ws_short), expect=expect)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def deep_inputs(case):
    """the case's inputs with K = N, and one background row copied from a row of x: zx - zb = 0 exactly there"""
    (x, bg, w1, b1, w2, _), _ = R.ops_inputs(case)
    bg = bg.copy()
    bg[-1] = x[0]
    return x, bg, w1, b1, w2


@pytest.fixture(scope="module")
def deep_runs():
    """one ecgmm_shap_deep call per case, shared by the DeepLIFT test and the bit-equality test of z"""
    return {}


def run_deep(deep_runs, case):
    if case not in deep_runs:
        deep_runs[case] = (deep_inputs(case), deep(*deep_inputs(case)))
    return deep_runs[case]


@pytest.mark.parametrize("case", R.OPS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gradient(case, deep_runs):
    B, N, K, D, H, C = case
    (x, bg, w1, b1, w2, _), (ridx, t) = R.ops_inputs(case)
    assert len(np.unique(ridx[0])) < K or K == 1, "the draws must repeat a background row"
    out = gradient(x, bg, ridx, t, w1, b1, w2)
    phi, var, z = out["phi"], out["var"], out["z"]
    # z against float64 of the same points
    p, pabs = R.points(x, bg, ridx, t)
    rz = Bd.ratio(np.abs(z - R.preact(p, w1, b1)), Bd.z_bound(pabs, w1, b1, interpolated=True))
    # phi and var against float64 with the gates 1[z > 0] of the device's own z: every element
    prod, absprod, G = R.products(x, R.f64(bg)[ridx], R.gate_gradient(z), w1, w2)
    phi64, var64 = R.mean_and_variance(prod)
    phi_b = Bd.phi_bound(absprod, phi64, H, ratio_gates=False)
    rp = Bd.ratio(np.abs(phi - phi64), phi_b)
    rv = Bd.ratio(np.abs(var - var64), Bd.var_bound(prod, absprod, var64, H))
    print("gradient %s: worst ratios z %.3g phi %.3g var %.3g over %d / %d elements" % (case, rz, rp, rv, z.size, phi.size))
    assert rz <= 1.0 and rp <= 1.0 and rv <= 1.0 and phi.size == B * D * C
    # negative control: one 16 x 16 tile of G zeroed in the float64 product must leave the bound
    G0 = G.copy()
    G0[0, :16, 0, :16] = 0.0
    diff = R.f64(x)[:, None, :] - R.f64(bg)[ridx]
    broken = (G0 * diff[:, :, None, :]).mean(1).transpose(0, 2, 1)
    assert Bd.ratio(np.abs(broken - phi64), phi_b) > 1.0, "the phi bound cannot reject a missing tile"
    # t = 0 / t = 1 pairs: z bit-equal to zb / zx of the deep entry on the same rows (bg row N - 1 differs there)
    (dx, dbg, *_), dout = run_deep(deep_runs, case)
    for b in range(B):
        assert np.array_equal(bits(z[b, 1]), bits(dout["zx"][b])) if K > 1 else True
        if ridx[b, 0] != N - 1:
            assert np.array_equal(bits(z[b, 0]), bits(dout["zb"][ridx[b, 0]]))
    # without the optional outputs phi is unchanged
    bare = gradient(x, bg, ridx, t, w1, b1, w2, var=False, z=False)
    assert np.array_equal(bits(bare["phi"]), bits(phi))


@pytest.mark.parametrize("case", R.OPS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_deep(case, deep_runs):
    B, N, _, D, H, C = case
    (x, bg, w1, b1, w2), out = run_deep(deep_runs, case)
    phi, zx, zb = out["phi"], out["zx"], out["zb"]
    dzx, dzb = Bd.z_bound(np.abs(R.f64(x)), w1, b1, False), Bd.z_bound(np.abs(R.f64(bg)), w1, b1, False)
    rzx = Bd.ratio(np.abs(zx - R.preact(x, w1, b1)), dzx)
    rzb = Bd.ratio(np.abs(zb - R.preact(bg, w1, b1)), dzb)
    # the branch is decided in float64 on the stored values; none of them may sit on the threshold
    gap = np.abs(R.f64(zx)[:, None, :] - R.f64(zb)[None, :, :])
    assert not (np.abs(gap - R.THRESHOLD) <= 2 * Bd.U * R.THRESHOLD).any()
    branch = R.rescale_branch(zx, zb)
    assert branch[0, N - 1].all() and (gap[0, N - 1] == 0).all(), "the copied row must take the threshold branch"
    gates = R.gate_rescale(zx, zb)
    assert (gates >= 0).all() and (gates <= 1).all()
    rows = np.broadcast_to(R.f64(bg)[None], (B, N, D))
    prod, absprod, _ = R.products(x, rows, gates, w1, w2)
    phi64 = R.mean_and_variance(prod)[0]
    phi_b = Bd.phi_bound(absprod, phi64, H, ratio_gates=True)
    rp = Bd.ratio(np.abs(phi - phi64), phi_b)
    # additivity against the float64 network
    b2 = np.zeros(C)
    delta = R.forward(x, w1, b1, w2, b2) - R.forward(bg, w1, b1, w2, b2).mean(0)
    ra = Bd.ratio(np.abs(R.f64(phi).sum(1) - delta), Bd.additivity_bound(phi_b, w2, dzx, dzb, branch))
    print("deep %s: worst ratios zx %.3g zb %.3g phi %.3g additivity %.3g" % (case, rzx, rzb, rp, ra))
    assert rzx <= 1.0 and rzb <= 1.0 and rp <= 1.0 and ra <= 1.0
    bare = deep(x, bg, w1, b1, w2, z=False)
    assert np.array_equal(bits(bare["phi"]), bits(phi))


def test_one_call_equals_one_call_per_sample_bit_for_bit():
    case = R.OPS_CASES[0]
    (x, bg, w1, b1, w2, _), (ridx, t) = R.ops_inputs(case)
    whole = gradient(x, bg, ridx, t, w1, b1, w2)
    dwhole = deep(x, bg, w1, b1, w2)
    assert case[0] == 3
    for b in range(3):
        one = gradient(x[b:b + 1], bg, ridx[b:b + 1], t[b:b + 1], w1, b1, w2)
        for k in ("phi", "var", "z"):
            assert np.array_equal(bits(one[k][0]), bits(whole[k][b])), k
        done = deep(x[b:b + 1], bg, w1, b1, w2)
        assert np.array_equal(bits(done["phi"][0]), bits(dwhole["phi"][b]))
        assert np.array_equal(bits(done["zx"][0]), bits(dwhole["zx"][b]))
    # K past one tile: the ordered combine of the pair slices
    case = R.OPS_CASES[3]
    (x, bg, w1, b1, w2, _), (ridx, t) = R.ops_inputs(case)
    whole = gradient(x, bg, ridx, t, w1, b1, w2, z=False)
    one = gradient(x[1:2], bg, ridx[1:2], t[1:2], w1, b1, w2, z=False)
    assert np.array_equal(bits(one["phi"][0]), bits(whole["phi"][1])) and np.array_equal(bits(one["var"][0]), bits(whole["var"][1]))


def test_out_of_range_ridx_gives_nan_for_that_sample_only():
    case = R.OPS_CASES[0]
    (x, bg, w1, b1, w2, _), (ridx, t) = R.ops_inputs(case)
    clean = gradient(x, bg, ridx, t, w1, b1, w2)
    for wrong in (case[1], -1, 2 ** 31 - 1):
        bad = ridx.copy()
        bad[1, 3] = wrong
        out = gradient(x, bg, bad, t, w1, b1, w2)
        assert np.isnan(out["phi"][1]).all() and np.isnan(out["var"][1]).all()
        for b in (0, 2):
            assert np.array_equal(bits(out["phi"][b]), bits(clean["phi"][b]))
            assert np.array_equal(bits(out["var"][b]), bits(clean["var"][b]))


def test_refusals_return_their_code_and_write_nothing():
    case = R.OPS_CASES[0]
    B, N, K, D, H, C = case
    (x, bg, w1, b1, w2, _), (ridx, t) = R.ops_inputs(case)
    for dims in [(0, N, K, D, H, C), (B, 0, K, D, H, C), (B, N, 0, D, H, C), (B, N, 4097, D, H, C), (B, N, K, 0, H, C),
                 (B, N, K, 4097, H, C), (B, N, K, D, 0, C), (B, N, K, D, 257, C), (B, N, K, D, H, 0), (B, N, K, D, H, 9)]:
        gradient(x, bg, ridx, t, w1, b1, w2, expect=ERR_SHAPE, dims=dims)
        assert b"shap_gradient" in L.lib().ecgmm_last_error()
    for dims in [(0, N, D, H, C), (B, 0, D, H, C), (B, 4097, D, H, C), (B, N, 0, H, C), (B, N, 4097, H, C),
                 (B, N, D, 257, C), (B, N, D, H, 9)]:
        deep(x, bg, w1, b1, w2, expect=ERR_SHAPE, dims=dims)
        assert b"shap_deep" in L.lib().ecgmm_last_error()
    gradient(x, bg, ridx, t, w1, b1, w2, expect=ERR_WORKSPACE, ws_short=1)
    deep(x, bg, w1, b1, w2, expect=ERR_WORKSPACE, ws_short=1)
    assert b"workspace" in L.lib().ecgmm_last_error()
