"""The entry points of csrc/lime.hip through ctypes against tests/lime_ref.py, within the bounds of tests/lime_bounds.py.

Every output is a 0xFF-filled view (NaN for floats, 255 / -1 for integers) into one byte arena with a zone of sentinel bytes
before and after it, checked after every call; the ridge workspace has exactly the size the library reports and is followed
by sentinels.  Worst measured ratios on the MI355X are recorded in DESIGN.md section 21."""
import numpy as np
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream
from ecgmm.lime_tabular import QuartileDiscretizer

from . import lime_bounds as Bd
from . import lime_ref as R
from .lime_ref import SEED, crafted_background

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENT, ERR_SHAPE = 1024, 0xA5, 1
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
    return {k: v.cpu().numpy() for k, v in ar.views.items()}


# ------------------------------------------------------------------------------------------------------------------
# perturbation
# ------------------------------------------------------------------------------------------------------------------
def background(D):
    """the crafted columns of tests/test_lime_cpu.py (tied quartiles, a constant column, an empty bin) in the first five
    positions, hash-free normal columns of different location and scale behind them"""
    rng = np.random.default_rng(17)
    c = crafted_background()
    bg = rng.normal(size=(c.shape[0], D)) * rng.uniform(0.05, 3.0, size=D) + rng.normal(size=D)
    bg[:, :5] = c
    return bg.astype(np.float32)


def perturb(x, tab, N, b0, offset, uniforms=True, expect=0, S=None, D=None):
    B = x.shape[0]
    D = x.shape[1] if D is None else D
    S = tab["cdf"].shape[1] if S is None else S
    Dd = x.shape[1]
    shapes = {"Z": ("u8", (B, N, Dd)), "inverse": ("f32", (B, N, Dd)), "d2": ("i32", (B, N))}
    if uniforms:
        shapes["u"] = ("f64", (B, N, Dd, 2))
    x_ = torch.from_numpy(x).to(DEV)
    return call("ecgmm_lime_perturb", shapes,
                lambda v: (ptr(x_), ptr(tab["qts"]), ptr(tab["cdf"]), ptr(tab["stats"]), ptr(tab["lim"]), ptr(tab["nbins"]),
                           S, B, b0, N, D, SEED, offset, ptr(v["Z"]), ptr(v["inverse"]), ptr(v["d2"]), ptr(v.get("u"))),
                expect=expect)


def value_ratio(got, uv, mean, std, lo, hi, lo32, hi32):
    """worst |value - reference| / bound over EVERY element given (bare-std bins included: their reference is the mean)"""
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)
    got, uv, mean, std, lo, hi, lo32, hi32 = (flat(a) for a in (got, uv, mean, std, lo, hi, lo32, hi32))
    ref, z = R.truncnorm_value(uv, mean, std, lo, hi)
    assert np.isfinite(ref).all()
    live = std > 1e-11                       # a bare bin's mean may lie outside its own limits only when it is empty
    assert (ref[live] >= lo[live]).all() and (ref[live] <= hi[live]).all()
    ref = np.where(live, ref, np.clip(ref, lo, hi))
    bound = Bd.value_bound(ref, np.where(live, z, 0.0), mean, std, lo, hi, clamped=(got == lo32) | (got == hi32))
    return Bd.ratio(np.abs(got.astype(np.float64) - ref), bound), got.size


@pytest.mark.parametrize("B,N,D", [(3, 37, 21), (2, 130, 65), (1, 1000, 768)])
def test_perturb(B, N, D):
    bg = background(D)
    disc = QuartileDiscretizer(bg)
    host, tab = disc.host_table(), disc.table(DEV)
    assert any((c == 0).any() for c in disc.bin_counts), "the table must hold a bin of zero frequency"
    x = bg[3:3 + B].copy()
    x[:, 5:] += 0.01
    b0, offset = 5, (7 << 32) | 9
    out = perturb(x, tab, N, b0, offset)
    Z, inv, d2, u = out["Z"], out["inverse"], out["d2"], out["u"]
    # the uniforms: bit-equal to the numpy Philox at the documented counters
    bb, nn, ff = np.meshgrid(np.arange(B) + b0, np.arange(N), np.arange(D), indexing="ij")
    ub, uv = R.perturb_uniforms(SEED, offset, bb, nn, ff)
    assert np.array_equal(u[..., 0], ub) and np.array_equal(u[..., 1], uv)
    # bins by the float64 rule, Z, d2 and row 0
    bins = R.draw_bins(u[..., 0], host["cdf"], host["nbins"])
    xb = disc.discretize(x)
    want_Z = (bins == xb[:, None, :]).astype(np.uint8)
    want_Z[:, 0] = 1
    assert np.array_equal(Z, want_Z)
    assert np.array_equal(d2, (want_Z == 0).sum(2))
    assert np.array_equal(inv[:, 0], x)
    f = np.broadcast_to(np.arange(D), bins.shape)
    counts = np.zeros(host["cdf"].shape, dtype=np.int64)
    for j, c in enumerate(disc.bin_counts):
        counts[j, :len(c)] = c
    assert (counts[f, bins][:, 1:] > 0).all(), "a bin of zero frequency was drawn"
    # values: inside the bin's fp32 limits, and within the derived bound of scipy's truncated normal
    sel = (slice(None), slice(1, None))
    bn, fn_ = bins[sel], f[sel]
    mean, std, lo, hi = (host["stats"][i][fn_, bn] for i in range(4))
    lo32, hi32 = host["lim"][0][fn_, bn], host["lim"][1][fn_, bn]
    got = inv[sel]
    assert (got >= lo32).all() and (got <= hi32).all()
    bare = std <= 1e-11
    assert bare.any() and np.array_equal(got[bare], np.clip(mean[bare].astype(np.float32), lo32[bare], hi32[bare]))
    r, count = value_ratio(got, uv[sel], mean, std, lo, hi, lo32, hi32)
    print("perturb [%d, %d, %d]: worst |value - truncnorm.ppf| / bound %.3g over all %d values" % (B, N, D, r, count))
    assert r <= 1.0 and count == B * (N - 1) * D
    # one call with B rows == B calls with one row each, bit for bit; without u_out the rest is unchanged
    for b in range(B):
        one = perturb(x[b:b + 1], tab, N, b0 + b, offset, uniforms=False)
        assert np.array_equal(one["Z"][0], Z[b]) and np.array_equal(one["d2"][0], d2[b])
        assert np.array_equal(one["inverse"][0].view(np.uint32), inv[b].view(np.uint32))


def test_perturb_tail_and_point_bins_of_a_hand_built_table():
    """Bins no QuartileDiscretizer produces, which the kernel still has to get right: an interval wholly above its mean
    (a > 0: drawn from the mirrored interval), wholly below it (b < 0), far in either tail, and min == max with a real std
    (a == b: the common point).  D = 300 runs the strided feature loop; feature f uses row f % 6 of the table."""
    rows = [  # mean, std, min, max
        (0.0, 1.0, 2.0, 4.0), (0.0, 1.0, -4.0, -2.0), (1.5, 0.25, 3.5, 4.0), (-2.0, 3.0, -30.0, -20.0),
        (0.3, 2.0, 1.7, 1.7), (5.0, 0.5, 4.0, 7.0)]
    D, S, N, B = 300, 2, 64, 2
    t = np.array(rows)[np.arange(D) % len(rows)]                      # [D, 4]
    stats = np.zeros((4, D, S))
    stats[:, :, 0] = t.T
    stats[:, :, 1] = t.T                                              # bin 1 has no mass: never drawn
    host = {"qts": np.zeros((D, S)), "cdf": np.ones((D, S)), "stats": stats, "lim": stats[2:4].astype(np.float32),
            "nbins": np.full(D, 2, dtype=np.int32)}
    host["qts"][:, 0] = 1e30                                          # every x falls in bin 0
    tab = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in host.items()}
    x = np.zeros((B, D), dtype=np.float32)
    out = perturb(x, tab, N, 0, 3)
    assert (out["Z"] == 1).all() and (out["d2"] == 0).all() and np.array_equal(out["inverse"][:, 0], x)
    got, uv = out["inverse"][:, 1:], out["u"][:, 1:, :, 1]
    full = lambda i: np.broadcast_to(stats[i, :, 0], got.shape)
    lo32, hi32 = (np.broadcast_to(host["lim"][i][:, 0], got.shape) for i in range(2))
    assert (got >= lo32).all() and (got <= hi32).all()
    point = np.broadcast_to(np.arange(D) % len(rows) == 4, got.shape)
    assert (got[point] == np.float32(1.7)).all()
    r, count = value_ratio(got, uv, full(0), full(1), full(2), full(3), lo32, hi32)
    print("perturb, hand-built tail / point bins: worst ratio %.3g over %d values" % (r, count))
    assert r <= 1.0


def test_perturb_refuses_bad_shapes():
    bg = background(21)
    tab = QuartileDiscretizer(bg).table(DEV)
    x = bg[:2]
    for kw in (dict(D=0), dict(D=4097), dict(S=0), dict(S=17), dict(N=0), dict(b0=-1), dict(b0=1 << 18)):
        a = dict(N=8, b0=0)
        a.update(kw)
        perturb(x, tab, a.pop("N"), a.pop("b0"), 0, expect=ERR_SHAPE, **a)


# ------------------------------------------------------------------------------------------------------------------
# ridge
# ------------------------------------------------------------------------------------------------------------------
def ridge(Z, d2, y, kw, alpha, cols=None, expect=0, K=None, Lr=None):
    B, N, D = Z.shape
    Lr = y.shape[1] if Lr is None else Lr
    K = (D if cols is None else cols.shape[1]) if K is None else K
    Ko = D if cols is None else cols.shape[1]
    nb = L.lib().ecgmm_lime_ridge_workspace(B, N, D)
    assert nb > 0 and nb % 4 == 0
    ws = torch.full((nb + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[nb:] = SENT
    Z_, d2_, y_ = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (Z, d2, y))
    c_ = None if cols is None else torch.from_numpy(np.ascontiguousarray(cols.astype(np.int32))).to(DEV)
    shapes = {"coef": ("f32", (B, y.shape[1], Ko)), "intercept": ("f32", (B, y.shape[1])), "w": ("f32", (B, N)),
              "score": ("f32", (B, y.shape[1])), "local_pred": ("f32", (B, y.shape[1]))}
    out = call("ecgmm_lime_ridge", shapes,
               lambda v: (ptr(Z_), ptr(d2_), ptr(y_), ptr(c_), B, N, D, K, Lr, kw, alpha, ptr(v["coef"]), ptr(v["intercept"]),
                          ptr(v["w"]), ptr(v["score"]), ptr(v["local_pred"]), ptr(ws), nb), expect=expect)
    assert bool((ws[nb:] == SENT).all()), "written past the end of the workspace"
    return out


def ridge_inputs(B, N, D, Lr=2, bins=4):
    parts = [R.ridge_case(N, D, Lr, bins, seed=100 + b) for b in range(B)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


@pytest.mark.parametrize("B,N,D,K", [(3, 37, 21, None), (2, 64, 64, None), (2, 130, 65, None), (2, 1000, 768, None),
                                     (2, 130, 65, 17), (1, 40, 1100, 17)])
def test_ridge(B, N, D, K):
    Z, d2, y = ridge_inputs(B, N, D)
    kw, alpha = 0.75 * np.sqrt(D), 1.0
    cols = None
    if K is not None:   # kept columns: the all-ones column 1, the duplicated pair 2, 3 and a different random rest per sample
        rng = np.random.default_rng(3)
        cols = np.stack([np.sort(np.concatenate([[1, 2, 3], 4 + rng.permutation(D - 4)[:K - 3]])) for _ in range(B)])
    out = ridge(Z, d2, y, kw, alpha, cols)
    assert all(np.isfinite(v).all() for v in out.values())
    worst = {}
    for b in range(B):
        w64 = R.kernel_weights(d2[b], kw)
        worst["w"] = max(worst.get("w", 0.0), Bd.ratio(np.abs(out["w"][b] - w64), Bd.weight_bound(w64, d2[b], kw)))
        Zb = Z[b] if cols is None else Z[b][:, cols[b]]
        ref = R.RidgeRef(Zb, out["w"][b], y[b], alpha)          # the system from the device's own Z, stored w and y
        sk_coef, sk_icpt, _ = R.sklearn_ridge(Zb.astype(np.float64), out["w"][b].astype(np.float64), y[b].astype(np.float64), alpha)
        assert np.abs(ref.beta - sk_coef).max() <= 1e-10 and np.abs(ref.intercept - sk_icpt).max() <= 1e-10
        one = 1 if cols is None else int(np.flatnonzero(cols[b] == 1)[0])
        assert (Zb[:, one] == 1).all() and (out["coef"][b][:, one] == 0.0).all()   # centred column zero: exactly 0
        dup = (2, 3) if cols is None else tuple(int(np.flatnonzero(cols[b] == c)[0]) for c in (2, 3))
        assert np.array_equal(Zb[:, dup[0]], Zb[:, dup[1]])
        got = Bd.ridge_ratios(ref, out["coef"][b].astype(np.float64), out["intercept"][b], out["score"][b], out["local_pred"][b])
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # the same system solved in numpy fp32 must sit inside the same forward bound: a bound that means something
        f32 = R.RidgeRef(Zb, out["w"][b], y[b], alpha, dtype=np.float32)
        own = Bd.ridge_ratios(ref, f32.beta, f32.intercept, f32.score, f32.local_pred)
        worst["numpy fp32 coef"] = max(worst.get("numpy fp32 coef", 0.0), own["coef"])
        assert all(v <= 1.0 for v in own.values()), own
    print("ridge [%d, %d, %d] K=%s worst ratios: %s" % (B, N, D, K, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_ridge_refuses_bad_shapes_and_indices():
    Z, d2, y = ridge_inputs(2, 37, 21)
    kw = 0.75 * np.sqrt(21)
    cols = np.tile(np.arange(5), (2, 1))
    ridge(Z, d2, y, kw, 1.0, expect=ERR_SHAPE, K=20)                     # K != D without cols
    ridge(Z, d2, y, kw, 1.0, cols, expect=ERR_SHAPE, K=22)               # K > D
    ridge(Z, d2, y, kw, 1.0, expect=ERR_SHAPE, Lr=9)
    ridge(Z, d2, y, kw, 0.0, expect=ERR_SHAPE)
    ridge(Z, d2, y, -1.0, 1.0, expect=ERR_SHAPE)
    bad = cols.copy()
    bad[1, 2] = 21                                                       # outside [0, D): never addressed, flagged NaN
    out = ridge(Z, d2, y, kw, 1.0, bad)
    assert np.isnan(out["coef"][1, :, 2]).all() and np.isfinite(np.delete(out["coef"][1], 2, axis=1)).all()
    assert np.isfinite(out["coef"][0]).all() and np.isfinite(out["intercept"]).all()


def test_prob_is_a_softmax_column():
    rng = np.random.default_rng(2)
    logits = (rng.normal(size=(1000, 3)) * 4).astype(np.float32)
    lg = torch.from_numpy(logits).to(DEV)
    ref = torch.softmax(torch.from_numpy(logits).double(), dim=1).numpy()
    out = call("ecgmm_lime_prob", {"p": ("f32", (1000, 2))}, lambda v: (ptr(lg), 1000, 3, 2, ptr(v["p"]), 2))
    assert np.abs(out["p"][:, 0] - ref[:, 2]).max() <= 8 * Bd.U          # expf, the sum of three, the divide
    assert np.isnan(out["p"][:, 1]).all()                                # the stride is respected
    call("ecgmm_lime_prob", {"p": ("f32", (1000,))}, lambda v: (ptr(lg), 1000, 3, 3, ptr(v["p"]), 1), expect=ERR_SHAPE)
