"""The three filtfilt entry points -- ecgmm_signal_filter_zscore (csrc/physionet.hip), ecgmm_signal_preprocess and
ecgmm_signal_preprocess_i16 (csrc/preprocess.hip) -- against the long-double reference and the bound of tests/iir_ref.py, at
every order and cutoff of its grid, at the production shapes, at the edges of the chunking and at the boundary between the
LDS-resident and the workspace route.

All calls go through the C ABI with b, a and zi from scipy.  Outputs are NaN-filled between sentinel zones
(tests/lstm_abi.Arena) and the preprocess workspace is handed over at exactly the reported size, followed by sentinels.  A
case of the grid that is not refusable (iir_ref) must be served and must meet the bound; a refusable one may instead be refused
on the host with rc 1, a message naming order and coefficients, and an untouched output.  Every test prints its worst
err / bound (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal
import torch

from ecgmm import preprocess as PP
from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr, stream

from . import iir_ref as R
from . import lstm_abi
from . import ptbxl_util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DESIGNS = R.designs()
LOW = [d for d in DESIGNS if d.kind == "low"]


def _dbl(v):
    return (C.c_double * len(v))(*[float(t) for t in v])


def _zi(b, a):
    return np.zeros(len(a) - 1) if not np.any(np.asarray(a)[1:]) and not np.any(np.asarray(b)[1:]) else scipy.signal.lfilter_zi(b, a)


def _finish(rc, ar, refused_ok, what):
    torch.cuda.synchronize()
    assert not ar.touched(), "%s: written outside the output, next to: %s" % (what, ar.touched())
    out = ar.views["out"]
    if rc != 0:
        msg = L.lib().ecgmm_last_error().decode()
        assert bool(torch.isnan(out).all()), "%s: a refused call wrote to its output" % what
        assert refused_ok and rc == 1, "%s: refused (rc %d: %s)" % (what, rc, msg)
        return None, msg
    got = out.cpu().numpy()
    return got, None


def fz(x32, b, a, zscore=False, eps=1e-8, refused_ok=False, order=None, zi=None):
    """ecgmm_signal_filter_zscore -> (fp32 numpy or None when refused, message)"""
    x = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DEV)
    ar = lstm_abi.Arena({"out": tuple(x.shape)})
    zi = _zi(b, a) if zi is None else zi
    rc = L.lib().ecgmm_signal_filter_zscore(ptr(x), ptr(ar.views["out"]), x.shape[0], x.shape[1], _dbl(b), _dbl(a), _dbl(zi),
                                            len(a) - 1 if order is None else order, int(zscore), eps, stream())
    return _finish(rc, ar, refused_ok, "signal_filter_zscore")


def pre(x32, window, b, a, mean=None, scale=None, refused_ok=False, order=None, zi=None):
    """ecgmm_signal_preprocess with the workspace at exactly the reported size"""
    x = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DEV)
    S, Ln = x.shape
    n = len(a) - 1 if order is None else order
    ar = lstm_abi.Arena({"out": (S, Ln)})
    nb = L.lib().ecgmm_signal_preprocess_workspace(S, Ln, max(1, min(n, 7)))
    assert nb > 0 and nb % 4 == 0
    ws = lstm_abi.guarded_bytes(nb)
    sm = None if mean is None else torch.from_numpy(np.asarray(mean, dtype=np.float32)).to(DEV)
    ss = None if scale is None else torch.from_numpy(np.asarray(scale, dtype=np.float32)).to(DEV)
    zi = _zi(b, a) if zi is None else zi
    rc = L.lib().ecgmm_signal_preprocess(ptr(x), ptr(ar.views["out"]), S, Ln, ptr(sm), ptr(ss), window, _dbl(b), _dbl(a),
                                         _dbl(zi), n, ptr(ws), nb, stream())
    got = _finish(rc, ar, refused_ok, "signal_preprocess")
    assert not lstm_abi.tail_touched(ws), "signal_preprocess: written past the end of the workspace"
    return got


def i16(d, gain, base, window, b, a, refused_ok=False, order=None, out_len=None, step=1):
    """ecgmm_signal_preprocess_i16 on frames d [R, T, 1]"""
    R_, T, nsig = d.shape
    raw = torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
    g = torch.from_numpy(np.ascontiguousarray(gain[:, :1], dtype=np.float64)).to(DEV)
    bl = torch.from_numpy(np.ascontiguousarray(base[:, :1]).astype(np.int32)).to(DEV)
    out_len = -(-T // step) if out_len is None else out_len
    ar = lstm_abi.Arena({"out": (R_, 1, out_len)})
    rc = L.lib().ecgmm_signal_preprocess_i16(ptr(raw), R_, T, nsig, (C.c_int * 1)(0), 1, ptr(g), ptr(bl), step,
                                             ptr(ar.views["out"]), out_len, window, _dbl(b), _dbl(a), _dbl(_zi(b, a)),
                                             len(a) - 1 if order is None else order, stream())
    return _finish(rc, ar, refused_ok, "signal_preprocess_i16")


def judge(got, msg, r, design, what):
    """-> err / bound of a served case (0.0 for a legitimately refused one); asserts the contract of the module docstring"""
    if got is None:
        assert r.refusable, "%s: refused a case that must be served: %s" % (what, msg)
        assert str(design.N) in msg and ("%.6g" % design.a[1]) in msg, "%s: the refusal names neither order nor coefficients: %s" % (what, msg)
        print(f"{what}: refused ({msg})")
        return 0.0
    assert not np.isnan(got).any(), "%s: an element was not written" % what
    w = R.worst(got, r.ref, r.dseq)
    nl = R.lane_rule(design.a, r.ref.shape[-1] + 6 * (design.N + 1))
    print(f"{what}: err/bound {w:.3g} (d_seq {r.dseq:.3g}, refusable {r.refusable}, lanes {nl})")
    assert w <= 1.0, what
    return w


# ---------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", DESIGNS, ids=[d.name for d in DESIGNS])
def test_filter_zscore_grid(design):
    worst = 0.0
    for Ln in R.LENGTHS:
        n = R.length(design, Ln)
        salt = next(s for d, m, s in R.grid() if d.name == design.name and m == n)
        r = R.grid_ref(design, n, salt)
        got, msg = fz(r.x, design.b, design.a, refused_ok=r.refusable)
        worst = max(worst, judge(got, msg, r, design, f"filter_zscore {design.name} L={n}"))
    print(f"filter_zscore {design.name}: worst err/bound {worst:.3g}")


@pytest.mark.parametrize("design", [d for d in LOW if d.order <= 7], ids=[d.name for d in LOW if d.order <= 7])
def test_preprocess_grid(design):
    worst = 0.0
    for j, Ln in enumerate(R.LENGTHS):
        n = R.length(design, Ln)
        window = 3 if Ln == "min" else 200
        x = R.rows(n, 8100 + 10 * design.order + j)
        r = R.case_ref(design, x, window=window)
        got, msg = pre(x, window, design.b, design.a, refused_ok=r.refusable)
        worst = max(worst, judge(got, msg, r, design, f"preprocess {design.name} L={n} window={window}"))
    print(f"preprocess {design.name}: worst err/bound {worst:.3g}")


I16_DESIGNS = [d for d in LOW if d.order <= 7 and d.wn in (0.04, 0.32)]


@pytest.mark.parametrize("design", I16_DESIGNS, ids=[d.name for d in I16_DESIGNS])
def test_preprocess_i16_grid(design):
    worst = 0.0
    for Ln in (250, 1000):
        d, gain, base = ptbxl_util.make_frames(900 + Ln + design.order, 3, Ln, 1)
        p = (d[:, :, 0].astype(np.float64) - base[:, :1]) / gain[:, :1]           # wfdb's p_signal, exact inputs of the kernel
        r = R.case_ref(design, None, window=200, x64=p)
        got, msg = i16(d, gain, base, 200, design.b, design.a, refused_ok=r.refusable)
        worst = max(worst, judge(None if got is None else got[:, 0], msg, r, design, f"preprocess_i16 {design.name} L={Ln}"))
    print(f"preprocess_i16 {design.name}: worst err/bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# production shapes
# ---------------------------------------------------------------------------------------------------------------------
def _records(S, Ln, salt):
    x = R.fill.hash_tensor((S, Ln), salt, 1.0).numpy().astype(np.float64)
    t = np.arange(Ln) / 300.0
    x += 0.8 * np.exp(8.0 * (np.cos(2 * np.pi * 1.2 * t) - 1.0)) + 0.3 * np.sin(2 * np.pi * 0.4 * t)   # beats + wander
    return x.astype(np.float32)


@pytest.mark.parametrize("zscore", [False, True])
@pytest.mark.parametrize("Ln", [3000, 9000, 18000])
def test_physionet_band_pass(Ln, zscore):
    design = R.find("band4_wide")
    x = _records(3, Ln, 500 + Ln)
    x[1, Ln - Ln // 10:] = 0.0          # a zero-padded short record
    r = R.case_ref(design, x, zscore=zscore)       # the bound is evaluated on the z-scored reference
    assert not r.refusable
    got, msg = fz(x, design.b, design.a, zscore=zscore)
    judge(got, msg, r, design, f"band-pass L={Ln} zscore={zscore}")


def test_default_low_pass_256x5000_with_scaler():
    design = R.find("low5_wn0.1")
    S, Ln = 256, 5000
    x = R.fill.hash_tensor((S, Ln), 909, 1.5).numpy().astype(np.float64) + 0.5 * np.cos(np.arange(Ln) / 11.0)
    x32 = x.astype(np.float32)
    mean = (0.1 * R.fill.hash_uniform(Ln, 910)).astype(np.float32)
    scale = (1.0 + 0.3 * np.abs(R.fill.hash_uniform(Ln, 911))).astype(np.float32)
    xs = ((x32.astype(R.LD) - mean.astype(R.LD)) / scale.astype(R.LD)).astype(np.float64)
    r = R.case_ref(design, None, window=200, x64=xs)
    assert not r.refusable
    got, msg = pre(x32, 200, design.b, design.a, mean=mean, scale=scale)
    judge(got, msg, r, design, "default low-pass [256, 5000] with a scaler")
    # the Python wrapper, with its own filter design, is held to the same bound
    via = PP.preprocess_signal(torch.from_numpy(x32).to(DEV), scaler_mean=mean, scaler_scale=scale).cpu().numpy()
    judge(via, None, r, design, "preprocess_signal wrapper [256, 5000]")


def test_default_low_pass_2476():
    design = R.find("low5_wn0.32")                 # 40 Hz at 250 Hz, the PTB-XL trainer's filter
    x = R.rows(2476, 2476, n=5)
    r = R.case_ref(design, x, window=200)
    got, msg = pre(x, 200, design.b, design.a)
    judge(got, msg, r, design, "low-pass 40 / 125 at L=2476")
    design = R.find("low5_wn0.1")
    r = R.case_ref(design, x, window=200)
    got, msg = pre(x, 200, design.b, design.a)
    judge(got, msg, r, design, "default low-pass at L=2476")


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 2, 199, 200, 777])
def test_windows(window):
    design = R.find("low5_wn0.1")
    x = R.rows(777, 60 + window)
    r = R.case_ref(design, x, window=window)
    got, msg = pre(x, window, design.b, design.a)
    judge(got, msg, r, design, f"window {window} of L=777")
    if window == 1:
        assert np.all(got == 0.0) and np.all(r.ref == 0.0)        # x - x: exactly +0 or -0


# E = L + 36 at order 5.  92: ceil(E / 64) = 2 even, C = 3, 43 chunks (idle lanes), the last one partial.  156: ceil = 3 odd, 64
# full chunks.  157: ceil = 4, C = 5, 39 chunks, partial.  1201: C = 21, 59 chunks, partial.  28 = 64 - 36: E = 64, C = 1.
@pytest.mark.parametrize("Ln", [28, 92, 156, 157, 1201])
def test_chunk_edges(Ln):
    design = R.find("low5_wn0.1")
    x = R.rows(Ln, 70 + Ln, n=6)
    x[2] = 0.75                       # constant
    x[3] = 0.0                        # all zero
    x[4, Ln // 2:] = 0.0              # zero-padded behind a record
    window = min(50, Ln)
    r = R.case_ref(design, x)
    got, msg = fz(x, design.b, design.a)
    judge(got, msg, r, design, f"filter_zscore L={Ln} with constant / zero / padded rows")
    assert np.all(got[3] == 0.0)
    r = R.case_ref(design, x, window=window)
    got, msg = pre(x, window, design.b, design.a)
    judge(got, msg, r, design, f"preprocess L={Ln} window={window} with constant / zero / padded rows")
    assert np.all(got[3] == 0.0)


def test_one_row_equals_row_0_of_70():
    for design in (R.find("low5_wn0.1"), R.find("band4_wide"), R.find("low5_wn0.02")):
        x = R.rows(1000, 33, n=70)
        all70, _ = fz(x, design.b, design.a)
        one, _ = fz(x[:1], design.b, design.a)
        assert np.array_equal(one[0].view(np.uint32), all70[0].view(np.uint32)), design.name
        if design.kind == "low":
            all70, _ = pre(x, 200, design.b, design.a)
            one, _ = pre(x[:1], 200, design.b, design.a)
            assert np.array_equal(one[0].view(np.uint32), all70[0].view(np.uint32)), design.name


def test_identity_filter():
    one = np.array([1.0, 0.0])
    x = R.rows(1000, 44, n=4)
    got, _ = fz(x, one, one)
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))          # the fp32 input, bit for bit
    y = PP.remove_baseline_drift(torch.from_numpy(x).to(DEV)).cpu().numpy()
    ref = R.baseline_ld(x, 200)
    x64 = x.astype(np.float64)
    f64 = np.stack([r - np.convolve(r, np.ones(200) / 200, mode="same") for r in x64])
    dseq = float(np.abs(f64.astype(R.LD) - ref).max())
    w = R.worst(y, ref.astype(np.float64), dseq)
    print(f"remove_baseline_drift: err/bound {w:.3g}")
    assert w <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the boundary between the two routes of ecgmm_signal_preprocess
# ---------------------------------------------------------------------------------------------------------------------
def test_route_boundary():
    """order 5: L = 9934 is the last LDS-resident length, (2 * 9934 + 36 + 576) * 8 = 163840 bytes = 160 KiB exactly;
    L = 9935 is the first that takes the workspace kernel (S = 70: the second workgroup of 64 lanes is partial)"""
    design = R.find("low5_wn0.1")
    for S, Ln in ((2, 9934), (70, 9935)):
        x = R.rows(Ln, 9000 + S, n=S)
        r = R.case_ref(design, x, window=200)
        got, msg = pre(x, 200, design.b, design.a)
        judge(got, msg, r, design, f"preprocess [{S}, {Ln}]")


# ---------------------------------------------------------------------------------------------------------------------
# refusals write nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    design = R.find("low5_wn0.1")
    b, a = design.b, design.a
    nine = scipy.signal.butter(9, 0.3)
    x = R.rows(300, 5)
    frames = ptbxl_util.make_frames(17, 2, 300, 1)
    bad_a = a.copy()
    bad_a[0] = 2.0
    z5 = np.zeros(5)

    def refused(res, word):
        got, msg = res
        assert got is None and word in msg, (word, msg)

    refused(fz(x, b, a, order=0, refused_ok=True), "order")
    refused(fz(x, nine[0], nine[1], refused_ok=True), "order")
    refused(fz(x, b, bad_a, zi=z5, refused_ok=True), "a[0]")
    refused(fz(x[:, :18], b, a, refused_ok=True), "padlen")
    refused(pre(x, 200, b, a, order=0, refused_ok=True), "order")
    refused(pre(x, 200, nine[0], nine[1], refused_ok=True), "order")
    refused(pre(x, 200, b, bad_a, zi=z5, refused_ok=True), "a[0]")
    refused(pre(x[:, :18], 3, b, a, refused_ok=True), "3*(order+1)")
    refused(pre(x[:, :150], 200, b, a, refused_ok=True), "window")
    refused(i16(*frames, 200, b, a, order=0, refused_ok=True), "order")
    refused(i16(*frames, 200, nine[0], nine[1], refused_ok=True), "order")
    refused(i16(*frames, 200, b, bad_a, refused_ok=True), "a[0]")
    refused(i16(frames[0][:, :18], frames[1], frames[2], 3, b, a, refused_ok=True), "3*(order+1)")
    refused(i16(frames[0][:, :150], frames[1], frames[2], 200, b, a, refused_ok=True), "window")
