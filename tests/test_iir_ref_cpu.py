"""tests/iir_ref.py without a GPU: the long-double filtfilt against scipy on every design of the grid, the cap on refusable
cases, and the teeth of the bound -- the float64 restatement of the 64-lane chunk scheme must fail it on the narrow-band
designs and pass on the defaults, three wrong variants must fail at the default design -- and the lane rule: its restatement
equals the library's, and the scheme at the lanes it picks meets the bound on every case that must be served.
Every test prints the figures it asserts on (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from ecgmm.hip import lib as L

from . import iir_ref as R


def _case(name, Ln):
    for d, n, salt in R.grid():
        if d.name == name and n == Ln:
            return d, n, salt
    raise KeyError((name, Ln))


def _scheme(d, x32, nl):
    return R.chunk_scheme_f64(d.b, d.a, scipy.signal.lfilter_zi(d.b, d.a), np.asarray(x32, dtype=np.float64), nl)


def test_long_double_filtfilt_against_scipy_on_the_grid_and_the_cap():
    grid = R.grid()
    assert len(grid) == 156
    refusable, worst = [], 0.0
    for d, Ln, salt in grid:
        r = R.grid_ref(d, Ln, salt)
        assert np.isfinite(r.ref).all() and r.ref.shape == (3, Ln)
        if r.refusable:
            refusable.append("%s L=%d" % (d.name, Ln))
            continue
        rel = r.dseq / np.abs(r.ref).max()
        worst = max(worst, rel)
        assert rel <= 1e-9, (d.name, Ln, rel)
    print(f"grid: worst d_seq / max|ref| over the {len(grid) - len(refusable)} cases that must be served {worst:.3g}; "
          f"{len(refusable)} refusable: {refusable}")
    assert 5 * len(refusable) <= len(grid)          # the cap: at most one fifth


def test_baseline_and_zscore_against_numpy():
    for Ln, window in ((250, 200), (251, 3), (200, 200), (777, 199), (64, 1), (65, 2)):
        x = R.rows(Ln, 31 + Ln).astype(np.float64)
        want = np.stack([r - np.convolve(r, np.ones(window) / window, mode="same") for r in x])
        got = R.baseline_ld(x, window).astype(np.float64)
        err = np.abs(got - want).max()
        print(f"baseline_ld L={Ln} window={window}: max |diff| to numpy {err:.3g}")
        assert err <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(x).max())       # numpy's own summation of <= 200 terms
    assert np.all(R.baseline_ld(R.rows(64, 5), 1) == 0)
    y = R.rows(1000, 77).astype(np.float64) * 3.0 + 1.5
    want = (y - y.mean(-1, keepdims=True)) / (y.std(-1, keepdims=True) + 1e-8)
    err = np.abs(R.zscore_ld(y).astype(np.float64) - want).max()
    print(f"zscore_ld: max |diff| to numpy {err:.3g}")
    assert err <= 64 * np.finfo(np.float64).eps * np.abs(want).max()
    assert np.all(R.zscore_ld(np.zeros((2, 50))) == 0)                                # 0 / (0 + eps)


FAILS_TODAY = [("low5_wn0.02", 1000), ("low5_wn0.02", 5000), ("low6_wn0.04", 1000), ("low6_wn0.04", 5000),
               ("low8_wn0.1", 1000), ("band3_narrow", 1000), ("band3_narrow", 5000)]


@pytest.mark.parametrize("name,Ln", FAILS_TODAY)
def test_the_64_lane_scheme_fails_the_bound_on_narrow_designs(name, Ln):
    d, Ln, salt = _case(name, Ln)
    r = R.grid_ref(d, Ln, salt)
    assert not r.refusable
    w64 = R.worst(_scheme(d, r.x, 64), r.ref, r.dseq)
    w1 = R.worst(_scheme(d, r.x, 1), r.ref, r.dseq)
    print(f"{name} L={Ln}: 64 lanes err/bound {w64:.3g}, sequential {w1:.3g}")
    assert w64 > 1.0          # the bound has teeth: the scheme as it stood is caught
    assert w1 <= 1.0          # and the sequential pass of the same restatement is not


PASSES_TODAY = [("low5_wn0.1", Ln) for Ln in (250, 1000, 5000)] + [("low5_wn0.32", Ln) for Ln in (250, 1000, 5000)]


@pytest.mark.parametrize("name,Ln", PASSES_TODAY)
def test_the_64_lane_scheme_passes_at_the_default_low_pass(name, Ln):
    d, Ln, salt = _case(name, Ln)
    r = R.grid_ref(d, Ln, salt)
    w = R.worst(_scheme(d, r.x, 64), r.ref, r.dseq)
    print(f"{name} L={Ln}: 64 lanes err/bound {w:.3g}")
    assert not r.refusable and w <= 1.0


def test_the_64_lane_scheme_passes_at_the_production_band_pass():
    d = R.find("band4_wide")
    x = R.rows(3000, 4242)
    r = R.case_ref(d, x)
    w = R.worst(_scheme(d, x, 64), r.ref, r.dseq)
    print(f"band-pass order 4 on [16/150, 149/150], L=3000: 64 lanes err/bound {w:.3g}")
    assert not r.refusable and w <= 1.0


def test_three_wrong_variants_fail_at_the_default_design():
    d = R.find("low5_wn0.1")
    x = R.rows(1000, 99)
    r = R.case_ref(d, x, window=200)
    u = R.baseline_ld(x, 200).astype(np.float64)
    right = R._filtfilt(d.b, d.a, u, np.float64)
    variants = {
        "extension reflected one sample off": R._filtfilt(d.b, d.a, u, np.float64, ext_shift=1),
        "backward pass started from zi * x[0]": R._filtfilt(d.b, d.a, u, np.float64, back_state_from_input=True),
        "'same' window shifted by one": R._filtfilt(d.b, d.a, R.baseline_ld(x, 200, shift=1).astype(np.float64), np.float64),
    }
    w0 = R.worst(right, r.ref, r.dseq)
    print(f"float64 restatement err/bound {w0:.3g}")
    assert w0 <= 1.0
    for what, y in variants.items():
        w = R.worst(y, r.ref, r.dseq)
        print(f"{what}: err/bound {w:.3g}")
        assert w > 1.0, what


def test_ratio_convention():
    assert R.ratio(np.array([0.0, 1.0]), np.array([0.0, 2.0])) == 0.5
    assert R.ratio(np.array([1e-300]), np.array([0.0])) == float("inf")          # a zero bound means exact
    assert R.ratio(np.array([float("nan")]), np.array([1.0])) == float("inf")
    assert R.ratio(np.array([]), np.array([])) == 0.0


def test_lane_rule_restatement_equals_the_library_and_serves_the_grid():
    """the rule is a pure host function of (a, E): the library's answer without a GPU, its restatement, and the float64 scheme
    at the chosen lanes against the bound on every case that must be served"""
    lib = L.lib()
    chosen, worst, worst_at = {}, 0.0, None
    for d, Ln, salt in R.grid():
        nl = R.lane_rule(d.a, Ln + 6 * (d.N + 1))
        got = lib.ecgmm_signal_filter_lanes((C.c_double * len(d.a))(*d.a), d.N, Ln)
        assert got == nl, (d.name, Ln, got, nl)
        chosen.setdefault(d.name, []).append(nl)
        r = R.grid_ref(d, Ln, salt)
        w = R.worst(_scheme(d, r.x, nl), r.ref, r.dseq)
        if not r.refusable:
            assert w <= 1.0, (d.name, Ln, nl, w)
            if w > worst:
                worst, worst_at = w, (d.name, Ln, nl)
    print("lanes per design at L = min, 250, 1000, 5000:", chosen)
    print(f"worst err/bound of the scheme at the chosen lanes over the cases that must be served: {worst:.3g} at {worst_at}")
    for name in ("low5_wn0.1", "low5_wn0.32"):
        assert chosen[name] == [64, 64, 64, 64]           # the defaults keep all 64 lanes: the bits of before
    assert lib.ecgmm_signal_filter_lanes((C.c_double * 2)(1.0, 0.0), 1, 5000) == 64            # the identity filter
    assert lib.ecgmm_signal_filter_lanes((C.c_double * 2)(2.0, 0.0), 1, 5000) == 0 and b"a[0]" in lib.ecgmm_last_error()
    assert lib.ecgmm_signal_filter_lanes(None, 1, 5000) == 0
    assert lib.ecgmm_signal_filter_lanes((C.c_double * 2)(1.0, 0.0), 9, 5000) == 0
