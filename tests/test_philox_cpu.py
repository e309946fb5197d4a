"""The five users of the device Philox4x32-10 stream cannot draw from one counter block under one seed, and the Python side
advances the stream by exactly what a dropout launch consumes.  No GPU: the counters are restated in tests/philox_ref.py,
the limits behind them are read off the library's own refusals (argument checks run on the host, before any launch).

Counter word c3 per user, with the limit that bounds it and where the library enforces it:
  dropout            c2 = c3 = 0; c0, c1 = offset + element group          csrc/head.hip dropout_fwd_kernel
  LIME               0x40000000 | b << 12 | f    D <= 4096, rows < 2^18     csrc/lime.hip ecgmm_lime_perturb (LIME_MAX_D, LIME_MAX_B)
  augmentation noise 0x80000000 | g              L <= 2^30 (g < 2^28)       csrc/physionet.hip ecgmm_signal_gather_augment
  attention          0xC0000000 | x              S <= 32768 (x < 2^28)      csrc/attention.hip mha_geo, ecgmm_mha_keep_mask
  decision tags      0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF                     csrc/physionet.hip (weighted sample, row decisions)

Callers in ecgmm/ that launch a dropout of n elements, each of which takes n from _PhiloxState (found by reading
hip/functional.py, hip/encoders.py and the plans they drive):
  hip/functional.py DropoutFn.forward     take(x.numel())        ecgmm_dropout_fwd(..., x.numel(), ...)
  hip/encoders.py ResNet1DSpec.make_desc  take(x.shape[0] * 64)  csrc/plan_resnet1d.hip: ecg_dropout_fwd(..., (long)N * 64, ...)
  hip/encoders.py HeadFn.forward          take(B * spec.hidden)  csrc/plan_head.hip: ecg_dropout_fwd(..., (long)B * H, ...), H = d->hidden
Every other take() in ecgmm/ asks for one offset for a kernel that puts the call's offset into c0, c1 unchanged (take(1),
take(4): one block either way)."""
import ctypes as C
import itertools
import os
import re

import numpy as np

import ecgmm.hip.functional as HF
from ecgmm.hip import lib as L

from . import philox_ref as P

PKG = os.path.dirname(os.path.dirname(os.path.abspath(HF.__file__)))
ERR_SHAPE = 1


def test_c3_ranges_are_pairwise_disjoint():
    r = P.c3_ranges()
    assert set(r) == {"dropout", "lime", "noise", "attention", "weighted_sample", "row_scale_shift", "row_flags"}
    for (a, (alo, ahi)), (b, (blo, bhi)) in itertools.combinations(r.items(), 2):
        assert alo <= ahi and blo <= bhi
        assert ahi < blo or bhi < alo, "%s [%#x, %#x] meets %s [%#x, %#x]" % (a, alo, ahi, b, blo, bhi)
    assert all(hi <= 0xFFFFFFFF for _, hi in r.values())
    # the ranges are what the counter functions give at the limits
    assert int(P.ctr_lime(0, 0, P.MAX_ROWS - 1, P.MAX_D - 1)[3]) == r["lime"][1] and int(P.ctr_lime(0, 0, 0, 0)[3]) == r["lime"][0]
    assert int(P.ctr_noise(0, 0, (P.MAX_L + 3) // 4 - 1)[3]) == r["noise"][1]
    SB = (P.MAX_S + 3) // 4
    assert int(P.ctr_attention(0, 0, (P.MAX_S - 1) * SB + (P.MAX_S - 1) // 4)[3]) == r["attention"][1]
    # the fields do not run into the tag bits: OR and + agree
    assert r["lime"][1] == 0x40000000 + ((P.MAX_ROWS - 1) << 12) + (P.MAX_D - 1) < 0x80000000
    assert r["noise"][1] == 0x80000000 + (P.MAX_L + 3) // 4 - 1 < 0xC0000000
    assert r["attention"][1] < P.TAG_SAMPLE


def test_dropout_alone_uses_c2_c3_zero():
    c = P.ctr_dropout(5, np.arange(8))
    assert c[2] == 0 and c[3] == 0
    for name, (lo, _) in P.c3_ranges().items():
        assert (lo == 0) == (name == "dropout")
    # the carry of offset + g into c1, and the wrap at 2^64
    lo, hi, _, _ = P.ctr_dropout(2 ** 32 - 2, np.arange(4))
    assert lo.tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1] and hi.tolist() == [0, 0, 1, 1]


def test_the_library_enforces_the_limits():
    lib = L.lib()
    dummy = C.c_void_p(16)
    err = lambda: lib.ecgmm_last_error()  # noqa: E731
    # L <= 2^30: csrc/physionet.hip, ecgmm_signal_gather_augment
    assert lib.ecgmm_signal_gather_augment(dummy, 4, P.MAX_L + 1, dummy, 8, dummy, None, 1, 0.5, 0.01, 0.8, 1.2, -10, 10, 1, 0,
                                           None) == ERR_SHAPE and b"2^30" in err()
    # S <= 32768: csrc/attention.hip, ecgmm_mha_keep_mask whatever p is; mha_geo (forward / backward) under dropout
    for p in (0.0, 0.1):
        d = L.MHADesc(P.MAX_S + 1, 1, 1, 16, 0, p)
        assert lib.ecgmm_mha_keep_mask(C.byref(d), dummy, 1, 0, None) == ERR_SHAPE and b"32768" in err()
    d = L.MHADesc(P.MAX_S + 1, 1, 1, 16, 0, 0.1)
    assert lib.ecgmm_mha_forward(C.byref(d), dummy, dummy, dummy, 1, 0, None) == ERR_SHAPE and b"32768" in err()
    # D <= 4096 and b0 + B <= 2^18: csrc/lime.hip, ecgmm_lime_perturb
    perturb = lambda B, b0, D: lib.ecgmm_lime_perturb(dummy, dummy, dummy, dummy, dummy, dummy, 4, B, b0, 10, D, 1, 0,  # noqa: E731
                                                      dummy, dummy, dummy, None, None)
    assert perturb(1, 0, P.MAX_D + 1) == ERR_SHAPE and b"4096" in err()
    assert perturb(1, P.MAX_ROWS, 8) == ERR_SHAPE and b"262144" in err()
    assert perturb(2, P.MAX_ROWS - 1, 8) == ERR_SHAPE


def test_take_advances_by_whole_counter_blocks():
    saved = (HF._PhiloxState.seed, HF._PhiloxState.offset)
    try:
        HF.manual_seed(1234)
        assert (HF._PhiloxState.seed, HF._PhiloxState.offset) == (1234, 0)
        at = 0
        for n in (1, 3, 4, 5, 10, 1023, 300001, 64 * 32):
            seed, off = HF._PhiloxState.take(n)
            assert (seed, off) == (1234, at)
            at += -(-n // 4)                                   # ceil(n / 4): the blocks a dropout of n elements consumes
            assert HF._PhiloxState.offset == at
    finally:
        HF._PhiloxState.seed, HF._PhiloxState.offset = saved


def _read(*parts):
    with open(os.path.join(PKG, *parts)) as f:
        return f.read()


def test_every_dropout_caller_takes_what_it_launches():
    """the take() sites of the package, by source: a new one, or one whose argument changes, makes this list stale"""
    found = []
    for root, _, files in os.walk(PKG):
        for name in sorted(files):
            if name.endswith(".py"):
                rel = os.path.relpath(os.path.join(root, name), PKG)
                for m in re.finditer(r"_PhiloxState\.take\(([^\n]*?)\)(?= if|\n|$)", _read(rel)):
                    found.append((rel.replace(os.sep, "/"), m.group(1)))
    assert sorted(found) == sorted([
        ("hip/functional.py", "x.numel()"),            # DropoutFn: n = x.numel()
        ("hip/encoders.py", "x.shape[0] * 64"),        # ResNet1DSpec: the plan drops N * 64 features
        ("hip/encoders.py", "B * spec.hidden"),        # HeadFn: the plan drops B * hidden activations
        ("hip/functional.py", "4"),                    # lime_perturb: one offset
        ("hip/functional.py", "4"),                    # MultiHeadAttentionFn: one offset
        ("preprocess.py", "1"),                        # weighted_sample: one offset
        ("preprocess.py", "1"),                        # gather_augment: one offset
        ("lime_tabular.py", "4"),                      # the explainer's own offset
    ]), found
    # ... and the launches behind the three dropout callers have those sizes
    fn = _read("hip", "functional.py")
    assert "ecgmm_dropout_fwd(ptr(x), ptr(y), ptr(mask), x.numel(), p, seed, off, stream())" in fn
    r1d = _read("csrc", "plan_resnet1d.hip")
    assert "ecg_dropout_fwd(w.h1, w.hd, w.dmask, (long)N * 64, r.d.dropout_p, r.d.seed, r.d.offset, s)" in r1d
    head = _read("csrc", "plan_head.hip")
    assert head.count("ecg_dropout_fwd(w.h, w.hd, w.mask, (long)B * H, d->dropout_p, d->seed, d->offset, s)") == 2
    assert head.count("ecg_dropout_fwd(") == 2 and "H = d->hidden" in head
