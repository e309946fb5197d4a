"""The float64 checks under every start-up-only switch's other value: one child process per leg of tests/startup_legs.py.

Twelve ECGMM_* switches are read once per process (csrc/switches.h, runtime == false); this process, started without them,
runs their default side only.  Each test below starts `python -m tests.startup_legs NAME` with the leg's environment and
holds it to exit status 0 and to its last line, `leg NAME ok: K checks`, K written out here.  The checks are the suite's own
(the plan replay, the conv edge cases, the dense tails, the inference chain) with their per-op float64 bounds unchanged; what
a leg adds is the proof, from the stored data, that the other path ran (PATHS lines, see tests/startup_legs.py).

  leg                        environment                                            K   reaches
  stem_se_two_pass           ECGMM_STEM_FUSE=0 ECGMM_SE_MERGE=0                     7   max-pool backward + training BatchNorm backward of the
                                                                                        stem (dbias of the 1-D stem); SE gate gradient + gated
                                                                                        bn2 backward writing dz and the conv2 bias gradient
  down_unfolded_bn_unfused   ECGMM_DOWN_FOLD=0 ECGMM_DOWN_SIDE=0 ECGMM_BN_FUSE=0    9   downsample input gradient through dtmp; forward downsample
                                                                                        on the caller's stream; no fused reduction at MIN_M = 0
  relu_reread                ECGMM_RELU_BITS=0                                      3   bn2 backward masks from `out` (dual pass, fused reduction)
  halo_generic_wgs6          ECGMM_HALO_NCS1=0 ECGMM_WGRAD_WGS=6                   40   launch_halo<64, 9, *> with one K slice; pick_nsplit, 6 slots
  dense_per_op               ECGMM_HEAD_FUSED=0 ECGMM_SE_MLP_FUSED=0               18   head as per-op launches; SE MLP as linear + act + axpby
  dense16_off                ECGMM_DENSE16=0                                       47   Linear on the igemm / VALU routes at dense16's shapes

Measured on the MI355X, worst |err| / bound per op class and leg (every entry <= 1 by construction of the bounds; 1 is a bf16
rounding tie, the stored rounding term alone, with the worst fp32 case of the leg behind it in brackets; 0 is an exact
comparison; `-` = the leg runs no such op; the children print them: REPLAY / CHAIN / WORST lines):

  op class (plan replay)           stem_se_two_pass   down_unfolded_bn_unfused   relu_reread   halo_generic_wgs6   dense_per_op
  conv (y0 y1 y2 yd)               1 (0.37)           1 (0.37)                   1             1                   1 (0.37)
  coef + running stats             0.25               0.25                       0.25          0.25                0.25
  maxpool p0 / idx0                1 (0.33)           1 (0.33)                   1             1                   1 (0.33)
  pack, bits                       0                  0                          0 (no bits)   0                   0
  bn_act (a1, out)                 1 (0.45)           1 (0.45)                   1             1                   1 (0.42)
  avgpool (pooled, m)              0.18               0.18                       0.058         0.017               0.041
  se_mlp (h g ds dh dm dw db)      0.71               0.71                       -             0.71                0.71
  linear (fc / classifier)         0.43               0.43                       0.42          0.42                0.36
  dropout (hd, dfeat_h)            0.32               0.32                       -             0.28                0.34
  bcast X[0]                       1 (0.48)           1 (0.48)                   1             1                   1 (0.48)
  se gate grad dg                  0.026              0.026                      -             0.026               0.026
  bn_bwd (dy dz dgamma dbeta db)   1 (0.79)           1 (0.78)                   1             1                   1 (0.68)
  dw (dw1 dw2 dwd dw0)             0.11               0.13                       0.078         0.095               0.058
  dgrad (da dtmp X)                1 (0.027)          1 (0.049)                  1             1                   1 (0.028)
  stem_bwd (big0 big1 dgamma0 ..)  1 (0.48)           1 (0.36)                   1             1                   1 (0.31)
  stem input gradient              0.37               0.40                       0.38          0.30                0.18

  halo_generic_wgs6, the conv cases: halo y / dx 1 (half-ulp rounding), statistics rows 0.043, reduction rows 0.20 (2x2_images);
    weight gradients with 6 slots 0.18 (bf16) and 0.57 (fp32), both at odd_steps_two_groups, one split over 48 / 96 steps,
    against 0.045 / 0.081 with the default 512 slots -- longer fp32 chains per split, which the bound allows for
  dense_per_op: head per-op 0.55 (the 3 x 512 / NC = 4 case on the 24-values-per-lane LayerNorm included); inference chain
    conv / stem / gate_res_relu 1 (bf16 ties; fp32 0.84 / 0.32 / 0.25), se_mlp 0.067, avgpool 0.045, linear 0.012; plan
    features equal the chain bit for bit
  dense16_off: Linear 0.71 (dz of the sigmoid, as with dense16 on), SE MLP 0.73, head per-op fallback 0.64

Found by this file: with ECGMM_HEAD_FUSED=0 the head refused three 512-wide branches (`layernorm: D=1536 > 1024`), a shape the
row kernels serve; the per-op LayerNorm now has a 24-values-per-lane instantiation for 1024 < D <= 1536 (csrc/head.hip).
No fallback kernel broke a bound.

Run time on the MI355X: stem_se_two_pass 5.2 s, down_unfolded_bn_unfused 5.6 s, relu_reread 5.1 s, halo_generic_wgs6 4.6 s,
dense_per_op 4.0 s, dense16_off 2.6 s (process start and the first plan are about 2.5 s of each; the one-group child of
tests/test_conv_edges_f64_gpu.py takes 3 s); the 7 tests of this module 27 s in all, beside about 91 s for the suite
before it (118 s with it).

Children run one after another (at most two processes hold the GPU).  A child that dies on a signal, aborts or runs into
the 120 s limit -- the limit of the one-group child of tests/test_conv_edges_f64_gpu.py -- makes every leg after it fail at
once, without starting a process: nothing is started on a GPU that may just have faulted, and nothing is retried or skipped.
"""
import os
import subprocess
import sys

import pytest

from ecgmm.hip import lib as L

from .startup_legs import LEGS
from .util import switch_get

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# checks per leg, as the table above (tests/test_startup_legs_cpu.py holds LEGS to it)
K = {"stem_se_two_pass": 7, "down_unfolded_bn_unfused": 9, "relu_reread": 3, "halo_generic_wgs6": 40, "dense_per_op": 18,
     "dense16_off": 47}
DIED = []          # the leg whose child died on a signal, aborted or timed out: no further child is started


@pytest.mark.parametrize("name", list(K))
def test_leg(name):
    assert not DIED, "not started: the child of leg %s died (%s)" % tuple(DIED[0])
    env, _ = LEGS[name]
    try:
        r = subprocess.run([sys.executable, "-m", "tests.startup_legs", name], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        DIED.append((name, "no end after 120 s"))
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("leg %s: no end after 120 s\n%s" % (name, out[-3000:]))
    # (a GPU fault can also surface as a HIP error in a Python exception, exit status 1)
    fault = [w for w in ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR") if w in r.stderr + r.stdout]
    if r.returncode < 0 or r.returncode in (134, 139) or fault:
        DIED.append((name, "exit status %d%s" % (r.returncode, ", " + fault[0] if fault else "")))
    tail = r.stdout[-6000:] + r.stderr[-4000:]
    print(r.stdout[-20000:])
    assert r.returncode == 0, "leg %s: exit status %d\n%s" % (name, r.returncode, tail)
    assert ("leg %s ok: %d checks" % (name, K[name])) in r.stdout.splitlines(), tail


def test_every_switch_of_a_leg_is_refused_after_start_up():
    """what a leg holds cannot be reached from this process: ecgmm_switch_set refuses it and changes nothing"""
    lib = L.lib()
    held = sorted({n for env, _ in LEGS.values() for n in env})
    assert len(held) == 11
    for n in held:
        before = switch_get(lib, n)
        assert lib.ecgmm_switch_set(n.encode(), 0 if before else 1) == 1          # ECGMM_ERR_SHAPE
        assert ("%s is read once at start-up" % n) in lib.ecgmm_last_error().decode()
        assert switch_get(lib, n) == before
