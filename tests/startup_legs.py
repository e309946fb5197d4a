"""The float64 checks of this suite under the OTHER value of every switch the library reads once at start-up.

Twelve switches of csrc/switches.h have runtime == false: the library reads them once per process and ecgmm_switch_set refuses
them afterwards, so a pytest process started without any ECGMM_* variable only ever runs their default side.  Each leg of
LEGS is one child process: `python -m tests.startup_legs NAME` from the repository root, started by
tests/test_startup_legs_gpu.py with the leg's environment.  The child
  1. asserts through ecgmm_switch_get that every variable of the leg reads back as set and that every other start-up-only
     switch has the default of tests/test_switches_cpu.py::DEFAULTS (unless the parent's environment sets it: an A/B run),
  2. runs the leg's checks in order -- the suite's own functions, imported and called as the tests call them; a failed
     assertion ends the process with a traceback,
  3. prints `leg NAME ok: K checks` behind the REPLAY / PATHS lines of the replays it ran.
A process holds more than one switch only where they touch disjoint ops.

A leg that took the default path after all would pass and test nothing, so each replay check also asserts, from what the
plan left in its workspaces (Plan.seen, byte by byte against the 0xFF fill, and the branch the replay itself took), that the
other path ran: big0 written by the two-pass stem, the merged SE pass's sa1 / sa2 / sa3 / se_rows untouched, dtmp written by
every downsample block, no ReLU bits after the forward and after the backward, dz written by every block and no fused
reduction although the kernel could.  The halo cases prove their kernel by the statistics-row count (_halo_case), the dense
legs by the routes their tests print.  ECGMM_DOWN_SIDE and ECGMM_SE_MLP_FUSED leave no trace in the data: the same tensors,
held to the same bounds (and, for the inference plan, to the per-op chain bit for bit).

Left out on purpose (EXEMPT): ECGMM_WGRAD_GROUPS has its child in tests/test_conv_edges_f64_gpu.py; ECGMM_SIDE_WGRAD only
sets the initial value of what ecgmm_side_wgrad() changes at run time (test_plan_replays_with_the_side_streams_off).

A new start-up-only switch needs a leg here or a reason in EXEMPT: tests/test_startup_legs_cpu.py fails otherwise.
"""
import contextlib
import io
import os
import sys

from ecgmm.hip import lib as L

from . import f64check as F64
from . import plan_replay as PR
from . import test_conv_edges_f64_gpu as CE
from . import test_dense_f64_gpu as DN
from . import test_infer_chain_gpu as IC
from . import test_plan_replay_gpu as RP
from .test_switches_cpu import DEFAULTS, names
from .util import switch_get, switches

EXEMPT = {
    "ECGMM_WGRAD_GROUPS": "its own child: test_conv_edges_f64_gpu.py::test_d_weight_gradient_one_group_in_a_fresh_process",
    "ECGMM_SIDE_WGRAD": "initial value of ecgmm_side_wgrad()'s run-time state: test_plan_replays_with_the_side_streams_off",
}
HALO_RING = dict(ECGMM_CONV_HALO=2, ECGMM_WGRAD_RING=2)
HALO_RING_FUSE = dict(HALO_RING, ECGMM_BN_FUSE_MIN_M=0)       # (the switches of test_plan_replays_with_halo_ring_and_fused_reductions)
BF16, F32 = L.BF16, L.F32
DT_NAME = {L.BF16: "bf16", L.F32: "fp32"}


def startup_only(lib):
    """the switches ecgmm_switch_set refuses even at their current value"""
    return [n for n in names(lib) if lib.ecgmm_switch_set(n.encode(), switch_get(lib, n)) != 0]


# ------------------------------------------------------------------------------------------------ replay checks
LEG_WORST = PR.Rep()           # worst ratio per op class over the replays of this process


def two_pass_stem(plan, rep):
    assert plan.seen["big0"] is True and rep.paths["stem bwd"] == "two passes", (plan.seen["big0"], rep.paths)
    assert "stem_bwd" in rep.worst and "bn_bwd" in rep.worst


def unmerged_se(plan, rep):
    if plan.net.se:
        assert plan.seen["se_merged"] == {0: False, 1: False, 2: False}, plan.seen["se_merged"]


def unfolded_downsample(plan, rep):
    down = [k.i for k in plan.net.blocks if k.down]
    assert down and plan.seen["dtmp"] == {i: True for i in down}, plan.seen["dtmp"]
    assert all(rep.paths["blk%d din" % i] == "dtmp" for i in down), rep.paths


def unfused_bn(plan, rep):
    assert plan.net.fused2 == set() and all(plan.seen["dz"].values()) and len(plan.seen["dz"]) == len(plan.net.blocks)


def unfused_bn_although_capable(plan, rep):
    unfused_bn(plan, rep)
    assert RP.fused_blocks(plan, capable_only=True) == {0, 2}


def no_relu_bits(plan, rep):
    assert plan.net.kind == "r18" and plan.net.bf16 and not plan.net.bits and "bits" not in rep.worst
    assert plan.seen["bits"] == "none after the forward, none after the backward", plan.seen["bits"]


def still_fused(plan, rep):
    assert plan.net.fused2 == {0, 2}, plan.net.fused2


def replay(kind, shape, dt, sw=None, expect=()):
    """Plan + staged() of tests/test_plan_replay_gpu.py under run-time switches `sw`, then the leg's evidence"""
    lib = L.lib()
    what = "%s %s %s%s" % (kind, shape, DT_NAME[dt], "".join(" %s=%d" % kv for kv in sorted((sw or {}).items())))
    with switches(lib, **(sw or {})):
        plan = RP.Plan(kind, shape, dt)
        plan.net.fused2 = RP.fused_blocks(plan)
        rep = PR.Rep()
        RP.staged(plan, rep)
    rep.show(what)
    RP.show_paths(plan, what)
    for e in expect:
        e(plan, rep)
    for cls, r in rep.worst.items():
        LEG_WORST(cls, r)


def plan_cases(kind=None, dt=None, first=False):
    return [c for c in RP.CASES if kind in (None, c[0]) and dt in (None, c[2]) and (not first or c[1] == RP.SHAPES[c[0]][0])]


def replays(cases, sw=None, expect=()):
    return [(replay, (k, s, dt, sw, expect)) for k, s, dt in cases]


# ------------------------------------------------------------------------------------------------ dense checks
def printed(fn, args, must, never=()):
    """fn(*args) with its output passed on and held to the route it names"""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        try:
            fn(*args)
        finally:
            sys.__stdout__.write(buf.getvalue())
    out = buf.getvalue()
    assert must in out and not any(n in out for n in never), "%s%s printed no %r (or one of %r)" % (fn.__name__, args, must, never)


DENSE16_SHAPES = [s for s, (routes, _) in DN.LINEAR_REACHES.items() if routes == ("dense16",) * 3]


def linear_off_dense16(shape, act):
    """test_linear_against_float64 with ECGMM_DENSE16=0: the shapes dense16_kernel serves by default go the implicit-GEMM way"""
    if shape in DENSE16_SHAPES:
        routes = DN.linear_routes(*shape, act, bool(switch_get(L.lib(), "ECGMM_DENSE16")))
        assert "dense16" not in routes and routes[1:] == ("igemm", "igemm"), routes
        return printed(DN.test_linear_against_float64, (shape, act), "routes %s" % (routes,), never=("dense16",))
    DN.test_linear_against_float64(shape, act)


def head_per_op(case, kind):
    printed(DN.test_fused_head_against_float64, (case, kind), "%s per-op]" % kind, never=(" fused]",))


# ------------------------------------------------------------------------------------------------ the legs
def _halo(case, variant=None):
    if variant is None:
        return (CE._halo_case, (case, 64, 64, 3000 + 10 * CE.C_PARAMS.index((case, 64, 64)), {}, ""))
    c, ci, co, sw = CE.C_VARIANTS[variant]
    assert (c, ci, co) == (case, 64, 64)
    return (CE._halo_case, (c, ci, co, 3900 + 10 * list(CE.C_VARIANTS).index(variant), sw, " " + variant))


# name -> (environment of the child, [(callable, arguments), ...])
LEGS = {
    # training stem backward as ecg_maxpool_relu_bwd into big0 + the training bn_bwd_mode into big1 (with the 1-D stem's dbias);
    # ecg_se_gate_grad + the gated bn_bwd_mode that writes dz and the conv2 bias gradient itself
    "stem_se_two_pass": (
        {"ECGMM_STEM_FUSE": "0", "ECGMM_SE_MERGE": "0"},
        replays(plan_cases("r1d") + plan_cases("r18", first=True), None, (two_pass_stem, unmerged_se))
        + replays([("r1d", RP.HALO_SHAPES["r1d"], BF16)], HALO_RING, (two_pass_stem, unmerged_se))),
    # every downsample input gradient through dtmp and back as an addend; the forward downsample branch on the caller's
    # stream; no fused BatchNorm-backward reduction although ECGMM_BN_FUSE_MIN_M = 0 allows it and the kernel could
    "down_unfolded_bn_unfused": (
        {"ECGMM_DOWN_FOLD": "0", "ECGMM_DOWN_SIDE": "0", "ECGMM_BN_FUSE": "0"},
        replays(plan_cases(), None, (unfolded_downsample, unfused_bn))
        + replays([("r18", RP.HALO_SHAPES["r18"], BF16)], HALO_RING_FUSE, (unfolded_downsample, unfused_bn_although_capable))),
    # bn2's backward re-reads `out` for the mask: ecg_bn_bwd_dual with a null bit pointer, the fused reduction's mask
    "relu_reread": (
        {"ECGMM_RELU_BITS": "0"},
        replays(plan_cases("r18", BF16), None, (no_relu_bits,))
        + replays([("r18", RP.HALO_SHAPES["r18"], BF16)], HALO_RING_FUSE, (no_relu_bits, still_fused))),
    # 64 -> 64 channel 3x3 tiles on the generic launch_halo<64, 9, 0 / 1 / 2> with one K slice; pick_nsplit with 6 slots:
    # several steps per split, and a single split over many steps (the comment above D_CASES has the counts)
    "halo_generic_wgs6": (
        {"ECGMM_HALO_NCS1": "0", "ECGMM_WGRAD_WGS": "6"},
        [_halo(c) for c in ("w63", "one_pixel_images", "2x2_images", "3x5_images")] + [_halo("3x5_images", "3x5_images_3cus")]
        + [(CE._wgrad_case, (case, dt, mode + " wgs6", dict(ECGMM_WGRAD_RING=0) if mode == "ring0" else {}))
           for case in CE.D_CASES for dt, mode in CE.D_MODES]
        + replays([("r18", RP.HALO_SHAPES["r18"], BF16)], HALO_RING_FUSE, (still_fused,))
        + replays(plan_cases("r1d", BF16, first=True))),
    # the fusion head as per-op launches; the SE MLP as ecg_linear_* + ecg_act_bwd + ecg_axpby in the training and the
    # inference plan (the per-op chain of tests/infer_chain.py follows the same switch)
    "dense_per_op": (
        {"ECGMM_HEAD_FUSED": "0", "ECGMM_SE_MLP_FUSED": "0"},
        [(head_per_op, p) for p in DN.HEAD_PARAMS]
        + replays(plan_cases("r1d", first=True))
        + [(IC.test_every_chain_tensor_against_float64, c) for c in IC.LIVE_CASES if c[0] == "r1d"]
        + [(IC.test_plan_features_equal_the_chain_bit_for_bit, c + (None,)) for c in IC.LIVE_CASES if c[0] == "r1d"]),
    # batch-sized Linear layers through the implicit-GEMM / VALU routes at the shapes dense16_kernel always takes today
    "dense16_off": (
        {"ECGMM_DENSE16": "0"},
        [(linear_off_dense16, (s, a)) for s in F64.LINEAR_CASES for a in DN.ACT]
        + [(DN.test_se_mlp_against_float64, (s,)) for s in F64.SE_CASES]
        + [(DN.test_head_per_op_fallback_against_float64, (c,))
           for c in ((24, (256, 256, 256), 128, 2), (1028, (72, 40, 48), 16, 3))]),
}


def leg_values(name):
    """{switch: the value the leg's environment must parse to}"""
    return {k: int(v) for k, v in LEGS[name][0].items()}


def main(name):
    env, checks = LEGS[name]
    lib = L.lib()
    want = leg_values(name)
    for n in startup_only(lib):
        got = switch_get(lib, n)
        if n in want:
            assert got == want[n], "%s reads %d, the leg sets %s" % (n, got, env[n])
            assert got != DEFAULTS[n], "%s: the leg sets the default" % n
        elif n not in os.environ:
            assert got == DEFAULTS[n], "%s reads %d without being set (default %d)" % (n, got, DEFAULTS[n])
    assert set(want) <= set(startup_only(lib)), "not start-up-only: %s" % sorted(set(want) - set(startup_only(lib)))
    print("leg %s: %s" % (name, " ".join("%s=%s" % kv for kv in sorted(env.items()))))
    for fn, args in checks:
        fn(*args)
    if LEG_WORST.worst:
        LEG_WORST.show("leg %s, worst over its replays" % name)
    print("leg %s ok: %d checks" % (name, len(checks)))


if __name__ == "__main__":
    main(sys.argv[1])
