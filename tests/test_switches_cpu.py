"""The library's ECGMM_* switches live in one table (csrc/switches.h).  Checked here without a GPU: the table enumerates
every switch the sources read and INTEGRATION.md lists them all; start-up parsing per kind, in child processes (a switch is
read once per process); the named setters and ecgmm_switch_set clamp alike and read back through ecgmm_switch_get; and the
table is what the dispatch consults, seen through the host-only query ecgmm_conv_bwd_data_bnred_rows."""
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

import pytest

from ecgmm.hip import lib as L

from .util import switch_get, switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecg-multimodal-model_amd", "csrc")
NEVER = 1 << 40
# what the library starts with when no ECGMM_* variable is set
DEFAULTS = {
    "ECGMM_CONV_HALO": 1, "ECGMM_HALO_CUS": 0, "ECGMM_HALO_W4": 0, "ECGMM_HALO_STAGGER": 1, "ECGMM_HALO_STREAM": 1,
    "ECGMM_HALO_PP": 1, "ECGMM_HALO_NCS1": 1, "ECGMM_WGRAD_RING": 1, "ECGMM_WGRAD_PP": 0, "ECGMM_WGRAD_GROUPS": 0,
    "ECGMM_WGRAD_WGS": 0, "ECGMM_BN_FOLD": 1, "ECGMM_BN_FOLD_SLICE": 1, "ECGMM_BN_FUSE": 1, "ECGMM_BN_FUSE_MIN_M": NEVER,
    "ECGMM_RELU_BITS": 1, "ECGMM_STEM_FUSE": 1, "ECGMM_STEM_RECOMPUTE": 0, "ECGMM_DOWN_FOLD": 1, "ECGMM_DOWN_SIDE": 1,
    "ECGMM_SIDE_WGRAD": 1, "ECGMM_INFER_DOWN_SIDE": 0, "ECGMM_SE_MERGE": 1, "ECGMM_SE_MLP_FUSED": 1, "ECGMM_HEAD_FUSED": 1,
    "ECGMM_DENSE16": 1,
}
ENV_CALL = r"\b(?:env_on|env_off|env_int|env_level|getenv)\s*\("


def names(lib):
    out, i = [], 0
    while True:
        n = lib.ecgmm_switch_name(i)
        if n is None:
            return out
        out.append(n.decode())
        i += 1


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_enumeration_covers_the_sources_and_the_documentation():
    lib = L.lib()
    ns = names(lib)
    assert len(ns) >= 26 and len(set(ns)) == len(ns) and all(n.startswith("ECGMM_") for n in ns)
    assert lib.ecgmm_switch_name(-1) is None and lib.ecgmm_switch_name(len(ns)) is None
    assert set(ns) == set(DEFAULTS)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in ns:
        assert re.search(r"\b%s\b" % n, doc), n + " is not in INTEGRATION.md"
    for path in sources():
        src = open(path).read()
        # a variable name handed to an env_* helper or to getenv, and every ECGMM_* string literal (the table's own entries)
        read = re.findall(ENV_CALL + r'\s*"(ECGMM_[A-Z0-9_]+)"', src) + re.findall(r'"(ECGMM_[A-Z0-9_]+)"', src)
        assert set(read) <= set(ns), (os.path.basename(path), sorted(set(read) - set(ns)))
        if os.path.basename(path) not in ("common.h", "switches.h"):
            assert not re.search(ENV_CALL, src), os.path.basename(path) + " reads the environment itself"


_CHILD = """
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from ecgmm.hip import lib as L
lib = L.lib()
for call in json.loads(sys.argv[2]):          # setters to run before anything reads the table
    getattr(lib, call[0])(*call[1:])
out = {}
for name in json.loads(sys.argv[3]):
    v = C.c_int64()
    assert lib.ecgmm_switch_get(name.encode(), C.byref(v)) == 0, name
    out[name] = v.value
print(json.dumps(out))
"""


def child(env_set, query, before=()):
    """switch values as a fresh process sees them: no ECGMM_* switch in its environment but env_set"""
    env = {k: v for k, v in os.environ.items() if k not in DEFAULTS}
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(list(before)), json.dumps(list(query))], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_unset_environment_gives_the_defaults():
    assert child({}, DEFAULTS) == DEFAULTS


@pytest.mark.parametrize("name,text,want", [
    ("ECGMM_HALO_PP", "0", 0),                    # on unless the value starts with '0'
    ("ECGMM_HALO_W4", "1", 1),                    # off unless it starts with '1'
    ("ECGMM_HALO_W4", "yes", 0),
    ("ECGMM_CONV_HALO", "2", 2),                  # one digit 0..2
    ("ECGMM_CONV_HALO", "7", 1),                  # ... anything else: the default
    ("ECGMM_HALO_CUS", "-5", 0),                  # integer; negative = no cap
    ("ECGMM_BN_FUSE_MIN_M", "400000", 400000),
    ("ECGMM_BN_FUSE_MIN_M", "-1", NEVER),         # negative = never, as ecgmm_bn_fuse_min_pixels(-1)
])
def test_start_up_parsing(name, text, want):
    assert child({name: text}, [name]) == {name: want}


def test_a_setter_before_the_first_read_wins_over_the_environment():
    got = child({"ECGMM_HALO_PP": "0", "ECGMM_CONV_HALO": "0", "ECGMM_HALO_W4": "1"},
                ["ECGMM_HALO_PP", "ECGMM_CONV_HALO", "ECGMM_HALO_W4"],
                before=[["ecgmm_conv_halo_pingpong", 1], ["ecgmm_conv_halo_enable", 2]])
    assert got == {"ECGMM_HALO_PP": 1, "ECGMM_CONV_HALO": 2, "ECGMM_HALO_W4": 1}   # (W4: no setter ran, the environment holds)


# the 13 named setters that need no GPU (ecgmm_side_wgrad creates the side streams): (setter, switch, argument, read back)
SETTERS = [
    ("ecgmm_conv_halo_enable", "ECGMM_CONV_HALO", 9, 2), ("ecgmm_conv_halo_enable", "ECGMM_CONV_HALO", -3, 0),
    ("ecgmm_conv_halo_enable", "ECGMM_CONV_HALO", 1, 1),
    ("ecgmm_conv_halo_cus", "ECGMM_HALO_CUS", -1, 0), ("ecgmm_conv_halo_cus", "ECGMM_HALO_CUS", 7, 7),
    ("ecgmm_conv_halo_w4", "ECGMM_HALO_W4", 5, 1), ("ecgmm_conv_halo_w4", "ECGMM_HALO_W4", 0, 0),
    ("ecgmm_conv_halo_stagger", "ECGMM_HALO_STAGGER", 0, 0), ("ecgmm_conv_halo_stagger", "ECGMM_HALO_STAGGER", -1, 1),
    ("ecgmm_conv_halo_stream", "ECGMM_HALO_STREAM", 0, 0), ("ecgmm_conv_halo_stream", "ECGMM_HALO_STREAM", 2, 1),
    ("ecgmm_conv_halo_pingpong", "ECGMM_HALO_PP", 0, 0), ("ecgmm_conv_halo_pingpong", "ECGMM_HALO_PP", 1, 1),
    ("ecgmm_conv_wgrad_pingpong", "ECGMM_WGRAD_PP", 1, 1), ("ecgmm_conv_wgrad_pingpong", "ECGMM_WGRAD_PP", 0, 0),
    ("ecgmm_conv_wgrad_ring_enable", "ECGMM_WGRAD_RING", 9, 2), ("ecgmm_conv_wgrad_ring_enable", "ECGMM_WGRAD_RING", -1, 0),
    ("ecgmm_bn_fold", "ECGMM_BN_FOLD", 0, 0), ("ecgmm_bn_fold", "ECGMM_BN_FOLD", 3, 1),
    ("ecgmm_bn_fold_slice", "ECGMM_BN_FOLD_SLICE", 0, 0), ("ecgmm_bn_fold_slice", "ECGMM_BN_FOLD_SLICE", 1, 1),
    ("ecgmm_bn_fuse_min_pixels", "ECGMM_BN_FUSE_MIN_M", -1, NEVER), ("ecgmm_bn_fuse_min_pixels", "ECGMM_BN_FUSE_MIN_M", 0, 0),
    ("ecgmm_bn_fuse_min_pixels", "ECGMM_BN_FUSE_MIN_M", 1 << 33, 1 << 33),
    ("ecgmm_stem_recompute", "ECGMM_STEM_RECOMPUTE", 1, 1), ("ecgmm_stem_recompute", "ECGMM_STEM_RECOMPUTE", 0, 0),
    ("ecgmm_infer_down_side", "ECGMM_INFER_DOWN_SIDE", 1, 1), ("ecgmm_infer_down_side", "ECGMM_INFER_DOWN_SIDE", 0, 0),
]


def test_named_setters_and_set_by_name_clamp_alike_and_read_back():
    lib = L.lib()
    assert len({s for s, _, _, _ in SETTERS}) == 13
    touched = sorted({n for _, n, _, _ in SETTERS})
    with switches(lib, **{n: switch_get(lib, n) for n in touched}):       # every value back on exit
        for setter, name, arg, want in SETTERS:
            assert getattr(lib, setter)(arg) == 0
            assert switch_get(lib, name) == want, (setter, arg)
            other = 0 if want else 1                                         # then the same argument by name
            assert lib.ecgmm_switch_set(name.encode(), other) == 0 and switch_get(lib, name) == other
            assert lib.ecgmm_switch_set(name.encode(), arg) == 0
            assert switch_get(lib, name) == want, (name, arg)
    # refused: a switch that is read once at start-up, the per-plan side-stream state, an unknown name
    for name, word in (("ECGMM_RELU_BITS", "start-up"), ("ECGMM_SIDE_WGRAD", "ecgmm_side_wgrad"), ("ECGMM_NO_SUCH", "unknown")):
        before = switch_get(lib, name) if name in DEFAULTS else None
        assert lib.ecgmm_switch_set(name.encode(), 0) == 1                # ECGMM_ERR_SHAPE
        msg = lib.ecgmm_last_error().decode()
        assert name in msg and word in msg, msg
        if before is not None:
            assert switch_get(lib, name) == before
    v = C.c_int64(-7)
    assert lib.ecgmm_switch_get(b"ECGMM_NO_SUCH", C.byref(v)) == 1 and v.value == -7
    assert "ECGMM_NO_SUCH" in lib.ecgmm_last_error().decode()


def test_the_dispatch_reads_the_table():
    """rows of the fused BatchNorm-backward reduction for the bf16 3x3 64 -> 64 convolution at N = 4, H = W = 16: 1024 pixels =
    four 256-pixel tiles, one channel tile -> one workgroup per tile unless ECGMM_HALO_CUS caps them, none with the halo
    kernel switched off"""
    lib = L.lib()
    d = L.ConvDesc(4, 16, 16, 64, 64, 3, 3, 1, 1, 1)

    def rows():
        return lib.ecgmm_conv_bwd_data_bnred_rows(L.BF16, C.byref(d))

    with switches(lib, ECGMM_CONV_HALO=DEFAULTS["ECGMM_CONV_HALO"], ECGMM_HALO_CUS=DEFAULTS["ECGMM_HALO_CUS"]):
        assert rows() == 4
        with switches(lib, ECGMM_HALO_CUS=3):
            assert rows() == 3
            with switches(lib, ECGMM_CONV_HALO=0):
                assert rows() == 0
        assert rows() == 4
