"""The table of tests/startup_legs.py cannot rot: every switch the library refuses to set after start-up is exercised at its
other value by a leg, or exempt with a reason; and every leg's environment parses to the values the leg means.  No GPU: the
library loads on the CPU as in tests/test_switches_cpu.py, and the legs' check lists are only counted here."""
from ecgmm.hip import lib as L

from .startup_legs import EXEMPT, LEGS, leg_values, startup_only
from .test_startup_legs_gpu import K
from .test_switches_cpu import DEFAULTS, child, names
from .util import switch_get


def test_every_start_up_only_switch_has_a_leg_or_a_reason():
    lib = L.lib()
    before = {n: switch_get(lib, n) for n in names(lib)}
    frozen = startup_only(lib)
    assert {n: switch_get(lib, n) for n in names(lib)} == before           # (asking changed nothing)
    assert len(frozen) >= 12 and set(frozen) <= set(DEFAULTS)
    led = {}
    for leg in LEGS:
        for n, v in leg_values(leg).items():
            assert n not in led, "%s is held by two legs: %s and %s" % (n, led[n], leg)
            assert n in frozen, "%s (leg %s) can be set at run time: it needs no process of its own" % (n, leg)
            assert v != DEFAULTS[n], "leg %s holds %s at its default" % (leg, n)
            led[n] = leg
    for n in frozen:
        assert (n in led) != (n in EXEMPT), \
            "%s is read once at start-up: give it a leg in tests/startup_legs.py (or one line in EXEMPT), not both" % n
    assert set(EXEMPT) <= set(frozen) and all(len(r) > 20 and "\n" not in r for r in EXEMPT.values())
    assert set(EXEMPT) == {"ECGMM_WGRAD_GROUPS", "ECGMM_SIDE_WGRAD"}          # (a third exemption is a decision: change it here too)


def test_each_leg_parses_to_its_values_in_a_fresh_process():
    for leg, (env, _) in LEGS.items():
        want = dict(DEFAULTS, **leg_values(leg))
        assert child(env, DEFAULTS) == want, leg


def test_the_parent_counts_the_checks_of_every_leg():
    assert {leg: len(checks) for leg, (_, checks) in LEGS.items()} == K
    for leg, (_, checks) in LEGS.items():
        assert all(callable(fn) and isinstance(args, tuple) for fn, args in checks), leg
