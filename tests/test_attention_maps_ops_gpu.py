"""ecgmm_mha_weights / ecgmm_mha_rollout_step through the C ABI on the GPU (call pattern and guard zones of tests/attn_abi.py:
every output is NaN-filled between sentinel zones and must come back finite).  With lengths the padded rows of qkv and the
padded entries of v hold NaN.  The lse is the one ecgmm_mha_forward(_varlen) stored for the same qkv.  Every element is held
to the derived bounds of tests/attn_maps_ref.py against the float64 restatement from the stored qkv and lse; the padding must
be exact zeros; the bit identities of the contract are checked as such."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from ecgmm.hip.functional import ptr
from oracle import fill

from . import attn_bounds as AB
from . import attn_maps_ref as MR
from . import attn_varlen_ref as VR

pytestmark = pytest.mark.gpu

SIZES = {1: 37, 5: 37, 8: 37, 15: 5, 16: 5, 17: 5, 33: 5, 64: 5, 65: 5, 130: 5}      # S -> N (S <= 8: the packed regime)
HEADS = ((64, 4), (64, 2), (32, 1))                                                  # (E, heads): head size 16, 32, 32
MODES = ("null", "full", "ragged", "clamped")
CASES = [(S, E, h, bf) for S in SIZES for (E, h), bf in itertools.product(HEADS, (0, 1))]
IDS = ["S%d_E%d_h%d_bf%d" % c for c in CASES]
A = 0.5


def lengths_of(mode, S, N):
    """null; all S; ragged: S, 1, the largest multiple of 16 (S itself below 16), S - 1, 9 .. in turn; clamped: a device tensor
    that also holds 0, a negative value and values above S"""
    if mode == "null":
        return None
    if mode == "full":
        return [S] * N
    m16 = S // 16 * 16 or S
    base = [S, 1, m16, max(S - 1, 1), min(9, S)] if mode == "ragged" else [0, S + 3, 1, -2, max(S - 2, 1), S + 100]
    return [base[i % len(base)] for i in range(N)]


def test_cases_cover_what_the_kernels_branch_on():
    assert set(SIZES) == {1, 5, 8, 15, 16, 17, 33, 64, 65, 130} and all(SIZES[S] == 37 for S in (1, 5, 8))
    assert {E // h for E, h in HEADS} == {16, 32} and {h for _, h in HEADS} == {1, 2, 4}
    for S, N in SIZES.items():
        r, c = lengths_of("ragged", S, N), lengths_of("clamped", S, N)
        assert len(r) == N and 1 in r and S in r and all(1 <= v <= S for v in r)
        assert S < 16 or any(v % 16 == 0 for v in r)
        assert 0 in c and max(c) > S and min(c) < 0


def _inputs(S, N, E, bf, lengths, salt=0):
    """qkv [S * N, 3E] and v [N, S] from the hash filler; NaN in the padded rows of qkv and the padded entries of v"""
    qkv = fill.hash_tensor((S * N, 3 * E), 930 + S + salt, 1.0)
    v = fill.hash_tensor((N, S), 931 + S + salt, 1.0)
    if lengths is not None:
        qkv[~VR.live_rows(lengths, S, N, bool(bf))] = float("nan")
        v[torch.arange(S)[None, :] >= torch.tensor(VR.clamp(lengths, S))[:, None]] = float("nan")
    return qkv, v


def _dev_lengths(lengths):
    from .attn_abi import DEV
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)


def forward_lse(qkv, lengths, S, N, heads, bf):
    """the lse [N, heads, S] (cpu) the forward stores for qkv"""
    from . import attn_abi as AA
    E = qkv.shape[1] // 3
    d = AA.desc(S, N, heads, E // heads, bf)
    q, ln = AA.dev(qkv), _dev_lengths(lengths)
    if lengths is None:
        return AA.forward(qkv, S, N, heads, bf)["lse"]
    return AA.call("ecgmm_mha_forward_varlen", {"out": (S * N, E), "lse": (N, heads, S)},
                   lambda v: (C.byref(d), ptr(q), ptr(ln), ptr(v["out"]), ptr(v["lse"]), 0, 0))["lse"]


def weights(qkv, lse, lengths, S, N, heads, bf, per_head, p=0.0, expect=0):
    from . import attn_abi as AA
    E = qkv.shape[1] // 3
    d = AA.desc(S, N, heads, E // heads, bf, p)
    q, l, ln = AA.dev(qkv), AA.dev(lse), _dev_lengths(lengths)
    r = AA.call("ecgmm_mha_weights", {"w": (N, heads, S, S) if per_head else (N, S, S)},
                lambda v: (C.byref(d), ptr(q), ptr(l), ptr(ln), ptr(v["w"]), int(per_head)), expect=expect)
    return None if expect else r["w"]


def rollout_step(qkv, lse, v, lengths, S, N, heads, bf, a, expect=0):
    from . import attn_abi as AA
    E = qkv.shape[1] // 3
    d = AA.desc(S, N, heads, E // heads, bf)
    q, l, vi, ln = AA.dev(qkv), AA.dev(lse), AA.dev(v), _dev_lengths(lengths)
    r = AA.call("ecgmm_mha_rollout_step", {"y": (N, S)},
                lambda o: (C.byref(d), ptr(q), ptr(l), ptr(ln), ptr(vi), ptr(o["y"]), a), expect=expect)
    return None if expect else r["y"]


@functools.lru_cache(maxsize=None)
def _run(S, E, heads, bf, mode):
    """forward + both maps + one rollout step, shared by the tests below (read only)"""
    N = SIZES[S]
    lengths = lengths_of(mode, S, N)
    qkv, v = _inputs(S, N, E, bf, lengths if mode in ("ragged", "clamped") else None)
    lse = forward_lse(qkv, lengths, S, N, heads, bf)
    return dict(N=N, lengths=lengths, qkv=qkv, v=v, lse=lse,
                ph=weights(qkv, lse, lengths, S, N, heads, bf, 1), avg=weights(qkv, lse, lengths, S, N, heads, bf, 0),
                y=rollout_step(qkv, lse, v, lengths, S, N, heads, bf, A))


def _check(tag, r, S, heads, bf, a=A, y=None):
    """every element within its bound, row sums and mass within theirs, exact zeros in the padding -> the worst ratios"""
    N = r["N"]
    m = MR.Maps(r["qkv"], r["lse"], S, N, heads, bf, r["lengths"])
    y = r["y"] if y is None else y
    live = m.live
    figs = {"per head": AB.ratio((r["ph"].double() - m.P).abs(), m.weights_bound(True)),
            "average": AB.ratio((r["avg"].double() - m.average()).abs(), m.weights_bound(False)),
            "rows": AB.ratio((r["ph"].double().sum(-1) - live[:, None, :].double()).abs(), m.rowsum_bound(True)),
            "rows avg": AB.ratio((r["avg"].double().sum(-1) - live.double()).abs(), m.rowsum_bound(False)),
            "rollout": AB.ratio((y.double() - m.rollout_step(r["v"], a)).abs(), m.rollout_bound(r["v"], a)),
            "mass": AB.ratio((y.double().sum(-1) - m._v(r["v"]).sum(-1)).abs(), m.mass_bound(r["v"], a))}
    print("%-28s " % tag + "  ".join("%s %.3g" % kv for kv in figs.items()))
    assert max(figs.values()) <= 1.0, "of the bound: %s" % figs
    dead = ~live
    assert bool((r["avg"][dead] == 0).all()) and bool((r["avg"].transpose(1, 2)[dead] == 0).all()), "average: padding not 0"
    assert bool((r["ph"].transpose(1, 2)[dead] == 0).all()), "per head: a padded query row is not 0"
    assert bool((r["ph"].permute(0, 3, 1, 2)[dead] == 0).all()), "per head: a padded key column is not 0"
    assert bool((y[dead] == 0).all()), "rollout: a padded entry is not 0"
    return figs


@pytest.mark.parametrize("S,E,heads,bf", CASES, ids=IDS)
def test_maps_and_rollout_within_the_bounds_with_exact_zeros_in_the_padding(S, E, heads, bf):
    for mode in MODES:
        r = _run(S, E, heads, bf, mode)
        _check("S%d E%d h%d bf%d %s" % (S, E, heads, bf, mode), r, S, heads, bf)
        # the averaged output is the ordered fp32 head sum of the per-head output times the fp32 1 / heads
        assert torch.equal(r["avg"], MR.head_average_fp32(r["ph"])), mode
    # null lengths equal full lengths, bit for bit (so do lengths clamped down to S)
    a, b = _run(S, E, heads, bf, "null"), _run(S, E, heads, bf, "full")
    for k in ("lse", "ph", "avg", "y"):
        assert torch.equal(a[k], b[k]), k
    N = a["N"]
    over = [S + 1 + n for n in range(N)]
    assert torch.equal(weights(a["qkv"], a["lse"], over, S, N, heads, bf, 0), a["avg"])
    assert torch.equal(rollout_step(a["qkv"], a["lse"], a["v"], over, S, N, heads, bf, A), a["y"])


@pytest.mark.parametrize("S,E,heads,bf", [(5, 64, 4, 0), (17, 64, 2, 1), (65, 32, 1, 0), (130, 64, 4, 1)])
def test_two_calls_give_the_same_bits_and_residual_zero_is_the_pure_product(S, E, heads, bf):
    r = _run(S, E, heads, bf, "ragged")
    N, ln = r["N"], r["lengths"]
    assert torch.equal(weights(r["qkv"], r["lse"], ln, S, N, heads, bf, 1), r["ph"])
    assert torch.equal(weights(r["qkv"], r["lse"], ln, S, N, heads, bf, 0), r["avg"])
    assert torch.equal(rollout_step(r["qkv"], r["lse"], r["v"], ln, S, N, heads, bf, A), r["y"])
    # p_drop of the descriptor is ignored: the maps are the undropped probabilities
    assert torch.equal(weights(r["qkv"], r["lse"], ln, S, N, heads, bf, 0, p=0.25), r["avg"])
    y0 = rollout_step(r["qkv"], r["lse"], r["v"], ln, S, N, heads, bf, 0.0)
    _check("S%d residual 0" % S, r, S, heads, bf, a=0.0, y=y0)
    y25 = rollout_step(r["qkv"], r["lse"], r["v"], ln, S, N, heads, bf, 0.25)
    _check("S%d residual 0.25" % S, r, S, heads, bf, a=0.25, y=y25)


@pytest.mark.parametrize("S,E,heads,bf", [(17, 64, 4, 1), (33, 64, 2, 0), (65, 64, 4, 0), (130, 32, 1, 1), (130, 64, 4, 0)])
def test_a_record_alone_has_the_bits_of_its_block_in_the_padded_batch(S, E, heads, bf):
    """S > 8 and length > 8: the tiles, and their order, of the record run alone with S = its length"""
    r = _run(S, E, heads, bf, "ragged")
    N, seen = r["N"], 0
    for n, ln in enumerate(VR.clamp(r["lengths"], S)):
        if ln < 9:
            continue
        rows = VR.rows(S, N, n, ln, bool(bf))
        q1, l1, v1 = r["qkv"][rows], r["lse"][n:n + 1, :, :ln].contiguous(), r["v"][n:n + 1, :ln].contiguous()
        assert torch.equal(forward_lse(q1, None, ln, 1, heads, bf), l1), (n, ln)
        assert torch.equal(weights(q1, l1, None, ln, 1, heads, bf, 1)[0], r["ph"][n, :, :ln, :ln]), (n, ln)
        assert torch.equal(weights(q1, l1, None, ln, 1, heads, bf, 0)[0], r["avg"][n, :ln, :ln]), (n, ln)
        assert torch.equal(rollout_step(q1, l1, v1, None, ln, 1, heads, bf, A)[0], r["y"][n, :ln]), (n, ln)
        seen += 1
    assert seen >= 3


def test_large_scores():
    """q . k = +-80 before scaling (tests/test_attention_ops_gpu.py): finite, within the bounds, rows sum to one"""
    S, N, heads, hd = 33, 3, 2, 16
    E = heads * hd
    for bf, lengths in ((0, None), (1, [33, 17, 9])):
        qkv, v = _inputs(S, N, E, bf, None, salt=7)
        sign = torch.where(fill.hash_tensor((S * N, 1), 780, 1.0) > 0, 1.0, -1.0)
        qkv[:, :E] = 2.5 * sign                                     # 2.5 * 2 * 16 = 80 exactly
        qkv[:, E:2 * E] = 2.0 * sign
        m = MR.Maps(qkv, None, S, N, heads, bf, lengths)
        assert abs(float(m.s.abs().max()) * hd ** 0.5 - 80.0) < 1e-9
        lse = forward_lse(qkv, lengths, S, N, heads, bf)
        r = dict(N=N, lengths=lengths, qkv=qkv, v=v, lse=lse, ph=weights(qkv, lse, lengths, S, N, heads, bf, 1),
                 avg=weights(qkv, lse, lengths, S, N, heads, bf, 0), y=rollout_step(qkv, lse, v, lengths, S, N, heads, bf, A))
        _check("scores +-80 bf%d" % bf, r, S, heads, bf)


def test_refused_calls_write_nothing():
    S, N, heads, E = 17, 2, 4, 64
    qkv, v = _inputs(S, N, E, 0, None)
    lse = torch.zeros(N, heads, S)
    for bad in (1.0, -0.5, float("nan")):
        rollout_step(qkv, lse, v, None, S, N, heads, 0, bad, expect=1)
    weights(qkv, lse, None, S, N, heads, 0, 2, expect=1)
    weights(qkv, lse, None, S, N, heads, 0, 0, p=1.0, expect=1)
