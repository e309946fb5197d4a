"""ecgmm_mha_forward_varlen / ecgmm_mha_backward_varlen through the C ABI on the GPU (call pattern and guard zones of
tests/attn_abi.py).  The padded rows of qkv and dout and every output buffer are NaN before the call.  Live rows are held
element by element to the derived bounds of tests/attn_bounds.py against the float64 reference of every attention-batch
element ALONE, trimmed to its length (tests/attn_varlen_ref.py); padded rows of out, lse and dqkv must be exact zeros.  Bit
identities: no lengths and all-full lengths against the entry points without lengths, a live element against the same element
alone, two calls, and another filling of the padding."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr
from oracle import fill

from . import attn_bounds as AB
from . import attn_ref as AR
from . import attn_varlen_ref as VR

pytestmark = pytest.mark.gpu

N, HEADS = 6, 2
# per S two draws from {0, 1, 15, 16, 17, S-1, S, S+3, -2} (S+3 and -2 are clamped; so is anything above S), each with a full row
LENGTHS = {5: ([5, 0, 1, 4, 8, -2], [4, 5, -2, 1, 0, 8]),
           8: ([7, 0, 1, 8, 11, -2], [8, 16, 7, 1, -2, 0]),
           17: ([16, 0, 17, 15, 1, 20], [17, -2, 16, 20, 1, 15]),
           33: ([32, 17, 33, -2, 15, 36], [33, 16, 1, 0, 36, 32]),
           40: ([39, 16, 40, 1, 43, 0], [40, 17, 15, -2, 0, 39])}
CASES = [(S, hd, bf) for S in LENGTHS for hd, bf in itertools.product((16, 32), (0, 1))]
IDS = ["S%d_d%d_bf%d" % c for c in CASES]
SEED, OFFSET = 4321, 23


def _lengths(S, hd, bf):
    return LENGTHS[S][(hd // 16 + bf) % 2]


def test_cases_cover_the_lengths_the_kernels_branch_on():
    for S, draws in LENGTHS.items():
        allowed = {0, 1, 15, 16, 17, S - 1, S, S + 3, -2}
        for d in draws:
            assert len(d) == N and set(d) <= allowed and S in d
        both = set(draws[0]) | set(draws[1])
        assert {0, 1, S - 1, S, S + 3, -2} <= both
        assert {v for v in (15, 16, 17) if v < S} <= both
    assert {c[0] for c in CASES} == {5, 8, 17, 33, 40}


def _inputs(S, hd, lengths, bf, garbage=float("nan")):
    """live rows from the hash filler; the padded rows of qkv and dout hold `garbage`"""
    E = HEADS * hd
    qkv = fill.hash_tensor((S * N, 3 * E), 900 + S, 1.0)
    dout = fill.hash_tensor((S * N, E), 901 + S, 1.0)
    dead = ~VR.live_rows(lengths, S, N, bool(bf))
    if isinstance(garbage, float):
        qkv[dead], dout[dead] = garbage, garbage
    else:   # (a, b): other finite and infinite garbage, varying along the row
        qkv[dead] = garbage[0] * fill.hash_tensor((int(dead.sum()), 3 * E), 77, 1.0)
        dout[dead] = garbage[1]
    return qkv, dout


def _dev_lengths(lengths):
    from .attn_abi import DEV
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)


def vforward(qkv, lengths, S, heads, bf, p=0.0, seed=0, offset=0, n=N):
    from . import attn_abi as A
    E = qkv.shape[1] // 3
    d = A.desc(S, n, heads, E // heads, bf, p)
    q, ln = A.dev(qkv), _dev_lengths(lengths)
    return A.call("ecgmm_mha_forward_varlen", {"out": (S * n, E), "lse": (n, heads, S)},
                  lambda v: (C.byref(d), ptr(q), ptr(ln), ptr(v["out"]), ptr(v["lse"]), seed, offset))


def vbackward(qkv, lengths, out, lse, dout, S, heads, bf, p=0.0, seed=0, offset=0, n=N):
    from . import attn_abi as A
    E = qkv.shape[1] // 3
    d = A.desc(S, n, heads, E // heads, bf, p)
    nb = L.lib().ecgmm_mha_bwd_workspace(C.byref(d))
    assert nb > 0 and nb % 4 == 0
    ws = A.guarded_bytes(nb)
    q, o, l, g, ln = A.dev(qkv), A.dev(out), A.dev(lse), A.dev(dout), _dev_lengths(lengths)
    r = A.call("ecgmm_mha_backward_varlen", {"dqkv": (S * n, 3 * E)},
               lambda v: (C.byref(d), ptr(q), ptr(ln), ptr(o), ptr(l), ptr(g), ptr(v["dqkv"]), ptr(ws), nb, seed, offset))
    assert not A.tail_touched(ws), "mha_backward_varlen wrote past its workspace"
    return r["dqkv"]


@functools.lru_cache(maxsize=None)
def _run(S, hd, bf, p):
    """one forward + backward with lengths on NaN padding, shared by the tests below (read only)"""
    lengths = _lengths(S, hd, bf)
    qkv, dout = _inputs(S, hd, lengths, bf)
    r = vforward(qkv, lengths, S, HEADS, bf, p, SEED, OFFSET)      # call() asserts that every output element is finite
    dqkv = vbackward(qkv, lengths, r["out"], r["lse"], dout, S, HEADS, bf, p, SEED, OFFSET)
    return lengths, qkv, dout, r, dqkv


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S,hd,bf", CASES, ids=IDS)
def test_live_rows_within_the_bounds_and_exact_zeros_in_the_padding(S, hd, bf, p):
    from . import attn_abi as A
    lengths, qkv, dout, r, dqkv = _run(S, hd, bf, p)
    keep = A.keep_mask(S, N, HEADS, hd, bf, p, SEED, OFFSET) if p > 0 else None
    live = VR.live_rows(lengths, S, N, bool(bf))
    E = HEADS * hd
    # the reference never sees the padding: NaN there would poison it if it did
    fs = VR.forward_alone(qkv, lengths, S, N, HEADS, bool(bf), keep, p)
    bs = VR.backward_alone(qkv, r["out"], r["lse"], dout, lengths, S, N, HEADS, bool(bf), keep, p)
    worst = {}
    for n, (f, bw, ln) in enumerate(zip(fs, bs, VR.clamp(lengths, S))):
        if f is None:
            continue
        rows = VR.rows(S, N, n, ln, bool(bf))
        fb, bb = AB.ForwardBounds(f), AB.BackwardBounds(bw)
        got = AR.split_heads(r["out"][rows], ln, 1, HEADS, bool(bf))
        figs = {"out": AB.ratio((got - f.out).abs(), fb.out),
                "lse": AB.ratio((r["lse"][n, :, :ln].double() - f.lse[0]).abs(), fb.lse[0])}
        for i, k in enumerate(("dq", "dk", "dv")):
            g = AR.split_heads(dqkv[rows][:, i * E:(i + 1) * E], ln, 1, HEADS, bool(bf))
            figs[k] = AB.ratio((g - getattr(bw, k)).abs(), getattr(bb, k))
        print("S%d d%d bf%d p%.2f n%d len%-2d " % (S, hd, bf, p, n, ln) + "  ".join("%s %.3g" % kv for kv in figs.items()))
        for k, v in figs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert worst and max(worst.values()) <= 1.0, "of the bound: %s" % worst
    assert bool((r["out"][~live] == 0).all()), "out is not exactly 0 at a padded query"
    pad = torch.arange(S)[None, :] >= torch.tensor(VR.clamp(lengths, S))[:, None]              # [N, S]
    assert bool((r["lse"].transpose(1, 2)[pad] == 0).all()), "lse is not 0 at a padded query"
    assert bool((dqkv[~live] == 0).all()), "dqkv is not exactly 0 at a padded position"


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S,hd,bf", [(5, 16, 0), (8, 32, 1), (17, 32, 0), (40, 16, 1)])
def test_null_and_all_full_lengths_are_the_entry_points_without_lengths(S, hd, bf, p):
    from . import attn_abi as A
    E = HEADS * hd
    qkv = fill.hash_tensor((S * N, 3 * E), 910, 1.0)
    dout = fill.hash_tensor((S * N, E), 911, 1.0)
    r0 = A.forward(qkv, S, N, HEADS, bf, p, SEED, OFFSET)
    g0 = A.backward(qkv, r0["out"], r0["lse"], dout, S, N, HEADS, bf, p, SEED, OFFSET)
    for lengths in (None, [S] * N, [S, S + 3, S, S + 1, S, S]):
        r = vforward(qkv, lengths, S, HEADS, bf, p, SEED, OFFSET)
        assert torch.equal(r["out"], r0["out"]) and torch.equal(r["lse"], r0["lse"]), lengths
        g = vbackward(qkv, lengths, r0["out"], r0["lse"], dout, S, HEADS, bf, p, SEED, OFFSET)
        assert torch.equal(g, g0), lengths


@pytest.mark.parametrize("S,hd", [(17, 16), (33, 32), (40, 16), (40, 32)])
def test_a_live_element_has_the_bits_of_the_same_element_alone(S, hd):
    """batch_first, no dropout, S > 8: an element of length >= 9 runs the tiles, in the order, of the kernels without lengths
    on that element alone with S = its length (shorter ones would take the packed form alone: left to the float64 check)"""
    from . import attn_abi as A
    lengths, qkv, dout, r, dqkv = _run(S, hd, 1, 0.0)
    seen = 0
    for n, ln in enumerate(VR.clamp(lengths, S)):
        if ln < 9:
            continue
        rows = VR.rows(S, N, n, ln, True)
        a = A.forward(qkv[rows], ln, 1, HEADS, 1)
        assert torch.equal(a["out"], r["out"][rows]) and torch.equal(a["lse"][0], r["lse"][n, :, :ln]), (n, ln)
        g = A.backward(qkv[rows], a["out"], a["lse"], dout[rows], ln, 1, HEADS, 1)
        assert torch.equal(g, dqkv[rows]), (n, ln)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("S,hd,bf,p", [(5, 32, 0, 0.25), (8, 16, 1, 0.0), (33, 16, 0, 0.25), (40, 32, 1, 0.0)])
def test_two_calls_and_another_filling_of_the_padding_give_identical_bits(S, hd, bf, p):
    lengths, qkv, dout, r, dqkv = _run(S, hd, bf, p)
    r2 = vforward(qkv, lengths, S, HEADS, bf, p, SEED, OFFSET)
    g2 = vbackward(qkv, lengths, r["out"], r["lse"], dout, S, HEADS, bf, p, SEED, OFFSET)
    assert torch.equal(r2["out"], r["out"]) and torch.equal(r2["lse"], r["lse"]) and torch.equal(g2, dqkv)
    for garbage in ((1e30, float("inf")), (-3.0, 1e38), 0.0):
        q3, d3 = _inputs(S, hd, lengths, bf, garbage)
        r3 = vforward(q3, lengths, S, HEADS, bf, p, SEED, OFFSET)
        g3 = vbackward(q3, lengths, r3["out"], r3["lse"], d3, S, HEADS, bf, p, SEED, OFFSET)
        assert torch.equal(r3["out"], r["out"]) and torch.equal(r3["lse"], r["lse"]) and torch.equal(g3, dqkv), garbage


def test_refused_calls_write_nothing():
    from . import attn_abi as A
    E = HEADS * 16
    qkv = fill.hash_tensor((4 * N, 3 * E), 912, 1.0)
    d = A.desc(4, N, HEADS, 16, 0, 1.0)                      # p_drop = 1
    q, ln = A.dev(qkv), _dev_lengths([4] * N)
    A.call("ecgmm_mha_forward_varlen", {"out": (4 * N, E), "lse": (N, HEADS, 4)},
           lambda v: (C.byref(d), ptr(q), ptr(ln), ptr(v["out"]), ptr(v["lse"]), 0, 0), expect=1)
