"""csrc/attention.hip through the C ABI on the GPU: forward and backward element by element against the float64 restatement
(tests/attn_ref.py) within the derived bounds (tests/attn_bounds.py), between sentinel zones with NaN-prefilled outputs
(tests/attn_abi.py); determinism; the dropout decisions; the embedding kernel against float64 conv1d."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import fill

from . import attn_bounds as AB
from . import attn_ref as AR
from . import f64check as FC

pytestmark = pytest.mark.gpu

S_EDGES = (1, 5, 15, 16, 17, 63, 64, 65, 130)
# every S with both layouts and both head sizes; N and heads alternate over the pairs instead of running the full cube
EDGE_CASES = [(S, (1, 3)[(i + bf + hd // 16) % 2], (1, 4)[(i + bf) % 2], hd, bf)
              for i, S in enumerate(S_EDGES) for bf, hd in itertools.product((0, 1), (16, 32))]


def _inputs(S, N, heads, hd, salt=0):
    E = heads * hd
    qkv = fill.hash_tensor((S * N, 3 * E), 700 + salt, 1.0)
    dout = fill.hash_tensor((S * N, E), 701 + salt, 1.0)
    return qkv, dout


def _check_forward(r, f, name):
    b = AB.ForwardBounds(f)
    got = AR.split_heads(r["out"], f.S, f.N, f.heads, f.batch_first)
    ro = AB.ratio((got - f.out).abs(), b.out)
    rl = AB.ratio((r["lse"].double() - f.lse).abs(), b.lse)
    seen = AB.seen_units(got, f.out, f.Aout)
    print("%-40s out %.3g  lse %.3g of the bound (out: %.2f u A_out seen)" % (name, ro, rl, seen))
    assert ro <= 1.0 and rl <= 1.0, "%s: out %.3g, lse %.3g of the bound" % (name, ro, rl)
    return ro, rl


def _check_backward(dqkv, bw, name):
    b = AB.BackwardBounds(bw)
    f = bw.f
    E = f.heads * f.d
    rs = {}
    for i, k in enumerate(("dq", "dk", "dv")):
        got = AR.split_heads(dqkv[:, i * E:(i + 1) * E], f.S, f.N, f.heads, f.batch_first)
        rs[k] = AB.ratio((got - getattr(bw, k)).abs(), getattr(b, k))
    print("%-40s dq %.3g  dk %.3g  dv %.3g of the bound" % (name, rs["dq"], rs["dk"], rs["dv"]))
    assert max(rs.values()) <= 1.0, "%s: %s of the bound" % (name, rs)
    return rs


def _both(qkv, dout, S, N, heads, bf, name, p=0.0, keep=None, seed=0, offset=0):
    from . import attn_abi as A
    r = A.forward(qkv, S, N, heads, bf, p, seed, offset)
    f = AR.Forward(qkv, S, N, heads, bool(bf), keep, p)
    _check_forward(r, f, name + " fwd")
    dqkv = A.backward(qkv, r["out"], r["lse"], dout, S, N, heads, bf, p, seed, offset)
    bw = AR.Backward(qkv, r["out"], r["lse"].reshape(-1), dout, S, N, heads, bool(bf), keep, p)
    _check_backward(dqkv, bw, name + " bwd")
    return r, dqkv, f


@pytest.mark.parametrize("S,N,heads,hd,bf", EDGE_CASES, ids=["S%d_N%d_h%d_d%d_bf%d" % c for c in EDGE_CASES])
def test_tile_edges(S, N, heads, hd, bf):
    qkv, dout = _inputs(S, N, heads, hd, S)
    _both(qkv, dout, S, N, heads, bf, "S%d N%d h%d d%d bf%d" % (S, N, heads, hd, bf))


def test_edge_cases_cover_every_size_with_both_layouts_and_head_sizes():
    for S in S_EDGES:
        assert {(hd, bf) for s, _, _, hd, bf in EDGE_CASES if s == S} == set(itertools.product((16, 32), (0, 1)))
    assert {c[1] for c in EDGE_CASES} == {1, 3} and {c[2] for c in EDGE_CASES} == {1, 4}


@pytest.mark.parametrize("hd,bf", [(32, 0), (16, 1)])
def test_tiny_sequence_many_pairs(hd, bf):
    """the reference's regime shrunk: S = 8, several (n, head) pairs share one wave"""
    S, N, heads = 8, 300, 4
    qkv, dout = _inputs(S, N, heads, hd, 8)
    _both(qkv, dout, S, N, heads, bf, "S8 N300 h4 d%d bf%d" % (hd, bf))


def test_late_and_early_maximum_over_many_key_tiles():
    S, N, heads, hd = 300, 1, 2, 16
    qkv, dout = _inputs(S, N, heads, hd, 300)
    qkv = qkv * 0.5
    E = heads * hd
    e0, e1 = torch.zeros(hd), torch.zeros(hd)
    e0[0], e1[1] = 6.0, 6.0
    for h in range(heads):
        qkv[0, h * hd:(h + 1) * hd] = e0                       # query 0: key 299 (the last tile) dominates
        qkv[299, E + h * hd:E + (h + 1) * hd] = e0
        qkv[1, h * hd:(h + 1) * hd] = e1                       # query 1: key 3 (the first tile) dominates
        qkv[3, E + h * hd:E + (h + 1) * hd] = e1
    f = AR.Forward(qkv, S, N, heads, False)
    assert int(f.s[0, 0, 0].argmax()) == 299 and int(f.s[0, 0, 1].argmax()) == 3
    assert float(f.P[0, 0, 0, 299]) > 0.9 and float(f.P[0, 0, 1, 3]) > 0.9
    _both(qkv, dout, S, N, heads, 0, "S300 late / early max")


def test_large_scores_stay_finite_and_rows_sum_to_one():
    """q . k = +-80 before scaling; column 0 of every head's V is 1, so that output column is the row sum of P"""
    S, N, heads, hd = 40, 2, 2, 16
    E = heads * hd
    qkv, dout = _inputs(S, N, heads, hd, 80)
    sign = torch.where(fill.hash_tensor((S * N, 1), 780, 1.0) > 0, 1.0, -1.0)
    qkv[:, :E] = 2.5 * sign                                     # 2.5 * 2 * 16 = 80 exactly
    qkv[:, E:2 * E] = 2.0 * sign
    f = AR.Forward(qkv, S, N, heads, False)
    assert abs(float(f.s.abs().max()) / f.scale - 80.0) < 1e-9
    qkv[:, 2 * E::hd] = 1.0
    r, dqkv, f = _both(qkv, dout, S, N, heads, 0, "scores +-80")      # call() asserts that every output is finite
    b = AB.ForwardBounds(f)
    got = AR.split_heads(r["out"], S, N, heads, False)[..., 0]
    assert AB.ratio((got - 1.0).abs(), b.out[..., 0]) <= 1.0


@pytest.mark.parametrize("S,N,heads,hd,bf,p", [(37, 2, 4, 16, 0, 0.0), (8, 50, 4, 32, 0, 0.0), (37, 2, 4, 32, 1, 0.25)])
def test_two_calls_give_identical_bits(S, N, heads, hd, bf, p):
    from . import attn_abi as A
    qkv, dout = _inputs(S, N, heads, hd, 5)
    r1, r2 = (A.forward(qkv, S, N, heads, bf, p, 3, 9) for _ in range(2))
    assert torch.equal(r1["out"], r2["out"]) and torch.equal(r1["lse"], r2["lse"])
    g1, g2 = (A.backward(qkv, r1["out"], r1["lse"], dout, S, N, heads, bf, p, 3, 9) for _ in range(2))
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("S,N,heads,hd,bf", [(37, 3, 4, 16, 0), (5, 7, 4, 32, 1), (130, 1, 2, 32, 0)])
def test_dropout(S, N, heads, hd, bf):
    from . import attn_abi as A
    p, seed, off = 0.25, 1234, 17
    m1 = A.keep_mask(S, N, heads, hd, bf, p, seed, off)
    m2 = A.keep_mask(S, N, heads, hd, bf, p, seed, off)
    m3 = A.keep_mask(S, N, heads, hd, bf, p, seed, off + 1)
    assert torch.equal(m1, m2) and not torch.equal(m1, m3)
    n = m1.numel()
    share, sigma = float(m1.double().mean()), (p * (1 - p) / n) ** 0.5
    print("kept share %.5f of %d, 1 - p = %.2f, sigma %.5f" % (share, n, 1 - p, sigma))
    assert abs(share - (1 - p)) <= 5 * sigma
    qkv, dout = _inputs(S, N, heads, hd, 25)
    _both(qkv, dout, S, N, heads, bf, "dropout S%d" % S, p=p, keep=m1, seed=seed, offset=off)


def test_refused_descriptors_write_nothing():
    from . import attn_abi as A
    qkv, _ = _inputs(4, 1, 1, 16)
    A.forward(qkv[:, :36].contiguous(), 4, 1, 1, False, expect=1)          # head_dim 12
    A.forward(qkv, 4, 1, 1, False, p=1.0, expect=1)


EMBED_CASES = list(itertools.product((1, 3), (1, 2, 47, 300), (64, 128)))


@pytest.mark.parametrize("Cin,Ln,D", EMBED_CASES, ids=["c%d_L%d_d%d" % c for c in EMBED_CASES])
def test_embed1d(Cin, Ln, D):
    from . import attn_abi as A
    B, pos_len = 3, Ln + 2
    x = fill.hash_tensor((B, Cin, Ln), 740, 1.0)
    w = fill.hash_tensor((D, Cin, 3), 741, 0.5)
    b = fill.hash_tensor((D,), 742, 0.5)
    pos = fill.hash_tensor((1, pos_len, D), 743, 0.3)
    dy = fill.hash_tensor((B, Ln, D), 744, 1.0)
    x64, w64, b64, p64, g64 = (t.double() for t in (x, w, b, pos, dy))
    ref = F.conv1d(x64, w64, b64, padding=1).permute(0, 2, 1) + p64[:, :Ln]
    mag = F.conv1d(x64.abs(), w64.abs(), b64.abs(), padding=1).permute(0, 2, 1) + p64[:, :Ln].abs()
    y = A.embed_fwd(x, w, b, pos)
    FC.check_dot(y, ref, mag, 3 * Cin + 2, "embed1d fwd")
    r = A.embed_bwd(x, w, dy, pos_len)
    gc = g64.permute(0, 2, 1)                                                    # [B, D, L]
    xp = F.pad(x64, (1, 1))
    win = torch.stack([xp[:, :, k:k + Ln] for k in range(3)], dim=-1)            # [B, Cin, L, 3]
    FC.check_dot(r["dw"], torch.einsum("bdl,bclk->dck", gc, win), torch.einsum("bdl,bclk->dck", gc.abs(), win.abs()),
                 B * Ln, "embed1d dw")
    FC.check_dot(r["db"], gc.sum((0, 2)), gc.abs().sum((0, 2)), B * Ln, "embed1d db")
    dpos = torch.zeros(pos_len, D, dtype=torch.float64)
    dpos[:Ln] = g64.sum(0)
    mpos = torch.zeros(pos_len, D, dtype=torch.float64)
    mpos[:Ln] = g64.abs().sum(0)
    FC.check_dot(r["dpos"], dpos, mpos, B, "embed1d dpos")
    FC.check_dot(r["dx"], F.conv_transpose1d(gc, w64, padding=1), F.conv_transpose1d(gc.abs(), w64.abs(), padding=1), 3 * D,
                 "embed1d dx")
    r2 = A.embed_bwd(x, w, dy, pos_len, null=("dx", "dpos"))
    assert torch.equal(r2["dw"], r["dw"]) and torch.equal(r2["db"], r["db"])
