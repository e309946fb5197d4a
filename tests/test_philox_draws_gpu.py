"""Every device copy of Philox4x32-10 against the host generator (tests/philox_ref.py, held to the Random123 known answers by
tests/test_lime_cpu.py), draw by draw at the counter each kernel documents: dropout_fwd_kernel (csrc/head.hip), the attention
keep mask (csrc/attention.hip), weighted_sample_kernel and signal_gather_augment_kernel (csrc/physionet.hip).  LIME's draws
are compared in tests/test_lime_ops_gpu.py.  A wrong key schedule, a word from the wrong lane, a counter field built
otherwise than documented, an offset that does not carry into the high word, or two calls that share a counter block leave
every statistic intact and fail here.  Key = (low, high word of the seed); every kernel sees a seed with a high word.

Outputs are tests/exact_abi.Guarded buffers (prefilled, between sentinel zones); the mask of attention comes through
tests/attn_abi.keep_mask, which guards it the same way.

The grid-stride loop of dropout: g1d (csrc/head.hip) caps the grid at 2048 blocks of 256 threads, one thread per group of four
elements, so the forward loops only when n > 4 * 2048 * 256 = 2097152.  N_LOOP = 2097153 is the smallest such n (the backward,
one thread per element, loops from n = 524289 on); n = 300001 fills 293 blocks without looping.

Augmentation noise.  The noise of OUTPUT elements 4g .. 4g+3 of row i comes from block (offset, i, 0x80000000 | g), as
signal_gather_augment_kernel documents: the deviate is keyed by where it lands, not by the source sample under it (the two
readings agree for a row that is not rolled; the noise is i.i.d., so the law of the result is the same).  With src = 0 a row
with the noise flag holds out[o] = sigma * z[o] * scale.  Elements 4g, 4g+1 come from words (r0, r1), 4g+2, 4g+3 from (r2, r3):
u = (float32(w0 >> 8) + 1) * 2^-24, z0 = sqrt(-2 ln u) cos(2 pi u01(w1)), z1 the same with sin.  The kernel evaluates this with
__logf / __cosf / __sinf and an fp32 angle; the reference evaluates the same formula from the same words in float64.
Measured on gfx950 (MI355X) at the first run, 600 rows of 3000 and of 1021 samples, 1.22 million deviates: worst
|z - z_ref| = 1.727e-06 (1.651e-06 at L = 1021), of which about 6e-07 is the two fp32 roundings of sigma * z * scale at
|z| = 5.  NOISE_BAR = 8 x 1.727e-06 = 1.3816e-05, far below the 1e-3 it may not exceed; a deviate taken from a wrong word or
block differs by order 1."""
import functools

import numpy as np
import pytest
import torch

import ecgmm.hip.functional as HF
from ecgmm import preprocess as PP
from ecgmm.hip import lib as L
from ecgmm.hip.functional import stream

from . import attn_abi as A
from . import philox_ref as P
from .exact_abi import DEV, Guarded, dev_bits, dptr

pytestmark = pytest.mark.gpu

SEED_LO = 20261019                  # high word 0
SEED_HI = 0x9E3779B97F4A7C15        # high word set: k1 enters the key schedule
N_LOOP = 2097153
NOISE_WORST = 1.727e-06             # worst |z - z_ref| of the first run on the MI355X
NOISE_BAR = 8 * NOISE_WORST


def words(seed, ctr):
    """[blocks, 4] uint64 of the blocks at counters ctr"""
    return np.stack(P.philox4x32_10(P.key(seed), ctr), axis=-1)


# ---- dropout --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def dropout_words(seed, offset, n):
    """word of element e = word e % 4 of the block at (offset + e // 4, 0, 0)"""
    return words(seed, P.ctr_dropout(offset, np.arange((n + 3) // 4, dtype=np.uint64))).reshape(-1)[:n]


def host_dropout(x, p, seed, offset):
    keep = P.u01(dropout_words(seed, offset, x.size)) >= np.float32(p)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    return keep, np.where(keep, x * scale, np.float32(0.0))


DROP_OFFSETS = [(0, SEED_LO), (7, SEED_HI), (2 ** 32 - 2, SEED_HI), (2 ** 40 + 3, SEED_LO)]


@pytest.mark.parametrize("offset,seed", DROP_OFFSETS, ids=["0", "7", "2^32-2", "2^40+3"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 300001, N_LOOP])
def test_dropout_forward_and_backward(n, offset, seed):
    assert ((N_LOOP + 3) // 4 > 2048 * 256) and ((N_LOOP - 1 + 3) // 4 <= 2048 * 256)      # the mirror of g1d's cap
    rng = np.random.default_rng(n)
    x, dy = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    x[::13] = -0.0
    xs, dys = dev_bits(x), dev_bits(dy)
    lib = L.lib()
    if offset == 2 ** 32 - 2 and n >= 16:       # the carry into the high counter word happens inside this call
        lo, hi = P.split64(np.uint64(offset) + np.arange((n + 3) // 4, dtype=np.uint64))
        assert int(hi[0]) == 0 and int(hi[-1]) == 1 and int(lo[2]) == 0
    for p in (0.0, 0.3, 0.5):
        keep, want = host_dropout(x, p, seed, offset)
        y, mask = Guarded(n, "f32"), Guarded(n, "u8")
        L.check(lib.ecgmm_dropout_fwd(dptr(xs), y.ptr, mask.ptr, n, p, seed, offset, stream()), "dropout_fwd")
        got_mask = mask.done("dropout mask")
        assert np.array_equal(got_mask, keep.astype(np.uint8)), "dropout mask: n=%d p=%g offset=%d" % (n, p, offset)
        assert np.array_equal(y.done("dropout y"), want.view(np.uint32)), "dropout y: n=%d p=%g offset=%d" % (n, p, offset)
        if p == 0.0:
            assert bool(keep.all())
        elif n == N_LOOP:
            assert abs(keep.mean() - (1 - p)) < 0.002
        dx = Guarded(n, "f32")
        L.check(lib.ecgmm_dropout_bwd(dptr(dys), mask.ptr, dx.ptr, n, p, stream()), "dropout_bwd")
        _, want_dx = host_dropout(dy, p, seed, offset)
        assert np.array_equal(dx.done("dropout dx"), want_dx.view(np.uint32)), "dropout dx: n=%d p=%g offset=%d" % (n, p, offset)


def test_consecutive_dropout_calls_continue_the_stream():
    """HF.dropout of 10 elements takes ceil(10 / 4) = 3 blocks: the second call starts at offset 3, no reuse and no gap"""
    saved = (HF._PhiloxState.seed, HF._PhiloxState.offset)
    try:
        for seed in (SEED_LO, SEED_HI):
            HF.manual_seed(seed)
            x = torch.ones(10, device=DEV)
            masks = [(HF.dropout(x, 0.5, True) != 0).cpu().numpy() for _ in range(2)]
            assert HF._PhiloxState.offset == 6
            for off, m in zip((0, 3), masks):
                assert np.array_equal(m, P.u01(dropout_words(seed, off, 10)) >= np.float32(0.5)), (seed, off)
            assert not np.array_equal(masks[0], masks[1])
    finally:
        HF._PhiloxState.seed, HF._PhiloxState.offset = saved


# ---- the attention keep mask -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,seed", [(17, SEED_HI), (2 ** 32 + 5, SEED_LO)], ids=["17", "2^32+5"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 4), (8, 50, 4), (16, 2, 2), (17, 3, 4), (130, 1, 2)],
                         ids=lambda s: "S%d-N%d-h%d" % s)
def test_attention_keep_mask(shape, offset, seed):
    """S = 8 is the packed path (two pairs to a wave); 5, 17 and 130 leave a ragged last block of four keys"""
    S, N, heads = shape
    SB = (S + 3) // 4
    pair = np.arange(N * heads, dtype=np.uint64)[:, None, None]
    q = np.arange(S, dtype=np.uint64)[None, :, None]
    kb = np.arange(SB, dtype=np.uint64)[None, None, :]
    w = words(seed, P.ctr_attention(offset, pair, q * np.uint64(SB) + kb))            # [P, S, SB, 4]: word = key % 4
    u = P.u01(w.reshape(N * heads, S, SB * 4)[:, :, :S]).reshape(N, heads, S, S)
    for batch_first in (False, True):
        for p in (0.1, 0.25):
            got = A.keep_mask(S, N, heads, 16, batch_first, p, seed, offset).numpy()
            assert np.array_equal(got, (u >= np.float32(p)).astype(np.uint8)), (shape, batch_first, p, offset)


# ---- the weighted sampler --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,seed", [(0, SEED_HI), (2 ** 33 + 1, SEED_LO)], ids=["0", "2^33+1"])
def test_weighted_sample_uniforms(offset, seed):
    """tests/test_ptbxl_gpu.py ties each index to its uniform; this ties the uniform to the stream (and the index again)"""
    count = 1000                                                     # four workgroups
    w = np.random.default_rng(3).random(37)
    w[[0, 5, 36]] = 0.0
    cdf, last = PP.weight_cdf(w)
    cdf_d = torch.from_numpy(cdf).to(DEV)
    out, u = Guarded(count, "i64"), Guarded(count, "f64")
    L.check(L.lib().ecgmm_weighted_sample(dptr(cdf_d), len(cdf), last, out.ptr, u.ptr, count, seed, offset, stream()),
            "weighted_sample")
    r = words(seed, P.ctr_tag(offset, np.arange(count, dtype=np.uint64), P.TAG_SAMPLE))
    want = P.u53(r[:, 0], r[:, 1])
    got = u.done("u_out")
    assert np.array_equal(got, want.view(np.uint64))
    idx = np.minimum(np.searchsorted(cdf, want * cdf[-1], side="right"), len(cdf))
    assert np.array_equal(out.done("out").view(np.int64), np.where(idx < len(cdf), idx, last))


# ---- gather + augment --------------------------------------------------------------------------------------------------------
AUG = dict(sigma=0.01, scale=(0.8, 1.2), shift=(-10, 10))


def augment(src, index, p, seed, offset):
    """the C entry point on guarded outputs -> (out [B, L] fp32 bits, dec [B, 4] fp32)"""
    n, Ln = src.shape
    B = index.size
    s, ix = dev_bits(src), torch.from_numpy(index).to(DEV)
    out, dec = Guarded(B * Ln, "f32"), Guarded(B * 4, "f32")
    L.check(L.lib().ecgmm_signal_gather_augment(dptr(s), n, Ln, dptr(ix), B, out.ptr, dec.ptr, 1, p, AUG["sigma"], AUG["scale"][0],
                                                AUG["scale"][1], AUG["shift"][0], AUG["shift"][1], seed, offset, stream()),
            "signal_gather_augment")
    return out.done("augment out").reshape(B, Ln), dec.done("augment decisions").view(np.float32).reshape(B, 4)


def host_decisions(B, p, seed, offset):
    """-> flags [B], shift [B], the two admissible fp32 scales ([B] fused, [B] every product rounded)"""
    i = np.arange(B, dtype=np.uint64)
    r = words(seed, P.ctr_tag(offset, i, P.TAG_ROW_R))
    q = words(seed, P.ctr_tag(offset, i, P.TAG_ROW_Q))
    pf = np.float32(p)
    flags = ((P.u01(r[:, 0]) < pf).astype(np.int64) | (P.u01(r[:, 1]) < pf).astype(np.int64) << 1
             | (P.u01(r[:, 2]) < pf).astype(np.int64) << 2)
    lo, hi = np.float32(AUG["scale"][0]), np.float32(AUG["scale"][1])
    shift_lo, shift_n = AUG["shift"][0], AUG["shift"][1] - AUG["shift"][0]
    shift = np.where(flags & 4, shift_lo + ((q[:, 1] * np.uint64(shift_n)) >> np.uint64(32)).astype(np.int64), 0)
    u, width = P.u01(q[:, 0]), hi - lo                                                   # width: one fp32 subtraction
    exact = u.astype(np.float64) * np.float64(width)                                       # 24 x 24 bits: exact
    fused = (np.float64(lo) + exact).astype(np.float32)
    plain = lo + exact.astype(np.float32)
    wrap = lambda s: np.where(flags & 2, np.where(s >= hi, lo, s), np.float32(1.0)).astype(np.float32)  # noqa: E731
    return flags, shift, wrap(fused), wrap(plain)


def check_decisions(dec, B, p, seed, offset):
    """flags and shift exact; the scale one of the two fp32 roundings, the same one in every row -> the scale in use"""
    flags, shift, fused, plain = host_decisions(B, p, seed, offset)
    assert np.array_equal(dec[:, 3], flags.astype(np.float32)) and np.array_equal(dec[:, 0], (flags & 1).astype(np.float32))
    assert np.array_equal(dec[:, 2], shift.astype(np.float32))
    got = dec[:, 1].view(np.uint32)
    f, pl = fused.view(np.uint32), plain.view(np.uint32)
    assert bool((got == f).all()) or bool((got == pl).all()), "scale: %d rows differ from the fused, %d from the unfused value" % (
        int((got != f).sum()), int((got != pl).sum()))
    for bit in (1, 2, 4):
        assert 0.3 * B * p < int(((flags & bit) > 0).sum()) < min(B, 3 * B * p)           # each decision is drawn in many rows
    assert len(set(shift[(flags & 4) > 0].tolist())) > 10
    return flags, shift, dec[:, 1]


@pytest.mark.parametrize("Ln,p,offset,seed", [(3000, 0.5, 9, SEED_HI), (1021, 0.3, 2 ** 32 + 5, SEED_LO)], ids=["L3000", "L1021"])
def test_augment_row_decisions(Ln, p, offset, seed):
    B, n = 600, 40
    rng = np.random.default_rng(Ln)
    src = rng.standard_normal((n, Ln)).astype(np.float32)
    index = rng.integers(0, n, B).astype(np.int64)
    out, dec = augment(src, index, p, seed, offset)
    flags, shift, scale = check_decisions(dec, B, p, seed, offset)
    # rows without noise are exact: one fp32 multiply, then the roll out[(t + shift) mod L] = v[t]
    for i in np.nonzero((flags & 1) == 0)[0]:
        v = src[index[i]] * scale[i] if flags[i] & 2 else src[index[i]]
        assert np.array_equal(out[i], np.roll(v, shift[i]).view(np.uint32)), "row %d" % i
    # the Python wrapper makes the same call
    o2, d2 = PP.gather_augment(torch.from_numpy(src).to(DEV), torch.from_numpy(index), augment=True, p=p, return_decisions=True,
                               seed_offset=(seed, offset), **AUG)
    assert np.array_equal(o2.cpu().numpy().view(np.uint32), out) and np.array_equal(d2.cpu().numpy(), dec)


def host_deviates(seed, offset, row, Ln):
    """float64 Box-Muller deviates of output elements 0 .. L-1 of row `row`"""
    G = (Ln + 3) // 4
    r = words(seed, P.ctr_noise(offset, row, np.arange(G, dtype=np.uint64)))              # [G, 4]
    w0, w1 = r[:, [0, 2]].reshape(-1), r[:, [1, 3]].reshape(-1)                            # pairs (r0, r1), (r2, r3)
    u = ((w0 >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u))
    ang = 2.0 * np.pi * P.u01(w1).astype(np.float64)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1)[:Ln]


@pytest.mark.parametrize("Ln,offset,seed", [(3000, 2 ** 32 + 5, SEED_HI), (1021, 9, SEED_LO)], ids=["L3000", "L1021"])
def test_augment_noise_deviates(Ln, offset, seed):
    B, p = 600, 0.5
    src = np.zeros((3, Ln), dtype=np.float32)
    index = (np.arange(B) % 3).astype(np.int64)
    out, dec = augment(src, index, p, seed, offset)
    flags, shift, scale = check_decisions(dec, B, p, seed, offset)
    out = out.view(np.float32)
    noisy = np.nonzero(flags & 1)[0]
    assert np.array_equal(out[(flags & 1) == 0], np.zeros((B - noisy.size, Ln), dtype=np.float32))
    assert noisy.size * Ln >= 100000 and bool(((flags[noisy] & 4) > 0).any()) and bool((shift[noisy] != 0).any())
    worst = 0.0
    for i in noisy:
        z = out[i].astype(np.float64) / (np.float64(np.float32(AUG["sigma"])) * np.float64(scale[i]))
        worst = max(worst, float(np.abs(z - host_deviates(seed, offset, int(i), Ln)).max()))
    print("augmentation noise, L=%d: %d deviates, worst |z - z_ref| = %.3e (bar %.3e)" % (Ln, noisy.size * Ln, worst, NOISE_BAR))
    assert NOISE_BAR <= 1e-3
    assert worst <= NOISE_BAR
