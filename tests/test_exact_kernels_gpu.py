"""The kernels whose right answer is a bit pattern, and on which every float64 check of the suite stands: ecgmm_cast,
ecgmm_uncast, ecgmm_nchw_to_nhwc, ecgmm_nhwc_to_nchw, ecgmm_pack_conv_weight (tests/util.py sends the operands and results
of every conv, BatchNorm and pool check through these), ecgmm_bcast_rows and ecgmm_axpby.

References are torch / numpy on the CPU; results are compared as integers, so -0 and NaN payloads count.  Every device
output is a tests/exact_abi.Guarded buffer: NaN-prefilled between sentinel zones.

The rounding table: all 65536 upper halves x the lower halves {0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF} as fp32 bit
patterns, 393216 values: every tie to bf16, both neighbours of every tie, +-inf, 1534 NaNs, +-0, the fp32 subnormals and the
finite values that round to infinity.  Expected bf16: torch's CPU .to(torch.bfloat16), which test_rounding_table_references
holds to the integer rule (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on every entry that is not a NaN.  A NaN must give a
NaN; its payload is free.

What the table showed on gfx950 (first run of this module): the device rounding (f2bf = v_cvt_pk_bf16_f32, scalar stores and
pack16<bf16_t>) agrees with torch on all 391682 non-NaN entries -- ties to even, overflow to infinity, +-0 and the
subnormals, which are kept, not flushed -- and every NaN stays a NaN.

ecgmm_axpby with b == 0 is a * x + 0.0f in fp32, which the compiler contracts to fma(a, x, +0) or not: the value is the one
multiply either way and only the sign of a zero result differs; the inputs hold -0 and products that underflow so both
cases are pinned (test_axpby_scale_does_not_read_y)."""
import numpy as np
import pytest
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import stream

from .exact_abi import Guarded, dev_bits, dptr

pytestmark = pytest.mark.gpu
KIND = {L.F32: "f32", L.BF16: "bf16"}
ERR_DTYPE = 2
BAD_DTYPE = 7
DTYPES = [L.F32, L.BF16]
ids_dt = lambda dt: KIND[dt] if dt in KIND else None  # noqa: E731


# ---- references ---------------------------------------------------------------------------------------------------------
def rounding_table():
    hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    return (hi[:, None] | lo[None, :]).reshape(-1)


TABLE = rounding_table()


def is_nan32(b):
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def is_nan16(b):
    return (b & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def rne_torch(bits32):
    """fp32 bit patterns -> bf16 bit patterns, torch's CPU conversion"""
    t = torch.from_numpy(np.ascontiguousarray(bits32).view(np.float32).copy())
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).reshape(bits32.shape)


def rne_integer(bits32):
    b = bits32.astype(np.uint64)
    return (((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def widen(bits16):
    return bits16.astype(np.uint32) << np.uint32(16)


def store_bits(f32_bits, dt):
    """what a kernel that stores the fp32 values `f32_bits` as dt must write"""
    return f32_bits if dt == L.F32 else rne_torch(f32_bits)


def assert_bits(got, want, what):
    """equal bit for bit; where `want` is a NaN any NaN is accepted (the payload is free), and nothing else"""
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = is_nan32(want) if want.dtype == np.uint32 else is_nan16(want)
    bad = np.nonzero((got != want) & ~nan)[0]
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x, want %#x" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])
    gn = is_nan32(got[nan]) if want.dtype == np.uint32 else is_nan16(got[nan])
    assert bool(gn.all()), "%s: a NaN input did not give a NaN" % what


def assert_exact(got, want, what):
    """equal bit for bit, NaN payloads included"""
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x, want %#x" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def draw_table(rng, n):
    """n unrounded fp32 bit patterns: table entries (ties, NaNs, infinities, subnormals) among random finite values"""
    out = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    pick = rng.random(n) < 0.5
    out[pick] = TABLE[rng.integers(0, TABLE.size, int(pick.sum()))]
    return out


def finite_values(rng, shape):
    """normal-range fp32 values over a few binades whose products with the test scales neither overflow nor underflow"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, shape))).astype(np.float32)


# ---- the table itself ---------------------------------------------------------------------------------------------------
def test_rounding_table_references():
    assert TABLE.size == 393216 and int(is_nan32(TABLE).sum()) == 1534
    ok = ~is_nan32(TABLE)
    assert np.array_equal(rne_torch(TABLE)[ok], rne_integer(TABLE)[ok])
    assert bool(is_nan16(rne_torch(TABLE)[~ok]).all())
    t = rne_torch(TABLE)
    assert int((t[ok] == 0x7F80).sum()) > 1 and int((t[ok] == 0xFF80).sum()) > 1      # finite values that round to +-inf
    sub = ok & ((TABLE & np.uint32(0x7F800000)) == 0) & ((TABLE & np.uint32(0x007FFFFF)) != 0)
    assert int(sub.sum()) == 2 * (128 * 6 - 1) and int((t[sub] != 0).sum()) > 0 and int(((t[sub] & 0x7FFF) == 0).sum()) > 0


# ---- cast / uncast --------------------------------------------------------------------------------------------------------
def _cast(dt, src_bits, expect=0):
    src = dev_bits(src_bits)
    out = Guarded(src_bits.size, KIND.get(dt, "f32"))
    rc = L.lib().ecgmm_cast(dt, dptr(src), out.ptr, src_bits.size, stream())
    assert rc == expect, (rc, L.lib().ecgmm_last_error())
    return out


def _uncast(dt, src_bits, expect=0):
    src = dev_bits(src_bits)
    out = Guarded(src_bits.size, "f32")
    rc = L.lib().ecgmm_uncast(dt, dptr(src), out.ptr, src_bits.size, stream())
    assert rc == expect, (rc, L.lib().ecgmm_last_error())
    return out


SUB = TABLE[3::1531]        # 257 entries spread over the table: 257 = one block and one element


@pytest.mark.parametrize("n", [393216, 257, 1])
def test_cast_bf16_rounds_to_nearest_even(n):
    src = TABLE if n == TABLE.size else SUB[:n] if n > 1 else np.array([0x3F818000], dtype=np.uint32)   # n = 1: a tie that goes up
    assert src.size == n
    want = rne_torch(src)
    ok = ~is_nan32(src)
    assert np.array_equal(want[ok], rne_integer(src)[ok])          # the two references agree
    got = _cast(L.BF16, src).done("cast")
    assert_bits(got, want, "cast bf16, n=%d" % n)
    if n == 1:
        assert got[0] == 0x3F82


def test_uncast_bf16_is_the_exact_widening():
    pat = np.arange(65536, dtype=np.uint16)
    assert_exact(_uncast(L.BF16, pat).done("uncast"), widen(pat), "uncast bf16")
    for n in (1, 257):
        assert_exact(_uncast(L.BF16, pat[32000:32000 + n]).done("uncast"), widen(pat[32000:32000 + n]), "uncast bf16, n=%d" % n)


@pytest.mark.parametrize("n", [393216, 257, 1])
def test_cast_and_uncast_fp32_copy_bits(n):
    src = TABLE if n == TABLE.size else SUB[:n] if n > 1 else np.array([0x7FA00001], dtype=np.uint32)   # n = 1: a signalling NaN
    assert_exact(_cast(L.F32, src).done("cast"), src, "cast fp32")
    assert_exact(_uncast(L.F32, src).done("uncast"), src, "uncast fp32")


def test_bad_dtype_is_refused_and_writes_nothing():
    src = SUB.copy()
    assert _cast(BAD_DTYPE, src, expect=ERR_DTYPE).untouched()
    assert _uncast(BAD_DTYPE, src, expect=ERR_DTYPE).untouched()
    lib = L.lib()
    s, out, out2 = dev_bits(src), Guarded(256, "f32"), Guarded(256, "f32")
    assert lib.ecgmm_nchw_to_nhwc(BAD_DTYPE, dptr(s), out.ptr, 2, 8, 16, stream()) == ERR_DTYPE and out.untouched()
    assert lib.ecgmm_nhwc_to_nchw(BAD_DTYPE, dptr(s), out.ptr, 2, 8, 16, stream()) == ERR_DTYPE and out.untouched()
    assert lib.ecgmm_pack_conv_weight(BAD_DTYPE, dptr(s), out.ptr, out2.ptr, 4, 8, 8, stream()) == ERR_DTYPE
    assert out.untouched() and out2.untouched()
    assert lib.ecgmm_bcast_rows(BAD_DTYPE, dptr(s), out.ptr, 2, 16, 8, 1.0, stream()) == ERR_DTYPE and out.untouched()   # vec path
    assert lib.ecgmm_bcast_rows(BAD_DTYPE, dptr(s), out.ptr, 2, 16, 7, 1.0, stream()) == ERR_DTYPE and out.untouched()   # scalar path


# ---- NCHW <-> NHWC --------------------------------------------------------------------------------------------------------
# every combination of full and ragged 32-tiles on both axes, and N > 1
LAYOUT_SHAPES = [(1, 1, 1), (2, 3, 50), (1, 12, 1000), (3, 31, 33), (2, 32, 32), (1, 33, 31), (2, 64, 65), (1, 72, 97),
                 (2, 128, 1), (1, 512, 7)]


@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nchw_to_nhwc(shape, dt):
    N, Cn, HW = shape
    rng = np.random.default_rng(1000 + Cn * HW + N)
    x = draw_table(rng, N * Cn * HW).reshape(N, Cn, HW)            # unrounded
    src = dev_bits(x)
    out = Guarded(x.size, KIND[dt])
    L.check(L.lib().ecgmm_nchw_to_nhwc(dt, dptr(src), out.ptr, N, Cn, HW, stream()))
    perm = np.ascontiguousarray(x.transpose(0, 2, 1))
    if dt == L.F32:
        assert_exact(out.done("nchw_to_nhwc"), perm, "nchw_to_nhwc fp32 %s" % (shape,))     # the exact permutation of any bits
    else:
        assert_bits(out.done("nchw_to_nhwc"), rne_torch(perm), "nchw_to_nhwc bf16 %s" % (shape,))


@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nhwc_to_nchw(shape, dt):
    N, Cn, HW = shape
    rng = np.random.default_rng(2000 + Cn * HW + N)
    if dt == L.F32:
        x = draw_table(rng, N * HW * Cn).reshape(N, HW, Cn)
        want = x
    else:
        x = rng.integers(0, 65536, (N, HW, Cn)).astype(np.uint16)  # any bf16 pattern, NaNs and subnormals among them
        want = widen(x)
    src = dev_bits(x)
    out = Guarded(x.size, "f32")
    L.check(L.lib().ecgmm_nhwc_to_nchw(dt, dptr(src), out.ptr, N, Cn, HW, stream()))
    assert_exact(out.done("nhwc_to_nchw"), np.ascontiguousarray(want.transpose(0, 2, 1)), "nhwc_to_nchw %s %s" % (KIND[dt], shape))


# ---- weight packing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 3), (7, 5, 9), (33, 31, 25), (64, 32, 1)], ids=lambda s: "x".join(map(str, s)))
def test_pack_conv_weight(shape, dt):
    Cout, Cin, RS = shape
    rng = np.random.default_rng(3000 + Cout * Cin * RS)
    w = draw_table(rng, Cout * Cin * RS).reshape(Cout, Cin, RS)    # unrounded
    src = dev_bits(w)
    want_f = store_bits(np.ascontiguousarray(w.transpose(0, 2, 1)), dt)      # [Cout][RS][Cin]
    want_d = store_bits(np.ascontiguousarray(w.transpose(1, 2, 0)), dt)      # [Cin][RS][Cout]
    for use_f, use_d in ((True, True), (False, True), (True, False)):
        f, d = Guarded(w.size, KIND[dt]), Guarded(w.size, KIND[dt])
        L.check(L.lib().ecgmm_pack_conv_weight(dt, dptr(src), f.ptr if use_f else None, d.ptr if use_d else None,
                                               Cout, Cin, RS, stream()))
        what = "pack_conv_weight %s %s fwd=%d dgrad=%d" % (KIND[dt], shape, use_f, use_d)
        cmp_ = assert_exact if dt == L.F32 else assert_bits
        if use_f:
            cmp_(f.done(what), want_f, what + ": fwd")
        else:
            assert f.untouched(), what + ": wrote the forward pack although its pointer was null"
        if use_d:
            cmp_(d.done(what), want_d, what + ": dgrad")
        else:
            assert d.untouched(), what + ": wrote the dgrad pack although its pointer was null"


# ---- bcast_rows -----------------------------------------------------------------------------------------------------------
SCALES = [1.0, 0.25, 1.0 / 313.0]


def vec_path(dt, Cn, skew):
    """the rule of ecg_bcast_rows (csrc/elementwise.hip): the 16-byte kernel iff C is a whole number of 16-byte chunks, that
    number divides 1024, and the output is 16-byte aligned"""
    vecw = 8 if dt == L.BF16 else 4
    return Cn % vecw == 0 and Cn // vecw <= 1024 and 1024 % (Cn // vecw) == 0 and skew == 0


def _bcast(dt, v_bits, N, R, Cn, scale, skew=0):
    """-> (device bits [N, R, C], expected bits): out[n][r][c] = T(v[n][c] * scale), one fp32 multiply then the store rounding"""
    src = dev_bits(v_bits)
    out = Guarded(N * R * Cn, KIND[dt], skew=skew)
    assert (out.address % 16 == 0) == (skew == 0)
    L.check(L.lib().ecgmm_bcast_rows(dt, dptr(src), out.ptr, N, R, Cn, scale, stream()))
    with np.errstate(all="ignore"):
        prod = (v_bits.view(np.float32).reshape(N, Cn) * np.float32(scale)).view(np.uint32)
    want = np.broadcast_to(store_bits(prod, dt)[:, None, :], (N, R, Cn))
    return out.done("bcast_rows").reshape(N, R, Cn), np.ascontiguousarray(want)


# (dtype, C, skew, the path this selects)
BCAST_PATHS = [(L.F32, 4, 0, True), (L.F32, 64, 0, True), (L.BF16, 8, 0, True), (L.BF16, 64, 0, True),
               (L.F32, 12, 0, False), (L.F32, 20, 0, False), (L.BF16, 12, 0, False), (L.BF16, 64, 1, False), (L.F32, 64, 1, False)]


@pytest.mark.parametrize("scale", SCALES, ids=["1", "quarter", "1over313"])
@pytest.mark.parametrize("case", BCAST_PATHS, ids=lambda c: "%s-C%d-skew%d-%s" % (KIND[c[0]], c[1], c[2], "vec" if c[3] else "scalar"))
def test_bcast_rows_both_paths(case, scale):
    dt, Cn, skew, vec = case
    assert vec_path(dt, Cn, skew) == vec          # the case still selects the kernel it is here for
    N, R = 3, 5
    v = finite_values(np.random.default_rng(4000 + Cn), (N, Cn)).view(np.uint32)
    got, want = _bcast(dt, v, N, R, Cn, scale, skew)
    assert_exact(got, want, "bcast_rows %s C=%d scale=%r" % (KIND[dt], Cn, scale))


@pytest.mark.parametrize("dt,Cn,skew", [(L.BF16, 64, 0), (L.BF16, 64, 1), (L.F32, 64, 0)], ids=["pack16-bf16", "scalar-bf16", "vec-fp32"])
def test_bcast_rows_rounding_table(dt, Cn, skew):
    """scale = 1 and bf16 is the only public route to pack16<bf16_t> (the 16-byte path); the scalar path stores through f2bf
    like ecgmm_cast.  fp32: v * 1.0f keeps every bit of a value that is not a NaN, subnormals included."""
    N = TABLE.size // Cn
    got, want = _bcast(dt, TABLE, N, 2, Cn, 1.0, skew)
    assert_bits(got, want, "bcast_rows %s, the rounding table" % KIND[dt])


@pytest.mark.parametrize("R", [1, 2, 3, 7, 313, 625, 1000, 4096, 99991])
def test_bcast_rows_row_to_sample_division(R):
    """the magic-number row -> sample division of the 16-byte kernel at power-of-two and other divisors: every sample holds
    other values, so a row given to the wrong sample differs"""
    N, Cn = 3, 4
    assert vec_path(L.F32, Cn, 0)
    v = finite_values(np.random.default_rng(5000 + R), (N, Cn)).view(np.uint32)
    got, want = _bcast(L.F32, v, N, R, Cn, 1.0 / 313.0)
    assert_exact(got, want, "bcast_rows R=%d" % R)


@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
def test_bcast_rows_large_row_index_small_divisor(dt):
    N, R, Cn = 70001, 3, 8
    assert vec_path(dt, Cn, 0)
    v = finite_values(np.random.default_rng(5500), (N, Cn)).view(np.uint32)
    got, want = _bcast(dt, v, N, R, Cn, 0.25)
    assert_exact(got, want, "bcast_rows N=70001 R=3 %s" % KIND[dt])


# ---- axpby ------------------------------------------------------------------------------------------------------------------
AXPBY_N = [1, 255, 256, 100003]


def _axpby(a, x, b, y0, alias=False):
    """y <- a * x + b * y on the device; y0 None: y keeps the NaN prefill (b == 0 must not read it).  alias: x is y."""
    n = x.size
    y = Guarded(n, "f32", prefill=None if y0 is None else y0.view(np.uint32))
    xs = None if alias else dev_bits(x)
    L.check(L.lib().ecgmm_axpby(a, y.ptr if alias else dptr(xs), b, y.ptr, n, stream()))
    return y.done("axpby")


def _axpby_inputs(n, seed):
    rng = np.random.default_rng(seed)
    x, y = finite_values(rng, n), finite_values(rng, n)
    x[::17] = -0.0
    x[5::29] = np.float32(1e-44)            # a subnormal: a * x underflows for a = 1/7
    x[7::31] = np.float32(-1e-45)           # ... to -0
    return x, y


@pytest.mark.parametrize("n", AXPBY_N)
def test_axpby_add(n):
    x, y = _axpby_inputs(n, 6000 + n)
    assert_exact(_axpby(1.0, x, 1.0, y), (x + y).view(np.uint32), "axpby (1, 1) n=%d" % n)


@pytest.mark.parametrize("alias", [False, True], ids=["y-unread", "x-is-y"])
@pytest.mark.parametrize("n", AXPBY_N)
def test_axpby_scale_does_not_read_y(n, alias):
    """b == 0: y's NaN prefill must not leak, and the result is the one multiply a * x -- bit for bit wherever the product is
    not a zero.  The kernel's expression is a * x + 0.0f, so the sign of a zero result depends on the contraction the compiler
    chose, as in the general case below: fma(a, x, +0) keeps the sign of a product that underflows (-tiny + 0 rounds to -0)
    and gives +0 for a true -0 product; the unfused form gives +0 for both.  Exactly these two are accepted, one of them for
    the whole kernel.  x == y is the call plan_resnet1d makes (the mean's 1 / L in place)."""
    x, _ = _axpby_inputs(n, 6100 + n)
    a = np.float32(1.0 / 7.0)
    with np.errstate(all="ignore"):
        ax = a.astype(np.float64) * x.astype(np.float64)                  # exact
        fused = (ax + 0.0).astype(np.float32).view(np.uint32)
        plain = (ax.astype(np.float32) + np.float32(0.0)).view(np.uint32)
        one_multiply = (a * x).view(np.uint32)
    got = _axpby(float(a), x, 0.0, x if alias else None, alias=alias)
    assert not bool(is_nan32(got).any()), "axpby (1/7, 0): the NaN prefill of y leaked"
    nonzero = (one_multiply & np.uint32(0x7FFFFFFF)) != 0
    assert_exact(got[nonzero], one_multiply[nonzero], "axpby (1/7, 0) n=%d" % n)
    assert bool((got == fused).all()) or bool((got == plain).all()), "axpby (1/7, 0) n=%d: %d differ from fma(a, x, 0), %d from a * x + 0" % (
        n, int((got != fused).sum()), int((got != plain).sum()))
    if n > 200:
        assert bool((fused != plain).any()) and bool((~nonzero).any())


@pytest.mark.parametrize("n", AXPBY_N)
def test_axpby_general_is_one_of_two_roundings(n):
    """a * x + b * y: the compiler may contract the sum with a * x into one fma or not.  Exactly two results are right, and the
    compiler's choice is one for the whole kernel: every element equals the fused candidate or every element the other."""
    x, y = _axpby_inputs(n, 6200 + n)
    a, b = np.float32(0.3), np.float32(1.7)
    with np.errstate(all="ignore"):
        by = (b.astype(np.float64) * y.astype(np.float64)).astype(np.float32)          # fl(b * y)
        ax = a.astype(np.float64) * x.astype(np.float64)                               # exact: 24 + 24 bits
        fused = (ax + by.astype(np.float64)).astype(np.float32)                        # fl(a * x + fl(b * y))
        plain = (ax.astype(np.float32).astype(np.float64) + by.astype(np.float64)).astype(np.float32)
    got = _axpby(float(a), x, float(b), y)
    f, p = fused.view(np.uint32), plain.view(np.uint32)
    assert bool(((got == f) | (got == p)).all()), "axpby (0.3, 1.7): a value that is neither rounding"
    assert bool((got == f).all()) or bool((got == p).all()), "axpby (0.3, 1.7): fused and unfused results mixed"
    if n > 1000:
        assert bool((f != p).any())           # the two candidates do differ somewhere: the test can tell them apart
