"""ecgmm_signal_resample on the GPU, through the C ABI between guard zones (tests/resample_abi.py), element by element against
the long-double direct sum (tests/resample_ref.py) under the derived bound (tests/resample_bounds.py), plus the exact
properties: the copy at equal lengths, exact zeros, a row's bits depending on that row alone, determinism.
Every test prints the worst ratio it asserts on (run with -s)."""
import functools

import numpy as np
import pytest

from . import resample_abi as A
from . import resample_bounds as RB
from . import resample_ref as RR

pytestmark = pytest.mark.gpu

# both table digits (r = 256 a + b) and the carry between them
UNIFORM_N = (1, 2, 3, 15, 16, 17, 255, 256, 257, 511, 513)
LENGTHS = (0, 1, 2, 16, 257, 299, 300)
L_PAD = 300
A_ERR = 1          # ECGMM_ERR_SHAPE


def _nums(N):
    c = {1, N - 1, N, N + 1, N // 2, 2 * N, int(0.6 * N), int(1.2 * N)}
    return sorted(v for v in c if v >= 1)


def _rows3(N, seed):
    """all zeros | a constant | noise scaled by 1e4 (fp32 values)"""
    rng = np.random.RandomState(seed)
    x = np.zeros((3, N), dtype=np.float32)
    x[1] = np.float32(0.37)
    x[2] = (rng.randn(N) * 1e4).astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _uniform_case(N, num):
    x = _rows3(N, 1000 + 3 * N + num)
    x.setflags(write=False)
    ref = RR.resample_ref(x.astype(np.float64), num)
    ref.setflags(write=False)
    return x, ref


def _check_uniform(N, num):
    x, ref = _uniform_case(N, num)
    got = A.resample(x, num=num)
    assert got.shape == (3, num)
    if num == N:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32)), "num == N must copy the row bit for bit"
        return 0.0
    assert np.all(got[0] == 0), "an all-zero row must give exact zeros"
    r = RB.check_rows(got, ref, x.astype(np.float64), [(N, num)] * 3, "resample %d -> %d" % (N, num))
    const = RB.bound(np.full(num, 0.37), x[1].astype(np.float64), N, num)
    assert np.all(np.abs(got[1].astype(np.float64) - np.float64(np.float32(0.37))) <= const), "a constant row must stay constant"
    return r.ratio


@pytest.mark.parametrize("N", UNIFORM_N)
def test_uniform_against_the_direct_sum(N):
    worst = max(_check_uniform(N, num) for num in _nums(N))
    print("N=%d: worst ratio %.3g over num in %s" % (N, worst, _nums(N)))


@pytest.mark.parametrize("N,num", [(5000, 3000), (3000, 5000)])
def test_record_lengths(N, num):
    rng = np.random.RandomState(N)
    x = np.zeros((4, N), dtype=np.float32)
    x[1] = np.float32(-1.25)
    x[2] = (rng.randn(N) * 1e4).astype(np.float32)
    t = np.arange(N) / 500.0
    x[3] = (0.9 * np.exp(8.0 * (np.cos(2 * np.pi * 1.2 * t) - 1.0)) + 0.05 * rng.randn(N)).astype(np.float32)
    got = A.resample(x, num=num)
    ref = RR.resample_ref(x.astype(np.float64), num)
    assert np.all(got[0] == 0)
    RB.check_rows(got, ref, x.astype(np.float64), [(N, num)] * 4, "resample %d -> %d" % (N, num))
    assert np.array_equal(A.resample(x, num=num).view(np.uint32), got.view(np.uint32)), "two calls must give the same bits"


def _padded(lengths, Ln, seed):
    """rows of noise, NaN from each row's (clamped) length on"""
    rng = np.random.RandomState(seed)
    x = rng.randn(len(lengths), Ln).astype(np.float32)
    for s, n in enumerate(lengths):
        x[s, min(max(n, 0), Ln):] = np.nan
    return x


@pytest.mark.parametrize("ratio", [0.6, 1.2])
def test_lengths_against_the_direct_sum(ratio):
    x = _padded(LENGTHS, L_PAD, 21)
    T_out = int(L_PAD * ratio)
    got, nums = A.resample(x, ratio=ratio, lengths=LENGTHS, out_lengths=True)
    ref, want = RR.resample_lengths_ref(x, LENGTHS, ratio)
    assert got.shape == (len(LENGTHS), T_out)
    assert nums.tolist() == want.tolist() == [int(n * ratio) for n in LENGTHS]
    for s, num in enumerate(want):
        assert np.all(got[s, num:] == 0), "row %d: exact zeros from num_s on" % s
    xs = [np.nan_to_num(x[s].astype(np.float64)) for s in range(len(LENGTHS))]
    RB.check_rows(got, ref, xs, list(zip(LENGTHS, want)), "resample lengths, ratio %g" % ratio)
    # without out_lengths, and again: the same bits
    again = A.resample(x, ratio=ratio, lengths=LENGTHS)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_lengths_are_clamped_on_the_device():
    x = _padded((L_PAD, 0, 16), L_PAD, 22)
    got, nums = A.resample(x, ratio=0.6, lengths=(303, -2, 16), out_lengths=True)
    want, wn = A.resample(x, ratio=0.6, lengths=(L_PAD, 0, 16), out_lengths=True)
    assert nums.tolist() == wn.tolist() == [180, 0, 9]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[1] == 0)


@pytest.mark.parametrize("ratio", [0.6, 1.2])
def test_a_rows_bits_depend_on_that_row_alone(ratio):
    n = 257
    x = _padded(LENGTHS, L_PAD, 23)
    row = LENGTHS.index(n)
    num = int(n * ratio)
    batch = A.resample(x, ratio=ratio, lengths=LENGTHS)[row]
    alone = A.resample(x[row:row + 1], ratio=ratio, lengths=[n])[0]
    assert np.array_equal(alone.view(np.uint32), batch.view(np.uint32)), "S = 1 against the batch"
    other = _padded((300, 5, n, 120), L_PAD, 24)
    other[2] = x[row]
    moved = A.resample(other, ratio=ratio, lengths=(300, 5, n, 120))[2]
    assert np.array_equal(moved.view(np.uint32), batch.view(np.uint32)), "other neighbours, another position"
    wide = np.full((2, 320), np.nan, dtype=np.float32)
    wide[:, :n] = x[row, :n]
    wide[1, :n] = 1.0
    longer = A.resample(wide, ratio=ratio, lengths=[n, n])[0]
    assert np.array_equal(longer[:num].view(np.uint32), batch[:num].view(np.uint32)), "a larger L"
    assert np.all(longer[num:] == 0)
    # the row cut to its own length through the form without lengths
    cut = A.resample(np.ascontiguousarray(x[row:row + 1, :n]), num=num)[0]
    assert np.array_equal(cut.view(np.uint32), batch[:num].view(np.uint32)), "the uniform form on the trimmed row"


@pytest.mark.parametrize("ratio", [0.6, 1.2])
def test_all_lengths_equal_to_L_is_the_uniform_form(ratio):
    rng = np.random.RandomState(25)
    x = rng.randn(3, L_PAD).astype(np.float32)
    num = int(L_PAD * ratio)
    with_lengths, nums = A.resample(x, ratio=ratio, lengths=[L_PAD] * 3, out_lengths=True)
    uniform = A.resample(x, num=num)
    assert nums.tolist() == [num] * 3
    assert np.array_equal(with_lengths.view(np.uint32), uniform.view(np.uint32))


def test_uniform_output_wider_than_num_is_zero_padded():
    x = _rows3(17, 26)
    got = A.resample(x, num=9, T_out=300)
    assert np.array_equal(got[:, :9].view(np.uint32), A.resample(x, num=9).view(np.uint32))
    assert np.all(got[:, 9:] == 0)


def test_refused_calls_write_nothing():
    x = _rows3(100, 27)
    A.resample(x, num=61, T_out=60, expect=A_ERR)                                       # num > T_out
    A.resample(x, num=60, ratio=0.6, lengths=[100, 50, 3], T_out=60, expect=A_ERR)      # num with lengths
    A.resample(x, ratio=-0.6, lengths=[100, 50, 3], T_out=60, out_lengths=True, expect=A_ERR)
    A.resample(x, ratio=0.6, lengths=[100, 50, 3], T_out=59, out_lengths=True, expect=A_ERR)   # T_out < int(L * ratio)

