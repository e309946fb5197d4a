"""Guarded device buffers of any element width, as bit patterns, for the exact-answer tests (tests/test_exact_kernels_gpu.py,
tests/test_philox_draws_gpu.py): the counterpart of tests/lstm_abi.Arena for outputs that are bf16, bytes or int64, or whose
fp32 bits matter (-0, NaN payloads).

A Guarded output is [guard | skew | payload | guard]: the guards (and the skew elements, which move the payload off 16-byte
alignment) hold a sentinel pattern, the payload a prefill pattern that no expected value equals -- for the float types a NaN
whose payload the inputs never carry.  done() checks every sentinel and returns the payload's bits, so an element written
outside the output, or one inside it that was never written, fails the comparison that follows."""
import ctypes as C

import numpy as np
import torch

DEV = "cuda:0"
GUARD_BYTES = 1024
_F32_SENTINEL = int(np.float32(-12345.671875).view(np.uint32))
_F64_SENTINEL = int(np.float64(-12345.671875).view(np.uint64))
# element width -> (torch integer type of that width, numpy unsigned type, sentinel bits, prefill bits)
KINDS = {
    "f32": (torch.int32, np.uint32, _F32_SENTINEL, 0x7FC12345),   # sentinel -12345.671875 (tests/lstm_abi.SENTINEL); prefill a NaN
    "bf16": (torch.int16, np.uint16, 0x5A5A, 0x7FC1),             # prefill a NaN
    "u8": (torch.uint8, np.uint8, 77, 99),
    "f64": (torch.int64, np.uint64, _F64_SENTINEL, 0x7FF8000012345678),   # sentinel -12345.671875; prefill a NaN
    "i64": (torch.int64, np.uint64, 0x5A5A5A5A5A5A5A5A, 0x7B7B7B7B7B7B7B7B),
}


def _signed(bits, ttype):
    """the Python integer torch wants for a bit pattern of its signed integer type"""
    width = {torch.uint8: 8, torch.int16: 16, torch.int32: 32, torch.int64: 64}[ttype]
    return bits - (1 << width) if ttype != torch.uint8 and bits >= 1 << (width - 1) else bits


class Guarded:
    def __init__(self, n, kind, skew=0, prefill=None):
        """n elements of `kind`; skew: elements by which the payload starts past a 256-byte aligned address; prefill: the
        payload's initial bits (a numpy array of the kind's unsigned type) where the call reads or accumulates into it"""
        self.ttype, self.ntype, sent, fill = KINDS[kind]
        self.kind, self.n = kind, int(n)
        size = np.dtype(self.ntype).itemsize
        self.lo = GUARD_BYTES // size + skew
        total = self.lo + self.n + GUARD_BYTES // size
        self.buf = torch.full((total,), _signed(sent, self.ttype), dtype=self.ttype, device=DEV)
        self.buf[self.lo:self.lo + self.n] = _signed(fill, self.ttype)
        if prefill is not None:
            self.buf[self.lo:self.lo + self.n] = dev_bits(prefill.reshape(-1))
        self.sent, self.fill = sent, fill
        self.address = self.buf.data_ptr() + self.lo * size
        assert (self.buf.data_ptr() % 256) == 0

    @property
    def ptr(self):
        return C.c_void_p(self.address)

    def bits(self):
        """the payload's bits now (numpy, unsigned), without any check"""
        return self.buf[self.lo:self.lo + self.n].cpu().numpy().view(self.ntype)

    def done(self, what="output"):
        """after the call (synchronises): no sentinel changed -> the payload's bits"""
        torch.cuda.synchronize()
        s = _signed(self.sent, self.ttype)
        head, tail = self.buf[:self.lo], self.buf[self.lo + self.n:]
        assert bool((head == s).all()), "%s: written before its first element" % what
        assert bool((tail == s).all()), "%s: written past its last element" % what
        return self.bits()

    def untouched(self):
        """the whole payload still holds the prefill pattern (a refused call, a null-pointer sibling)"""
        return bool((self.done() == self.ntype(self.fill)).all())


def dev_bits(a):
    """a device copy of the numpy array `a` (any dtype), bit for bit, as the signed integer tensor of the same width"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(DEV)


def dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
