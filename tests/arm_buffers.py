"""
Guarded device buffers for the tests that call the C ABI directly (tests/test_gpu_dispatch_arms.py,
tests/test_gpu_warp_backward_arms.py, tests/test_gpu_filter_arms.py, tests/test_gpu_conv_fwd_arms.py, tests/test_gpu_lc3d_arms.py,
tests/test_gpu_conv_bf16_arms.py, tests/test_gpu_warp_forward_arms.py, tests/test_gpu_dice_cce_arms.py, tests/test_gpu_warp_dice_arms.py): the alignment of every pointer is exact, and a write outside an output is caught.
"""

import numpy as np
import torch

from neurite_amd import _lib

F = np.float32
PAD = 8                     # guard floats on each side of a buffer the test owns (32 bytes: the payload stays 16-byte aligned)
FILL = -12345.0


def N(t):
    return t.detach().cpu().numpy()


class Buf:
    """n floats with PAD guard floats on each side.  off = 0: the payload starts 16-byte aligned; off = 1: one float later, which
    is what sends a dispatcher to its unaligned arm."""

    def __init__(self, dev, n, off=0, data=None):
        _lib.require_device(torch.empty(1, device=dev))
        self.whole = torch.full((n + 2 * PAD + 1,), FILL, dtype=torch.float32, device=dev)
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.n = PAD + off, n
        self.t = self.whole[self.lo:self.lo + n]
        assert (self.t.data_ptr() % 16 == 0) == (off == 0)
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, F).reshape(-1)))

    @property
    def p(self):
        return _lib.ptr(self.t)

    def get(self, shape=None):
        """the payload, after checking that nothing outside it was written"""
        w = N(self.whole)
        assert (w[:self.lo] == F(FILL)).all() and (w[self.lo + self.n:] == F(FILL)).all(), 'a write outside the output'
        out = w[self.lo:self.lo + self.n]
        return out.reshape(shape) if shape is not None else out


class Bytes:
    """a workspace of exactly n bytes (64-byte aligned) with GUARD guard bytes on each side"""

    GUARD, MARK = 64, 0xA5

    def __init__(self, dev, n):
        _lib.require_device(torch.empty(1, device=dev))
        self.whole = torch.full((n + 2 * self.GUARD,), self.MARK, dtype=torch.uint8, device=dev)
        assert self.whole.data_ptr() % 64 == 0
        self.n = n
        self.t = self.whole[self.GUARD:self.GUARD + n]

    @property
    def p(self):
        return _lib.ptr(self.t)

    def check(self):
        """nothing outside the n bytes was written"""
        w = N(self.whole)
        assert (w[:self.GUARD] == self.MARK).all() and (w[self.GUARD + self.n:] == self.MARK).all(), 'a write outside the workspace'


class Raw:
    """n bytes of any element type (float32, bfloat16 as bits, 16- or 32-bit patterns) with GUARD guard bytes on each side, compared
    byte for byte.  off = 0: the payload starts 16-byte aligned; off = k: k bytes later.  data: a numpy array whose bytes fill the
    payload; without it the payload holds MARK bytes like the guards, so `untouched` can tell that nothing was written at all."""

    GUARD, MARK = 64, 0xA5

    def __init__(self, dev, n, off=0, data=None):
        _lib.require_device(torch.empty(1, device=dev))
        self.whole = torch.full((n + 2 * self.GUARD + 16,), self.MARK, dtype=torch.uint8, device=dev)
        assert self.whole.data_ptr() % 16 == 0 and 0 <= off < 16
        self.lo, self.n = self.GUARD + off, n
        self.t = self.whole[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == off
        if data is not None:
            raw = np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8)
            assert raw.size == n, (raw.size, n)
            self.t.copy_(torch.from_numpy(raw.copy()))

    @property
    def p(self):
        return _lib.ptr(self.t)

    def zero(self):
        self.t.zero_()
        return self

    def get(self, dtype, shape=None):
        """the payload as `dtype`, after checking that nothing outside it was written"""
        w = N(self.whole)
        assert (w[:self.lo] == self.MARK).all() and (w[self.lo + self.n:] == self.MARK).all(), 'a write outside the output'
        out = np.frombuffer(w[self.lo:self.lo + self.n].tobytes(), dtype)
        return out.reshape(shape) if shape is not None else out

    def untouched(self):
        """not one byte of the buffer, payload included, was written (the buffer was created without data)"""
        return bool((N(self.whole) == self.MARK).all())


call = _lib.call                                 # the product's own launch helper: device guard, stream, status check
