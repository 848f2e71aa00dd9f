"""Guarded operands for the GPU conformance suites (tests/test_conv_conformance_gpu.py, tests/test_train_conformance_gpu.py,
tests/test_dbscan_conformance_gpu.py).

Every operand lives inside a larger buffer with guard regions before and after it.  Everything that is not an operand --
pitch padding, gaps between images, the guards -- holds a fixed NaN bit pattern: a read of it poisons a result, and a
write into it shows up in the bitwise comparison after the call.
"""
import torch

NAN_BITS = 0x7FC0BEEF                 # a quiet NaN with a payload no kernel produces
GUARD = 1 << 16                       # floats of guard on each side of an operand
BYTE_FILL = 0xA5                      # what GuardedBytes holds outside its view


def layout(n_img, n_inner, bs, outer, pixels, pitch, c):
    """Flat float offsets [n_img, pixels, c] of image i at (i % n_inner) * bs + (i // n_inner) * outer."""
    i = torch.arange(n_img, dtype=torch.int64)
    base = (i % n_inner) * bs + (i // n_inner) * outer
    return base[:, None, None] + torch.arange(pixels, dtype=torch.int64)[None, :, None] * pitch + torch.arange(c)[None, None, :]


class Guarded:
    """An operand at flat offsets ``idx`` (+ ``off`` floats) inside a NaN-filled buffer with guards on both sides."""

    def __init__(self, idx, device, off=0):
        self.shape = idx.shape
        span = int(idx.max()) + 1 if idx.numel() else 1
        self.base = GUARD + off
        self.buf = torch.full((self.base + span + GUARD,), NAN_BITS, dtype=torch.int32, device=device)
        self.idx = (idx.reshape(-1) + self.base).to(device)
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=device)
        self.outside[self.idx] = False

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.base

    def put(self, values):
        """float32 values, or int32 words (the split activation format)"""
        v = values.reshape(-1).to(self.buf.device)
        self.buf[self.idx] = v.view(torch.int32) if v.dtype == torch.float32 else v

    def words(self):
        return self.buf[self.idx].reshape(self.shape).cpu()

    def get(self):
        return self.words().view(torch.float32)

    def untouched_outside(self):
        return bool(torch.all(self.buf[self.outside] == NAN_BITS))

    def untouched(self):
        """no word of the whole buffer, view included, was written (a refusal)"""
        return bool(torch.all(self.buf == NAN_BITS))

    def reset(self):
        self.buf.fill_(NAN_BITS)


class GuardedBytes:
    """``nbytes`` bytes, ``off`` bytes past a 256-byte boundary, inside a buffer of BYTE_FILL with GUARD bytes on both sides: byte
    operands (flags) and workspaces, whose size is no multiple of a word"""

    def __init__(self, nbytes, device, off=0):
        self.nbytes, self.base = int(nbytes), GUARD + off
        self.buf = torch.full((self.base + self.nbytes + GUARD,), BYTE_FILL, dtype=torch.uint8, device=device)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.base

    def put(self, values):
        self.buf[self.base:self.base + self.nbytes] = values.reshape(-1).to(device=self.buf.device, dtype=torch.uint8)

    def bytes(self):
        return self.buf[self.base:self.base + self.nbytes].cpu()

    def untouched_outside(self):
        return bool(torch.all(self.buf[:self.base] == BYTE_FILL)) and bool(torch.all(self.buf[self.base + self.nbytes:] == BYTE_FILL))
