"""Operands for the -m gpu tests that drive kernels through the C ABI with ctypes (tests/test_gpu_row_norm.py,
tests/test_gpu_copy_kernels.py): carved out of a larger NaN-filled buffer, on a 16-byte boundary or a chosen number of
floats past it, so that alignment is the test's to choose and the NaN canaries on both sides show a write out of bounds."""
import torch

DEV = torch.device("cuda", 0)
PAD = 64                            # canary floats in front of and behind every carved operand (a multiple of 4)
NAN_BITS = 0x7FC00000               # torch.full(nan)


class Carved(object):
    """``n`` floats inside a NaN-filled buffer, ``off`` floats past a 16-byte boundary, PAD canary floats either side."""

    def __init__(self, n, off=0, values=None):
        self.buf = torch.full((PAD + off + n + PAD,), float("nan"), device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.n = PAD + off, n
        self.t = self.buf[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == 4 * (off % 4)
        if values is not None:
            self.t.copy_(values.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        bits = self.buf.view(torch.int32)
        return bool((bits[:self.lo] == NAN_BITS).all()) and bool((bits[self.lo + self.n:] == NAN_BITS).all())


def chunk_map(idx, mb, L, T, N, A, first_only=False):
    """Source row of every output row (l, j) -> l * mb + j: include/mappo_hip.h, mappo_gather_chunks."""
    ls = torch.zeros(1, dtype=torch.int64, device=DEV) if first_only else torch.arange(L, device=DEV)
    f = (idx[None, :] * L + ls[:, None]).reshape(-1)
    n, rem = f // (A * T), f % (A * T)
    return ((rem % T) * N + n) * A + rem // T
