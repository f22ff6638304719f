"""Device operands between marker bytes (a test helper, not a conftest): the helper of tests/test_ml.py for the
modules that came after it.

    d = Dev(torch, x, off=1)     a device copy of x whose first element sits `off` elements past a 16-byte boundary,
                                 in an allocation filled with 0x5A bytes, GUARD such bytes after its end
    d.ptr                        its address;  d.get() -> the words now, after asserting that every byte around them
                                 still is 0x5A
    marker(shape, dtype)         an array of 0x5A bytes: an output before the call;  untouched(x): still all 0x5A
"""
import numpy as np

GUARD = 32
FILL = 0x5A


class Dev:
    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.lo, self.nb, self.shape, self.dtype = off * x.itemsize, x.nbytes, x.shape, x.dtype
        raw = np.full(self.lo + self.nb + GUARD, FILL, dtype=np.uint8)
        raw[self.lo:self.lo + self.nb] = x.reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(raw).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == FILL).all() and (b[self.lo + self.nb:] == FILL).all(), "guard bytes"
        return b[self.lo:self.lo + self.nb].view(self.dtype).reshape(self.shape)


def marker(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype).reshape(shape)


def untouched(x):
    return bool((np.ascontiguousarray(x).view(np.uint8) == FILL).all())
