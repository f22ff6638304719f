"""Operands at an element offset into a guarded flat buffer (a test helper, not a conftest).

Freshly allocated device tensors are 512-B aligned, so a kernel that is handed them only ever sees
addresses = 0 mod 16.  `Padded` puts an operand of any of the suite's dtypes (int8, int16, int32,
float32) at element offset `o` into a flat buffer with PAD guard elements on each side:

* the operand's address is (o * itemsize) mod 16: the premise is asserted, not assumed;
* written guards: `fetch()` returns the operand and whether both pads still hold their fill,
  compared by bits (a NaN fill compares equal to itself);
* read guards: the fill is a parameter.  Integer operands use FILL_A / FILL_B (0x55.. / 0xAA..):
  an output that depends on a word outside an input differs between the two runs.  f32 inputs use
  NAN_FILL: an input word read from outside the operand and used poisons an output, which then
  differs from the reference.  f32 outputs and states use the finite F32_SENTINEL.

The device is a parameter, so the helper (and its negative control, test_padded.py) runs on "cpu".
"""
import numpy as np

PAD = 64                                    # guard elements on each side of an operand

_BITS = {1: "int8", 2: "int16", 4: "int32"}
FILL_A, FILL_B = 0x55, 0xAA                 # the repeated byte of the two integer fills
NAN_FILL = "nan"                            # f32 inputs: quiet NaN 0x7FC00000
F32_SENTINEL = "sentinel"                   # f32 outputs / states: -1.7014e38 (0xFF000000 .. finite)
_F32_WORD = {NAN_FILL: 0x7FC00000, F32_SENTINEL: 0xFEFEFEFE}


def fill_word(np_dtype, fill):
    """The pad's bit pattern, as a signed integer of the dtype's width."""
    dt = np.dtype(np_dtype)
    if dt == np.float32:
        w = _F32_WORD[fill]
        return int(np.array([w], np.uint32).view(np.int32)[0])
    raw = np.full(dt.itemsize, fill, np.uint8)
    return int(raw.view(_BITS[dt.itemsize])[0])


class Padded:
    """A contiguous operand of `shape` at element offset `o` into a flat buffer on `device`, PAD guard
    elements on each side; the whole buffer (the operand too) starts out as the fill.  `.t` is the
    operand (a torch view), `.ptr` its address."""

    def __init__(self, torch, np_dtype, shape, o, fill, device="cuda"):
        self.dt = np.dtype(np_dtype)
        self.shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
        n = int(np.prod(self.shape, dtype=np.int64))
        self.o, self.fill = o, fill
        self.lo, self.hi = PAD + o, PAD + o + n
        self.word = fill_word(self.dt, fill)
        bits = getattr(torch, _BITS[self.dt.itemsize])
        self._bits = torch.full((self.hi + PAD,), self.word, dtype=bits, device=device)
        tdt = {"int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "float32": torch.float32}[self.dt.name]
        self.flat = self._bits.view(tdt)
        self.t = self.flat[self.lo:self.hi].view(self.shape)
        self.ptr = self.t.data_ptr()
        if n:                               # the allocator's base alignment is part of the premise
            assert self.ptr % 16 == (o * self.dt.itemsize) % 16, (self.ptr, o, self.dt)

    def put(self, torch, arr):
        """Copy a numpy array of the operand's shape and dtype in; returns self."""
        a = np.ascontiguousarray(arr, dtype=self.dt).reshape(self.shape)
        self.t.copy_(torch.from_numpy(a.copy()))
        return self

    def reset(self):
        """The operand's own words back to the fill (an output before a call)."""
        self._bits[self.lo:self.hi] = self.word

    def fetch(self):
        """-> (operand as numpy, both pads still hold their fill bit for bit)"""
        h = self._bits.cpu().numpy()
        ok = bool((h[:self.lo] == self.word).all() and (h[self.hi:] == self.word).all())
        return h[self.lo:self.hi].view(self.dt).reshape(self.shape).copy(), ok
