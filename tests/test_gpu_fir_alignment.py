"""GPU parity of the i8-MFMA FIR kernels (csrc/fir_mfma.hip) under pointer alignment.

Freshly allocated tensors are 512-B aligned, so the other FIR tests only ever hand the kernels
pointers = 0 mod 16.  The kernels choose their window mode (16-B aligned or shifted) and their
store path (16-B or per element) from the pointers, and the q7 / q15 ones derive the window
shift d from the address of the block input.  Here every operand is a view at an element offset
into a padded flat buffer: src alone, dst alone, and src + dst + hist together; and the drop-in
arm_fir_* is called with one block large enough (>= 256 chunks of 4096 outputs) to take the MFMA
kernels with batch == 1, on host buffers (for q7 the zero-copy route, which filters from
state + numTaps - 1: misaligned whenever (numTaps - 1) % 4 != 0) and on device pointers.

Every comparison is byte equality with the reference build; the guard pads round dst, hist and
the drop-in's device state must keep their sentinel.
"""
import ctypes as C

import numpy as np
import pytest

import refs

pytestmark = pytest.mark.gpu

PAD = 64                                   # guard elements on each side of an operand
BATCH = 257                                # the smallest batch of one-chunk blocks on the MFMA path (>= 256 items)
SENTINEL = {"q7": 0x55, "q15": 0x5555, "q31": 0x55555555}
BLOCKS = [64, 67, 4096, 4100]
TAPS = {"q7": [1, 33, 34, 35, 36, 157], "q15": [2, 34, 36, 160], "fast_q15": [2, 34, 36, 160],
        "q31": [1, 33, 34, 161]}
OFFSETS = {"q7": [0, 1, 2, 3, 4, 16], "q15": [0, 1, 2, 4, 8], "fast_q15": [0, 1, 2, 4, 8], "q31": [0, 1, 2, 4]}
MIN_TAPS = {"q7": 35, "q15": 36, "fast_q15": 36, "q31": 34}


def _base(kind):
    return kind.split("_")[-1]


class _Padded:
    """A [rows, n] operand at element offset `o` into a flat device buffer with PAD guard
    elements on each side; the whole buffer starts out as the sentinel."""

    def __init__(self, torch, kind, rows, n, o):
        dt = refs.DTYPE[_base(kind)]
        self.sent = SENTINEL[_base(kind)]
        self.lo, self.hi = PAD + o, PAD + o + rows * n
        tdt = {np.int8: torch.int8, np.int16: torch.int16, np.int32: torch.int32}[dt]
        self.flat = torch.full((self.hi + PAD,), self.sent, dtype=tdt, device="cuda")
        self.t = self.flat[self.lo:self.hi].view(rows, n)
        if rows * n:                       # the allocator's base alignment is part of the test's premise
            assert self.t.data_ptr() % 16 == (o * np.dtype(dt).itemsize) % 16, (self.t.data_ptr(), o)

    def fetch(self):
        """-> (operand as numpy, pads untouched)"""
        h = self.flat.cpu().numpy()
        return h[self.lo:self.hi].reshape(self.t.shape), bool((h[:self.lo] == self.sent).all() and
                                                              (h[self.hi:] == self.sent).all())


def _fir_data(kind, taps, block, fill, batch, seed):
    """coeffs and blocks[call] = [batch, block] arrays: random full range, or ("min") every sample at
    the type's minimum (q7: the taps too, the output saturating; the others: random taps)."""
    dt = refs.DTYPE[_base(kind)]
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    coeffs = rng.integers(info.min, info.max, taps, endpoint=True).astype(dt)
    if fill == "min":
        if _base(kind) == "q7":
            coeffs = np.full(taps, info.min, dt)
        blocks = [np.full((batch, block), info.min, dt) for _ in range(2)]
    else:
        blocks = [rng.integers(info.min, info.max, (batch, block), endpoint=True).astype(dt) for _ in range(2)]
    return coeffs, blocks


def _instance(dsp, torch, kind, coeffs, state_ptr=None):
    S = getattr(dsp, f"arm_fir_instance_{_base(kind)}")()
    S.numTaps = len(coeffs)
    dc = torch.from_numpy(coeffs.copy()).cuda()
    S.pCoeffs = C.cast(dc.data_ptr(), S._fields_[2][1])
    if state_ptr is not None:
        S.pState = C.cast(state_ptr, S._fields_[1][1])
    return S, dc


_CASES = [(k, t, b, None) for k in TAPS for t in TAPS[k] for b in BLOCKS] + \
         [(k, MIN_TAPS[k], b, "min") for k in TAPS for b in BLOCKS]


@pytest.mark.parametrize("kind,taps,block,fill", _CASES, ids=lambda v: str(v))
def test_fir_mfma_offset_pointers(dsp, torch_gpu, ref, kind, taps, block, fill):
    """257 filters (the smallest batch on the MFMA path), two consecutive calls each (state carry),
    with the operands at element offsets: (a) src alone, (b) dst alone, (c) src, dst and hist
    together, every offset of the kind in each ("min" fill: offset 1 only).  Every filter's
    outputs and final history equal the reference build's, and the pads round dst and hist keep
    their sentinel.  Blocks: 64 (a short chunk of whole 16s), 67 (ragged: each filter's row starts
    on another alignment), 4096 (a full chunk: the 16-B store path when dst allows it), 4100 (a
    second chunk of 4 outputs: waves 1-3 skip the MFMA block).  Taps: every (numTaps - 1) % 4 and
    both ends of the kernel's range."""
    torch = torch_gpu
    coeffs, blocks = _fir_data(kind, taps, block, fill, BATCH, seed=taps * 43 + block)
    want = [np.empty_like(b) for b in blocks]
    want_hist = np.empty((BATCH, taps - 1), coeffs.dtype)
    for f in range(BATCH):
        y, state = ref.fir(kind, coeffs, [blocks[0][f], blocks[1][f]])
        want[0][f], want[1][f] = y
        want_hist[f] = state[:taps - 1]
    S, _keep = _instance(dsp, torch, kind, coeffs)
    offsets = [1] if fill == "min" else OFFSETS[kind]
    runs = [("aligned", 0, 0, 0)] if fill != "min" else []
    for o in offsets:
        if o:
            runs += [("src", o, 0, 0), ("dst", 0, o, 0), ("all", o, o, o)]
    bad = []
    for mode, o_src, o_dst, o_hist in runs:
        src = _Padded(torch, kind, BATCH, block, o_src)
        dst = _Padded(torch, kind, BATCH, block, o_dst)
        hist = _Padded(torch, kind, BATCH, taps - 1, o_hist)
        hist.t.zero_()
        for k in range(2):
            src.t.copy_(torch.from_numpy(blocks[k]))
            dst.t.fill_(dst.sent)
            dsp.fir_batch(S, src.t, dst.t, hist.t, kind=kind)
            got, pads_ok = dst.fetch()
            if got.tobytes() != want[k].tobytes():
                rows = np.flatnonzero((got != want[k]).any(axis=1))
                f = int(rows[0])
                bad.append((mode, o_src or o_dst, "call", k, "filters", len(rows), "first", f,
                            np.flatnonzero(got[f] != want[k][f])[:4].tolist()))
            if not pads_ok:
                bad.append((mode, o_src or o_dst, "call", k, "dst pad written"))
        got_hist, pads_ok = hist.fetch()
        if got_hist.tobytes() != want_hist.tobytes():
            bad.append((mode, o_src or o_dst, "hist", np.flatnonzero((got_hist != want_hist).any(axis=1))[:4].tolist()))
        if not pads_ok:
            bad.append((mode, o_src or o_dst, "hist pad written"))
    assert not bad, bad[:12]


# ------------------------------------------------------------------ the drop-in, one block on the MFMA path
B_RAGGED = 255 * 4096 + 1                  # 256 chunks, the last of 1 output
B_WHOLE = 256 * 4096
FN = {"q7": "arm_fir_q7", "q15": "arm_fir_q15", "fast_q15": "arm_fir_fast_q15", "q31": "arm_fir_q31"}
WARM = 200                                 # a short first call: the big one starts from a non-zero history


def _dropin_data(kind, taps, block, seed):
    dt = refs.DTYPE[_base(kind)]
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    coeffs = rng.integers(info.min, info.max, taps, endpoint=True).astype(dt)
    return coeffs, [rng.integers(info.min, info.max, n, endpoint=True).astype(dt) for n in (WARM, block)]


# (kind, route, numTaps, blockSize, pSrc element offset)
_DROPIN = [("q7", "host", t, B_RAGGED, 0) for t in (33, 34, 35, 36)] + \
          [(k, "host", t, B_RAGGED, 0) for k, t in (("q15", 34), ("fast_q15", 34), ("q31", 33))] + \
          [("q7", "device", 35, b, o) for b in (B_RAGGED, B_WHOLE) for o in (0, 1, 2, 3)] + \
          [(k, "device", t, B_RAGGED, o) for k, t in (("q15", 34), ("fast_q15", 34), ("q31", 33)) for o in (0, 1)]


@pytest.mark.parametrize("kind,route,taps,block,o", _DROPIN, ids=lambda v: str(v))
def test_fir_dropin_single_block_mfma(dsp, torch_gpu, ref, kind, route, taps, block, o):
    """One drop-in call with blockSize = 1,044,481 (or 1,048,576, whole chunks): batch == 1 reaches
    the MFMA kernels (256 items), after a short first call so that the history is not zero.
    host: host buffers through the wrapper classes.  q7 fits the zero-copy route, which filters from
    state + numTaps - 1: numTaps 33 .. 36 put that at 0 .. 3 mod 4; q15 / q31 exceed the zero-copy
    size and run the scratch path.  device: pSrc, pDst and pState on the device, pSrc at element
    offset o, and the pads round pDst and pState keep their sentinel.  Outputs and the final state
    buffer [new history ; block input] equal the reference's."""
    torch = torch_gpu
    coeffs, blocks = _dropin_data(kind, taps, block, seed=taps + 11 * o + (block & 1))
    want, want_state = ref.fir(kind, coeffs, blocks)
    if route == "host":
        cls = {"q7": dsp.FirQ7, "q15": dsp.FirQ15, "fast_q15": dsp.FirFastQ15, "q31": dsp.FirQ31}[kind]
        filt = cls(coeffs, block)
        for k in range(2):
            got = filt(blocks[k])
            assert got.tobytes() == want[k].tobytes(), (k, np.flatnonzero(got != want[k])[:4])
        assert filt.state.tobytes() == want_state.tobytes()
        return
    state = _Padded(torch, kind, 1, taps - 1 + block, 0)
    state.t.zero_()
    S, _keep = _instance(dsp, torch, kind, coeffs, state.t.data_ptr())
    fn = getattr(dsp.lib, FN[kind])
    for k in range(2):
        n = len(blocks[k])
        src = _Padded(torch, kind, 1, n, o)
        dst = _Padded(torch, kind, 1, n, 0)
        src.t.copy_(torch.from_numpy(blocks[k][None]))
        fn(C.byref(S), C.c_void_p(src.t.data_ptr()), C.c_void_p(dst.t.data_ptr()), n)
        dsp._check_void(FN[kind])
        torch.cuda.synchronize()
        got, pads_ok = dst.fetch()
        assert got[0].tobytes() == want[k].tobytes(), (k, np.flatnonzero(got[0] != want[k])[:4])
        assert pads_ok, ("dst pad written", k)
    got_state, pads_ok = state.fetch()
    assert got_state[0].tobytes() == want_state.tobytes(), np.flatnonzero(got_state[0] != want_state)[:4]
    assert pads_ok, "state pad written"
