"""The use cases behind the support functions, on device pointers with no host copy in between.

f32 -> q15 -> FIR -> f32: arm_float_to_q15_batch on a batch of float32 signals, arm_fir_q15_batch on the q15 words,
arm_q15_to_float_batch on the filter's output.  The q15 words and the final floats must equal the numpy restatements
applied to the previous stage's own output, bit for bit.

Peak picking: arm_cmplx_mag_f32_batch on a batch of spectra, then arm_sort_f32_batch descending: the first k words of
every item are the k largest magnitudes of that item."""
import ctypes as C

import numpy as np
import pytest

import cmplx_math_ref as cm
import support_ref as sr

SIGNALS, BLOCK, TAPS = 12, 600, 16
SPECTRA, BINS, K = 5, 1000, 8


@pytest.mark.gpu
def test_float_to_q15_fir_q15_to_float_on_device(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(101)
    coeffs = (rng.standard_normal(TAPS) / TAPS * 32768).clip(-32768, 32767).astype(np.int16)
    dc = torch.from_numpy(coeffs.copy()).cuda()
    S = dsp.arm_fir_instance_q15()
    S.numTaps = TAPS
    S.pCoeffs = C.cast(dc.data_ptr(), S._fields_[2][1])
    x = rng.uniform(-1.1, 1.1, (SIGNALS, BLOCK)).astype(np.float32)           # a few samples saturate
    src = torch.from_numpy(x).cuda()
    q = torch.from_numpy(sr.marked("q15", (SIGNALS, BLOCK))).cuda()
    y = torch.from_numpy(sr.marked("q15", (SIGNALS, BLOCK))).cuda()
    out = torch.from_numpy(sr.marked("f32", (SIGNALS, BLOCK))).cuda()
    hist = torch.zeros((SIGNALS, TAPS - 1), dtype=torch.int16, device="cuda")
    dsp.convert_batch(src, q)
    dsp.fir_batch(S, q, y, hist)
    dsp.convert_batch(y, out)
    torch.cuda.synchronize()
    qh, yh = q.cpu().numpy(), y.cpu().numpy()
    assert src.cpu().numpy().tobytes() == x.tobytes()
    assert qh.tobytes() == sr.float_to_q(x, "q15").tobytes() and (np.abs(qh.astype(np.int32)) >= 32767).any()
    assert (yh != 0x5A5A).any() and (yh != qh).any()
    assert out.cpu().numpy().tobytes() == sr.convert("q15", "f32", yh).tobytes()


@pytest.mark.gpu
def test_cmplx_mag_then_sort_descending_gives_the_peaks(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(103)
    spec = rng.standard_normal((SPECTRA, 2 * BINS)).astype(np.float32)
    s = torch.from_numpy(spec).cuda()
    mag = torch.from_numpy(sr.marked("f32", (SPECTRA, BINS))).cuda()
    top = torch.from_numpy(sr.marked("f32", (SPECTRA, BINS))).cuda()
    dsp.cmplx_mag_batch(s, mag)
    dsp.sort_batch(mag, top, dsp.ARM_SORT_DESCENDING)
    torch.cuda.synchronize()
    m, t = mag.cpu().numpy(), top.cpu().numpy()
    assert m.tobytes() == cm.mag("f32", spec).tobytes()
    assert t.tobytes() == sr.total_order_sort(m, False).tobytes()
    for i in range(SPECTRA):
        assert t[i, :K].tolist() == np.sort(m[i])[::-1][:K].tolist()
        assert t[i, 0] == m[i].max() and t[i, -1] == m[i].min()
