"""The use cases behind the basic math functions, on device pointers with no host copy in between.

Window -> spectrum -> peak: arm_mult_f32_batch (a Hann window, repeated per frame, on a batch of frames, in
place) -> arm_rfft_fast_f32_batch -> arm_cmplx_mag_f32_batch -> arm_max_f32_batch.  Each frame holds
a tone on its own bin, so the peak's index is known; the windowed frames, the magnitudes and the maxima must equal the
numpy restatements applied to the previous stage's own output, bit for bit.

Template correlation: arm_fir_q15_batch on a bank of signals, then arm_dot_prod_q15_batch of every filtered signal
against one shared template (bStride 0) must equal the restated dot product of the FIR's own output."""
import ctypes as C

import numpy as np
import pytest

import basic_math_ref as br
import cmplx_math_ref as cm

FRAMES, N = 8, 1024
SIGNALS, BLOCK, TAPS = 12, 600, 16


@pytest.mark.gpu
def test_window_rfft_mag_max_chain_on_device(dsp, torch_gpu):
    torch = torch_gpu
    k = np.arange(N)
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * k / N)).astype(np.float32)
    bins = [37 + 29 * i for i in range(FRAMES)]
    rng = np.random.default_rng(89)
    frames = np.stack([np.cos(2.0 * np.pi * b * k / N) + 0.01 * rng.standard_normal(N) for b in bins]).astype(np.float32)
    x = torch.from_numpy(frames.copy()).cuda()
    w = torch.from_numpy(np.tile(window, (FRAMES, 1))).cuda()
    spec = torch.from_numpy(cm.marked("f32", (FRAMES, N))).cuda()
    mag = torch.from_numpy(cm.marked("f32", (FRAMES, N // 2))).cuda()
    val = torch.from_numpy(cm.marked("f32", FRAMES)).cuda()
    idx = torch.from_numpy(cm.marked("u32", FRAMES).view(np.int32)).cuda()
    S = dsp.const_instance(f"arm_rfft_fast_sR_f32_len{N}")
    dsp.mult_batch(x, w, x)                                 # in place: dst == srcA
    windowed = x.clone()
    dsp.rfft_fast_batch(S, x, spec, 0)
    dsp.cmplx_mag_batch(spec, mag)
    dsp.max_batch(mag[:, 1:].contiguous(), val, idx)        # bin 0 packs the DC and Nyquist terms: leave it out
    torch.cuda.synchronize()
    assert windowed.cpu().numpy().tobytes() == br.run("mult_f32", frames, np.tile(window, (FRAMES, 1)))["dst"].tobytes()
    s, m = spec.cpu().numpy(), mag.cpu().numpy()
    assert not (s.view(np.uint32) == 0x5A5A5A5A).any()
    assert m.tobytes() == cm.mag("f32", s).tobytes()
    wv, wi = cm.extreme("max", np.ascontiguousarray(m[:, 1:]))
    assert val.cpu().numpy().tobytes() == wv.tobytes()
    assert (idx.cpu().numpy().view(np.uint32) + 1).tolist() == bins == (wi + 1).tolist()


@pytest.mark.gpu
def test_fir_q15_then_template_dot_prod(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(97)
    coeffs = (rng.standard_normal(TAPS) / TAPS * 32768).clip(-32768, 32767).astype(np.int16)
    dc = torch.from_numpy(coeffs.copy()).cuda()
    S = dsp.arm_fir_instance_q15()
    S.numTaps = TAPS
    S.pCoeffs = C.cast(dc.data_ptr(), S._fields_[2][1])
    x = br.rand("q15", (SIGNALS, BLOCK), rng)
    template = br.rand("q15", BLOCK, rng)
    src, tpl = torch.from_numpy(x).cuda(), torch.from_numpy(template).cuda()
    dst = torch.from_numpy(cm.marked("q15", (SIGNALS, BLOCK))).cuda()
    hist = torch.zeros((SIGNALS, TAPS - 1), dtype=torch.int16, device="cuda")
    res = torch.from_numpy(br.marked("q63", SIGNALS)).cuda()
    dsp.fir_batch(S, src, dst, hist)
    dsp.dot_prod_batch(dst, tpl, res)
    torch.cuda.synchronize()
    y = dst.cpu().numpy()
    assert (y != 0x5A5A).any() and tpl.cpu().numpy().tobytes() == template.tobytes()
    assert res.cpu().numpy().tobytes() == br.run("dot_prod_q15", y, template)["value"].tobytes()
