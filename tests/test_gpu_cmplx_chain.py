"""The use case behind the complex math functions: arm_cfft_f32_batch -> arm_cmplx_mag_f32_batch ->
arm_max_f32_batch on device pointers, with no host copy in between.  Eight copies of the FFT-bin example's 10 kHz
test signal, each scaled by its own power of two (the mirror bin 811 is as large up to rounding, so a scale that
changed the rounding could move the peak there), must all peak at bin 213, and the magnitudes must equal the numpy
restatement applied to the CFFT's own output, bit for bit."""
import os

import numpy as np
import pytest

import cmplx_math_ref as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, N = 8, 1024


@pytest.mark.gpu
def test_cfft_mag_max_chain_on_device(dsp, torch_gpu):
    torch = torch_gpu
    x = np.load(os.path.join(ROOT, "tests", "golden", "reference_patterns.npz"))["kat_fftbin_input"].astype(np.float32)
    assert x.size == 2 * N
    sig = np.stack([x * np.float32(2.0 ** (i - 3)) for i in range(BATCH)])
    data = torch.from_numpy(sig).cuda()
    mag = torch.from_numpy(cm.marked("f32", (BATCH, N))).cuda()
    val = torch.from_numpy(cm.marked("f32", BATCH)).cuda()
    idx = torch.from_numpy(cm.marked("u32", BATCH).view(np.int32)).cuda()
    S = dsp.const_instance("arm_cfft_sR_f32_len1024")
    dsp.cfft_batch(S, data, 0, 1)
    dsp.cmplx_mag_batch(data, mag)
    dsp.max_batch(mag, val, idx)
    torch.cuda.synchronize()
    spec, m = data.cpu().numpy(), mag.cpu().numpy()
    assert idx.cpu().numpy().tolist() == [213] * BATCH
    assert m.tobytes() == cm.mag("f32", spec).tobytes()
    wv, wi = cm.extreme("max", m)
    assert val.cpu().numpy().tobytes() == wv.tobytes() and wi.tolist() == [213] * BATCH
