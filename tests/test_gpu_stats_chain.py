"""The use case behind the statistics functions: a level and a peak of a filtered signal without a host copy.
arm_fir_f32_batch on 8 streams, each followed on its stream by arm_rms_f32_batch and arm_absmax_f32_batch on the FIR's
output; both results must equal the numpy restatement applied to the FIR's own output, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import statistics_ref as sr

cm = sr.cm
STREAMS, ITEMS, BLOCK, TAPS = 8, 6, 1000, 32


@pytest.mark.gpu
def test_fir_rms_absmax_chain_on_eight_streams(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(61)
    coeffs = (rng.standard_normal(TAPS) / np.sqrt(TAPS)).astype(np.float32)
    dc = torch.from_numpy(coeffs.copy()).cuda()
    S = dsp.arm_fir_instance_f32()
    S.numTaps = TAPS
    S.pCoeffs = C.cast(dc.data_ptr(), S._fields_[2][1])
    x = rng.uniform(-1, 1, (STREAMS, ITEMS, BLOCK)).astype(np.float32)
    src = [torch.from_numpy(x[s]).cuda() for s in range(STREAMS)]
    dst = [torch.from_numpy(cm.marked("f32", (ITEMS, BLOCK))).cuda() for _ in range(STREAMS)]
    hist = [torch.zeros((ITEMS, TAPS - 1), dtype=torch.float32, device="cuda") for _ in range(STREAMS)]
    rms = [torch.from_numpy(cm.marked("f32", ITEMS)).cuda() for _ in range(STREAMS)]
    peak = [torch.from_numpy(cm.marked("f32", ITEMS)).cuda() for _ in range(STREAMS)]
    at = [torch.from_numpy(cm.marked("u32", ITEMS).view(np.int32)).cuda() for _ in range(STREAMS)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(STREAMS)]
    for s, st in enumerate(streams):
        dsp.fir_batch(S, src[s], dst[s], hist[s], stream=st)
        dsp.rms_batch(dst[s], rms[s], stream=st)
        dsp.absmax_batch(dst[s], peak[s], at[s], stream=st)
    torch.cuda.synchronize()
    for s in range(STREAMS):
        y = dst[s].cpu().numpy()
        assert not (y.view(np.uint32) == 0x5A5A5A5A).any()
        assert rms[s].cpu().numpy().tobytes() == sr.run("rms_f32", y)["value"].tobytes(), s
        want = sr.run("absmax_f32", y)
        assert peak[s].cpu().numpy().tobytes() == want["value"].tobytes(), s
        assert at[s].cpu().numpy().view(np.uint32).tolist() == want["index"].tolist(), s
