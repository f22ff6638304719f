"""The reference's InterpolationTests{F32,Q31,Q15,Q7} and QuaternionTestsF32 (tests/suite_replay_interp.py) replayed
against the GPU library, one case per `Test` line.  First through the drop-ins, called through ctypes on host buffers
exactly as the suite calls arm_math.h: every line passes the suite's own thresholds, gives the words the reference
build gave and leaves every output's tail alone.  The one-sample linear and bilinear drop-ins run on the host, so every
line then runs a second time through the _batch form on device tensors, which must give the same words."""
import numpy as np
import pytest

import suite_replay_interp as sri
from f32_classes import assert_same_words
from test_suites_interp import FIX, LINES, check_line

BATCH_FUNC = {"arm_quaternion_prod_single_f32": "product", "arm_quaternion_product_f32": "product"}


def same(got, want, what):
    if want.dtype == np.float32:
        assert_same_words(got, want, what)
    else:
        assert np.array_equal(got, want), what


@pytest.mark.gpu
@pytest.mark.parametrize("e", LINES, ids=sri.line_id)
def test_line_on_the_gpu_library(dsp, torch_gpu, e):
    torch = torch_gpu

    def after(name):
        assert dsp.last_error()[0] == 0, (name, dsp.last_error())
    outs = check_line(sri.Ctypes(dsp.lib, dsp._abi, after), e)
    pats = sri.patterns(FIX, e["suite"])
    t = sri.SUITES[e["suite"]]
    want = outs["output"].words
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    tdt = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16, "q7": torch.int8}[t]
    out = torch.zeros(want.size, dtype=tdt, device="cuda")
    method = e["method"]
    if e["suite"] == "QuaternionTestsF32":
        func, src, _ = sri.QUATERNION[method]
        a = dev(pats[src])
        if "prod" in method:
            dsp.quaternion_product_batch(a.view(-1, 4), dev(pats["Input2"]).view(-1, 4), out.view(-1, 4))
        else:
            name = func[len("arm_"):-len("_f32")]
            wa, wd = dsp._abi.QUATERNION_FUNCS[name]
            n = want.size // wd
            dsp.quaternion_batch(name, a[:n * wa].view(n, wa), out.view(n, wd))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if method == "test_rotation2quaternion_f32":
            q = got.reshape(-1, 4)
            q[q[:, 0] < 0] *= np.float32(-1)
    elif method in sri.SPLINES:
        k, n, spline_type, block = sri.SPLINES[method]
        x, y, xq = dev(pats["InputX" + k][:n]), dev(pats["InputY" + k][:n]).view(1, n), dev(pats["OutputX" + k][:block])
        coeffs = torch.zeros((1, 3 * (n - 1)), dtype=torch.float32, device="cuda")
        temp = torch.zeros((1, 2 * n - 1), dtype=torch.float32, device="cuda")
        dsp.spline_init_batch(spline_type, x, y, coeffs, temp)
        dsp.spline_batch(x, y, coeffs, xq, out.view(1, block))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        same(coeffs.cpu().numpy()[0], outs["splineCoefs"].words, sri.line_id(e) + " coeffs, _batch")
        same(temp.cpu().numpy()[0], outs["buffer"].words, sri.line_id(e) + " temp, _batch")
    elif method.startswith("test_bilinear"):
        cfg, inp = pats["Config2"], pats["Input2"]
        S, keep = dsp.bilinear_interp_instance(t, dev(pats["YVals2"][:int(cfg[0]) * int(cfg[1])]).view(int(cfg[1]), int(cfg[0])))
        dsp.bilinear_interp_batch(t, S, dev(inp[0::2]), dev(inp[1::2]), out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    else:
        table = dev(pats["YVals1"])
        arg = dsp.linear_interp_instance(0.0, 1.0, table)[0] if t == "f32" else table
        dsp.linear_interp_batch(t, arg, dev(pats["Input1"]), out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    same(got, want, sri.line_id(e) + " through the _batch form")
