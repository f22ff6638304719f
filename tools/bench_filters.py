#!/usr/bin/env python3
"""Throughput of the filtering functions outside bench.py's workloads (round 2 additions):
arm_fir_q7, arm_fir_decimate_*, arm_fir_interpolate_*, arm_fir_sparse_*, arm_fir_lattice_*, the biquad cascades, the IIR
lattice and the LMS / normalised LMS filters through the batched device API on one GPU, HIP-event timed on the launch stream after a clock-settle phase, each with a bit-exact
check of 2 streams against the CPU checker (the reference build when present; the biquad rows
against tests/biquad_ref.py and the IIR lattice / LMS rows against tests/adaptive_ref.py, the numpy
restatements that equal the committed reference fixtures).  fir_f32_t32 and fir_lattice_f32 are the
yardsticks of the 32-tap / 32-stage adaptive rows: the nearest existing filters of the same arithmetic class.
Usage: python tools/bench_filters.py [name ...]  -> one JSON line per workload."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import cmsisdsp_amd as dsp  # noqa: E402
from cmsisdsp_amd import _abi  # noqa: E402
import adaptive_ref  # noqa: E402
import biquad_ref  # noqa: E402
import refs  # noqa: E402

BATCH, BLOCK, TAPS = 1 << 16, 4096, 128
SP_TAPS, SP_DELAY = 32, 1024            # sparse: 32 nonzero taps at delays in [0, 1024]
LAT_STAGES = 32                         # lattice: 32 stages
# name: (function, factor, dtype)
CASES = {
    "fir_q7": ("q7", 1, "q7"),
    "fir_decimate_f32_m4": ("decimate_f32", 4, "f32"),
    "fir_decimate_q15_m4": ("decimate_q15", 4, "q15"),
    "fir_decimate_fast_q31_m4": ("decimate_fast_q31", 4, "q31"),
    "fir_decimate_q31_m4": ("decimate_q31", 4, "q31"),
    "fir_interpolate_f32_l4": ("interpolate_f32", 4, "f32"),
    "fir_interpolate_q31_l4": ("interpolate_q31", 4, "q31"),
    "fir_sparse_f32": ("sparse_f32", 1, "f32"),
    "fir_sparse_q31": ("sparse_q31", 1, "q31"),
    "fir_sparse_q15": ("sparse_q15", 1, "q15"),
    "fir_sparse_q7": ("sparse_q7", 1, "q7"),
    "fir_lattice_f32": ("lattice_f32", 1, "f32"),
    "fir_lattice_q31": ("lattice_q31", 1, "q31"),
    "fir_lattice_q15": ("lattice_q15", 1, "q15"),
}
# biquad rows: one JSON line per (numStages, batch) of BQ_SHAPES
BIQUAD = {
    "biquad_df1_f32": "arm_biquad_cascade_df1_f32",
    "biquad_df1_q31": "arm_biquad_cascade_df1_q31",
    "biquad_df1_q15": "arm_biquad_cascade_df1_q15",
    "biquad_df1_fast_q31": "arm_biquad_cascade_df1_fast_q31",
    "biquad_df1_fast_q15": "arm_biquad_cascade_df1_fast_q15",
    "biquad_df2T_f32": "arm_biquad_cascade_df2T_f32",
    "biquad_stereo_df2T_f32": "arm_biquad_cascade_stereo_df2T_f32",
    "biquad_32x64_q31": "arm_biquad_cas_df1_32x64_q31",
}
BQ_SHAPES = [(4, BATCH), (32, BATCH), (4, 256), (32, 256)]
# IIR lattice and LMS rows: one JSON line per numStages / numTaps of AD_SIZES, then the arm_fir_f32 yardstick
ADAPTIVE = {"iir_lattice_f32": "arm_iir_lattice_f32", "iir_lattice_q31": "arm_iir_lattice_q31",
            "iir_lattice_q15": "arm_iir_lattice_q15", "lms_f32": "arm_lms_f32", "lms_q31": "arm_lms_q31",
            "lms_q15": "arm_lms_q15", "lms_norm_f32": "arm_lms_norm_f32", "lms_norm_q15": "arm_lms_norm_q15"}
AD_SIZES = [4, 32]
HBM_PEAK = 8e12                         # bytes/s
TDT = {"f32": torch.float32, "q15": torch.int16, "q31": torch.int32, "q7": torch.int8}


def checker():
    try:
        return refs.ref_lib(), "reference"
    except (FileNotFoundError, OSError):
        return refs.oracle_lib(), "oracle"


def timed(launch, steps=10, warmup=3, settle_ms=40.0):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(64):
        launch()
        e1.record(st)
        e1.synchronize()
        if e0.elapsed_time(e1) >= settle_ms:
            break
    for _ in range(warmup):
        launch()
    e0.record(st)
    for _ in range(steps):
        launch()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def run(name):
    fn, factor, kind = CASES[name]
    rng = np.random.default_rng(7)
    dt = refs.DTYPE[kind]
    sparse = fn.startswith("sparse")
    lattice = fn.startswith("lattice")
    taps = SP_TAPS if sparse else LAT_STAGES if lattice else TAPS
    if lattice and kind == "f32":
        c = rng.uniform(-0.9, 0.9, taps).astype(np.float32)
    elif kind == "f32":
        c = (rng.standard_normal(taps) / np.sqrt(taps)).astype(np.float32)
    else:
        info = np.iinfo(dt)
        c = rng.integers(info.min, info.max, taps, endpoint=True).astype(dt)
    delays = np.sort(rng.choice(SP_DELAY + 1, taps, replace=False)).astype(np.int32)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    if kind == "f32":
        src = torch.rand((BATCH, BLOCK), generator=g, device="cuda") - 0.5
    else:
        info = np.iinfo(dt)
        src = torch.randint(int(info.min), int(info.max) + 1, (BATCH, BLOCK), generator=g, device="cuda",
                            dtype=torch.int64).to(TDT[kind])
    dc = torch.from_numpy(c.copy()).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if lattice:
        S = _abi.arm_fir_lattice_instance(numStages=taps, pState=None, pCoeffs=dc.data_ptr())
        H, nout, f = taps, BLOCK, getattr(dsp.lib, f"arm_fir_{fn}_batch")
    elif sparse:
        dd = torch.from_numpy(delays.copy()).cuda()
        S = _abi.arm_fir_sparse_instance(numTaps=taps, pCoeffs=dc.data_ptr(), maxDelay=SP_DELAY,
                                         pTapDelay=dd.data_ptr())
        H, nout, f = SP_DELAY, BLOCK, getattr(dsp.lib, f"arm_fir_{fn}_batch")
    elif fn == "q7":
        S = _abi.arm_fir_instance_q7(numTaps=TAPS, pState=None, pCoeffs=dc.data_ptr())
        H, nout, f = TAPS - 1, BLOCK, dsp.lib.arm_fir_q7_batch
    elif fn.startswith("decimate"):
        S = _abi.arm_fir_decimate_instance(M=factor, numTaps=TAPS, pCoeffs=dc.data_ptr(), pState=None)
        H, nout, f = TAPS - 1, BLOCK // factor, getattr(dsp.lib, f"arm_fir_{fn}_batch")
    else:
        S = _abi.arm_fir_interpolate_instance(L=factor, phaseLength=TAPS // factor, pCoeffs=dc.data_ptr(),
                                              pState=None)
        H, nout, f = TAPS // factor - 1, BLOCK * factor, getattr(dsp.lib, f"arm_fir_{fn}_batch")
    dst = torch.empty((BATCH, nout), dtype=TDT[kind], device="cuda")
    hist = torch.zeros((BATCH, H), dtype=TDT[kind], device="cuda")

    def launch(d=dst, h=hist, s=src, b=BATCH):
        rc = f(C.byref(S), C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()), BLOCK, b, C.c_void_p(h.data_ptr()),
               stream)
        assert rc == 0, dsp.last_error()

    ms = timed(launch)
    host, hk = checker()
    d2 = torch.empty((2, nout), dtype=TDT[kind], device="cuda")
    h2 = torch.zeros((2, H), dtype=TDT[kind], device="cuda")
    launch(d2, h2, src[:2].contiguous(), 2)
    torch.cuda.synchronize()
    ok = True
    for i in range(2):
        x = src[i].cpu().numpy()
        if lattice:
            want = host.lattice(kind, c, [x])[0][0]
        elif sparse:
            want = host.sparse(kind, c, delays, SP_DELAY, [x])[0][0]
        elif fn == "q7":
            want = host.fir("q7", c, [x])[0][0]
        else:
            want = host.multirate(fn, factor, c, [x])[1][0]
        ok &= d2[i].cpu().numpy().tobytes() == want.tobytes()
    macs = BATCH * (BLOCK * taps * (2 if lattice else 1) if fn == "q7" or sparse or lattice else (BLOCK // factor) * TAPS if fn.startswith("decimate")
                    else BLOCK * TAPS)
    esz = np.dtype(dt).itemsize
    extra = {"maxDelay": SP_DELAY} if sparse else {"numStages": taps} if lattice else {}
    return {"workload": name, "function": f"arm_fir_{fn}", "numTaps": taps, **extra, "factor": factor, "blockSize": BLOCK,
            "batch": BATCH, "avg_kernel_ms": round(ms, 4),
            "input_gsamples_per_s": round(BATCH * BLOCK / (ms * 1e-3) * 1e-9, 2),
            "output_gsamples_per_s": round(BATCH * nout / (ms * 1e-3) * 1e-9, 2),
            "gmacs_per_s": round(macs / (ms * 1e-3) * 1e-9, 1),
            "hbm_gbs": round(BATCH * (BLOCK + nout) * esz / (ms * 1e-3) * 1e-9, 1),
            "bit_exact": bool(ok), "checker": hk}


def run_biquad(name, stages, batch):
    func = BIQUAD[name]
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    ps = 1 if func in biquad_ref.HAS_SHIFT else 0
    c = biquad_ref.stable_coeffs(func, stages, ps, 7)
    tdt = {np.float32: torch.float32, np.int32: torch.int32, np.int16: torch.int16, np.int64: torch.int64}
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    if dt == np.float32:
        src = torch.rand((batch, BLOCK * ch), generator=g, device="cuda") - 0.5
    else:
        info = np.iinfo(dt)
        src = torch.randint(int(info.min) // 2, int(info.max) // 2, (batch, BLOCK * ch), generator=g, device="cuda",
                            dtype=torch.int64).to(tdt[dt])
    dc = torch.from_numpy(c.copy()).cuda()
    inst = _abi.BIQUAD_FUNCS[func][0]
    kw = {"postShift": ps} if any(f == "postShift" for f, _ in inst._fields_) else {}
    S = inst(numStages=stages, pState=None, pCoeffs=dc.data_ptr(), **kw)
    f = getattr(dsp.lib, func + "_batch")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dst = torch.empty_like(src)
    state = torch.zeros((batch, ks * stages), dtype=tdt[sdt], device="cuda")

    def launch(d=dst, h=state, s=src, b=batch):
        rc = f(C.byref(S), C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()), BLOCK, b, C.c_void_p(h.data_ptr()),
               stream)
        assert rc == 0, dsp.last_error()

    ms = timed(launch)
    state.zero_()                          # parity: the first and the last stream from a zero state
    launch()
    torch.cuda.synchronize()
    rows = [0, batch - 1]
    want, wstate = biquad_ref.run(func, c, ps, src[rows].cpu().numpy(), np.zeros((2, ks * stages), dtype=sdt))
    ok = dst[rows].cpu().numpy().tobytes() == want.tobytes() and state[rows].cpu().numpy().tobytes() == wstate.tobytes()
    esz = np.dtype(dt).itemsize
    rate = batch * BLOCK * ch / (ms * 1e-3)      # words per second
    return {"workload": name, "function": func, "numStages": stages, "blockSize": BLOCK, "batch": batch,
            "avg_kernel_ms": round(ms, 4), "gsamples_per_s": round(rate * 1e-9, 2),
            "gstage_samples_per_s": round(rate * stages * 1e-9, 1),
            "hbm_gbs": round(rate * 2 * esz * 1e-9, 1), "hbm_fraction": round(rate * 2 * esz / HBM_PEAK, 3),
            "bit_exact": bool(ok), "checker": "biquad_ref"}


def run_adaptive(name, n, batch=BATCH):
    """IIR lattice: n stages, shared k / v; LMS: n taps, every stream its own taps, history and energy."""
    func = ADAPTIVE[name]
    dt, fam = adaptive_ref.FUNCS[func]
    tdt = {np.float32: torch.float32, np.int32: torch.int32, np.int16: torch.int16}[dt]
    inst = _abi.ADAPTIVE_FUNCS[func][0]
    g = torch.Generator(device="cuda")
    g.manual_seed(11)

    def noise(shape, scale):
        u = (torch.rand(shape, generator=g, device="cuda") - 0.5) * (2 * scale)
        return u if dt == np.float32 else (u * float(-int(np.iinfo(dt).min))).to(tdt)

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    f = getattr(dsp.lib, func + "_batch")
    # normalised: small enough that the q15 energy (32 taps) never saturates, so the reciprocal's argument stays defined
    src, rows = noise((batch, BLOCK), 0.1 if fam == "nlms" else 0.5), [0, batch - 1]
    esz = np.dtype(dt).itemsize
    if fam == "iir":
        k, v = adaptive_ref.lattice_coeffs(func, n, 7)
        dk, dv = torch.from_numpy(k.copy()).cuda(), torch.from_numpy(v.copy()).cuda()
        S = inst(numStages=n, pState=None, pkCoeffs=dk.data_ptr(), pvCoeffs=dv.data_ptr())
        dst, state = torch.empty_like(src), torch.zeros((batch, n), dtype=tdt, device="cuda")

        def launch():
            assert f(C.byref(S), ptr(src), ptr(dst), BLOCK, batch, ptr(state), stream) == 0, dsp.last_error()

        ms = timed(launch)
        state.zero_()
        launch()
        torch.cuda.synchronize()
        want, wstate = adaptive_ref.iir_lattice(func, k, v, src[rows].cpu().numpy(), np.zeros((2, n), dtype=dt))
        ok = dst[rows].cpu().numpy().tobytes() == want.tobytes() and state[rows].cpu().numpy().tobytes() == wstate.tobytes()
        bytes_per_sample, size = 2 * esz, {"numStages": n}
    else:
        mu, ps = adaptive_ref.default_mu(func), (1 if dt != np.float32 else 0)
        kw = {"postShift": ps} if any(fn == "postShift" for fn, _ in inst._fields_) else {}
        S = inst(numTaps=n, pState=None, pCoeffs=None, mu=mu, **kw)
        ref, out, err = noise((batch, BLOCK), 0.5), torch.empty_like(src), torch.empty_like(src)
        c0 = noise((batch, n), 0.1)
        coeffs, state = c0.clone(), torch.zeros((batch, max(n - 1, 1)), dtype=tdt, device="cuda")
        ex = torch.zeros((batch, 2), dtype=tdt, device="cuda")
        tail = [ptr(coeffs), ptr(state)] + ([ptr(ex)] if fam == "nlms" else []) + [stream]

        def launch():
            assert f(C.byref(S), ptr(src), ptr(ref), ptr(out), ptr(err), BLOCK, batch, *tail) == 0, dsp.last_error()

        ms = timed(launch)
        coeffs.copy_(c0), state.zero_(), ex.zero_()
        launch()
        torch.cuda.synchronize()
        cpu = lambda t: t[rows].cpu().numpy()   # noqa: E731
        wy, we, wc, wst, wex = adaptive_ref.lms(func, mu, ps, cpu(src), cpu(ref), cpu(c0), np.zeros((2, n - 1), dtype=dt),
                                                np.zeros((2, 2), dtype=dt) if fam == "nlms" else None)
        ok = (cpu(out).tobytes() == wy.tobytes() and cpu(err).tobytes() == we.tobytes() and
              cpu(coeffs).tobytes() == wc.tobytes() and cpu(state)[:, :n - 1].tobytes() == wst.tobytes() and
              (fam != "nlms" or cpu(ex).tobytes() == wex.tobytes()))
        bytes_per_sample, size = 4 * esz, {"numTaps": n}
    rate = batch * BLOCK / (ms * 1e-3)
    return {"workload": name, "function": func, **size, "blockSize": BLOCK, "batch": batch, "avg_kernel_ms": round(ms, 4),
            "gsamples_per_s": round(rate * 1e-9, 2), "gtap_samples_per_s": round(rate * n * 1e-9, 1),
            "hbm_bytes_per_sample": bytes_per_sample, "hbm_gbs": round(rate * bytes_per_sample * 1e-9, 1),
            "hbm_fraction": round(rate * bytes_per_sample / HBM_PEAK, 3), "bit_exact": bool(ok), "checker": "adaptive_ref"}


def run_fir_f32_t32():
    """arm_fir_f32 at 32 taps, the standard shape: the yardstick of the 32-tap LMS rows."""
    taps = 32
    rng = np.random.default_rng(7)
    c = (rng.standard_normal(taps) / np.sqrt(taps)).astype(np.float32)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    src = torch.rand((BATCH, BLOCK), generator=g, device="cuda") - 0.5
    dc = torch.from_numpy(c.copy()).cuda()
    S = _abi.arm_fir_instance_f32(numTaps=taps, pState=None, pCoeffs=C.cast(dc.data_ptr(), _abi.c_f32p))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(d, h, s, b):
        rc = dsp.lib.arm_fir_f32_batch(C.byref(S), C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()), BLOCK, b,
                                       C.c_void_p(h.data_ptr()), stream)
        assert rc == 0, dsp.last_error()

    dst, hist = torch.empty_like(src), torch.zeros((BATCH, taps - 1), device="cuda")
    ms = timed(lambda: launch(dst, hist, src, BATCH))
    host, hk = checker()
    d2, h2 = torch.empty((2, BLOCK), device="cuda"), torch.zeros((2, taps - 1), device="cuda")
    launch(d2, h2, src[:2].contiguous(), 2)
    torch.cuda.synchronize()
    ok = all(d2[i].cpu().numpy().tobytes() == host.fir("f32", c, [src[i].cpu().numpy()])[0][0].tobytes() for i in range(2))
    rate = BATCH * BLOCK / (ms * 1e-3)
    return {"workload": "fir_f32_t32", "function": "arm_fir_f32", "numTaps": taps, "blockSize": BLOCK, "batch": BATCH,
            "avg_kernel_ms": round(ms, 4), "gsamples_per_s": round(rate * 1e-9, 2),
            "gtap_samples_per_s": round(rate * taps * 1e-9, 1), "hbm_gbs": round(rate * 8 * 1e-9, 1),
            "bit_exact": bool(ok), "checker": hk}


if __name__ == "__main__":
    for name in sys.argv[1:] or list(CASES) + list(BIQUAD) + list(ADAPTIVE) + ["fir_f32_t32"]:
        if name in ADAPTIVE:
            for n in AD_SIZES:
                print(json.dumps(run_adaptive(name, n)), flush=True)
                torch.cuda.empty_cache()
            continue
        if name == "fir_f32_t32":
            print(json.dumps(run_fir_f32_t32()), flush=True)
            torch.cuda.empty_cache()
            continue
        if name in BIQUAD:
            for stages, batch in BQ_SHAPES:
                print(json.dumps(run_biquad(name, stages, batch)), flush=True)
                torch.cuda.empty_cache()
            continue
        print(json.dumps(run(name)), flush=True)
        torch.cuda.empty_cache()
