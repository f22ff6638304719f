#!/usr/bin/env python3
"""Throughput of the complex matrix multiplies, arm_mat_cmplx_mult_{f32,q31,q15}_batch, on one GPU.

Workload: complex 512 x 512 x 512, batch 64.  Yardstick: the real product of the same type at the embedded
shape (512 x 1024 x 1024, batch 64), which issues the same MFMA work and reads twice the B bytes.  Both are
timed in the same process with HIP events on the launch stream after a clock-settle phase, alternating,
REPEATS times each over a window of at least a second, so the repeat spread of each is visible next to their
ratio.  Rows 0..15 of item 0 are checked bit for bit against the CPU checker first (q15 / q31:
tests/cmplx_mat_ref.py; f32: the stated fmaf chain, oracle.mat_mult_fmaf on the embedded operands).
Operations are counted as 8 M N K per complex product (4 multiplies and 4 adds per complex MAC).
Usage: python tools/bench_matrix.py [f32|q31|q15 ...]  -> one JSON line per workload."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import cmsisdsp_amd as dsp  # noqa: E402
import cmplx_mat_ref as cr  # noqa: E402
import refs  # noqa: E402

M = K = N = 512
BATCH = 64
REPEATS = 3
WINDOW_MS = 1000.0
FP32_PEAK_TFLOPS = 157.3        # dense f32 MFMA
I8_PEAK_TOPS = 5000.0           # dense i8 MFMA
PLANES = {"q15": 4, "q31": 16}  # byte-plane products per exact product
TDT = {"f32": torch.float32, "q15": torch.int16, "q31": torch.int32}


def settle(launch, settle_ms=40.0):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(64):
        launch()
        e1.record(st)
        e1.synchronize()
        if e0.elapsed_time(e1) >= settle_ms:
            break


def timed(launch, steps, warmup=3):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        launch()
    e0.record(st)
    for _ in range(steps):
        launch()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def run(kind):
    rng = np.random.default_rng(17)
    # scaled fixed-point operands: outputs spread over the range instead of sitting on the clip
    a, b = cr.operands(kind, "uniform" if kind == "f32" else "scaled", M, K, N, rng, BATCH)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dc = torch.zeros((BATCH, M, 2 * N), dtype=TDT[kind], device="cuda")
    # the yardstick's operands: the same A, and a real B of the embedded shape
    rb = torch.from_numpy(cr.embed(b) if kind == "f32" else
                          cr.fill_fixed(kind, "scaled", (BATCH, 2 * K, 2 * N), K, rng)).cuda()
    rc = torch.zeros_like(dc)

    def cx():
        dsp.mat_cmplx_mult_batch(da, db, dc)

    def real():
        dsp.mat_mult_batch(da, rb, rc)

    cx()
    torch.cuda.synchronize()
    got = dc[0, :16].cpu().numpy()
    if kind == "f32":
        want = refs.oracle_lib().mat_mult_fmaf(a[0, :16], cr.embed(b[0]))[1]
    else:
        want = cr.mult_fixed(kind, a[0, :16], b[0])
    ok = got.tobytes() == want.tobytes()

    settle(cx)
    steps = {}
    for name, f in (("cx", cx), ("real", real)):
        steps[name] = max(3, int(np.ceil(WINDOW_MS / timed(f, 5))))
    ms = {"cx": [], "real": []}
    for _ in range(REPEATS):
        for name, f in (("cx", cx), ("real", real)):
            ms[name].append(timed(f, steps[name]))
    ops = 8.0 * M * N * K * BATCH
    best = {k: min(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in ms.items()}
    rate = ops / (best["cx"] * 1e-3) * 1e-12
    line = {"workload": f"mat_cmplx_mult_{kind}", "shape": [M, K, N], "batch": BATCH, "bitexact_rows_0_15": ok,
            "value": round(rate, 3), "unit": "TFLOP/s" if kind == "f32" else "TOPS (8 M N K per complex product)",
            "ms": [round(x, 4) for x in ms["cx"]], "spread": round(spread["cx"], 4),
            "yardstick": {"workload": f"mat_mult_{kind} {M}x{2 * K}x{2 * N}", "ms": [round(x, 4) for x in ms["real"]],
                          "value": round(ops / (best["real"] * 1e-3) * 1e-12, 3), "spread": round(spread["real"], 4)},
            "ratio_to_yardstick": round(best["real"] / best["cx"], 4), "steps": steps, "version": dsp.version()}
    if kind == "f32":
        line["roofline"] = {"bound": "mfma", "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                            "frac": round(rate / FP32_PEAK_TFLOPS, 4)}
    else:
        i8 = rate * PLANES[kind]
        line["roofline"] = {"bound": "mfma", "achieved": round(i8, 2), "peak": I8_PEAK_TOPS,
                            "unit": "TOPS (i8 MFMA issued incl. the byte-plane products)",
                            "frac": round(i8 / I8_PEAK_TOPS, 4)}
    print(json.dumps(line), flush=True)
    return ok


def main():
    kinds = sys.argv[1:] or ["f32", "q31", "q15"]
    bad = [k for k in kinds if not run(k)]
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
