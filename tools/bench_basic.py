#!/usr/bin/env python3
"""Throughput of the basic math functions on one GPU (arm_{add .. not}_*_batch, arm_dot_prod_*_batch).

    python tools/bench_basic.py [ew|dot|single ...] [--gib G] [--window MS]

Timing is tools/bench_cmplx.py's: a clock-settle phase, then REPEATS windows of about --window ms between HIP events;
a line reports the best window, the repeat spread and the fraction of the 8 TB/s HBM peak its algorithmic bytes reach.

  ew      every element-wise function on items of 1024 words, G GiB (default 1) of traffic per call: words read and
          written once, so three streams for the two-source functions and two for the one-source ones.  The yardstick
          is arm_mat_add_<type>_batch on the same tensors in the same process (q7 and the bitwise types:
          arm_mat_add_q15_batch on the reinterpreted bytes; a one-source function runs over half as many items again,
          so it moves G GiB too, and is compared per byte moved, i.e. by HBM fraction).  The yardstick is timed before and after each type's
          functions; "yardstick_spread" is the range of those fractions, and "below_yardstick" marks a function whose
          fraction falls below the lowest of them by more than that.
  dot     arm_dot_prod_<type>_batch at 64 and 1024 words per item, one b per item and one shared b (bStride 0), in
          M items/s, against arm_mse_<type>_batch on the same tensors (the same two sources through the same mapping)
          and, for f32, arm_cmplx_dot_prod_f32_batch on the same bytes.
  single  arm_dot_prod_f32 (the synchronous drop-in) on one 2^20-word vector, device and host pointers: ns per sample
          of wall-clock time.

The first and last item of every result are checked bit for bit against tests/basic_math_ref.py first."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import basic_math_ref as br  # noqa: E402
import bench_cmplx as bc  # noqa: E402
import cmsisdsp_amd as dsp  # noqa: E402

HBM_TBPS = bc.HBM_TBPS
TDT = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16, "q7": torch.int8, "u32": torch.int32,
       "u16": torch.int16, "u8": torch.uint8}
RDT = {"f32": torch.float32, "q31": torch.int64, "q15": torch.int64, "q7": torch.int32}
N = 1024


def frac(nbytes, ms):
    return nbytes / (ms * 1e-3) / (HBM_TBPS * 1e12)


def rnd(t, gen, *shape):
    if t == "f32":
        return torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
    info = torch.iinfo(TDT[t])
    return torch.randint(info.min, info.max + 1, shape, generator=gen, device="cuda", dtype=TDT[t])


def as_np(t, x):
    return x.cpu().numpy().view(br.DT[t])


def mat_add_yardstick(t, a, b, d):
    """arm_mat_add_<t>_batch (q7, u8, u16, u32: _q15 on the reinterpreted bytes) over the three tensors."""
    v = (lambda x: x) if t in ("f32", "q31", "q15") else (lambda x: x.view(torch.int16))
    x, y, z = (v(k).view(-1, 32, 32) for k in (a, b, d))
    ms, steps = bc.measure(lambda: dsp.mat_add_batch(x, y, z))
    return {"workload": f"arm_mat_add_{t if t in ('f32', 'q31', 'q15') else 'q15'}_batch, same tensors",
            "ms": [round(k, 4) for k in ms], "steps": steps, "frac": round(frac(3 * a.numel() * a.element_size(), min(ms)), 4)}


def run_ew_type(t, gib):
    ops = ["and", "or", "xor", "not"] if t in br.BITS_TYPES else \
        ["add", "sub", "mult", "offset", "scale", "clip", "abs", "negate"] + (["shift"] if t != "f32" else [])
    size = torch.empty(0, dtype=TDT[t]).element_size()
    # G GiB per call: `batch` items for the three streams of a two-source function, half as many again for the two
    # streams of a one-source function (the first `batch` rows of the same tensors serve the two-source ones)
    batch = max(2, int(gib * 2 ** 30 / (size * N * 3)) // 2 * 2)
    big = batch * 3 // 2
    gen = torch.Generator(device="cuda").manual_seed(7)
    a_all, b_all = rnd(t, gen, big, N), rnd(t, gen, batch, N)
    d_all = torch.zeros_like(a_all)
    lines, ok_all = [], True
    yards = [mat_add_yardstick(t, a_all[:batch], b_all, d_all[:batch])]
    gen_np = np.random.default_rng(11)
    for op in ops:
        func = f"{op}_{t}"
        two = br.two_sources(func)
        rows = batch if two else big
        a, b, dst = a_all[:rows], b_all, d_all[:rows]
        scalars = br.rand_scalars(func, gen_np)
        fn = getattr(dsp, op + "_batch")
        if op == "scale":
            ours = lambda: fn(a, scalars[0], dst, *scalars[1:])                     # noqa: E731
        elif two:
            ours = lambda: fn(a, b, dst)                                            # noqa: E731
        else:
            ours = lambda: fn(a, *scalars, dst)                                     # noqa: E731
        ours()
        torch.cuda.synchronize()
        ok = all(br.same_words(as_np(t, dst[i]), br.run(func, as_np(t, a[i]), as_np(t, b[i]) if two else None,
                                                        scalars)["dst"], t == "f32") for i in (0, rows - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        nbytes = size * N * rows * (3 if two else 2)
        lines.append({"workload": func, "n": N, "batch": rows, "bitexact_first_last": ok, "streams": 3 if two else 2,
                      "value": round(rows / (min(ms) * 1e-3) * 1e-6, 4), "unit": "M items/s",
                      "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": HBM_TBPS,
                                   "frac": round(frac(nbytes, min(ms)), 4)},
                      "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4),
                      "steps": steps})
    yards.append(mat_add_yardstick(t, a_all[:batch], b_all, d_all[:batch]))
    fr = [y["frac"] for y in yards]
    spread = round(max(fr) - min(fr), 4)
    for line in lines:
        line["yardstick"] = yards
        line["yardstick_spread"] = spread
        line["below_yardstick"] = bool(line["roofline"]["frac"] < min(fr) - spread)
        line["version"] = dsp.version()
        print(json.dumps(line), flush=True)
    return ok_all


def run_dot(t, n, gib):
    size = torch.empty(0, dtype=TDT[t]).element_size()
    batch = max(1, int(gib * 2 ** 30 / (size * 2 * n)))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a, b = rnd(t, gen, batch, n), rnd(t, gen, batch, n)
    res = torch.zeros(batch, dtype=RDT[t], device="cuda")
    ok_all = True
    for shared in (False, True):
        bb = b[0].contiguous() if shared else b
        ours = lambda: dsp.dot_prod_batch(a, bb, res)                               # noqa: E731
        ours()
        torch.cuda.synchronize()
        ok = all(br.same_words(res[i].cpu().numpy(),
                               br.run(f"dot_prod_{t}", as_np(t, a[i]), as_np(t, bb if shared else b[i]))["value"],
                               t == "f32") for i in (0, batch - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        best = min(ms)
        nbytes = size * n * (batch + (1 if shared else batch))
        line = {"workload": f"dot_prod_{t}" + (" shared b (bStride 0)" if shared else ""), "n": n, "batch": batch,
                "bitexact_first_last": ok, "value": round(batch / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
                "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": HBM_TBPS, "frac": round(frac(nbytes, best), 4)},
                "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps}
        if not shared:
            out = torch.zeros(batch, dtype=TDT[t], device="cuda")
            bc.yardstick(line, "yardstick", f"arm_mse_{t}_batch, same tensors", lambda: dsp.mse_batch(a, b, out), best)
            if t == "f32":
                re, im = (torch.zeros(batch, dtype=torch.float32, device="cuda") for _ in range(2))
                bc.yardstick(line, "yardstick_cmplx", "arm_cmplx_dot_prod_f32_batch, same bytes",
                             lambda: dsp.cmplx_dot_prod_batch(a, b, re, im), best)
        line["version"] = dsp.version()
        print(json.dumps(line), flush=True)
    return ok_all


def run_single(n=2 ** 20):
    rng = np.random.default_rng(1)
    ha, hb = br.rand("f32", n, rng), br.rand("f32", n, rng)
    da, db = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
    dres, hres = torch.zeros(1, dtype=torch.float32, device="cuda"), np.zeros(1, dtype=np.float32)
    for where, args in (("device pointers", (da.data_ptr(), db.data_ptr(), n, dres.data_ptr())),
                        ("host pointers", (ha.ctypes.data, hb.ctypes.data, n, hres.ctypes.data))):
        times = []
        for _ in range(2 + bc.REPEATS):
            t0 = time.perf_counter()
            dsp.lib.arm_dot_prod_f32(*args)
            times.append((time.perf_counter() - t0) * 1e3)
        ms = times[2:]
        best = min(ms)
        print(json.dumps({"workload": f"arm_dot_prod_f32 drop-in, one vector, {where}", "n": n, "batch": 1,
                          "value": round(best * 1e6 / n, 4), "unit": "ns/sample (wall clock)",
                          "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - best) / best, 4),
                          "version": dsp.version()}), flush=True)
    torch.cuda.synchronize()
    return dres.cpu().numpy().tobytes() == hres.tobytes()


def main():
    args = sys.argv[1:]
    gib = 1.0
    for flag in ("--gib", "--window"):
        if flag in args:
            i = args.index(flag)
            if flag == "--gib":
                gib = float(args[i + 1])
            else:
                bc.window_ms = float(args[i + 1])
            del args[i:i + 2]
    groups = args or ["ew", "dot", "single"]
    bad = []
    if "ew" in groups:
        bad += [f"ew {t}" for t in br.TYPES + br.BITS_TYPES if not run_ew_type(t, gib)]
    if "dot" in groups:
        bad += [f"dot_prod_{t} n={n}" for t in br.TYPES for n in (64, 1024) if not run_dot(t, n, gib)]
    if "single" in groups and not run_single():
        bad += ["single: device and host results differ"]
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
