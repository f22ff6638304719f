#!/usr/bin/env python3
"""Throughput of the statistics functions on one GPU (arm_{mean,power,rms,var,std,mse}_*_batch,
arm_accumulate_f32_batch, arm_absmax_*_batch, arm_max_no_idx_*_batch).

    python tools/bench_stats.py [int|f32|single ...] [--gib G] [--window MS]

Every workload reads about G GiB (default 1) of source words per call (mse: over its two sources), at item lengths
64, 1024 and 2^20.  Timing as tools/bench_cmplx.py: HIP events after a clock-settle phase, the best of three
windows, the repeat spread on every line.  The first and last item are checked bit for bit against
tests/statistics_ref.py before timing.  The yardsticks run in the same process on the same tensor:

  int     the integer sums and the new searches against arm_max_<type>_batch at the same length: the same bytes
          through the same lanes-per-item mapping ("ratio_to_max": our time over its time; mse reads two sources, so
          its ratio is taken per byte).
  f32     the ordered chains against arm_cmplx_dot_prod_f32_batch at the same number of samples per item (it reads
          four words per sample and chains two dependent adds; "items_vs_dot": our items/s over its items/s), and var
          / std against mean ("time_vs_mean").
  single  one 2^20-word vector through the drop-ins on a device pointer: ns per sample."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_cmplx as bc  # noqa: E402  (settle / timed / measure / rnd / emit; puts the package and tests/ on the path)
import torch  # noqa: E402

import cmsisdsp_amd as dsp  # noqa: E402
import statistics_ref as sr  # noqa: E402

LENGTHS = (64, 1024, 2 ** 20)
RDT = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16, "q7": torch.int8, "q63": torch.int64}
INT_OPS = {"q31": ("mean", "power", "rms", "var", "std", "mse", "absmax", "max_no_idx"),
           "q15": ("mean", "power", "rms", "var", "std", "mse", "absmax", "max_no_idx"),
           "q7": ("mean", "power", "mse", "absmax", "max_no_idx")}
F32_OPS = ("mean", "accumulate", "power", "rms", "mse", "var", "std", "absmax", "max_no_idx")


def operands(func, t, n, gib):
    """Sources of about gib GiB in all, inside the reference's contract (q31 var / std at amplitude 2^-4, var / std_q15
    at 2^20 words at 2^-2, as the fixtures)."""
    two = sr.two_sources(func)
    size = torch.empty(0, dtype=RDT[t]).element_size()
    batch = max(1, int(gib * 2 ** 30 / (size * n * (2 if two else 1))))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = bc.rnd(t, gen, batch, n)
    b = bc.rnd(t, gen, batch, n) if two else None
    sh = sr.amp_shift(func, n)
    if t == "q7" and n > 2 ** 16:
        sh = 2                                              # the 32-bit sums of squares of power_q7 / mse_q7
    if sh:
        a >>= sh
    return a, b, batch, size * n * batch * (2 if two else 1)


def launcher(func, a, b):
    op, t = sr.split(func)
    batch = a.shape[0]
    res = torch.zeros(batch, dtype=RDT[sr.result_type(func)], device="cuda")
    fn = getattr(dsp, op + "_batch")
    if sr.has_index(func):
        idx = torch.zeros(batch, dtype=torch.int32, device="cuda")
        return (lambda: fn(a, res, idx)), res
    if b is not None:
        return (lambda: fn(a, b, res)), res
    return (lambda: fn(a, res)), res


def bitexact(func, a, b, res, n):
    """First and last item against the restatement (the f32 chains only up to 1024 words: a Python loop)."""
    if func.endswith("f32") and n > 1024 and sr.split(func)[0] in sr.SUM_OPS:
        return None
    ok = True
    for i in (0, a.shape[0] - 1):
        want = sr.run(func, a[i].cpu().numpy(), b[i].cpu().numpy() if b is not None else None)["value"]
        ok = ok and sr.same_words(res[i].cpu().numpy().reshape(()), np.asarray(want).reshape(()), sr.nan_rule(func))
    return bool(ok)


_yard = {}


def max_yardstick(t, n, a):
    """arm_max_<t>_batch on the same tensor, once per (type, length)."""
    if (t, n) not in _yard:
        val = torch.zeros(a.shape[0], dtype=RDT[t], device="cuda")
        idx = torch.zeros(a.shape[0], dtype=torch.int32, device="cuda")
        ms, steps = bc.measure(lambda: dsp.max_batch(a, val, idx))
        _yard[(t, n)] = {"workload": f"arm_max_{t}_batch, same tensor", "ms": [round(x, 4) for x in ms], "steps": steps,
                         "ms_per_byte": min(ms) / (a.numel() * a.element_size())}
    return _yard[(t, n)]


def dot_yardstick(n, gib):
    """arm_cmplx_dot_prod_f32_batch with n samples per item and as many items as a one-source f32 workload has."""
    if ("dot", n) not in _yard:
        batch = max(1, int(gib * 2 ** 30 / (4 * n)))
        gen = torch.Generator(device="cuda").manual_seed(n + 1)
        a, b = bc.rnd("f32", gen, batch, 2 * n), bc.rnd("f32", gen, batch, 2 * n)
        re, im = (torch.zeros(batch, dtype=torch.float32, device="cuda") for _ in range(2))
        ms, steps = bc.measure(lambda: dsp.cmplx_dot_prod_batch(a, b, re, im))
        _yard[("dot", n)] = {"workload": "arm_cmplx_dot_prod_f32_batch, same samples per item", "batch": batch,
                             "ms": [round(x, 4) for x in ms], "steps": steps,
                             "items_per_s": batch / (min(ms) * 1e-3)}
    return _yard[("dot", n)]


def run(func, n, gib, means):
    op, t = sr.split(func)
    a, b, batch, nbytes = operands(func, t, n, gib)
    ours, res = launcher(func, a, b)
    ours()
    torch.cuda.synchronize()
    ok = bitexact(func, a, b, res, n)
    ms, steps = bc.measure(ours)
    best = min(ms)
    extra = {"ns_per_sample": round(best * 1e6 / (n * batch), 6)}
    if t != "f32" or op not in sr.SUM_OPS:
        y = max_yardstick(t, n, a)
        extra["yardstick"] = {k: v for k, v in y.items() if k != "ms_per_byte"}
        extra["ratio_to_max"] = round((best / nbytes) / y["ms_per_byte"], 3)
    else:
        y = dot_yardstick(n, gib)
        extra["yardstick"] = {k: v for k, v in y.items() if k != "items_per_s"}
        extra["items_vs_dot"] = round(batch / (best * 1e-3) / y["items_per_s"], 3)
        if op == "mean":
            means[n] = best
        if op in ("var", "std") and n in means:
            extra["time_vs_mean"] = round(best / means[n], 3)
    bc.emit(op, t, n, batch, ok, ms, steps, nbytes, extra)
    return ok is not False


def run_single(n=2 ** 20):
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = bc.rnd("f32", gen, n)
    for op in ("mean", "rms", "var"):
        res = torch.zeros(1, dtype=torch.float32, device="cuda")
        fn = getattr(dsp.lib, f"arm_{op}_f32")
        ms, steps = bc.measure(lambda: fn(a.data_ptr(), n, res.data_ptr()))
        best = min(ms)
        line = {"workload": f"arm_{op}_f32 drop-in, one device vector", "n": n, "batch": 1,
                "value": round(best * 1e6 / n, 4), "unit": "ns/sample", "ms": [round(x, 4) for x in ms],
                "spread": round((max(ms) - best) / best, 4), "steps": steps, "version": dsp.version()}
        print(json.dumps(line), flush=True)


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
    groups = args or ["int", "f32", "single"]
    bad, means = [], {}
    if "int" in groups:
        for t, ops in INT_OPS.items():
            for n in LENGTHS:
                bad += [f"{op}_{t} n={n}" for op in ops if not run(f"{op}_{t}", n, gib, means)]
                _yard.clear()
    if "f32" in groups:
        for n in LENGTHS:
            bad += [f"{op}_f32 n={n}" for op in F32_OPS if not run(f"{op}_f32", n, gib, means)]
            _yard.clear()
    if "single" in groups:
        run_single()
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
