#!/usr/bin/env python3
"""Throughput of the distance functions on one GPU.

    python tools/bench_distance.py [f32|bool|dtw ...] [--gib G] [--window MS]

Timing is tools/bench_cmplx.py's: a clock-settle phase, then REPEATS windows of about --window ms between HIP events;
a line reports the best window, the repeat spread and the fraction of the 8 TB/s HBM peak its algorithmic bytes reach.

  f32   the eight f32 distances at item lengths 64 and 1024, G GiB (default 1) of source words per call, each next to
        arm_dot_prod_f32_batch (one ordered chain over the same two streams) on the same tensors in the same run;
        euclidean with bStride 0 (one query against the bank); one vector of 2^20 words through the euclidean drop-in
        on device pointers.
  bool  the nine boolean distances at 2048 and 32768 booleans per item, next to arm_dot_prod_q31_batch on the same
        words reinterpreted.
  dtw   arm_dtw_distance_f32_batch at 64 x 64 and 256 x 256, without a window and under a Sakoe-Chiba window of a
        tenth of the length, in G cells/s and as a fraction of the HBM bound of 9 bytes per cell (4 read, 4 written,
        1 of window); the cell count is the whole matrix in both cases.
  dtw_ref [--ref DIR]   (alone, no GPU) the reference's scalar arm_dtw_distance_f32 on one CPU thread, same shapes.

The first and last item of every result are checked bit for bit against tests/distance_ref.py first."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_cmplx as bc  # noqa: E402
import cmsisdsp_amd as dsp  # noqa: E402
import distance_ref as dr  # noqa: E402

HBM_TBPS = bc.HBM_TBPS


def frac(nbytes, ms):
    return nbytes / (ms * 1e-3) / (HBM_TBPS * 1e12)


def emit(workload, n, batch, ok, ms, steps, nbytes, **extra):
    best = min(ms)
    line = {"workload": workload, "n": n, "batch": batch, "bitexact_first_last": ok,
            "value": round(batch / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
            "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps,
            "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": HBM_TBPS, "frac": round(frac(nbytes, best), 4)}}
    line.update(extra)
    return line


def out(line):
    line["version"] = dsp.version()
    print(json.dumps(line), flush=True)


def f32_want(func, a, b):
    v = dr.distance_f32(func, a.cpu().numpy(), b.cpu().numpy())
    return v[0] if func == "correlation" else v


def run_f32(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(17)
    for n in (64, 1024):
        batch = max(1, int(gib * 2 ** 30 / (8 * n)))
        a = torch.rand((batch, n), generator=gen, device="cuda", dtype=torch.float32) + 0.01    # positive: jensenshannon
        b = torch.rand((batch, n), generator=gen, device="cuda", dtype=torch.float32) + 0.01
        res = torch.zeros(batch, dtype=torch.float32, device="cuda")
        yname, yf = "arm_dot_prod_f32_batch, same tensors", lambda: dsp.dot_prod_batch(a, b, res)   # noqa: E731
        for func in dr.F32_FUNCS:
            ours = lambda: dsp.distance_batch(func, a, b, res)                      # noqa: E731
            ours()
            torch.cuda.synchronize()
            ok = all(dr.same_word(res[i].item(), f32_want(func, a[i], b[i])) for i in (0, batch - 1))
            ok_all = ok_all and ok
            ms, steps = bc.measure(ours)
            line = emit(f"{func}_distance_f32", n, batch, ok, ms, steps, 8 * n * batch)
            bc.yardstick(line, "yardstick", yname, yf, min(ms))
            out(line)
        ours = lambda: dsp.distance_batch("euclidean", a, b[0], res)                # noqa: E731
        ours()
        torch.cuda.synchronize()
        ok = all(dr.same_word(res[i].item(), f32_want("euclidean", a[i], b[0])) for i in (0, batch - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = emit("euclidean_distance_f32, bStride 0", n, batch, ok, ms, steps, 4 * n * batch)
        bc.yardstick(line, "yardstick", yname, yf, min(ms))
        out(line)
        del a, b
    n = 2 ** 20
    a = torch.rand((1, n), generator=gen, device="cuda", dtype=torch.float32)
    b = torch.rand((1, n), generator=gen, device="cuda", dtype=torch.float32)
    fn = dsp.lib.arm_euclidean_distance_f32
    got = np.float32(fn(a.data_ptr(), b.data_ptr(), n))
    ok = dr.same_word(got, f32_want("euclidean", a[0], b[0]))
    ms, steps = bc.measure(lambda: fn(a.data_ptr(), b.data_ptr(), n))
    out(emit("euclidean_distance_f32, drop-in on device pointers (synchronous)", n, 1, ok, ms, steps, 8 * n))
    return ok_all and ok


def run_bool(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(19)
    for n in (2048, 32768):
        w = n // 32
        batch = max(1, int(gib * 2 ** 30 / (8 * w)))
        a = torch.randint(-2 ** 31, 2 ** 31, (batch, w), generator=gen, device="cuda", dtype=torch.int32)
        b = torch.randint(-2 ** 31, 2 ** 31, (batch, w), generator=gen, device="cuda", dtype=torch.int32)
        res = torch.zeros(batch, dtype=torch.float32, device="cuda")
        res64 = torch.zeros(batch, dtype=torch.int64, device="cuda")
        yname, yf = "arm_dot_prod_q31_batch, same words", lambda: dsp.dot_prod_batch(a, b, res64)   # noqa: E731
        for func in dr.BOOL_FUNCS:
            ours = lambda: dsp.boolean_distance_batch(func, a, b, n, res)           # noqa: E731
            ours()
            torch.cuda.synchronize()
            ok = all(dr.same_word(res[i].item(), dr.boolean_distance(func, a[i].cpu().numpy().view(np.uint32),
                                                                     b[i].cpu().numpy().view(np.uint32), n))
                     for i in (0, batch - 1))
            ok_all = ok_all and ok
            ms, steps = bc.measure(ours)
            line = emit(f"{func}_distance", n, batch, ok, ms, steps, 8 * w * batch)
            bc.yardstick(line, "yardstick", yname, yf, min(ms))
            out(line)
        del a, b
    return ok_all


def run_dtw(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(23)
    for n in (64, 256):
        batch = max(1, int(gib * 2 ** 30 / (4 * n * n)))
        d = torch.rand((batch, n, n), generator=gen, device="cuda", dtype=torch.float32)
        cost = torch.zeros_like(d)
        res = torch.zeros(batch, dtype=torch.float32, device="cuda")
        status = torch.zeros(batch, dtype=torch.int32, device="cuda")
        window = torch.zeros((n, n), dtype=torch.int8, device="cuda")
        dsp.dtw_init_window_batch(dsp.ARM_DTW_SAKOE_CHIBA_WINDOW, n // 10, window.view(1, n, n))
        for name, w in (("no window", None), (f"Sakoe-Chiba {n // 10}", window)):
            ours = lambda: dsp.dtw_distance_batch(d, w, cost, res, status)          # noqa: E731
            ours()
            torch.cuda.synchronize()
            ok = True
            for i in (0, batch - 1):
                st, want, wcost = dr.dtw_distance(d[i].cpu().numpy(), None if w is None else w.cpu().numpy())
                ok = ok and st == int(status[i]) == 0 and dr.same_word(res[i].item(), want) and \
                    cost[i].cpu().numpy().tobytes() == wcost.tobytes()
            ok_all = ok_all and ok
            ms, steps = bc.measure(ours)
            cells = n * n * batch
            out(emit(f"dtw_distance_f32 {n}x{n}, {name}", n * n, batch, ok, ms, steps, 9 * cells,
                     Gcells_per_s=round(cells / (min(ms) * 1e-3) * 1e-9, 3)))
        del d, cost
    return ok_all


def run_dtw_ref(ref):
    """The reference's arm_dtw_distance_f32 (scalar build, oracle/ref.mk's flags) on one CPU thread, the same shapes
    and windows; needs the reference tree, no GPU."""
    import ctypes as C
    import subprocess
    import tempfile
    import time
    from cmsisdsp_amd import _abi
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libdtw_ref.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w",
                        "-shared", "-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude"),
                        os.path.join(ref, "Source", "DistanceFunctions", "arm_dtw_distance_f32.c"), "-o", so],
                       check=True)
        lib = C.CDLL(so)
        lib.arm_dtw_distance_f32.restype, lib.arm_dtw_distance_f32.argtypes = _abi.DISTANCE["arm_dtw_distance_f32"]
        rng = np.random.default_rng(23)
        for n in (64, 256):
            d = rng.uniform(0, 1, (n, n)).astype(np.float32)
            cost, value = np.zeros_like(d), np.zeros(1, np.float32)
            win = dr.init_window(dr.SAKOE_CHIBA, n // 10, n, n)
            dm = _abi.arm_matrix_instance_f32(n, n, C.cast(d.ctypes.data, _abi.c_f32p))
            cm = _abi.arm_matrix_instance_f32(n, n, C.cast(cost.ctypes.data, _abi.c_f32p))
            wm = _abi.arm_matrix_instance_q7(n, n, C.cast(win.ctypes.data, _abi.MAT_PTR["q7"]))
            for name, w in (("no window", None), (f"Sakoe-Chiba {n // 10}", C.byref(wm))):
                reps = max(20, 2 ** 22 // (n * n))
                best = 1e9
                for _ in range(5):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        lib.arm_dtw_distance_f32(C.byref(dm), w, C.byref(cm), value.ctypes.data)
                    best = min(best, (time.perf_counter() - t0) / reps)
                print(json.dumps({"workload": f"reference arm_dtw_distance_f32 {n}x{n}, {name}, one CPU thread",
                                  "us_per_matrix": round(best * 1e6, 2),
                                  "Gcells_per_s": round(n * n / best * 1e-9, 4)}), flush=True)
    return True


def main():
    args = sys.argv[1:]
    gib = 1.0
    if "dtw_ref" in args:
        i = args.index("--ref") if "--ref" in args else -1
        import re
        mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()                   # the default tree of oracle/ref.mk
        return run_dtw_ref(args[i + 1] if i >= 0 else re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    for flag in ("--gib", "--window"):
        if flag in args:
            i = args.index(flag)
            if flag == "--gib":
                gib = float(args[i + 1])
            else:
                bc.window_ms = float(args[i + 1])
            del args[i:i + 2]
    groups = args or ["f32", "bool", "dtw"]
    bad = []
    for name, fn in (("f32", run_f32), ("bool", run_bool), ("dtw", run_dtw)):
        if name in groups and not fn(gib):
            bad.append(name)
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
