#!/usr/bin/env python3
"""Throughput of the complex math functions and the max / min searches on one GPU
(arm_cmplx_{mag,mag_squared,conj,mult_cmplx,mult_real,dot_prod}_*_batch, arm_{max,min}_*_batch).

    python tools/bench_cmplx.py [ew|dot|search|single ...] [--gib G] [--window MS]

Every workload moves about G GiB (default 1) of algorithmic traffic per call: words read and written once
(mag / mag_squared 2 + 1 words per sample, conj 2 + 2, mult_cmplx 4 + 2, mult_real 3 + 2; the dot products read
4 words per sample, max / min one word per element).  Each line reports items/s, the fraction of the 8 TB/s HBM
peak the algorithmic bytes reach, the repeat spread, and the yardsticks timed in the same process on the same
tensors with HIP events after a clock-settle phase:

  ew      items of 1024 samples.  arm_mat_add_f32_batch at G GiB (the project's own streaming kernel, measured
          once per run), and for f32 the torch equivalent: torch.abs of a complex view, conj().resolve_conj(), complex
          mul, complex times real mul.
  dot     item lengths 64, 1024 and 2^20 with one B per item; f32 against torch.linalg.vecdot on complex views.
  search  item lengths 64, 1024 and 2^20 against torch.max / torch.min(dim=-1).
  single  arm_cmplx_dot_prod_f32_batch with batch 1 (the shape of the drop-in on one vector): ns per sample.

The first and last item are checked bit for bit against tests/cmplx_math_ref.py first (the f32 dot product only
up to 1024 samples: its restatement is a Python loop)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import cmsisdsp_amd as dsp  # noqa: E402
import cmplx_math_ref as cm  # noqa: E402

REPEATS = 3
HBM_TBPS = 8.0
TDT = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16, "q7": torch.int8}
ODT = {"f32": torch.float32, "q31": torch.int64, "q15": torch.int32}
EW_WORDS = {"mag": (2, 0, 1), "mag_squared": (2, 0, 1), "conj": (2, 0, 2), "mult_cmplx": (2, 2, 2),
            "mult_real": (2, 1, 2)}
LENGTHS = (64, 1024, 2 ** 20)
window_ms = 500.0


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


def measure(f):
    settle(f)
    steps = max(3, min(400, int(np.ceil(window_ms / max(timed(f, 3), 1e-3)))))
    return [timed(f, steps) for _ in range(REPEATS)], steps


def rnd(t, gen, *shape):
    if t == "f32":
        return torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
    info = torch.iinfo(TDT[t])
    return torch.randint(info.min, info.max + 1, shape, generator=gen, device="cuda", dtype=TDT[t])


def emit(name, t, n, batch, ok, ms, steps, nbytes, extra):
    best = min(ms)
    line = {"workload": f"{name}_{t}", "n": n, "batch": batch, "bitexact_first_last": ok,
            "value": round(batch / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
            "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": HBM_TBPS,
                         "frac": round(nbytes / (best * 1e-3) / (HBM_TBPS * 1e12), 4)},
            "ms": [round(x, 4) for x in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps}
    line.update(extra)
    line["version"] = dsp.version()
    print(json.dumps(line), flush=True)


def yardstick(line, key, name, f, best):
    ms, steps = measure(f)
    line[key] = {"workload": name, "ms": [round(x, 4) for x in ms], "steps": steps}
    line["ratio_to_" + key] = round(min(ms) / best, 3)


_mat_add = None


def mat_add_yardstick(gib):
    """The project's own streaming kernel, arm_mat_add_f32_batch, at G GiB (three f32 streams), measured once."""
    global _mat_add
    if _mat_add is None:
        k = max(1, int(gib * 2 ** 30 / (12 * 1024)))
        x, y, z = (torch.zeros((k, 32, 32), dtype=torch.float32, device="cuda") for _ in range(3))
        ms, steps = measure(lambda: dsp.mat_add_batch(x, y, z))
        nbytes = 12 * 1024 * k
        _mat_add = {"workload": "arm_mat_add_f32_batch, same process", "ms": [round(v, 4) for v in ms],
                    "frac": round(nbytes / (min(ms) * 1e-3) / (HBM_TBPS * 1e12), 4), "steps": steps}
    return _mat_add


def run_ew(op, t, gib, n=1024):
    wa, wb, wd = EW_WORDS[op]
    size = torch.empty(0, dtype=TDT[t]).element_size()
    batch = max(1, int(gib * 2 ** 30 / (size * n * (wa + wb + wd))))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = rnd(t, gen, batch, 2 * n)
    b = rnd(t, gen, batch, wb * n) if wb else None
    dst = torch.zeros((batch, wd * n), dtype=TDT[t], device="cuda")
    fn = getattr(dsp, f"cmplx_{op}_batch")
    ours = (lambda: fn(a, b, dst)) if wb else (lambda: fn(a, dst))
    ours()
    torch.cuda.synchronize()
    key = "r" if op == "mult_real" else "b"
    def want(i):
        g = {"a": a[i].cpu().numpy(), **({key: b[i].cpu().numpy()} if wb else {})}
        return cm.run(f"cmplx_{op}_{t}", g)["dst"]

    ok = all(dst[i].cpu().numpy().tobytes() == want(i).tobytes() for i in (0, batch - 1))
    ms, steps = measure(ours)
    best, nbytes = min(ms), size * n * (wa + wb + wd) * batch
    extra = {}
    if t == "f32":
        za = torch.view_as_complex(a.view(batch, n, 2))
        if op == "mag":
            out = torch.empty((batch, n), dtype=torch.float32, device="cuda")
            yardstick(extra, "yardstick", "torch.abs of a complex view", lambda: torch.abs(za, out=out), best)
        elif op == "conj":
            yardstick(extra, "yardstick", "x.conj().resolve_conj()", lambda: za.conj().resolve_conj(), best)
        elif op == "mult_cmplx":
            zb, out = torch.view_as_complex(b.view(batch, n, 2)), torch.empty_like(za)
            yardstick(extra, "yardstick", "torch.mul (complex)", lambda: torch.mul(za, zb, out=out), best)
        elif op == "mult_real":
            out = torch.empty_like(za)
            yardstick(extra, "yardstick", "torch.mul (complex by real)", lambda: torch.mul(za, b, out=out), best)
        del za
    extra["mat_add"] = mat_add_yardstick(gib)
    emit(f"cmplx_{op}", t, n, batch, ok, ms, steps, nbytes, extra)
    return ok


def run_dot(t, n, gib):
    size = torch.empty(0, dtype=TDT[t]).element_size()
    batch = max(1, int(gib * 2 ** 30 / (size * 4 * n)))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a, b = rnd(t, gen, batch, 2 * n), rnd(t, gen, batch, 2 * n)
    re, im = (torch.zeros(batch, dtype=ODT[t], device="cuda") for _ in range(2))
    ours = lambda: dsp.cmplx_dot_prod_batch(a, b, re, im)                           # noqa: E731
    ours()
    torch.cuda.synchronize()
    ok = None
    if t != "f32" or n <= 1024:
        ok = True
        for i in (0, batch - 1):
            w = cm.run(f"cmplx_dot_prod_{t}", {"a": a[i].cpu().numpy(), "b": b[i].cpu().numpy()})
            ok = ok and re[i].cpu().numpy().tobytes() == w["re"].tobytes()
            ok = ok and im[i].cpu().numpy().tobytes() == w["im"].tobytes()
    ms, steps = measure(ours)
    best, nbytes = min(ms), size * 4 * n * batch
    extra = {"ns_per_sample": round(best * 1e6 / (n * batch), 6)}
    if t == "f32":
        za, zb = torch.view_as_complex(a.view(batch, n, 2)), torch.view_as_complex(b.view(batch, n, 2))
        yardstick(extra, "yardstick", "torch.linalg.vecdot (complex)", lambda: torch.linalg.vecdot(za, zb), best)
    emit("cmplx_dot_prod", t, n, batch, ok, ms, steps, nbytes, extra)
    return ok is not False


def run_search(op, t, n, gib):
    size = torch.empty(0, dtype=TDT[t]).element_size()
    batch = max(1, int(gib * 2 ** 30 / (size * n)))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = rnd(t, gen, batch, n)
    val = torch.zeros(batch, dtype=TDT[t], device="cuda")
    idx = torch.zeros(batch, dtype=torch.int32, device="cuda")
    fn = dsp.max_batch if op == "max" else dsp.min_batch
    ours = lambda: fn(a, val, idx)                                                  # noqa: E731
    ours()
    torch.cuda.synchronize()
    ok = True
    for i in (0, batch - 1):
        wv, wi = cm.extreme(op, a[i].cpu().numpy())
        ok = ok and val[i].cpu().numpy().tobytes() == wv.tobytes() and int(idx[i]) == int(wi)
    ms, steps = measure(ours)
    best, nbytes = min(ms), size * n * batch
    extra = {}
    tf = torch.max if op == "max" else torch.min
    yardstick(extra, "yardstick", f"torch.{op}(dim=-1)", lambda: tf(a, dim=-1), best)
    emit(op, t, n, batch, ok, ms, steps, nbytes, extra)
    return ok


def run_single(n=2 ** 20):
    gen = torch.Generator(device="cuda").manual_seed(1)
    a, b = rnd("f32", gen, 1, 2 * n), rnd("f32", gen, 1, 2 * n)
    re, im = (torch.zeros(1, dtype=torch.float32, device="cuda") for _ in range(2))
    ours = lambda: dsp.cmplx_dot_prod_batch(a, b, re, im)                           # noqa: E731
    ms, steps = measure(ours)
    best = min(ms)
    line = {"workload": "cmplx_dot_prod_f32 single vector", "n": n, "batch": 1,
            "value": round(best * 1e6 / n, 4), "unit": "ns/sample", "ms": [round(x, 4) for x in ms],
            "spread": round((max(ms) - best) / best, 4), "steps": steps, "version": dsp.version()}
    print(json.dumps(line), flush=True)
    return True


def main():
    global window_ms
    args = sys.argv[1:]
    gib = 1.0
    for flag in ("--gib", "--window"):
        if flag in args:
            i = args.index(flag)
            if flag == "--gib":
                gib = float(args[i + 1])
            else:
                window_ms = float(args[i + 1])
            del args[i:i + 2]
    groups = args or ["ew", "dot", "search", "single"]
    bad = []
    if "ew" in groups:
        bad += [f"{op}_{t}" for op in EW_WORDS for t in ("f32", "q31", "q15") if not run_ew(op, t, gib)]
    if "dot" in groups:
        bad += [f"dot_prod_{t} n={n}" for t in ("f32", "q31", "q15") for n in LENGTHS if not run_dot(t, n, gib)]
    if "search" in groups:
        bad += [f"{op}_{t} n={n}" for op, t in (("max", "f32"), ("max", "q31"), ("max", "q15"), ("max", "q7"),
                                                  ("min", "f32")) for n in LENGTHS if not run_search(op, t, n, gib)]
    if "single" in groups:
        run_single()
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
