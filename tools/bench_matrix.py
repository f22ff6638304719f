#!/usr/bin/env python3
"""Throughput of the complex matrix multiplies, arm_mat_cmplx_mult_{f32,q31,q15}_batch, on one GPU.

Workload: complex 512 x 512 x 512, batch 64.  Yardstick: the real product of the same type at the embedded
shape (512 x 1024 x 1024, batch 64), which issues the same MFMA work and reads twice the B bytes.  Both are
timed in the same process with HIP events on the launch stream after a clock-settle phase, alternating,
REPEATS times each over a window of at least a second, so the repeat spread of each is visible next to their
ratio.  Rows 0..15 of item 0 are checked bit for bit against the CPU checker first (q15 / q31:
tests/cmplx_mat_ref.py; f32: the stated fmaf chain, oracle.mat_mult_fmaf on the embedded operands).
Operations are counted as 8 M N K per complex product (4 multiplies and 4 adds per complex MAC).
Usage: python tools/bench_matrix.py [f32|q31|q15 ...]  -> one JSON line per workload.

Inverse, Cholesky, LDLT and triangular solves (arm_mat_{inverse,cholesky,ldlt,solve_*_triangular}_f32_batch):
    python tools/bench_matrix.py [inverse|cholesky|ldlt|solve_lower|solve_upper ...] [--gib G]
n in 4, 8, 16, 32, 64, the batch sized so that the algorithmic traffic is about G GiB (default 1): words read
and written once, inverse n^2 + 2 n^2, Cholesky n^2 + n (n + 1) / 2, LDLT n^2 + 2 n^2 (+ n / 2 for pp), solves
(4 right-hand sides) n^2 + 4 n + 4 n.  Each line reports matrices/s, flop/s (inverse 3 n^3: 2 n^3 on dst and n^3
on the shrinking src; Cholesky n^3 / 3; LDLT n^3, three operations per word of the trailing square; solves
n^2 cols) and the fraction of 8 TB/s the algorithmic bytes reach.  Yardstick, on the same tensors in the same
process: torch.linalg.inv, torch.linalg.cholesky, torch.linalg.solve_triangular (LDLT has none that pivots on
the diagonal and is listed alone).  The first and last item are checked bit for bit against
tests/mat_solve_ref.py first.

Element-wise add / sub / scale, the transposes and matrix x vector (arm_mat_{add,sub,scale,trans,cmplx_trans,
vec_mult}_*_batch), each workload with a type argument after a colon (none: every type it has):
    python tools/bench_matrix.py [add|sub|scale|trans|cmplx_trans|vec_mult][:f32|:q31|:q15|:q7] ... [--gib G]
n x n items, n in 4, 16, 64, 1024, the batch sized for about G GiB (default 1) of algorithmic traffic: elements
read and written once (add / sub 3 n^2, scale and the transposes 2 n^2, a complex element two words; vec_mult
n^2 + 2 n with one matrix per item).  Each line reports items/s and the fraction of 8 TB/s the algorithmic bytes
reach, the same operation in torch on the same tensors in the same process (torch.add / sub / mul,
transpose(1, 2).contiguous(), torch.bmm for the f32 vec_mult; the integer matrix-vector products have none) and,
for the element-wise and transpose workloads, a torch copy of the same byte count (half read, half written).  The
first and last item are checked bit for bit against tests/mat_basic_ref.py first."""
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


HBM_TBPS = 8.0
SOLVE_SIZES = (4, 8, 16, 32, 64)
SOLVE_COLS = 4
SOLVE_WINDOW_MS = 300.0


def solve_counts(func, n):
    """(words moved, flops) per item."""
    if func == "inverse":
        return 3 * n * n, 3.0 * n ** 3
    if func == "cholesky":
        return n * n + n * (n + 1) // 2, n ** 3 / 3.0
    if func == "ldlt":
        return 3 * n * n + (n + 1) // 2, 1.0 * n ** 3
    return n * n + 2 * n * SOLVE_COLS, 1.0 * n * n * SOLVE_COLS


def run_solve(func, n, gib):
    import mat_solve_ref as mr
    words, flops = solve_counts(func, n)
    batch = max(1, int(gib * 2 ** 30 / (4 * words)))
    gen = torch.Generator(device="cuda").manual_seed(n)
    rnd = lambda *shape: torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1   # noqa: E731
    status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    if func == "inverse":
        src = rnd(batch, n, n)
        work, dst = torch.empty_like(src), torch.empty_like(src)

        def ours():                          # the call destroys its source: the copy is part of neither count
            dsp.mat_inverse_batch(work, dst, status=status)

        def prep():
            work.copy_(src)

        def yard():
            return torch.linalg.inv(src)
        operands, outs = {"src": src}, lambda i: {"dst": dst[i], "src_after": work[i]}   # noqa: E731
    elif func in ("cholesky", "ldlt"):
        b = rnd(batch, n, n + 3)
        src = torch.bmm(b, b.transpose(1, 2)).contiguous()
        del b
        dst = torch.zeros_like(src)
        if func == "cholesky":
            def ours():
                dsp.mat_cholesky_batch(src, dst, status=status)

            def yard():
                return torch.linalg.cholesky(src)
            outs = lambda i: {"dst": dst[i]}                                             # noqa: E731
        else:
            dd, pp = torch.zeros_like(src), torch.zeros((batch, n), dtype=torch.int16, device="cuda")

            def ours():
                dsp.mat_ldlt_batch(src, dst, dd, pp)
            yard = None
            outs = lambda i: {"l": dst[i], "d": dd[i], "pp": pp[i]}                      # noqa: E731
        prep, operands = None, {"src": src}
    else:
        lower = func == "solve_lower"
        t = rnd(batch, n, n)
        t = (torch.tril(t, -1) if lower else torch.triu(t, 1)) + torch.diag_embed(1 + rnd(batch, n).abs())
        a, dst = rnd(batch, n, SOLVE_COLS), torch.zeros((batch, n, SOLVE_COLS), device="cuda")

        def ours():
            dsp.mat_solve_triangular_batch(t, a, dst, lower=lower, status=status)

        def yard():
            return torch.linalg.solve_triangular(t, a, upper=not lower)
        prep, operands, outs = None, {"t": t, "a": a}, lambda i: {"dst": dst[i]}         # noqa: E731

    if prep:
        prep()
    ours()
    torch.cuda.synchronize()
    ok = not bool(status.any())
    for i in (0, batch - 1):
        want = mr.run(func, {k: v[i].cpu().numpy() for k, v in operands.items()})
        for k, v in outs(i).items():
            got, exp = v.cpu().numpy(), want[k]
            if func == "cholesky":           # the strict upper triangle is not written
                got, exp = np.tril(got), np.tril(exp)
            ok = ok and mr.same_words(got.view(np.uint16) if k == "pp" else got, exp)

    def timed_ours(steps):
        # the inverse restores its source before every call, outside the timed interval
        if not prep:
            return timed(ours, steps)
        st = torch.cuda.current_stream()
        total = 0.0
        for _ in range(steps):
            prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ours()
            e1.record(st)
            e1.synchronize()
            total += e0.elapsed_time(e1)
        return total / steps

    settle(ours if not prep else lambda: (prep(), ours()))
    steps = max(3, min(200, int(np.ceil(SOLVE_WINDOW_MS / max(timed_ours(3), 1e-3)))))
    ms = [timed_ours(steps) for _ in range(REPEATS)]
    best = min(ms)
    line = {"workload": f"mat_{func}_f32", "n": n, "batch": batch, "bitexact_first_last": ok,
            "value": round(batch / (best * 1e-3) * 1e-6, 3), "unit": "M matrices/s",
            "gflops": round(flops * batch / (best * 1e-3) * 1e-9, 1),
            "roofline": {"bound": "hbm", "bytes": 4 * words * batch, "peak_TBps": HBM_TBPS,
                         "frac": round(4.0 * words * batch / (best * 1e-3) / (HBM_TBPS * 1e12), 4)},
            "ms": [round(x, 4) for x in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps,
            "version": dsp.version()}
    if func in ("solve_lower", "solve_upper"):
        line["cols"] = SOLVE_COLS
    if yard:
        try:
            ysteps = max(1, min(50, int(np.ceil(SOLVE_WINDOW_MS / max(timed(yard, 1, warmup=1), 1e-3)))))
            yms = [timed(yard, ysteps, warmup=0) for _ in range(REPEATS)]
            name = {"inverse": "torch.linalg.inv", "cholesky": "torch.linalg.cholesky"}.get(
                func, "torch.linalg.solve_triangular")
            line["yardstick"] = {"workload": name, "ms": [round(x, 4) for x in yms],
                                 "value": round(batch / (min(yms) * 1e-3) * 1e-6, 3), "steps": ysteps}
            line["ratio_to_yardstick"] = round(min(yms) / best, 3)
        except RuntimeError as e:          # e.g. out of memory in the library's workspace
            line["yardstick"] = {"error": str(e).splitlines()[0][:200]}
    print(json.dumps(line), flush=True)
    return ok


BASIC_OPS = {"add": ("f32", "q31", "q15"), "sub": ("f32", "q31", "q15"), "scale": ("f32", "q31", "q15"),
             "trans": ("f32", "q31", "q15", "q7"), "cmplx_trans": ("f32", "q31", "q15"),
             "vec_mult": ("f32", "q31", "q15", "q7")}
BASIC_SIZES = (4, 16, 64, 1024)
BASIC_TDT = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16, "q7": torch.int8}
BASIC_SCALE = {"f32": 0.75, "q31": 0x60000000, "q15": 0x6000}


def run_basic(op, t, n, gib):
    import mat_basic_ref as mb
    size = torch.empty(0, dtype=BASIC_TDT[t]).element_size()
    cw = 2 if op == "cmplx_trans" else 1
    elems = {"add": 3 * n * n, "sub": 3 * n * n, "vec_mult": n * n + 2 * n}.get(op, 2 * n * n * cw)
    batch = max(1, int(gib * 2 ** 30 / (size * elems)))
    gen = torch.Generator(device="cuda").manual_seed(n)

    def rnd(*shape, amp=None):
        if t == "f32":
            return torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
        info = torch.iinfo(BASIC_TDT[t])
        lo, hi = (info.min, info.max + 1) if amp is None else (-amp, amp + 1)
        return torch.randint(lo, hi, shape, generator=gen, device="cuda", dtype=BASIC_TDT[t])

    if op == "vec_mult":
        amp = {"q7": 40 if n <= 64 else 15, "q15": 4000}.get(t)
        a, b = rnd(batch, n, n, amp=amp), rnd(batch, n, amp=amp)
        dst = torch.zeros((batch, n), dtype=BASIC_TDT[t], device="cuda")
        ours = lambda: dsp.mat_vec_mult_batch(a, b, dst)                                 # noqa: E731
        yard, yname = (lambda: torch.bmm(a, b.unsqueeze(2))), "torch.bmm"               # noqa: E731
        if t != "f32":
            yard = None
        want = lambda i: mb.vec_mult(t, a[i].cpu().numpy(), b[i].cpu().numpy())          # noqa: E731
    elif op in ("trans", "cmplx_trans"):
        a = rnd(batch, n, n * cw)
        dst = torch.zeros_like(a)
        ours = (lambda: dsp.mat_trans_batch(a, dst)) if cw == 1 else (lambda: dsp.mat_cmplx_trans_batch(a, dst))
        yard = (lambda: a.transpose(1, 2).contiguous()) if cw == 1 else \
            (lambda: a.view(batch, n, n, 2).transpose(1, 2).contiguous())
        yname = "transpose(1, 2).contiguous()"
        want = lambda i: (mb.trans if cw == 1 else mb.cmplx_trans)(a[i].cpu().numpy())   # noqa: E731
    else:
        a, b = rnd(batch, n, n), rnd(batch, n, n) if op != "scale" else None
        dst, ydst = torch.zeros_like(a), torch.empty_like(a)
        sc = BASIC_SCALE[t]
        if op == "scale":
            ours = lambda: dsp.mat_scale_batch(a, sc, dst, shift=0)                      # noqa: E731
            yard, yname = (lambda: torch.mul(a, sc if t == "f32" else 3, out=ydst)), "torch.mul"   # noqa: E731
            want = lambda i: mb.scale(t, a[i].cpu().numpy(), sc, 0)                      # noqa: E731
        else:
            ours = (lambda: dsp.mat_add_batch(a, b, dst)) if op == "add" else (lambda: dsp.mat_sub_batch(a, b, dst))
            yard = (lambda: torch.add(a, b, out=ydst)) if op == "add" else (lambda: torch.sub(a, b, out=ydst))
            yname = f"torch.{op}"
            want = lambda i: (mb.add if op == "add" else mb.sub)(t, a[i].cpu().numpy(), b[i].cpu().numpy())  # noqa: E731

    ours()
    torch.cuda.synchronize()
    ok = all(dst[i].cpu().numpy().tobytes() == want(i).tobytes() for i in (0, batch - 1))

    def measure(f):
        settle(f)
        steps = max(3, min(400, int(np.ceil(SOLVE_WINDOW_MS / max(timed(f, 3), 1e-3)))))
        ms = [timed(f, steps) for _ in range(REPEATS)]
        return ms, steps

    ms, steps = measure(ours)
    best = min(ms)
    nbytes = size * elems * batch
    line = {"workload": f"mat_{op}_{t}", "n": n, "batch": batch, "bitexact_first_last": ok,
            "value": round(batch / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
            "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": HBM_TBPS,
                         "frac": round(nbytes / (best * 1e-3) / (HBM_TBPS * 1e12), 4)},
            "ms": [round(x, 4) for x in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps,
            "version": dsp.version()}
    if yard:
        yms, ysteps = measure(yard)
        line["yardstick"] = {"workload": yname, "ms": [round(x, 4) for x in yms], "steps": ysteps}
        line["ratio_to_yardstick"] = round(min(yms) / best, 3)
    if op != "vec_mult":
        half = torch.empty(nbytes // 2, dtype=torch.int8, device="cuda")
        other = torch.empty_like(half)
        cms, csteps = measure(lambda: other.copy_(half))
        line["copy"] = {"workload": "torch copy of the same byte count", "ms": [round(x, 4) for x in cms],
                        "TBps": round(nbytes / (min(cms) * 1e-3) * 1e-12, 3), "steps": csteps}
        line["ratio_to_copy"] = round(min(cms) / best, 3)
    print(json.dumps(line), flush=True)
    return ok


def main():
    args = sys.argv[1:]
    gib = 1.0
    if "--gib" in args:
        i = args.index("--gib")
        gib = float(args[i + 1])
        del args[i:i + 2]
    basics = [k for k in args if k.split(":")[0] in BASIC_OPS]
    if basics:
        bad = []
        for k in basics:
            op, _, t = k.partition(":")
            for ty in ([t] if t else BASIC_OPS[op]):
                if ty not in BASIC_OPS[op]:
                    sys.exit(f"{op} has no {ty} form")
                bad += [f"{op}_{ty} n={n}" for n in BASIC_SIZES if not run_basic(op, ty, n, gib)]
        if bad:
            sys.exit(f"not bit-exact: {bad}")
        args = [k for k in args if k not in basics]
        if not args:
            return
    solves = [k for k in args if k in ("inverse", "cholesky", "ldlt", "solve_lower", "solve_upper")]
    if solves:
        bad = [f"{f} n={n}" for f in solves for n in SOLVE_SIZES if not run_solve(f, n, gib)]
        if bad:
            sys.exit(f"not bit-exact: {bad}")
        args = [k for k in args if k not in solves]
        if not args:
            return
    kinds = args or ["f32", "q31", "q15"]
    bad = [k for k in kinds if not run(k)]
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
