#!/usr/bin/env python3
"""Throughput of the interpolation and quaternion _batch forms on one GPU.

    python tools/bench_interp.py [linear|bilinear|spline|quaternion ...] [--gib G] [--window MS]

Timing is tools/bench_cmplx.py's: a clock-settle phase, then REPEATS windows of about --window ms between HIP events;
a line reports the best window, the repeat spread and the fraction of the 8 TB/s HBM peak its algorithmic bytes reach,
next to arm_mat_add_f32_batch at G GiB (default 1) in the same process.

  linear      the four types against a 4096-entry table (in LDS), f32 also against 2^20 entries (global memory), G GiB
              of samples and results per call; f32 beside a torch gather + lerp.
  bilinear    the four types on a 1024 x 1024 table (fits L2) and, f32, on 16384 x 16384 (1 GiB, larger than L2) at
              uniformly random points; G GiB of coordinates and results per call; f32 beside a torch gather + lerp.
  spline      init and evaluation at 64 and 1024 knots and queries per item, 2^16 and 2^12 items.
  quaternion  the seven _batch forms at G GiB per call; the product beside a torch formulation from element-wise ops.

The first and last words of every result are checked bit for bit against tests/interp_ref.py / quaternion_ref.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import interp_ref as ir  # noqa: E402
import quaternion_ref as qr  # noqa: E402

EDGE = 64                                                    # words checked at either end of a result


def gpu_modules():
    global torch, bc, dsp
    import torch
    import bench_cmplx as bc
    import cmsisdsp_amd as dsp


def emit(workload, n, items, ok, ms, steps, nbytes, gib, **extra):
    best = min(ms)
    line = {"workload": workload, "n": n, "batch": items, "bitexact_first_last": ok,
            "value": round(items / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
            "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps,
            "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": bc.HBM_TBPS,
                         "frac": round(nbytes / (best * 1e-3) / (bc.HBM_TBPS * 1e12), 4)},
            "yardstick": bc.mat_add_yardstick(gib)}
    line.update(extra)
    line["version"] = dsp.version()
    print(json.dumps(line), flush=True)


def ends(t):
    h = t.reshape(-1)
    return np.concatenate([h[:EDGE].cpu().numpy(), h[-EDGE:].cpu().numpy()])


def coords(kind, count, lo, hi, gen):
    """Uniform coordinates over [lo, hi): float32, or 12.20 words."""
    u = torch.rand(count, generator=gen, device="cuda", dtype=torch.float64) * (hi - lo) + lo
    return u.to(torch.float32) if kind == "f32" else (u * (1 << 20)).to(torch.int32)


def run_linear(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(41)
    for kind, n in (("f32", 4096), ("f32", 1 << 20), ("q31", 4096), ("q15", 4096), ("q7", 4096)):
        size = np.dtype(ir.NP[kind]).itemsize
        count = int(gib * 2 ** 30 / (4 + size))
        tab = bc.rnd(kind, gen, n)
        hi = min(n, 2048) if kind != "f32" else n
        x = coords(kind, count, -1.0, hi + 1.0, gen)
        y = torch.zeros(count, dtype=tab.dtype, device="cuda")
        arg = dsp.linear_interp_instance(0.0, 1.0, tab)[0] if kind == "f32" else tab
        ours = lambda: dsp.linear_interp_batch(kind, arg, x, y)                      # noqa: E731
        ours()
        torch.cuda.synchronize()
        h = tab.cpu().numpy()
        want = ir.linear_f32(h, 0.0, 1.0, ends(x)) if kind == "f32" else ir.linear_q(kind, h, ends(x))
        ok = ir.same_word(ends(y), want)
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = {}
        if kind == "f32":
            def lerp():
                i = x.floor().clamp(0, n - 2)
                j = i.long()
                return torch.lerp(tab[j], tab[j + 1], x - i)
            bc.yardstick(line, "torch", "torch gather + lerp, same tensors (not bit-exact)", lerp, min(ms))
        emit(f"linear_interp_{kind}", n, count, ok, ms, steps, (4 + size) * count, gib, **line)
    return ok_all


def run_bilinear(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(43)
    for kind, edge in (("f32", 1024), ("f32", 16384), ("q31", 1024), ("q15", 1024), ("q7", 1024)):
        size = np.dtype(ir.NP[kind]).itemsize
        count = int(gib * 2 ** 30 / (8 + size))
        tab = bc.rnd(kind, gen, edge, edge)
        S, keep = dsp.bilinear_interp_instance(kind, tab)
        X, Y = coords(kind, count, 0.0, edge - 1.0, gen), coords(kind, count, 0.0, edge - 1.0, gen)
        out = torch.zeros(count, dtype=tab.dtype, device="cuda")
        ours = lambda: dsp.bilinear_interp_batch(kind, S, X, Y, out)                 # noqa: E731
        ours()
        torch.cuda.synchronize()
        if edge == 1024:
            h = tab.cpu().numpy()
            want = ir.bilinear_f32(h, ends(X), ends(Y)) if kind == "f32" else ir.bilinear_q(kind, h, ends(X), ends(Y))
        else:
            # the 1 GiB table stays on the device: each checked point against its own 2 x 2 corner block, at the
            # point's offset into the block (X - floor(X) is exact, so the restatement forms the same xdiff)
            hx, hy = ends(X), ends(Y)
            xi, yi = np.floor(hx).astype(np.int64), np.floor(hy).astype(np.int64)
            want = np.array([ir.bilinear_f32(tab[j:j + 2, i:i + 2].cpu().numpy(), [a - np.float32(i)], [b - np.float32(j)])[0]
                             for a, b, i, j in zip(hx, hy, xi, yi)], dtype=np.float32)
        ok = ir.same_word(ends(out), want)
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = {}
        if kind == "f32":
            flat = tab.reshape(-1)

            def gather():
                xi, yi = X.floor().clamp(max=edge - 2), Y.floor().clamp(max=edge - 2)
                k = xi.long() + yi.long() * edge
                top = torch.lerp(flat[k], flat[k + 1], X - xi)
                return torch.lerp(top, torch.lerp(flat[k + edge], flat[k + edge + 1], X - xi), Y - yi)
            bc.yardstick(line, "torch", "torch gather + lerp, same tensors (not bit-exact)", gather, min(ms))
        emit(f"bilinear_interp_{kind}", edge * edge, count, ok, ms, steps, (8 + size) * count, gib,
             table_bytes=size * edge * edge, **line)
    return ok_all


def run_spline(gib):
    ok_all = True
    for n, batch in ((64, 1 << 16), (1024, 1 << 12)):
        rng = np.random.default_rng(n)
        x = np.cumsum(rng.uniform(0.1, 1.0, (batch, n)), axis=1).astype(np.float32)
        y = rng.normal(0.0, 1.0, (batch, n)).astype(np.float32)
        xq = np.sort(rng.uniform(0.0, 1.0, (batch, n)) * x[:, -1:], axis=1).astype(np.float32)
        dx, dy, dq = (torch.from_numpy(a).cuda() for a in (x, y, xq))
        coeffs = torch.zeros((batch, 3 * (n - 1)), dtype=torch.float32, device="cuda")
        temp = torch.zeros((batch, 2 * n - 1), dtype=torch.float32, device="cuda")
        out = torch.zeros((batch, n), dtype=torch.float32, device="cuda")
        init = lambda: dsp.spline_init_batch(0, dx, dy, coeffs, temp)               # noqa: E731
        ev = lambda: dsp.spline_batch(dx, dy, coeffs, dq, out)                       # noqa: E731
        init()
        ev()
        torch.cuda.synchronize()
        ok = True
        for i in (0, batch - 1):
            wc, wt = ir.spline_init(0, x[i], y[i])
            ok = ok and ir.same_word(coeffs[i].cpu().numpy(), wc) and ir.same_word(temp[i].cpu().numpy(), wt)
            ok = ok and ir.same_word(out[i].cpu().numpy(), ir.spline_eval(x[i], y[i], wc, xq[i]))
        ok_all = ok_all and ok
        ms, steps = bc.measure(init)
        emit("spline_init_f32", n, batch, ok, ms, steps, 4 * batch * (2 * n + 3 * (n - 1) + 2 * n - 1), gib)
        ms, steps = bc.measure(ev)
        emit("spline_f32", n, batch, ok, ms, steps, 4 * batch * (2 * n + 3 * (n - 1) + 2 * n), gib)
    return ok_all


def run_quaternion(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(47)
    for func in qr.FUNCS + ("product",):
        wa, wd = (4, 4) if func == "product" else qr.WORDS[func]
        wb = 4 if func == "product" else 0
        n = int(gib * 2 ** 30 / (4 * (wa + wb + wd)))
        a = torch.rand((n, wa), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
        b = torch.rand((n, 4), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1 if wb else None
        d = torch.zeros((n, wd), dtype=torch.float32, device="cuda")
        ours = (lambda: dsp.quaternion_product_batch(a, b, d)) if wb else (lambda: dsp.quaternion_batch(func, a, d))
        ours()
        torch.cuda.synchronize()
        ha = np.concatenate([a[:EDGE].cpu().numpy(), a[-EDGE:].cpu().numpy()])
        hd = np.concatenate([d[:EDGE].cpu().numpy(), d[-EDGE:].cpu().numpy()])
        if wb:
            want = qr.product(ha, np.concatenate([b[:EDGE].cpu().numpy(), b[-EDGE:].cpu().numpy()]))
        else:
            want = qr.apply(func, ha)
        ok = qr.same_word(hd.reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = {}
        if wb:
            def product():
                a0, a1, a2, a3 = a.unbind(1)
                b0, b1, b2, b3 = b.unbind(1)
                return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                                    a0 * b2 + a2 * b0 + a3 * b1 - a1 * b3, a0 * b3 + a3 * b0 + a1 * b2 - a2 * b1], dim=1)
            bc.yardstick(line, "torch", "torch element-wise ops, same tensors", product, min(ms))
        emit(f"{func}_f32", wa, n, ok, ms, steps, 4 * (wa + wb + wd) * n, gib, **line)
    return ok_all


def main():
    args = sys.argv[1:]
    gib = 1.0
    gpu_modules()
    for flag in ("--gib", "--window"):
        if flag in args:
            i = args.index(flag)
            if flag == "--gib":
                gib = float(args[i + 1])
            else:
                bc.window_ms = float(args[i + 1])
            del args[i:i + 2]
    runs = {"linear": run_linear, "bilinear": run_bilinear, "spline": run_spline, "quaternion": run_quaternion}
    ok = True
    for g in args or list(runs):
        ok = runs[g](gib) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
