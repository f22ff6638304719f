#!/usr/bin/env python3
"""Throughput of the support functions on one GPU.

    python tools/bench_support.py [ew|sort|mean ...] [--gib G] [--window MS]

Timing is tools/bench_cmplx.py's: a clock-settle phase, then REPEATS windows of about --window ms between HIP events;
a line reports the best window, the repeat spread and, for the streaming functions, the fraction of the 8 TB/s HBM
peak its algorithmic bytes reach.

  ew    the 12 conversions, arm_copy_* and arm_fill_* on items of 1024 words, about G GiB (default 1) of traffic per
        call (the source read once, the destination written once; fill writes only).  Next to each line:
        arm_mat_add_<type>_batch of the narrower type (q7: _q15 on the reinterpreted bytes) on G GiB in the same run,
        compared per byte moved.
  sort  arm_sort_f32_batch at item lengths 64, 1024 and kSortLdsMax (G / 4 GiB of items) and one vector of 2^20
        words, ascending, in M items/s and M keys/s, next to torch.sort(dim=-1) on the same tensor.
  mean  arm_weighted_average_f32_batch at 64 and 1024 words per item and arm_barycenter_f32_batch (64 vectors of 64
        dimensions), next to arm_dot_prod_f32_batch on the same bytes.

The first and last item of every result are checked bit for bit against tests/support_ref.py first."""
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
import support_ref as sr  # noqa: E402

HBM_TBPS = bc.HBM_TBPS
TDT = bc.TDT
N = 1024


def frac(nbytes, ms):
    return nbytes / (ms * 1e-3) / (HBM_TBPS * 1e12)


def line_of(workload, n, batch, ok, ms, steps, nbytes=None):
    best = min(ms)
    line = {"workload": workload, "n": n, "batch": batch, "bitexact_first_last": ok,
            "value": round(batch / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
            "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps}
    if nbytes is not None:
        line["roofline"] = {"bound": "hbm", "bytes": nbytes, "peak_TBps": HBM_TBPS, "frac": round(frac(nbytes, best), 4)}
    return line


def mat_add_yardstick(t, gib):
    """arm_mat_add_<t>_batch (q7: _q15 on the same bytes) over three tensors of G / 3 GiB each."""
    yt = "q15" if t == "q7" else t
    size = torch.empty(0, dtype=TDT[yt]).element_size()
    k = max(1, int(gib * 2 ** 30 / (3 * size * 1024)))
    x, y, z = (torch.zeros((k, 32, 32), dtype=TDT[yt], device="cuda") for _ in range(3))
    ms, steps = bc.measure(lambda: dsp.mat_add_batch(x, y, z))
    return {"workload": f"arm_mat_add_{yt}_batch, same run", "ms": [round(v, 4) for v in ms], "steps": steps,
            "frac": round(frac(3 * size * 1024 * k, min(ms)), 4)}


def run_ew(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(7)
    yards = {}
    for func in sr.CONVERSIONS + sr.COPIES + sr.FILLS:
        s, d = sr.types(func)
        ssz = 0 if s is None else np.dtype(sr.DT[s]).itemsize
        dsz = np.dtype(sr.DT[d]).itemsize
        batch = max(1, int(gib * 2 ** 30 / ((ssz + dsz) * N)))
        dst = torch.zeros((batch, N), dtype=TDT[d], device="cuda")
        if s is None:
            ours = lambda: dsp.fill_batch(3, dst)                                   # noqa: E731
        else:
            src = bc.rnd(s, gen, batch, N)
            ours = lambda: dsp.convert_batch(src, dst)                              # noqa: E731
        ours()
        torch.cuda.synchronize()
        if s is None:
            ok = bool((dst[0] == 3).all() and (dst[-1] == 3).all())
        else:
            ok = all(sr.same_words(dst[i].cpu().numpy(), sr.convert(s, d, src[i].cpu().numpy()), d == "f32")
                     for i in (0, batch - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = line_of(func, N, batch, ok, ms, steps, (ssz + dsz) * N * batch)
        narrow = d if s is None or dsz <= ssz else s
        if narrow not in yards:
            yards[narrow] = mat_add_yardstick(narrow, gib)
        line["yardstick"] = yards[narrow]
        line["frac_to_yardstick"] = round(line["roofline"]["frac"] / yards[narrow]["frac"], 3)
        line["version"] = dsp.version()
        print(json.dumps(line), flush=True)
        del dst
    return ok_all


def run_sort(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(9)
    for n, batch in ((64, None), (1024, None), (sr.SORT_LDS_MAX, None), (2 ** 20, 1)):
        batch = batch or max(1, int(gib / 4 * 2 ** 30 / (4 * n)))
        src = bc.rnd("f32", gen, batch, n)
        dst = torch.zeros_like(src)
        ours = lambda: dsp.sort_batch(src, dst)                                     # noqa: E731
        ours()
        torch.cuda.synchronize()
        ok = all(dst[i].cpu().numpy().tobytes() == sr.total_order_sort(src[i].cpu().numpy()).tobytes()
                 for i in (0, batch - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = line_of("sort_f32", n, batch, ok, ms, steps)
        line["Mkeys_per_s"] = round(batch * n / (min(ms) * 1e-3) * 1e-6, 1)
        line["pass_bytes_frac"] = round(frac(8 * n * batch, min(ms)), 4)           # one read and one write of the keys
        bc.yardstick(line, "yardstick", "torch.sort(dim=-1), same tensor", lambda: torch.sort(src, dim=-1), min(ms))
        line["version"] = dsp.version()
        print(json.dumps(line), flush=True)
        del src, dst
    return ok_all


def run_mean(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(13)
    for n in (64, 1024):
        batch = max(1, int(gib * 2 ** 30 / (8 * n)))
        a, w = bc.rnd("f32", gen, batch, n), torch.rand((batch, n), generator=gen, device="cuda", dtype=torch.float32)
        res = torch.zeros(batch, dtype=torch.float32, device="cuda")
        ours = lambda: dsp.weighted_average_batch(a, w, res)                        # noqa: E731
        ours()
        torch.cuda.synchronize()
        ok = all(sr.same_words(res[i:i + 1].cpu().numpy(),
                               sr.weighted_average(a[i:i + 1].cpu().numpy(), w[i:i + 1].cpu().numpy()), True)
                 for i in (0, batch - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = line_of("weighted_average_f32", n, batch, ok, ms, steps, 8 * n * batch)
        bc.yardstick(line, "yardstick", "arm_dot_prod_f32_batch, same tensors", lambda: dsp.dot_prod_batch(a, w, res),
                     min(ms))
        line["version"] = dsp.version()
        print(json.dumps(line), flush=True)
        del a, w
    nv = dim = 64
    batch = max(1, int(gib * 2 ** 30 / (4 * nv * dim)))
    a = bc.rnd("f32", gen, batch, nv, dim)
    w = torch.rand((batch, nv), generator=gen, device="cuda", dtype=torch.float32) + 0.1
    out = torch.zeros((batch, dim), dtype=torch.float32, device="cuda")
    ours = lambda: dsp.barycenter_batch(a, w, out)                                  # noqa: E731
    ours()
    torch.cuda.synchronize()
    ok = all(sr.same_words(out[i:i + 1].cpu().numpy(),
                           sr.barycenter(a[i:i + 1].cpu().numpy(), w[i:i + 1].cpu().numpy()), True)
             for i in (0, batch - 1))
    ms, steps = bc.measure(ours)
    line = line_of("barycenter_f32", nv * dim, batch, ok, ms, steps, 4 * (nv * dim + nv + dim) * batch)
    half = a.view(2, batch * nv // 2, dim)                  # the same bytes as the two sources of a dot product
    res = torch.zeros(batch * nv // 2, dtype=torch.float32, device="cuda")
    bc.yardstick(line, "yardstick", "arm_dot_prod_f32_batch, the same bytes as two sources of 64-word items",
                 lambda: dsp.dot_prod_batch(half[0], half[1], res), min(ms))
    line["version"] = dsp.version()
    print(json.dumps(line), flush=True)
    return ok_all and ok


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
    groups = args or ["ew", "sort", "mean"]
    bad = []
    for name, fn in (("ew", run_ew), ("sort", run_sort), ("mean", run_mean)):
        if name in groups and not fn(gib):
            bad.append(name)
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
