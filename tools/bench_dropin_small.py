#!/usr/bin/env python3
"""Host cost of a small synchronous drop-in call: the shapes where the work per call on the host is the whole cost.

    python tools/bench_dropin_small.py [--calls N] [--repeats R]

arm_add_f32 and arm_mean_f32 on 64 words, host pointers (staged in, launched, staged out, waited for) and device
pointers (launched and waited for).  Each repeat times N back-to-back calls on the host clock, ending in a device
synchronise, and gives microseconds per call; a line reports the median repeat and the spread of the repeats.
Compare two libraries by running it alternately with CMSISDSP_MI355X_LIB set to each."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
import torch  # noqa: E402

import cmsisdsp_amd as dsp  # noqa: E402

N = 64


def main():
    args = sys.argv[1:]
    calls = int(args[args.index("--calls") + 1]) if "--calls" in args else 2000
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 7
    rng = np.random.default_rng(1)
    ha, hb = rng.uniform(-1, 1, N).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32)
    hd, hr = np.zeros(N, dtype=np.float32), np.zeros(1, dtype=np.float32)
    da, db = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
    dd, dr = torch.zeros(N, device="cuda"), torch.zeros(1, device="cuda")
    add, mean = dsp.lib.arm_add_f32, dsp.lib.arm_mean_f32
    cases = (("arm_add_f32", "host", add, (ha.ctypes.data, hb.ctypes.data, hd.ctypes.data, N)),
             ("arm_add_f32", "device", add, (da.data_ptr(), db.data_ptr(), dd.data_ptr(), N)),
             ("arm_mean_f32", "host", mean, (ha.ctypes.data, N, hr.ctypes.data)),
             ("arm_mean_f32", "device", mean, (da.data_ptr(), N, dr.data_ptr())))
    for name, where, fn, a in cases:
        us = []
        for _ in range(2 + repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(*a)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6 / calls)
        us = sorted(us[2:])
        med = us[len(us) // 2]
        print(json.dumps({"workload": f"{name} drop-in, {N} words, {where} pointers", "n": N, "calls": calls,
                          "value": round(med, 3), "unit": "us/call (wall clock, median repeat)",
                          "us": [round(u, 3) for u in us], "spread": round((us[-1] - us[0]) / us[0], 4),
                          "version": dsp.version()}), flush=True)
    assert dsp.last_error()[0] == 0, dsp.last_error()
    assert hd.tobytes() == (ha + hb).tobytes() and dd.cpu().numpy().tobytes() == hd.tobytes()


if __name__ == "__main__":
    main()
