#!/usr/bin/env python3
"""Writes tests/golden/biquad.npz and tests/golden/abi_layout_biquad.json (development machine only).

oracle/ref.mk does not build the biquad cascades, so their checker is committed data: this script
compiles the reference's arm_biquad_cas* sources and inits with ref.mk's flags into a temporary
directory outside the tree, calls them through ctypes and records, per function and case, the
coefficients, postShift, the input blocks, the output of each of two consecutive calls and the final
state.  Nothing compiled and no reference text is kept; only these arrays.

    python tools/make_golden_biquad.py [--ref DIR]      (DIR: the reference tree, default as oracle/ref.mk)
"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd", "cmsisdsp_amd"))
import _abi  # noqa: E402  (the ctypes mirrors only; the product library is not loaded)
import biquad_ref  # noqa: E402

CFLAGS = ["-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w"]
# (numStages, [block of call 1, block of call 2]); postShift = index % 4 for the fixed-point kinds
MAIN = [(1, [1, 1]), (2, [7, 9]), (3, [37, 37]), (8, [130, 130]), (17, [64, 5]), (70, [96, 33])]
SEED = 20


def build(ref, out):
    srcs = [s for s in sorted(glob.glob(os.path.join(ref, "Source", "FilteringFunctions", "arm_biquad_cas*.c")))
            if not s.endswith(("f16.c", "f64.c"))]
    so = os.path.join(out, "libbiquad_ref.so")
    subprocess.run(["gcc", *CFLAGS, "-shared", "-I" + os.path.join(ref, "Include"),
                    "-I" + os.path.join(ref, "PrivateInclude"), *srcs, "-o", so], check=True)
    lib = C.CDLL(so)
    _abi.bind(lib, _abi.BIQUAD)
    exe = os.path.join(out, "abi_layout_biquad")
    subprocess.run(["gcc", "-D__GNUC_PYTHON__", "-I" + os.path.join(ref, "Include"),
                    "-I" + os.path.join(ref, "PrivateInclude"), os.path.join(ROOT, "tools", "abi_layout_biquad.c"),
                    "-o", exe], check=True)
    return lib, json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)


def design(rng, stages, post_shift):
    """Stable, bounded sections: conjugate poles of radius r in [0.3, 0.9] (a1 = 2 r cos t, a2 = -r^2)
    near one centre angle per cascade, zeros away from it, numerator scaled to a peak magnitude
    response of 1.  post_shift == 0 keeps |a1| < 1 so the fixed-point words hold it."""
    tc = rng.uniform(1.15, 1.95) if post_shift == 0 else rng.uniform(0.5, 2.6)
    w = np.linspace(0, np.pi, 2048)
    z1 = np.exp(-1j * w)
    rows = []
    for _ in range(stages):
        r = rng.uniform(0.3, 0.9 if stages <= 8 else 0.6)
        t = tc + rng.uniform(-0.05, 0.05)
        a1, a2 = 2 * r * np.cos(t), -r * r
        rho, phi = rng.uniform(0.3, 0.9), (tc + np.pi / 2) % np.pi
        b = np.array([1.0, -2 * rho * np.cos(phi), rho * rho])
        h = (b[0] + b[1] * z1 + b[2] * z1 * z1) / (1 - a1 * z1 - a2 * z1 * z1)
        b /= np.abs(h).max()
        rows.append([b[0], b[1], b[2], a1, a2])
    return np.array(rows)


def quantise(rows, func, post_shift):
    dt, _, _, nc, _ = biquad_ref.FUNCS[func]
    if dt == np.float32:
        return rows.astype(np.float32).reshape(-1)
    bits = 15 if dt == np.int16 else 31
    q = np.clip(np.round(rows / 2.0 ** post_shift * 2.0 ** bits), -2 ** bits, 2 ** bits - 1).astype(dt)
    if nc == 6:                                    # q15: {b0, 0, b1, b2, a1, a2}
        q = np.concatenate([q[:, :1], np.zeros((len(q), 1), dt), q[:, 1:]], axis=1)
    return q.reshape(-1)


def samples(rng, func, n, tc):
    dt, _, _, _, ch = biquad_ref.FUNCS[func]
    k = np.arange(n)[:, None]
    x = 0.5 * np.sin(tc * k + rng.uniform(0, 6, ch)) + rng.uniform(-0.4, 0.4, (n, ch))
    if dt == np.float32:
        return x.astype(np.float32).reshape(-1)
    bits = 15 if dt == np.int16 else 31
    return np.clip(np.round(x * 2.0 ** bits), -2 ** bits, 2 ** bits - 1).astype(dt).reshape(-1)


def run_ref(lib, func, coeffs, post_shift, blocks):
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    inst, init, ps_t = _abi.BIQUAD_FUNCS[func]
    stages = len(coeffs) // nc
    S = inst()
    state = np.full(ks * stages, 77, dtype=sdt)    # the init must zero it
    getattr(lib, init)(C.byref(S), stages, coeffs.ctypes.data, state.ctypes.data, *([post_shift] if ps_t else []))
    outs = []
    for x in blocks:
        y = np.zeros_like(x)
        getattr(lib, func)(C.byref(S), x.ctypes.data, y.ctypes.data, len(x) // ch)
        outs.append(y)
    return outs, state


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    args = ap.parse_args()
    rng = np.random.default_rng(SEED)
    data, index = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        lib, layout = build(args.ref, tmp)

        def record(func, case, coeffs, ps, blocks, main_case):
            outs, state = run_ref(lib, func, coeffs, ps, blocks)
            if biquad_ref.FUNCS[func][0] == np.float32:
                assert all(np.isfinite(y).all() for y in outs) and np.isfinite(state).all(), (func, case)
                if main_case:
                    peak = max(np.abs(y).max() for y in outs)
                    assert 1e-3 <= peak <= 1e3, (func, case, peak)
                    print(f"{func} {case}: max|y| = {peak:.3g}")
            key = f"{func}/{case}"
            data[key + "/coeffs"], data[key + "/ps"] = coeffs, np.int32(ps)
            for i, (x, y) in enumerate(zip(blocks, outs)):
                data[f"{key}/x{i}"], data[f"{key}/y{i}"] = x, y
            data[key + "/state"] = state
            index.append([func, case, len(blocks)])

        for func, (dt, sdt, ks, nc, ch) in biquad_ref.FUNCS.items():
            fixed = dt != np.float32
            for i, (stages, blks) in enumerate(MAIN):
                ps = i % 4 if fixed else 0
                rows = design(rng, stages, ps)
                tc = float(np.arccos(np.clip(rows[0, 3] / (2 * np.sqrt(-rows[0, 4])), -1, 1)))
                record(func, f"s{stages}_b{blks[0]}_{blks[1]}", quantise(rows, func, ps), ps,
                       [samples(rng, func, b, tc) for b in blks], True)
            if fixed:                              # all-minimum words: wrap-around and saturation
                lo = np.iinfo(dt).min
                c = np.full(nc * 2, lo, dtype=dt)
                if nc == 6:
                    c[1::6] = 0
                record(func, "extreme", c, 1, [np.full(9, lo, dtype=dt), np.full(5, lo, dtype=dt)], False)
                hi = np.iinfo(dt).max                # full-range random words: wraps and saturations that mix signs
                c = rng.integers(lo, hi, nc * 3, endpoint=True).astype(dt)
                if nc == 6:
                    c[1::6] = 0
                record(func, "fullrange", c, 2, [rng.integers(lo, hi, b, endpoint=True).astype(dt) for b in (33, 6)],
                       False)
            else:                                  # impulse + 400 zeros, pole radius 0.5: the state decays
                r, t = 0.5, 1.3                    # through the subnormal range to zero (a1 < 0.5)
                c = np.array([1.0, 0.3, 0.2, 2 * r * np.cos(t), -r * r], dtype=np.float32)
                x = np.zeros(401 * ch, dtype=np.float32)
                x[:ch] = 1.0
                outs, state = run_ref(lib, func, c, 0, [x])
                tiny = np.finfo(np.float32).tiny
                assert ((np.abs(outs[0]) > 0) & (np.abs(outs[0]) < tiny)).any() and not state.any(), func
                record(func, "decay", c, 0, [x, np.zeros(8 * ch, dtype=np.float32)], False)
    data["index"] = np.array(json.dumps(index))
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "biquad.npz"), **data)
    with open(os.path.join(gold, "abi_layout_biquad.json"), "w") as f:
        json.dump(layout, f, indent=1)
    print("wrote", len(index), "cases,", os.path.getsize(os.path.join(gold, "biquad.npz")), "bytes")


if __name__ == "__main__":
    main()
