#!/usr/bin/env python3
"""Writes tests/golden/adaptive.npz and tests/golden/abi_layout_adaptive.json (development machine only).

oracle/ref.mk does not build the IIR lattice or the LMS family, so their checker is committed data: this
script compiles the reference's arm_iir_lattice_*, arm_lms_* and arm_lms_norm_* sources, their inits and
the common tables with ref.mk's flags into a temporary directory outside the tree, calls them through
ctypes and records, per function and case, the coefficients (k and v, or the initial taps), mu, postShift,
the input and reference blocks, out and err of each of two consecutive calls, the final coefficients, the
live state and energy / x0, plus the 64 words of armRecipTableQ15.  Nothing compiled and no reference text
is kept; only these arrays.  Every case is also run through tests/adaptive_ref.py, which refuses the
arguments for which the reference's shift counts are undefined, and must agree with the reference.

    python tools/make_golden_adaptive.py [--ref DIR]      (DIR: the reference tree, default as oracle/ref.mk)
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
import adaptive_ref as ar  # noqa: E402

CFLAGS = ["-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w"]
# (numStages or numTaps, [block of call 1, block of call 2]); postShift = index % 4 for the fixed-point LMS kinds
MAIN = [(1, [1, 1]), (2, [7, 9]), (3, [37, 37]), (8, [130, 130]), (17, [64, 5]), (70, [96, 33])]
SEED = 21
F32 = np.float32


def build(ref, out):
    ff = os.path.join(ref, "Source", "FilteringFunctions")
    srcs = [s for pat in ("arm_iir_lattice_*.c", "arm_lms_*.c") for s in sorted(glob.glob(os.path.join(ff, pat)))
            if not s.endswith(("f16.c", "f64.c")) and "norm_q31" not in s and "norm_init_q31" not in s]
    srcs.append(os.path.join(ref, "Source", "CommonTables", "arm_common_tables.c"))
    inc = ["-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude")]
    so = os.path.join(out, "libadaptive_ref.so")
    subprocess.run(["gcc", *CFLAGS, "-shared", *inc, *srcs, "-o", so], check=True)
    lib = C.CDLL(so)
    _abi.bind(lib, _abi.ADAPTIVE)
    exe = os.path.join(out, "abi_layout_adaptive")
    subprocess.run(["gcc", "-D__GNUC_PYTHON__", *inc, os.path.join(ROOT, "tools", "abi_layout_adaptive.c"), "-o", exe],
                   check=True)
    table = np.array((C.c_int16 * 64).in_dll(lib, "armRecipTableQ15"), dtype=np.int16)
    return lib, json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout), table


def run_iir(lib, func, k, v, blocks):
    dt, _ = ar.FUNCS[func]
    inst, init, _ = _abi.ADAPTIVE_FUNCS[func]
    n, bmax = len(k), max(len(b) for b in blocks)
    S = inst()
    state = np.full(n + bmax, 77, dtype=dt)                # the init must zero it
    k, v = k.copy(), v.copy()
    getattr(lib, init)(C.byref(S), n, k.ctypes.data, v.ctypes.data, state.ctypes.data, bmax)
    assert not state.any(), func
    ys = []
    for x in blocks:
        y = np.zeros_like(x)
        getattr(lib, func)(C.byref(S), x.ctypes.data, y.ctypes.data, len(x))
        ys.append(y)
    return ys, state[:n].copy()


def run_lms(lib, func, taps0, mu, ps, xs, ds):
    dt, fam = ar.FUNCS[func]
    inst, init, extra = _abi.ADAPTIVE_FUNCS[func]
    n, bmax = len(taps0), max(len(b) for b in xs)
    S = inst()
    state = np.full(n + bmax - 1, 77, dtype=dt)
    c = taps0.copy()
    getattr(lib, init)(C.byref(S), n, c.ctypes.data, state.ctypes.data, mu, bmax, *([ps] if len(extra) == 2 else []))
    assert not state.any(), func
    outs, errs = [], []
    for x, d in zip(xs, ds):
        d, y, e = d.copy(), np.zeros_like(x), np.zeros_like(x)
        getattr(lib, func)(C.byref(S), x.ctypes.data, d.ctypes.data, y.ctypes.data, e.ctypes.data, len(x))
        outs.append(y), errs.append(e)
    ex = np.array([S.energy, S.x0], dtype=dt) if fam == "nlms" else None
    return outs, errs, c, state[:n - 1].copy(), ex


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    args = ap.parse_args()
    rng = np.random.default_rng(SEED)
    data, index = {}, []
    tiny = np.finfo(F32).tiny

    def subnormal(a):
        return bool(((np.abs(a) > 0) & (np.abs(a) < tiny)).any())

    with tempfile.TemporaryDirectory() as tmp:
        lib, layout, table = build(args.ref, tmp)
        assert table.tobytes() == ar.recip_table().tobytes(), "armRecipTableQ15 is not the closed form"
        data["armRecipTableQ15"] = table

        def rec_iir(func, case, k, v, blocks, bounded):
            dt, _ = ar.FUNCS[func]
            ys, state = run_iir(lib, func, k, v, blocks)
            st = np.zeros((1, len(k)), dtype=dt)
            for x, y in zip(blocks, ys):                      # the restatement agrees
                got, st = ar.iir_lattice(func, k, v, x[None], st)
                assert got[0].tobytes() == y.tobytes(), (func, case)
            assert st[0].tobytes() == state.tobytes(), (func, case)
            if dt == F32:
                assert all(np.isfinite(y).all() for y in ys) and np.isfinite(state).all(), (func, case)
                assert np.abs(k).max() < 1, (func, case)
                if bounded:
                    peak = max(np.abs(y).max() for y in ys)
                    assert 1e-4 <= peak <= 1e3, (func, case, peak)
            key = f"{func}/{case}"
            data[key + "/k"], data[key + "/v"], data[key + "/state"] = k, v, state
            for i, (x, y) in enumerate(zip(blocks, ys)):
                data[f"{key}/x{i}"], data[f"{key}/y{i}"] = x, y
            index.append([func, case])
            return ys, state

        def rec_lms(func, case, taps0, mu, ps, xs, ds):
            dt, fam = ar.FUNCS[func]
            outs, errs, c, state, ex = run_lms(lib, func, taps0, mu, ps, xs, ds)
            cc, st = taps0[None].copy(), np.zeros((1, len(taps0) - 1), dtype=dt)
            ee = np.zeros((1, 2), dtype=dt) if fam == "nlms" else None
            for x, d, y, e in zip(xs, ds, outs, errs):        # raises on an undefined shift count
                gy, ge, cc, st, ee = ar.lms(func, mu, ps, x[None], d[None], cc, st, ee)
                assert gy[0].tobytes() == y.tobytes() and ge[0].tobytes() == e.tobytes(), (func, case)
            assert cc[0].tobytes() == c.tobytes() and st[0].tobytes() == state.tobytes(), (func, case)
            assert ee is None or ee[0].tobytes() == ex.tobytes(), (func, case)
            if dt == F32:
                assert all(np.isfinite(a).all() for a in outs + errs + [c]), (func, case)
            key = f"{func}/{case}"
            data[key + "/coeffs0"], data[key + "/coeffs"], data[key + "/state"] = taps0, c, state
            data[key + "/mu"], data[key + "/ps"] = np.array(mu, dtype=dt), np.int32(ps)
            if ex is not None:
                data[key + "/ex"] = ex
            for i in range(len(xs)):
                data[f"{key}/x{i}"], data[f"{key}/d{i}"] = xs[i], ds[i]
                data[f"{key}/out{i}"], data[f"{key}/err{i}"] = outs[i], errs[i]
            index.append([func, case])
            return outs, errs, c, state, ex

        for func, (dt, fam) in ar.FUNCS.items():
            fixed = dt != F32
            lo, hi = (np.iinfo(dt).min, np.iinfo(dt).max) if fixed else (None, None)
            mu = ar.default_mu(func)
            mu = float(mu) if dt == F32 else int(mu)
            for i, (n, blks) in enumerate(MAIN):
                case = f"n{n}_b{blks[0]}_{blks[1]}"
                if fam == "iir":
                    k, v = ar.lattice_coeffs(func, n, int(rng.integers(1 << 30)))
                    rec_iir(func, case, k, v, [ar.signal(func, b, int(rng.integers(1 << 30))) for b in blks], True)
                else:
                    ps = i % 4 if fixed else 0
                    taps0 = ar.quantise(rng.uniform(-0.3, 0.3, n) / 2.0 ** ps, dt)
                    xs = [ar.signal(func, b, int(rng.integers(1 << 30))) for b in blks]
                    ds = [ar.signal(func, b, int(rng.integers(1 << 30))) for b in blks]
                    rec_lms(func, case, taps0, mu, ps, xs, ds)
            if fam == "iir" and not fixed:            # impulse, then zeros: the state decays through the subnormals
                k, v = np.array([0.3, -0.3], F32), np.array([0.5, 0.25, 1.0], F32)
                x = np.zeros(401, F32)
                x[0] = 1.0
                ys, state = rec_iir(func, "decay", k, v, [x, np.zeros(8, F32)], False)
                assert subnormal(ys[0]) and not state.any(), func
            if fam == "iir" and fixed:                # full-scale words: f and g saturate
                k = np.array([hi, lo, hi], dtype=dt)
                v = np.array([hi, lo, hi, lo], dtype=dt)
                xs = [rng.choice(np.array([lo, hi], dtype=dt), b) for b in (33, 6)]
                ys, state = rec_iir(func, "extreme", k, v, xs, False)
                assert np.isin(state, [lo, hi]).any(), func
            if fam != "iir":                          # identify a known FIR: the error decays, the taps move
                h = np.array([0.4, -0.3, 0.2, 0.25, -0.15, 0.1, 0.05, -0.05])
                sig = rng.uniform(-0.5, 0.5, 260 + len(h) - 1)
                want = np.convolve(sig, h, mode="valid")       # d[n] = sum_j h[j] x[n - j]
                x, d = ar.quantise(sig[len(h) - 1:], dt), ar.quantise(want, dt)
                muc = {"lms": 0.2, "nlms": 0.5}[fam]
                muc = muc if dt == F32 else int(ar.quantise(muc, dt))
                outs, errs, c, _, _ = rec_lms(func, "converge", np.zeros(len(h), dtype=dt), muc, 0,
                                              [x[:130], x[130:]], [d[:130], d[130:]])
                e = np.abs(np.concatenate(errs).astype(np.float64))
                print(f"{func} converge: mean|err| {e[:65].mean():.4g} -> {e[-65:].mean():.4g}")
                assert e[-65:].mean() < 0.5 * e[:65].mean(), func
                scale = 1.0 if dt == F32 else float(-int(lo))
                assert np.abs(c.astype(np.float64) / scale).max() > 0.2, func     # from zero towards h (peak 0.4)
            if fam != "iir" and not fixed:            # the input dies away: subnormals in the history and the taps' updates
                n = np.arange(280)
                sig = (0.7 ** n * rng.uniform(0.5, 1.0, 280)).astype(F32)
                d = (0.5 * sig + 0.25 * np.concatenate([[0], sig[:-1]])).astype(F32)
                outs, errs, c, state, ex = rec_lms(func, "decay", np.array([0.1, 0.2, -0.1], F32), mu, 0,
                                                   [sig[:250], sig[250:]], [d[:250], d[250:]])
                assert subnormal(sig) and subnormal(np.concatenate(outs)) and subnormal(state), func
            if fam != "iir" and fixed:                # full-scale words: the taps saturate, the q15 energy reaches 32767
                taps0 = np.array([hi, lo, 0, hi], dtype=dt)
                # normalised: +-32767 only, so the energy sits at 32767 (reciprocal argument 32772, wrapped to
                # -32764) and never at 32763 or -5, whose arguments -32768 and 0 are undefined in the reference
                pool = np.array([-hi, hi] if fam == "nlms" else [lo, hi, hi], dtype=dt)
                xs = [rng.choice(pool, b) for b in (33, 6)]
                ds = [rng.choice(np.array([lo, hi], dtype=dt), b) for b in (33, 6)]
                outs, errs, c, state, ex = rec_lms(func, "extreme", taps0, int(hi), 1, xs, ds)
                assert np.isin(c, [lo, hi]).any(), func
                assert ex is None or ex[0] == 32767, (func, ex)
    data["index"] = np.array(json.dumps(index))
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "adaptive.npz"), **data)
    with open(os.path.join(gold, "abi_layout_adaptive.json"), "w") as f:
        json.dump(layout, f, indent=1)
    print("wrote", len(index), "cases,", os.path.getsize(os.path.join(gold, "adaptive.npz")), "bytes")


if __name__ == "__main__":
    main()
