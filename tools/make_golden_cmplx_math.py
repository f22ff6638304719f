#!/usr/bin/env python3
"""Writes tests/golden/cmplx_math.npz (development machine only).

oracle/ref.mk builds none of the 26 complex-math and max / min functions as entry points of their own, so their
checker is committed data: this script compiles the reference's 26 files (plus arm_sqrt_q31.c and the common
tables it reads) with ref.mk's flags into a temporary directory outside the tree, calls them through ctypes and
records, per function and case, the operands and the output buffers (pre-filled with a marker word).  Nothing
compiled and no reference text is kept; only these arrays.  Every case is also run through
tests/cmplx_math_ref.py, which must agree bit for bit (cases with NaN: by the f32 rule of
tests/test_f32_classes.py); where they disagree the reference build is right.

    python tools/make_golden_cmplx_math.py [--ref DIR]      (DIR: the reference tree, default as oracle/ref.mk)
"""
import argparse
import ctypes as C
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
import cmplx_math_ref as cm  # noqa: E402

CFLAGS = ["-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w"]
SEED = 59


def build(ref, out):
    src = os.path.join(ref, "Source")
    files = [os.path.join(src, "ComplexMathFunctions" if f.startswith("cmplx") else "StatisticsFunctions",
                          f"arm_{f}.c") for f in cm.FUNCS]
    files += [os.path.join(src, "FastMathFunctions", "arm_sqrt_q31.c"),
              os.path.join(src, "CommonTables", "arm_common_tables.c")]
    inc = ["-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude")]
    so = os.path.join(out, "libcmplx_math_ref.so")
    subprocess.run(["gcc", *CFLAGS, "-shared", *inc, *files, "-o", so, "-lm"], check=True)
    lib = C.CDLL(so)
    for f in cm.FUNCS:
        fn = getattr(lib, "arm_" + f)
        fn.restype, fn.argtypes = _abi.CMPLX_MATH["arm_" + f]     # the reference's signatures
    return lib


def run(lib, func, g):
    """The reference on a case's operands -> the dict cmplx_math_ref.run returns."""
    op, t = cm.split(func)
    fn = getattr(lib, "arm_" + func)
    src = {k: v.copy() for k, v in g.items()}
    out = {k: cm.marked(ty, shape if shape else 1) for k, (ty, shape) in cm.out_spec(func, g).items()}
    p = lambda x: x.ctypes.data                                                   # noqa: E731
    if op in ("max", "min"):
        fn(p(src["a"]), src["a"].size, p(out["value"]), p(out["index"]))
    elif op == "dot_prod":
        fn(p(src["a"]), p(src["b"]), src["a"].size // 2, p(out["re"]), p(out["im"]))
    elif op == "mult_cmplx":
        fn(p(src["a"]), p(src["b"]), p(out["dst"]), src["a"].size // 2)
    elif op == "mult_real":
        fn(p(src["a"]), p(src["r"]), p(out["dst"]), src["r"].size)
    else:
        fn(p(src["a"]), p(out["dst"]), src["a"].size // 2)
    for k, v in g.items():
        assert src[k].tobytes() == v.tobytes(), (func, k)
    return {k: (v if k == "dst" else v.reshape(())) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    args = ap.parse_args()
    rng = np.random.default_rng(SEED)
    data, index = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(args.ref, tmp)
        for func in cm.FUNCS:
            for case in cm.case_names(func):
                g = cm.operands(func, case, rng)
                got = run(lib, func, g)
                want = cm.run(func, g)
                assert got.keys() == want.keys(), (func, case)
                for k, v in got.items():
                    assert cm.same_words(v, want[k], cm.nan_rule(case)), (func, case, k, v, want[k])
                key = f"{func}/{case}/"
                for k, v in {**g, **got}.items():
                    data[key + k] = v
                index.append([func, case])
    data["index"] = np.array(json.dumps(index))
    path = os.path.join(ROOT, "tests", "golden", "cmplx_math.npz")
    np.savez_compressed(path, **data)
    print("wrote", len(index), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
