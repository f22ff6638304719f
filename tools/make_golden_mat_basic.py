#!/usr/bin/env python3
"""Writes tests/golden/mat_basic.npz (development machine only).

oracle/ref.mk builds three of the 20 element-wise, transpose and matrix-vector functions, so their checker is
committed data: this script compiles the reference's 20 files with ref.mk's flags into a temporary directory
outside the tree, calls them through ctypes and records, per function and case, the operands, the output buffer
(pre-filled with a marker word) and the status.  Nothing compiled and no reference text is kept; only these
arrays.  Every case is also run through tests/mat_basic_ref.py, which must agree bit for bit (non-finite cases:
by the f32 rule of tests/test_f32_classes.py); where they disagree the reference build is right.

    python tools/make_golden_mat_basic.py [--ref DIR]      (DIR: the reference tree, default as oracle/ref.mk)
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
import mat_basic_ref as mb  # noqa: E402

CFLAGS = ["-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w"]
SEED = 53


def build(ref, out):
    mf = os.path.join(ref, "Source", "MatrixFunctions")
    inc = ["-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude")]
    so = os.path.join(out, "libmat_basic_ref.so")
    subprocess.run(["gcc", *CFLAGS, "-shared", *inc, *[os.path.join(mf, f"arm_mat_{f}.c") for f in mb.FUNCS], "-o", so,
                    "-lm"], check=True)
    lib = C.CDLL(so)
    for f in mb.FUNCS:
        fn = getattr(lib, "arm_mat_" + f)
        fn.restype, fn.argtypes = _abi.MAT_BASIC["arm_mat_" + f]     # the reference's signatures
    return lib


def inst(t, x, cmplx=False):
    return _abi.MAT_INST[t](x.shape[0], x.shape[1] // (2 if cmplx else 1), C.cast(x.ctypes.data, _abi.MAT_PTR[t]))


def run(lib, func, g):
    """The reference on a case's operands -> the dict mat_basic_ref.run returns."""
    op, t = mb.split(func)
    fn = getattr(lib, "arm_mat_" + func)
    if op in ("add", "sub"):
        a, b = g["a"].copy(), g["b"].copy()
        d = mb.marked(t, a.shape)
        st = fn(C.byref(inst(t, a)), C.byref(inst(t, b)), C.byref(inst(t, d)))
        return {"status": st, "dst": d}
    if op == "scale":
        a = g["a"].copy()
        d = mb.marked(t, a.shape)
        args = [g["scale"].item()] + ([int(g["shift"])] if t != "f32" else [])
        st = fn(C.byref(inst(t, a)), *args, C.byref(inst(t, d)))
        return {"status": st, "dst": d}
    if op in ("trans", "cmplx_trans"):
        a = g["a"].copy()
        cm = op == "cmplx_trans"
        d = mb.marked(t, (a.shape[1] // 2, a.shape[0] * 2) if cm else a.shape[::-1])
        st = fn(C.byref(inst(t, a, cm)), C.byref(inst(t, d, cm)))
        return {"status": st, "dst": d}
    m, v = g["m"].copy(), g["v"].copy()
    d = mb.marked(t, m.shape[0])
    fn(C.byref(inst(t, m)), v.ctypes.data, d.ctypes.data)
    return {"dst": d}


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    args = ap.parse_args()
    rng = np.random.default_rng(SEED)
    data, index = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(args.ref, tmp)
        for func in mb.FUNCS:
            for case in mb.case_names(func):
                g = mb.operands(func, case, rng)
                got = run(lib, func, g)
                want = mb.run(func, g)
                assert got.keys() == want.keys(), (func, case)
                for k, v in got.items():
                    if k == "status":
                        assert v == want[k], (func, case, v, want[k])
                    else:
                        assert mb.same_words(v, want[k], case.startswith("nonfinite")), (func, case, k, v, want[k])
                key = f"{func}/{case}/"
                for k, v in {**g, **got}.items():
                    data[key + k] = np.int32(v) if k == "status" else v
                index.append([func, case])
    data["index"] = np.array(json.dumps(index))
    path = os.path.join(ROOT, "tests", "golden", "mat_basic.npz")
    np.savez_compressed(path, **data)
    print("wrote", len(index), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
