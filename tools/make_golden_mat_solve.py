#!/usr/bin/env python3
"""Writes tests/golden/mat_solve.npz (development machine only).

oracle/ref.mk does not build the inverse, the decompositions or the triangular solves, so their checker is
committed data: this script compiles the reference's arm_mat_inverse_f32.c, arm_mat_cholesky_f32.c,
arm_mat_ldlt_f32.c and arm_mat_solve_{lower,upper}_triangular_f32.c with ref.mk's flags into a temporary
directory outside the tree, calls them through ctypes and records, per function and case, the operands, every
output buffer (pre-filled with a marker word, so the words a call leaves alone show), src after the inverse,
pp and the status.  Nothing compiled and no reference text is kept; only these arrays.  Every case is also run
through tests/mat_solve_ref.py, which must agree bit for bit (non-finite cases: by the f32 rule of
tests/test_f32_classes.py).

    python tools/make_golden_mat_solve.py [--ref DIR]      (DIR: the reference tree, default as oracle/ref.mk)
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
import mat_solve_ref as mr  # noqa: E402

CFLAGS = ["-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w"]
SEED = 47
FILES = ("arm_mat_inverse_f32", "arm_mat_cholesky_f32", "arm_mat_ldlt_f32", "arm_mat_solve_lower_triangular_f32",
         "arm_mat_solve_upper_triangular_f32")
MAT = _abi.arm_matrix_instance_f32
PM = C.POINTER(MAT)


def build(ref, out):
    mf = os.path.join(ref, "Source", "MatrixFunctions")
    inc = ["-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude")]
    so = os.path.join(out, "libmat_solve_ref.so")
    subprocess.run(["gcc", *CFLAGS, "-shared", *inc, *[os.path.join(mf, f + ".c") for f in FILES], "-o", so, "-lm"],
                   check=True)
    lib = C.CDLL(so)
    for f in FILES:
        fn = getattr(lib, f)
        fn.restype = C.c_int
        fn.argtypes = {"arm_mat_inverse_f32": [PM, PM], "arm_mat_cholesky_f32": [PM, PM],
                       "arm_mat_ldlt_f32": [PM, PM, PM, C.c_void_p]}.get(f, [PM, PM, PM])
    return lib


def inst(x):
    return MAT(x.shape[0], x.shape[1], C.cast(x.ctypes.data, _abi.c_f32p))


def run(lib, func, g, alias):
    """The reference on a case's operands -> the dict mat_solve_ref.run returns."""
    if func == "inverse":
        s = g["src"].copy()
        d = mr.marked(s.shape)
        st = lib.arm_mat_inverse_f32(C.byref(inst(s)), C.byref(inst(d)))
        return {"status": st, "src_after": s, "dst": d}
    if func == "cholesky":
        s = g["src"].copy()
        d = s if alias else mr.marked(s.shape)
        st = lib.arm_mat_cholesky_f32(C.byref(inst(s)), C.byref(inst(d)))
        return {"status": st, "dst": d}
    if func == "ldlt":
        s = g["src"].copy()
        l, d = mr.marked(s.shape), mr.marked(s.shape)
        pp = np.full(s.shape[0], mr.MARK16, dtype=np.uint16)
        st = lib.arm_mat_ldlt_f32(C.byref(inst(s)), C.byref(inst(l)), C.byref(inst(d)), pp.ctypes.data)
        assert s.tobytes() == g["src"].tobytes()
        return {"status": st, "l": l, "d": d, "pp": pp}
    t, a = g["t"].copy(), g["a"].copy()
    x = a if alias else mr.marked(a.shape)
    fn = lib.arm_mat_solve_lower_triangular_f32 if func == "solve_lower" else lib.arm_mat_solve_upper_triangular_f32
    st = fn(C.byref(inst(t)), C.byref(inst(a)), C.byref(inst(x)))
    return {"status": st, "dst": x}


def operands(func, case, rng):
    """The operands of a case named as mat_solve_ref.case_names does."""
    alias = case.startswith("alias_")
    name = case[len("alias_"):] if alias else case
    kind, size = name.rsplit("_", 1)
    if func.startswith("solve"):
        n, cols = (int(v) for v in size.split("x"))
        t = mr.failing(func, kind, n, rng) if kind in mr.FAILS[func] else mr.fill(func[len("solve_"):], n, rng)
        return {"t": t, "a": mr.rhs(n, cols, rng)}, alias
    n = int(size)
    if kind == "nonfinite":
        return {"src": mr.nonfinite(func, rng)}, alias
    if kind in mr.FAILS[func]:
        return {"src": mr.failing(func, kind, n, rng)}, alias
    return {"src": mr.fill(kind, n, rng)}, alias


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    args = ap.parse_args()
    rng = np.random.default_rng(SEED)
    data, index, seen = {}, [], {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(args.ref, tmp)
        for func in mr.FUNCS:
            for case in mr.case_names(func):
                g, alias = operands(func, case, rng)
                got = run(lib, func, g, alias)
                want = mr.run(func, g, alias)
                nonfinite = case.startswith("nonfinite")
                for k, v in got.items():
                    if k == "status":
                        assert v == want[k], (func, case, v, want[k])
                    else:
                        assert mr.same_words(v, want[k], nonfinite), (func, case, k)
                key = f"{func}/{case}/"
                for k, v in {**g, **got}.items():
                    data[key + k] = np.int32(v) if k == "status" else v
                index.append([func, case])
                seen.setdefault((func, int(got["status"])), []).append(case)
    for (func, st), cases in sorted(seen.items()):
        print(f"{func}: status {st}: {len(cases)} cases")
    data["index"] = np.array(json.dumps(index))
    path = os.path.join(ROOT, "tests", "golden", "mat_solve.npz")
    np.savez_compressed(path, **data)
    print("wrote", len(index), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
