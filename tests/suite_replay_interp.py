"""The reference's InterpolationTests{F32,Q31,Q15,Q7} and QuaternionTestsF32 (Testing/Source/Tests/*.cpp, driven by
Testing/desc.txt), restated beside tests/suite_replay.py, whose table (FAMILIES, ROWS) and manifest stay as they are.

A line is one `Test` line of a suite.  run_line() replays it against a "library": the patterns its setUp case loads,
the instance it fills, the call sequence of its test method (the linear and bilinear tests call the one-sample function
once per sample; test_quaternion_prod_single_f32 calls arm_quaternion_product_single_f32 once per quaternion;
test_rotation2quaternion_f32 then makes every real part positive) and the method's ASSERT_* lines with the suite's own
thresholds (TOL).  A library is an object whose arm_* attributes take numpy buffers, C scalars and Inst objects in the
order of arm_math.h.  Three exist: the reference build (tools/make_golden_suites_interp.py) and the GPU library
(tests/test_gpu_suites_interp.py), both through Ctypes, and the numpy restatements (Restatement,
tests/test_suites_interp.py).

Patterns are data: tests/golden/suites_interp.npz, keyed <SuiteClass>/<pattern file stem>, with the reference build's
output words of every line (<line id>/ref_<output>); tests/golden/suites_interp_manifest.json has one entry per `Test`
line.  Output buffers are suite_replay.Out: TAIL marker words follow them, which ASSERT_EMPTY_TAIL wants untouched."""
import json
import os

import numpy as np

import interp_ref as ir
import metrics
import quaternion_ref as qr
import suite_replay as sr

MANIFEST = os.path.join(sr.GOLDEN, "suites_interp_manifest.json")
FIXTURE = os.path.join(sr.GOLDEN, "suites_interp.npz")
SUITES = {"InterpolationTestsF32": "f32", "InterpolationTestsQ31": "q31", "InterpolationTestsQ15": "q15",
          "InterpolationTestsQ7": "q7", "QuaternionTestsF32": "f32"}
# SNR_THRESHOLD and REL_ERROR / ABS_ERROR_<type> / (ABS_ERROR, REL_ERROR) of each suite
TOL = {"InterpolationTestsF32": dict(snr=119, rel=8.0e-5),                   # InterpolationTestsF32.cpp:5,13
       "InterpolationTestsQ31": dict(snr=100, abs=2000),                     # InterpolationTestsQ31.cpp:5,13
       "InterpolationTestsQ15": dict(snr=70, abs=2),                         # InterpolationTestsQ15.cpp:5,13
       "InterpolationTestsQ7": dict(snr=20, abs=2),                          # InterpolationTestsQ7.cpp:5,13
       "QuaternionTestsF32": dict(snr=120, abs=1.0e-7, rel=1.0e-6)}          # QuaternionTestsF32.cpp:5,13-14
SUMMARY = ("The reference's InterpolationTests{F32,Q31,Q15,Q7} and QuaternionTestsF32 are replayed line by line, 19 "
           "lines with the reference's patterns, call sequences and thresholds, against the library on the GPU.")
# test method -> (pattern stems: input(s), reference), the spline tests also (knots, type, queries)
SPLINES = {"test_spline_square_f32": ("3", 4, 1, 20), "test_spline_sine_f32": ("4", 9, 0, 33),
           "test_spline_ramp_f32": ("5", 3, 1, 30)}
QUATERNION = {"test_quaternion_norm_f32": ("arm_quaternion_norm_f32", "Input1", "Reference1"),
              "test_quaternion_inverse_f32": ("arm_quaternion_inverse_f32", "Input1", "Reference2"),
              "test_quaternion_conjugate_f32": ("arm_quaternion_conjugate_f32", "Input1", "Reference3"),
              "test_quaternion_normalize_f32": ("arm_quaternion_normalize_f32", "Input1", "Reference4"),
              "test_quaternion_prod_single_f32": ("arm_quaternion_product_single_f32", "Input1", "Reference5"),
              "test_quaternion_product_f32": ("arm_quaternion_product_f32", "Input1", "Reference5"),
              "test_quaternion2rotation_f32": ("arm_quaternion2rotation_f32", "Input1", "Reference6"),
              "test_rotation2quaternion_f32": ("arm_rotation2quaternion_f32", "Input7", "Reference7")}


def manifest():
    return json.load(open(MANIFEST))


def line_id(e):
    return sr.row_id(e["suite"], e["index"], e["method"], e["label"])


class Inst:
    """An instance structure of arm_math.h: `kind` (linear_f32, bilinear, spline) and its members, arrays included."""

    def __init__(self, kind, **members):
        self.kind = kind
        self.__dict__.update(members)
        self._c = None

    def c(self, abi):
        """The ctypes mirror, made once (the library fills a spline instance in place)."""
        if self._c is None:
            if self.kind == "linear_f32":
                self._c = abi.arm_linear_interp_instance_f32(self.nValues, self.x1, self.xSpacing, self.pYData.ctypes.data)
            elif self.kind == "bilinear":
                self._c = abi.arm_bilinear_interp_instance(self.numRows, self.numCols, self.pData.ctypes.data)
            else:
                self._c = abi.arm_spline_instance_f32()
        return self._c


class Ctypes:
    """arm_* of a ctypes library whose functions carry _abi's argtypes."""

    def __init__(self, lib, abi, after=None):
        self.lib, self.abi, self.after = lib, abi, after

    def __getattr__(self, name):
        import ctypes
        fn = getattr(self.lib, name)

        def call(*args):
            for a in args:
                assert not isinstance(a, np.ndarray) or a.flags["C_CONTIGUOUS"], (name, "a buffer is not contiguous")
            r = fn(*[a.ctypes.data if isinstance(a, np.ndarray) else
                     ctypes.byref(a.c(self.abi)) if isinstance(a, Inst) else a for a in args])
            if self.after:
                self.after(name)
            return r
        return call


class Restatement:
    """tests/interp_ref.py and tests/quaternion_ref.py behind the C signatures."""

    def arm_linear_interp_f32(self, S, x):
        return ir.linear_f32(S.pYData[:S.nValues], S.x1, S.xSpacing, np.array([x], np.float32))[0]

    def arm_bilinear_interp_f32(self, S, X, Y):
        tab = S.pData[:S.numRows * S.numCols].reshape(S.numRows, S.numCols)
        return ir.bilinear_f32(tab, np.array([X], np.float32), np.array([Y], np.float32))[0]

    def arm_spline_init_f32(self, S, t, x, y, n, coeffs, temp):
        S.x, S.y, S.n_x, S.coeffs = x, y, n, coeffs
        coeffs[:3 * (n - 1)], temp[:2 * n - 1] = ir.spline_init(t, x[:n], y[:n])

    def arm_spline_f32(self, S, xq, dst, block):
        n = S.n_x
        dst[:block] = ir.spline_eval(S.x[:n], S.y[:n], S.coeffs[:3 * (n - 1)], xq[:block])

    def arm_quaternion_product_single_f32(self, a, b, r):
        r[:4] = qr.product(a[:4], b[:4])[0]

    def arm_quaternion_product_f32(self, a, b, r, n):
        r[:4 * n] = qr.product(a[:4 * n], b[:4 * n]).reshape(-1)

    def __getattr__(self, name):
        kind = name.rsplit("_", 1)[1]
        if name.startswith("arm_linear_interp_"):
            return lambda tab, x, n: ir.linear_q(kind, tab[:n], np.array([x], np.int32))[0]
        if name.startswith("arm_bilinear_interp_"):
            return lambda S, X, Y: ir.bilinear_q(kind, S.pData[:S.numRows * S.numCols].reshape(S.numRows, S.numCols),
                                                 np.array([X], np.int32), np.array([Y], np.int32))[0]
        func = name[len("arm_"):-len("_f32")]
        wa, wd = qr.WORDS[func]

        def call(src, dst, n):
            dst[:n * wd] = qr.apply(func, src[:n * wa]).reshape(-1)
        return call


def patterns(fixture, suite):
    """{pattern file stem without its type suffix: the words} of a suite."""
    out = {}
    for key in fixture.files:
        if key.startswith(suite + "/") and key.count("/") == 1:
            out[key.split("/")[1].rsplit("_", 1)[0]] = fixture[key]
    return out


def run_line(lib, e, pats):
    """Replays the manifest entry e on the suite's patterns -> ({output name: Out}, [the ASSERT_* lines that fail])."""
    suite, method, t = e["suite"], e["method"], SUITES[e["suite"]]
    tol, fails = TOL[suite], []
    cast = float if t == "f32" else int
    outs = {}
    if suite == "QuaternionTestsF32":
        func, src, refname = QUATERNION[method]
        inp, ref = pats[src], pats[refname]
        out = outs["output"] = sr.Out("f32", ref.size)
        if method == "test_quaternion_norm_f32":
            lib.arm_quaternion_norm_f32(inp, out.words, out.n)
        elif method == "test_quaternion_prod_single_f32":
            for i in range(inp.size >> 2):
                lib.arm_quaternion_product_single_f32(inp[4 * i:], pats["Input2"][4 * i:], out.words[4 * i:])
        elif method == "test_quaternion_product_f32":
            lib.arm_quaternion_product_f32(inp, pats["Input2"], out.words, inp.size >> 2)
        elif method == "test_rotation2quaternion_f32":
            lib.arm_rotation2quaternion_f32(inp, out.words, out.n >> 2)
            q = out.words.reshape(-1, 4)
            q[q[:, 0] < 0] *= np.float32(-1)                 # "Remove ambiguity": the real part positive
        else:
            getattr(lib, func)(inp, out.words, inp.size >> 2)
        if not metrics.close_error(out.words, ref, tol["abs"], tol["rel"]):
            fails.append("ASSERT_CLOSE_ERROR(output,ref,ABS_ERROR,REL_ERROR)")
    elif method in SPLINES:
        k, n, spline_type, block = SPLINES[method]
        ref = pats["Reference" + k][:block]
        out = outs["output"] = sr.Out("f32", ref.size)
        coeffs, temp = outs["splineCoefs"], outs["buffer"] = sr.Out("f32", 3 * (n - 1)), sr.Out("f32", 2 * n - 1)
        S = Inst("spline")
        lib.arm_spline_init_f32(S, spline_type, pats["InputX" + k][:n], pats["InputY" + k][:n], n, coeffs.words,
                                temp.words)
        lib.arm_spline_f32(S, pats["OutputX" + k][:block], out.words, block)
    else:
        bil = method.startswith("test_bilinear")
        inp, ref = pats["Input2" if bil else "Input1"], pats["Reference2" if bil else "Reference1"]
        y = pats["YVals2" if bil else "YVals1"]
        out = outs["output"] = sr.Out(t, ref.size)
        if bil:
            cfg = pats["Config2"]
            S = Inst("bilinear", numRows=int(cfg[1]), numCols=int(cfg[0]), pData=y)
            fn = getattr(lib, f"arm_bilinear_interp_{t}")
            for k in range(inp.size // 2):
                out.words[k] = fn(S, cast(inp[2 * k]), cast(inp[2 * k + 1]))
        elif t == "f32":
            S = Inst("linear_f32", nValues=y.size, x1=0.0, xSpacing=1.0, pYData=y)
            for k in range(inp.size):
                out.words[k] = lib.arm_linear_interp_f32(S, float(inp[k]))
        else:
            fn = getattr(lib, f"arm_linear_interp_{t}")
            for k in range(inp.size):
                out.words[k] = fn(y, int(inp[k]), y.size)
        if t == "f32":
            if not (metrics.rel_error(out.words, ref, tol["rel"]) and metrics.relative_error(out.words, ref, tol["rel"])):
                fails.append("ASSERT_REL_ERROR(output,ref,REL_ERROR)")
        elif not metrics.near_eq(out.words, ref, tol["abs"]):
            fails.append(f"ASSERT_NEAR_EQ(output,ref,ABS_ERROR_{t.upper()})")
    for name, o in outs.items():
        if not o.tail_empty():
            fails.append(f"ASSERT_EMPTY_TAIL({name})")
    scale = {"f32": 1.0, "q31": 2.0 ** -31, "q15": 2.0 ** -15, "q7": 2.0 ** -7}[t]
    if not metrics.snr_passes(ref.astype(np.float64) * scale, outs["output"].words.astype(np.float64) * scale, tol["snr"]):
        fails.append("ASSERT_SNR(output,ref,SNR_THRESHOLD)")
    return outs, fails
