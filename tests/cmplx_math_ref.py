"""numpy restatement of arm_cmplx_{mag,mag_squared,conj,mult_cmplx,mult_real,dot_prod}_{f32,q31,q15} and
arm_{max,min}_{f32,q31,q15,q7} (the reference's scalar branches built with -D__GNUC_PYTHON__
-DARM_MATH_LOOPUNROLL -ffp-contract=off), and the case list of tests/golden/cmplx_math.npz.  Complex vectors are
interleaved (re, im) words; n counts complex samples.

  mag          f32: s = re*re + im*im (each operation rounded), out = sqrtf(s) if s >= 0 else +0.0 (a NaN sum gives
               +0.0).  q31: sqrt_q31((re*re >> 33) + (im*im >> 33)).  q15: sqrt_q31(((u32)re*re + (u32)im*im) >> 1)
               >> 16.  sqrt_q31 is arm_sqrt_q31.c: three Newton steps on 1/sqrt from sqrt_initial_lut_q31, every
               intermediate truncated to int32; 0 for an input <= 0.
  mag_squared  f32: re*re + im*im.  q31: (re*re >> 33) + (im*im >> 33).  q15: (int16)((re*re + im*im) >> 17).
  conj         the imaginary word negated; fixed point: the minimum maps to the maximum; f32: the sign bit flips.
  mult_cmplx   f32: (a*c) - (b*d), (a*d) + (b*c).  q31: each product >> 33, then - / + in int32.  q15: each int32
               product >> 17, the difference / sum truncated to int16 (it cannot leave the range: |x| <= 16384).
  mult_real    f32: x * r.  q15: ssat16((x * r) >> 15).  q31: the int64 product >> 31 clipped to int32.
  dot_prod     f32: re = (re + a*c) - b*d, im = (im + a*d) + b*c, sample by sample from 0.0f (an ordered chain).
               q31: every product >> 14 summed mod 2^64, two int64 results.  q15: exact int64 sums of int32
               products, >> 6, truncated to int32.
  max / min    the result starts at element 0 and is replaced on a strict < / > only: the first index of the
               extreme; a NaN past position 0 is never selected, a NaN at position 0 never replaced.
"""
import os

import numpy as np

from f32_classes import f32_class_input

DT = {"f32": np.float32, "q31": np.int32, "q15": np.int16, "q7": np.int8}
# pre-fill of output buffers: 0x5A in every byte
MARK = {"f32": np.array([0x5A5A5A5A], dtype=np.uint32).view(np.float32)[0], "q31": np.int32(0x5A5A5A5A),
        "q15": np.int16(0x5A5A), "q7": np.int8(0x5A), "q63": np.int64(0x5A5A5A5A5A5A5A5A), "u32": np.uint32(0x5A5A5A5A)}
MDT = dict(DT, q63=np.int64, u32=np.uint32)
CTYPES = ("f32", "q31", "q15")
CMPLX_OPS = ("mag", "mag_squared", "conj", "mult_cmplx", "mult_real", "dot_prod")
FUNCS = tuple(f"cmplx_{op}_{t}" for op in CMPLX_OPS for t in CTYPES) + \
    tuple(f"{op}_{t}" for op in ("max", "min") for t in ("f32", "q31", "q15", "q7"))
DOT_OUT = {"f32": "f32", "q31": "q63", "q15": "q31"}          # the type of arm_cmplx_dot_prod_*'s two results

_LUT = np.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmsis-dsp_amd", "tables",
                                "sqrt_initial_lut_q31.bin"), dtype=np.int32).astype(np.int64)


def split(func):
    """"cmplx_mag_squared_q15" -> ("mag_squared", "q15"); "max_q7" -> ("max", "q7")."""
    op, t = func.rsplit("_", 1)
    return (op[len("cmplx_"):] if op.startswith("cmplx_") else op), t


def marked(t, shape):
    return np.full(shape, MARK[t], dtype=MDT[t])


def _i32(x):
    """int64 array -> its low 32 bits, sign-extended."""
    return ((np.asarray(x, dtype=np.int64) + 2**31) & 0xFFFFFFFF) - 2**31


def sqrt_q31(x):
    """arm_sqrt_q31 on an int64 array of int32 values -> int64 array."""
    x = np.asarray(x, dtype=np.int64)
    pos = x > 0
    v = np.where(pos, x, 1)
    clz = 32 - sum(((v >> k) != 0).astype(np.int64) for k in range(31))
    e = (clz - 1) & ~1                                   # signBits1 rounded down to even
    number = v << e
    var = _LUT[(number >> 26) - (0x20000000 >> 26)]
    for _ in range(3):
        t = _i32((var * var) >> 28)
        t = _i32((number * t) >> 31)
        t = 0x30000000 - t
        var = _i32((var * t) >> 29)
    var = _i32((number * var) >> 28)
    return np.where(pos, var >> (e >> 1), 0)


def _pairs(a):
    a = np.asarray(a)
    return a[..., 0::2], a[..., 1::2]


def _inter(re, im, dt):
    out = np.empty(re.shape[:-1] + (2 * re.shape[-1],), dtype=dt)
    out[..., 0::2], out[..., 1::2] = re, im
    return out


def mag(t, a):
    re, im = _pairs(a)
    if t == "f32":
        with np.errstate(all="ignore"):
            s = re * re + im * im
            return np.where(s >= 0, np.sqrt(s), np.float32(0.0)).astype(np.float32)
    re, im = re.astype(np.int64), im.astype(np.int64)
    if t == "q31":
        return sqrt_q31(((re * re) >> 33) + ((im * im) >> 33)).astype(np.int32)
    return (sqrt_q31(_i32(((re * re + im * im) & 0xFFFFFFFF) >> 1)) >> 16).astype(np.int16)


def mag_squared(t, a):
    re, im = _pairs(a)
    if t == "f32":
        with np.errstate(all="ignore"):
            return re * re + im * im
    re, im = re.astype(np.int64), im.astype(np.int64)
    if t == "q31":
        return (((re * re) >> 33) + ((im * im) >> 33)).astype(np.int32)
    return ((re * re + im * im) >> 17).astype(np.int16)


def conj(t, a):
    re, im = _pairs(a)
    if t == "f32":
        return _inter(re, -im, np.float32)
    i = np.iinfo(DT[t])
    return _inter(re, np.clip(-im.astype(np.int64), i.min, i.max), DT[t])


def mult_cmplx(t, x, y):
    a, b = _pairs(x)
    c, d = _pairs(y)
    if t == "f32":
        with np.errstate(all="ignore"):
            return _inter((a * c) - (b * d), (a * d) + (b * c), np.float32)
    a, b, c, d = (v.astype(np.int64) for v in (a, b, c, d))
    if t == "q31":
        return _inter(_i32(((a * c) >> 33) - ((b * d) >> 33)), _i32(((a * d) >> 33) + ((b * c) >> 33)), np.int32)
    re, im = ((a * c) >> 17) - ((b * d) >> 17), ((a * d) >> 17) + ((b * c) >> 17)
    return _inter(re.astype(np.int16), im.astype(np.int16), np.int16)


def mult_real(t, x, r):
    r2 = np.repeat(np.asarray(r), 2, axis=-1)
    if t == "f32":
        with np.errstate(all="ignore"):
            return x * r2
    p = x.astype(np.int64) * r2.astype(np.int64)
    i = np.iinfo(DT[t])
    return np.clip(p >> (15 if t == "q15" else 31), i.min, i.max).astype(DT[t])


def dot_prod(t, x, y):
    """x, y [..., 2n] -> (re, im) of shape [...]."""
    a, b = _pairs(x)
    c, d = _pairs(y)
    if t == "f32":
        re, im = np.zeros(a.shape[:-1], dtype=np.float32), np.zeros(a.shape[:-1], dtype=np.float32)
        with np.errstate(all="ignore"):
            for k in range(a.shape[-1]):
                re = (re + a[..., k] * c[..., k]) - b[..., k] * d[..., k]
                im = (im + a[..., k] * d[..., k]) + b[..., k] * c[..., k]
        return re, im
    a, b, c, d = (v.astype(np.int64) for v in (a, b, c, d))
    with np.errstate(over="ignore"):
        if t == "q31":
            re = ((a * c) >> 14).sum(axis=-1, dtype=np.int64) - ((b * d) >> 14).sum(axis=-1, dtype=np.int64)
            im = ((a * d) >> 14).sum(axis=-1, dtype=np.int64) + ((b * c) >> 14).sum(axis=-1, dtype=np.int64)
            return re, im
        re = (a * c - b * d).sum(axis=-1, dtype=np.int64)
        im = (a * d + b * c).sum(axis=-1, dtype=np.int64)
    return _i32(re >> 6).astype(np.int32), _i32(im >> 6).astype(np.int32)


def extreme(op, a):
    """a [..., n] -> (value, index uint32): the first index of the maximum / minimum; NaN as the reference's
    strict comparisons treat it."""
    a = np.asarray(a)
    flat = a.reshape(-1, a.shape[-1])
    val, idx = flat[:, 0].copy(), np.zeros(flat.shape[0], dtype=np.uint32)
    for k in range(1, flat.shape[1]):
        x = flat[:, k]
        with np.errstate(invalid="ignore"):
            better = val < x if op == "max" else val > x
        val = np.where(better, x, val)
        idx = np.where(better, np.uint32(k), idx)
    return val.reshape(a.shape[:-1]), idx.reshape(a.shape[:-1])


def run(func, g):
    """The restated function on a case's operands -> the dict of its outputs."""
    op, t = split(func)
    if op in ("mag", "mag_squared", "conj"):
        return {"dst": {"mag": mag, "mag_squared": mag_squared, "conj": conj}[op](t, g["a"])}
    if op == "mult_cmplx":
        return {"dst": mult_cmplx(t, g["a"], g["b"])}
    if op == "mult_real":
        return {"dst": mult_real(t, g["a"], g["r"])}
    if op == "dot_prod":
        re, im = dot_prod(t, g["a"], g["b"])
        return {"re": np.asarray(re, dtype=MDT[DOT_OUT[t]]), "im": np.asarray(im, dtype=MDT[DOT_OUT[t]])}
    v, i = extreme(op, g["a"])
    return {"value": np.asarray(v, dtype=DT[t]), "index": np.asarray(i, dtype=np.uint32)}


def out_spec(func, g):
    """{output name: (type name, shape)} of a call on the operands g (1-D operands: one item)."""
    op, t = split(func)
    a = g["a"]
    if op in ("mag", "mag_squared"):
        return {"dst": (t, a.shape[:-1] + (a.shape[-1] // 2,))}
    if op in ("conj", "mult_cmplx", "mult_real"):
        return {"dst": (t, a.shape)}
    if op == "dot_prod":
        return {"re": (DOT_OUT[t], a.shape[:-1]), "im": (DOT_OUT[t], a.shape[:-1])}
    return {"value": (t, a.shape[:-1]), "index": ("u32", a.shape[:-1])}


# ---- the fixture's cases ------------------------------------------------------------------------------
LENGTHS = (1, 3, 4, 5, 8, 67)
F32_CLASSES = ("subnormal", "signzero", "overflow", "nonfinite")
# max / min: the extreme at index 0, at the last index, in the tail after the 4-unrolled loop (which starts at
# index 1: n = 8 leaves 5, 6, 7), a tie, all-equal input
SEARCH_CASES = ("first_9", "last_9", "tail_8", "tie_9", "equal_6")
SEARCH_F32 = ("pznz_5", "nzpz_5", "nan0_6", "nanmid_6")


def case_names(func):
    op, t = split(func)
    names = [f"rand_{n}" for n in LENGTHS]
    if t == "f32":
        names += [f"{c}_8" for c in F32_CLASSES]
    else:
        names += ["min_5", "max_5", "ext_67"]
        if op == "mult_cmplx" and t == "q15":
            names += ["edge_4"]
    if op in ("max", "min"):
        names += list(SEARCH_CASES) + (list(SEARCH_F32) if t == "f32" else [])
    return names


def rand(t, shape, rng, amp=None):
    """Full-range words (f32: uniform(-1, 1)); amp: fixed point only, |x| <= amp."""
    if t == "f32":
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    i = np.iinfo(DT[t])
    lo, hi = (i.min, i.max) if amp is None else (-amp, amp)
    return rng.integers(lo, hi, shape, endpoint=True).astype(DT[t])


def extremes(t, shape, rng):
    """Fixed-point words drawn from the ends of the range and their neighbours."""
    i = np.iinfo(DT[t])
    return rng.choice(np.array([i.min, i.min + 1, -1, 0, 1, i.max - 1, i.max], dtype=DT[t]), shape)


def _named(op, a, b):
    if op in ("mult_cmplx", "dot_prod"):
        return {"a": a, "b": b}
    if op == "mult_real":
        return {"a": a, "r": np.ascontiguousarray(b[..., 0::2])}
    return {"a": a}


def operands(func, case, rng):
    op, t = split(func)
    kind, n = case.rsplit("_", 1)
    n = int(n)
    search = op in ("max", "min")
    words = n if search else 2 * n
    if kind == "rand":
        a, b = rand(t, words, rng), rand(t, words, rng)
    elif kind in ("min", "max"):
        i = np.iinfo(DT[t])
        a = np.full(words, i.min if kind == "min" else i.max, dtype=DT[t])
        b = a.copy()
    elif kind == "ext":
        a, b = extremes(t, words, rng), extremes(t, words, rng)
    elif kind == "edge":        # q15 mult_cmplx: the largest |difference| and |sum| there are, 16384 and -16384
        a = np.array([-32768, 32767, -32768, -32768, 32767, 32767, -32768, 32767], dtype=np.int16)
        b = np.array([-32768, -32768, 32767, -32768, 32767, -32768, -32768, 32767], dtype=np.int16)
    elif kind in F32_CLASSES:
        pa, pb = ((1, 3, 6), (0, 2, 5)) if search else ((2, 5, 11), (3, 5, 12))
        a = f32_class_input(kind, words, rng, scale=3.0e38 if op in ("max", "min", "conj") else 1.5e19, positions=pa)
        b = f32_class_input(kind, words, rng, scale=1.5e19, positions=pb)
    else:
        lo, hi = (-100, 100) if t == "q7" else (-1000, 1000)
        a = rng.integers(lo, hi, n, endpoint=True).astype(DT[t]) if t != "f32" else rand(t, n, rng)
        peak = DT[t](2 if t == "f32" else hi + 5) if op == "max" else DT[t](-2 if t == "f32" else lo - 5)
        if kind == "first":
            a[0] = peak
        elif kind == "last":
            a[-1] = peak
        elif kind == "tail":
            a[6] = peak
        elif kind == "tie":
            a[[2, 5, 7]] = peak
        elif kind == "equal":
            a[:] = peak
        elif kind in ("pznz", "nzpz"):
            a = np.array([-1.0, 0.0, -0.0, -2.0, 0.0] if kind == "pznz" else [-1.0, -0.0, 0.0, -2.0, -0.0],
                         dtype=np.float32)
            a = a if op == "max" else -a
        elif kind == "nan0":
            a[0] = np.nan
        elif kind == "nanmid":
            a[3] = np.nan
        else:
            raise ValueError(case)
        b = a
    return _named(op, np.ascontiguousarray(a), np.ascontiguousarray(b))


def nan_rule(case):
    """Cases compared by the f32 rule for non-finite inputs (tests/test_f32_classes.py)."""
    return str(case).startswith(("nonfinite", "nan"))


def same_words(got, want, nan_positions=False):
    """Bit equality; nan_positions: non-NaN words bit-equal, NaNs at the same positions."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not nan_positions or got.dtype != np.float32:
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all()) and got.view(np.uint32)[~gn].tobytes() == want.view(np.uint32)[~wn].tobytes()
