"""numpy / Python-int restatement of the basic math functions (the reference's scalar branches built with
-D__GNUC_PYTHON__ -DARM_MATH_LOOPUNROLL -ffp-contract=off, no ARM_MATH_DSP) and the case list of
tests/golden/basic_math.npz.  Element-wise functions take [..., n] arrays and return {"dst": [..., n]}; the dot
products return {"value": [...]}, one word per item.

  f32     a + b, a - b, a * b, x + offset, x * scale; abs clears the sign bit, negate flips it; dot_prod is one chain
          sum = sum + a*b in element order from 0.0f, the product rounded before the add.
  q31     add / sub / offset: the exact sum clipped to 32 bits.  mult: clip((a*b) >> 32 to 31 bits) << 1.  scale: in =
          (x * scaleFract) >> 32, k = shift + 1; k >= 0: out = wrap32(in << k), and 0x7FFFFFFF ^ (in >> 31) where
          (out >> k) != in; k < 0: in >> -k.  shift: the same on x with k = shiftBits.  dot_prod: the sum of
          (a*b) >> 14 mod 2^64.
  q15     clip16 of a + b, a - b, (a*b) >> 15, x + offset, (x * scaleFract) >> (15 - shift).  shift left:
          clip16(wrap32(x << s)); right: x >> -s.  dot_prod: the exact sum (int64).
  q7      as q15 with 8 bits, (a*b) >> 7 and (x * scaleFract) >> (7 - shift); dot_prod: a 32-bit sum.
  abs / negate of the most negative word give the most positive.  clip: x > high ? high : x < low ? low : x.
  u32 / u16 / u8   and, or, xor, not.

in_contract(func, a, b, scalars) says whether the reference's C is defined for the call: the shift counts below 32
either way on its promoted int operands (shift_*: -31 .. 31; scale_q31: -32 .. 30; scale_q15: -16 .. 15; scale_q7:
-24 .. 7), and the signed sums of dot_prod_q31 / _q15 (64 bits) and dot_prod_q7 (32 bits) inside their type after
every term.
"""
import zlib

import numpy as np

import cmplx_math_ref as cm

TYPES = ("f32", "q31", "q15", "q7")
BITS_TYPES = ("u32", "u16", "u8")
DT = dict(cm.DT, u32=np.uint32, u16=np.uint16, u8=np.uint8)
MDT = dict(cm.MDT, u16=np.uint16, u8=np.uint8)
MARK = dict(cm.MARK, u16=np.uint16(0x5A5A), u8=np.uint8(0x5A))
TWO = ("add", "sub", "mult", "and", "or", "xor")
DOT_OUT = {"f32": "f32", "q31": "q63", "q15": "q63", "q7": "q31"}
SHIFT_RANGE = {"shift_q31": (-31, 31), "shift_q15": (-31, 31), "shift_q7": (-31, 31), "scale_q31": (-32, 30),
               "scale_q15": (-16, 15), "scale_q7": (-24, 7)}
FLT_MAX = np.float32(3.4028234663852886e38)

FUNCS = tuple(f"{op}_{t}" for op in ("add", "sub", "mult", "offset", "scale") for t in TYPES) + \
    tuple(f"shift_{t}" for t in TYPES[1:]) + \
    tuple(f"{op}_{t}" for op in ("clip", "abs", "negate") for t in TYPES) + \
    tuple(f"{op}_{t}" for op in ("and", "or", "xor", "not") for t in BITS_TYPES) + \
    tuple(f"dot_prod_{t}" for t in TYPES)


def split(func):
    """"dot_prod_q15" -> ("dot_prod", "q15")."""
    op, t = func.rsplit("_", 1)
    return op, t


def is_dot(func):
    return func.startswith("dot_prod_")


def two_sources(func):
    return is_dot(func) or split(func)[0] in TWO


def result_type(func):
    op, t = split(func)
    return DOT_OUT[t] if op == "dot_prod" else t


def n_scalars(func):
    op, t = split(func)
    return {"offset": 1, "scale": 1 if t == "f32" else 2, "shift": 1, "clip": 2}.get(op, 0)


def marked(t, shape):
    return np.full(shape, MARK[t], dtype=MDT[t])


def _wrap32(x):
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31


def _sat(x, bits):
    return np.clip(x, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)


def _shl_q31(v, k):
    """The reference's saturating left shift of int32 words (int64 array) by 0 <= k <= 31."""
    out = _wrap32(v << k)
    return np.where((out >> k) != v, 0x7FFFFFFF ^ (v >> 31), out)


def _elementwise(op, t, a, b, scalars):
    if t in BITS_TYPES:
        return {"and": lambda: a & b, "or": lambda: a | b, "xor": lambda: a ^ b, "not": lambda: ~a}[op]()
    if op == "clip":
        low, high = (DT[t](v) for v in scalars)
        with np.errstate(invalid="ignore"):
            return np.where(a > high, high, np.where(a < low, low, a))
    if t == "f32":
        with np.errstate(all="ignore"):
            if op in ("offset", "scale"):
                s = np.float32(scalars[0])
                return a + s if op == "offset" else a * s
            return {"add": lambda: a + b, "sub": lambda: a - b, "mult": lambda: a * b, "abs": lambda: np.abs(a),
                    "negate": lambda: -a}[op]()
    bits = {"q31": 32, "q15": 16, "q7": 8}[t]
    x = a.astype(np.int64)
    y = b.astype(np.int64) if b is not None else None
    if op == "add":
        return _sat(x + y, bits)
    if op == "sub":
        return _sat(x - y, bits)
    if op == "offset":
        return _sat(x + int(scalars[0]), bits)
    if op == "abs":
        return np.where(x > 0, x, _sat(-x, bits))
    if op == "negate":
        return _sat(-x, bits)
    if op == "mult":
        if t == "q31":
            return _wrap32(_sat((x * y) >> 32, 31) << 1)
        return _sat((x * y) >> (bits - 1), bits)
    if op == "scale":
        frac, shift = int(scalars[0]), int(scalars[1])
        if t == "q31":
            # Python ints: x * frac needs 63 bits, which int64 holds
            v, k = (x * frac) >> 32, shift + 1
            return _shl_q31(v, k) if k >= 0 else v >> -k
        return _sat((x * frac) >> (bits - 1 - shift), bits)
    s = int(scalars[0])                                     # shift
    if s < 0:
        return x >> -s
    return _shl_q31(x, s) if t == "q31" else _sat(_wrap32(x << s), bits)


def _dot(t, a, b):
    """[items, n] -> [items]."""
    if t == "f32":
        acc = np.zeros(a.shape[0], dtype=np.float32)
        with np.errstate(all="ignore"):
            p = a * b
            for k in range(a.shape[1]):
                acc = acc + p[:, k]
        return acc
    x, y = a.astype(np.int64), b.astype(np.int64)
    p = (x * y) >> 14 if t == "q31" else x * y
    with np.errstate(over="ignore"):
        return p.sum(axis=1, dtype=np.int64)                # mod 2^64; q7: the low 32 bits are taken by the cast


def run(func, a, b=None, scalars=()):
    """The restated function on [..., n] operands."""
    op, t = split(func)
    a = np.asarray(a)
    if op == "dot_prod":
        flat = a.reshape(-1, a.shape[-1])
        fb = np.broadcast_to(np.asarray(b), a.shape).reshape(flat.shape)
        v = _dot(t, flat, fb)
        if t == "q7":
            v = _wrap32(v)
        return {"value": np.asarray(v).astype(MDT[DOT_OUT[t]]).reshape(a.shape[:-1])}
    return {"dst": np.asarray(_elementwise(op, t, a, None if b is None else np.asarray(b), scalars)).astype(DT[t])}


def in_contract(func, a=None, b=None, scalars=()):
    op, t = split(func)
    if func in SHIFT_RANGE:
        lo, hi = SHIFT_RANGE[func]
        return lo <= int(scalars[-1]) <= hi
    if op != "dot_prod" or t == "f32":
        return True
    x, y = np.asarray(a).astype(np.int64).reshape(-1), np.asarray(b).astype(np.int64).reshape(-1)
    terms = (x * y) >> 14 if t == "q31" else x * y
    bits = 32 if t == "q7" else 64
    # exact prefix sums: at most 2^62 per term, so Python ints where int64 could wrap
    if terms.size and int(np.abs(terms).max()) * terms.size < 2 ** 62:
        pre = np.cumsum(terms)
        return bool(((pre >= -(1 << (bits - 1))) & (pre < (1 << (bits - 1)))).all())
    s = 0
    for v in terms.tolist():
        s += v
        if not -(1 << (bits - 1)) <= s < (1 << (bits - 1)):
            return False
    return True


# ---- the fixture's cases ------------------------------------------------------------------------------
# lengths: every pack width's ragged ends, one tile of the kernel, more than one.  From STORE_MAX on the fixture keeps
# neither operands nor output words: the operands are regenerated by operands() and checked against a recorded CRC,
# the output against the CRC of the reference's output.
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257, 1023, 1025, 4097, 33000)
STORE_MAX = 257
INT_CASES = ("allmin_255", "allmax_255", "minmax_257", "alt_1025", "ext_67")
F32_CASES = ("subnormal_9", "signzero_9", "overflow_9", "nonfinite_9")
COUNT_N = 17                                                # length of the shift / scale count cases


def _int_info(t):
    return np.iinfo(DT[t])


def case_names(func):
    op, t = split(func)
    names = [f"rand_{n}" for n in LENGTHS]
    names += list(F32_CASES if t == "f32" else INT_CASES)
    if func in SHIFT_RANGE:
        lo, hi = SHIFT_RANGE[func]
        names += [f"cnt{c}_{COUNT_N}" for c in range(lo, hi + 1)]
        if op == "scale":
            names += [f"cntmax{c}_{COUNT_N}" for c in range(lo, hi + 1)]
    if op == "clip":
        names += ["clipeq_17", "clipinv_17", "clipext_17"] + (["clipnan_9"] if t == "f32" else [])
    return names


def case_n(case):
    return int(case.rsplit("_", 1)[1])


def stored(case):
    return case_n(case) <= STORE_MAX


def nan_rule(func):
    """f32 outputs are compared by the rule of tests/test_f32_classes.py: NaNs by position, other words by bits."""
    return result_type(func) == "f32"


def _rng(func, case):
    return np.random.default_rng(zlib.crc32(f"basic/{func}/{case}".encode()))


def rand(t, shape, rng):
    """f32: uniform(-1, 1); integers: the full range."""
    if t == "f32":
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    i = np.iinfo(DT[t])
    return rng.integers(i.min, i.max, shape, endpoint=True).astype(DT[t])


def extremes(t, shape, rng):
    i = np.iinfo(DT[t])
    if t in BITS_TYPES:
        return rng.choice(np.array([0, 1, i.max // 2, i.max // 2 + 1, i.max - 1, i.max], dtype=DT[t]), shape)
    return cm.extremes(t, shape, rng)


def count_vector(t, rng):
    """COUNT_N words: 1, -1, the two extremes, 0x4000.., its negative and its neighbours, then random words."""
    i = _int_info(t)
    q = (i.max + 1) // 2
    head = [1, -1, i.min, i.max, q, -q, q - 1, q + 1, 0, 2, -2, 3]
    v = rand(t, COUNT_N, rng)
    v[:len(head)] = np.array(head, dtype=np.int64).astype(DT[t])
    return v


def rand_scalars(func, rng):
    """Random in-contract scalars of a call."""
    op, t = split(func)
    if op == "offset" or (op == "scale" and t == "f32"):
        return (float(rand(t, 1, rng)[0]),) if t == "f32" else (int(rand(t, 1, rng)[0]),)
    if op == "scale":
        lo, hi = SHIFT_RANGE[func]
        return (int(rand(t, 1, rng)[0]), int(rng.integers(max(lo, -3), min(hi, 3), endpoint=True)))
    if op == "shift":
        return (int(rng.integers(-3, 3, endpoint=True)),)
    if op == "clip":
        if t == "f32":
            return (-0.5, 0.25)
        i = _int_info(t)
        return (int(i.min // 3), int(i.max // 2))
    return ()


def operands(func, case):
    """{"a", "b", "scalars"} of one case, the same words on every call."""
    rng = _rng(func, case)
    op, t = split(func)
    kind, n = case.rsplit("_", 1)
    n = int(n)
    a, b = rand(t, n, rng), rand(t, n, rng)
    scalars = rand_scalars(func, rng)
    if t != "f32":
        i = _int_info(t)
        even = np.arange(n) % 2 == 0
        if kind == "allmin":
            a[:], b[:] = i.min, i.min
        elif kind == "allmax":
            a[:], b[:] = i.max, i.max
        elif kind == "minmax":
            a[:], b[:] = i.min, i.max
        elif kind == "alt":                                 # alternating signs, opposite in b
            a, b = np.where(even, i.min, i.max).astype(DT[t]), np.where(even, i.max, i.min).astype(DT[t])
        elif kind == "ext":
            a, b = extremes(t, n, rng), extremes(t, n, rng)
        if kind in ("allmin", "allmax", "minmax", "alt", "ext") and t not in BITS_TYPES:
            ext = {"allmin": i.min, "allmax": i.max, "minmax": i.max, "alt": i.min, "ext": -1}[kind]
            if op == "offset":
                scalars = (int(ext),)
            elif op == "scale":
                scalars = (int(ext), 0)
            elif op == "shift":
                scalars = (1 if kind != "alt" else -1,)
        if kind.startswith("cnt"):
            a = count_vector(t, rng)
            c = int(kind[6:] if kind.startswith("cntmax") else kind[3:])
            frac = i.max if kind.startswith("cntmax") else (i.max + 1) // 2
            scalars = (c,) if op == "shift" else (int(frac), c)
        if kind == "clipeq":
            scalars = (int(i.max // 5), int(i.max // 5))
        elif kind == "clipinv":
            scalars = (int(i.max // 2), int(i.min // 2))
        elif kind == "clipext":
            a, scalars = extremes(t, n, rng), (int(i.min), int(i.max))
    else:
        if kind == "subnormal":
            k = rng.integers(-149, -130, n, endpoint=True)
            a = (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** k).astype(np.float32)
            b = (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** k).astype(np.float32)
            if op in ("mult", "dot_prod"):                  # products that stay subnormal
                b = rng.uniform(0.25, 1.0, n).astype(np.float32)
            scalars = {"offset": (float(np.float32(2.0 ** -140)),), "scale": (0.5,),
                       "clip": (float(np.float32(-2.0 ** -135)), float(np.float32(2.0 ** -140)))}.get(op, ())
        elif kind == "signzero":
            z = np.array([0.0, -0.0], dtype=np.float32)
            a, b = rng.choice(z, n), rng.choice(z, n)
            if op in ("mult", "dot_prod"):
                b = np.where(np.arange(n) % 2 == 0, np.float32(-1.0), np.float32(2.0)).astype(np.float32)
            scalars = {"offset": (-0.0,), "scale": (-1.0,), "clip": (-0.0, 0.0)}.get(op, ())
        elif kind == "overflow":                            # finite words whose sums and products overflow
            a = (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 3.0e38).astype(np.float32)
            b = np.where(np.arange(n) % 3 == 0, -a, a).astype(np.float32)
            if op == "sub":
                b = -b
            scalars = {"offset": (3.0e38,), "scale": (2.0,), "clip": (float(-FLT_MAX), float(FLT_MAX))}.get(op, ())
        elif kind == "nonfinite":
            a[[0, n // 2, n - 1]] = [np.inf, -np.inf, np.nan]
            b[[1, n // 2, n - 2]] = [np.nan, np.inf, -np.inf]
            scalars = {"offset": (1.0,), "scale": (0.0,), "clip": (-0.5, 0.5)}.get(op, ())
        elif kind == "clipeq":
            scalars = (0.125, 0.125)
        elif kind == "clipinv":
            scalars = (0.5, -0.5)
        elif kind == "clipext":
            a[:4] = [np.inf, -np.inf, FLT_MAX, -FLT_MAX]
            scalars = (float(-FLT_MAX), float(FLT_MAX))
        elif kind == "clipnan":
            a[[0, 4, 8]] = np.nan
            scalars = (-0.5, 0.5)
    out = {"a": np.ascontiguousarray(a), "scalars": tuple(scalars)}
    if two_sources(func):
        out["b"] = np.ascontiguousarray(b)
    return out


def crc(g):
    c = zlib.crc32(repr([float(v) for v in g.get("scalars", ())]).encode())
    for k in ("a", "b"):
        if k in g:
            c = zlib.crc32(np.ascontiguousarray(g[k]).tobytes(), c)
    return c


def out_crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def same_words(got, want, nan_positions=False):
    return cm.same_words(got, want, nan_positions)
