"""numpy / Python-int restatement of the statistics functions (the reference's scalar branches built with
-D__GNUC_PYTHON__ -DARM_MATH_LOOPUNROLL -ffp-contract=off, no ARM_MATH_DSP), of arm_sqrt_q15 and
arm_cmplx_mag_fast_q15, and the case list of tests/golden/statistics.npz.  Every function takes a [..., n] array
and returns one word per item.

  f32     every sum is one chain in element order from 0.0f, each term rounded before the add.  mean: sum / f(n);
          power: terms x*x; rms: sqrt_or_zero(power / f(n)); mse: terms (a-b)*(a-b), sum / f(n); var: the mean first,
          then terms (x-mean)*(x-mean), sum / (f(n) - 1.0f); std: sqrt_or_zero(var); accumulate: the sum.  f(n) is
          (float)n and sqrt_or_zero is arm_sqrt_f32: sqrtf for an input >= 0, otherwise (a NaN too) +0.0.  n <= 1
          gives 0 in var / std.
  q31     mean: trunc(sum / n).  power: sum of x*x >> 14 (int64).  rms: sqrt_q31(clip((sum of x*x mod 2^64, unsigned,
          // n) >> 31)).  mse: d = sat32((a >> 1) - (b >> 1)), sum of d*d >> 14, (int32)((sum / n) >> 15).  var: in =
          x >> 8, (trunc(sumsq / (n-1)) - trunc(sum*sum / u32(n*(n-1)))) >> 15, truncated to int32; std: its sqrt_q31.
  q15     mean: trunc(sum / n) (a 32-bit sum).  power: sum of x*x (int64).  rms: sqrt_q15(sat16((sum // n) >> 15)).
          mse: d = sat16((a >> 1) - (b >> 1)), sat16((sum of d*d / n) >> 13).  var: (i32(trunc(sumsq / (n-1))) -
          i32(trunc(sum*sum / u32(n*(n-1))))) >> 15, truncated to int16; std: sqrt_q15 of its saturation.  u32(n*(n-1))
          wraps from n = 65537 on.
  q7      mean: trunc(sum / n).  power: sum of x*x (int32).  mse: d = sat8((a >> 1) - (b >> 1)), sat8(i16(sum // n)
          >> 5).
  abs     (x > 0) ? x : -x, saturating in fixed point; f32: +0.0 -> -0.0, a NaN has its sign flipped.
  search  max / min of cmplx_math_ref.extreme (start at element 0, strict comparison, first index); _no_idx drops
          the index, except max_no_idx_f32 / min_no_idx_f32, which start from -FLT_MAX / FLT_MAX.
  sqrt_q15          arm_sqrt_q15.c: Newton on 1/sqrt, three steps from SQRT_Q15_LUT, every intermediate truncated to
                    int16; 0 for an input <= 0.  SQRT_Q15_LUT[k] = round(2^13 / sqrt(1 + k/4)).
  cmplx_mag_fast_q15   sqrt_q15((re*re + im*im) >> 17).

in_contract(func, a, b) says, in exact integers, whether every signed intermediate of the reference stays inside its
type for these operands; outside, the reference is undefined and no fixture is recorded.
"""
import math
import zlib

import numpy as np

import cmplx_math_ref as cm

DT, MDT, MARK = cm.DT, cm.MDT, cm.MARK
TYPES = ("f32", "q31", "q15", "q7")
SUM_OPS = ("mean", "power", "rms", "var", "std", "mse", "accumulate")
SEARCH_IDX = ("absmax", "absmin")
SEARCH_NO_IDX = ("max_no_idx", "min_no_idx", "absmax_no_idx", "absmin_no_idx")


def _types_of(op):
    if op == "accumulate":
        return ("f32",)
    return ("f32", "q31", "q15") if op in ("rms", "var", "std") else TYPES


STAT_FUNCS = tuple(f"{op}_{t}" for op in SUM_OPS + SEARCH_IDX + SEARCH_NO_IDX for t in _types_of(op))
FUNCS = STAT_FUNCS + ("cmplx_mag_fast_q15",)
POWER_OUT = {"f32": "f32", "q31": "q63", "q15": "q63", "q7": "q31"}
FLT_MAX = np.float32(3.4028234663852886e38)
SQRT_Q15_LUT = np.array([int(round(2.0 ** 13 / math.sqrt(1.0 + k / 4.0))) for k in range(16)], dtype=np.int64)


def split(func):
    """"absmax_no_idx_q7" -> ("absmax_no_idx", "q7")."""
    op, t = func.rsplit("_", 1)
    return op, t


def result_type(func):
    op, t = split(func)
    return POWER_OUT[t] if op == "power" else t


def has_index(func):
    return split(func)[0] in SEARCH_IDX


def two_sources(func):
    return split(func)[0] == "mse"


def _wrap(x, bits):
    """A Python int -> its low `bits` bits, sign-extended."""
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def _sat(x, bits):
    return max(-(1 << (bits - 1)), min((1 << (bits - 1)) - 1, x))


def _tdiv(a, b):
    """C division of Python ints: truncated toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def sqrt_q15(x):
    """arm_sqrt_q15 on an int array of int16 values -> int64 array."""
    x = np.asarray(x, dtype=np.int64)
    pos = x > 0
    v = np.where(pos, x, 1)
    clz = 32 - sum(((v >> k) != 0).astype(np.int64) for k in range(16))
    e = (clz - 17) & ~1                                   # signBits1 rounded down to even
    number = v << e
    i16 = lambda y: ((y + 2 ** 15) & 0xFFFF) - 2 ** 15    # noqa: E731
    var = SQRT_Q15_LUT[(number >> 11) - (0x2000 >> 11)]
    for _ in range(3):
        t = i16((var * var) >> 12)
        t = i16((number * t) >> 15)
        t = i16(0x3000 - t)
        var = i16((var * t) >> 13)
    var = i16((number * var) >> 12)
    return np.where(pos, var >> (e >> 1), 0)


def sqrt_q15_status(x):
    return np.where(np.asarray(x, dtype=np.int64) >= 0, 0, -1)


def cmplx_mag_fast_q15(a):
    re, im = a[..., 0::2].astype(np.int64), a[..., 1::2].astype(np.int64)
    return sqrt_q15((re * re + im * im) >> 17).astype(np.int16)


def _sqrt_or_zero(v):
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, np.sqrt(np.where(v >= 0, v, 0).astype(np.float32)), np.float32(0.0)).astype(np.float32)


def _chain(terms):
    """[items, n] float32 -> the ordered sums [items]."""
    acc = np.zeros(terms.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(terms.shape[1]):
            acc = acc + terms[:, k]
    return acc


def _sum_f32(op, a, b):
    n = a.shape[1]
    fn = np.float32(n)
    with np.errstate(all="ignore"):
        if op in ("var", "std"):
            if n <= 1:
                return np.zeros(a.shape[0], dtype=np.float32)
            mean = _chain(a) / fn
            d = a - mean[:, None]
            v = _chain(d * d) / np.float32(fn - np.float32(1.0))
            return v if op == "var" else _sqrt_or_zero(v)
        if op in ("mean", "accumulate"):
            s = _chain(a)
            return s if op == "accumulate" else s / fn
        if op == "mse":
            d = a - b
            return _chain(d * d) / fn
        s = _chain(a * a)
        return s if op == "power" else _sqrt_or_zero(s / fn)


def _sums_int(op, t, a, b):
    """[items, n] fixed-point operands -> the int64 sums [items] the epilogue needs (exact inside the contract;
    rms_q31: mod 2^64, as the reference's unsigned sum)."""
    x = a.astype(np.int64)
    zero = np.zeros(x.shape[0], dtype=np.int64)
    if op == "mean":
        return x.sum(axis=1), zero
    if op == "power":
        return ((x * x) >> (14 if t == "q31" else 0)).sum(axis=1), zero
    if op == "rms":
        with np.errstate(over="ignore"):
            return (x * x).astype(np.uint64).sum(axis=1, dtype=np.uint64), zero
    if op == "mse":
        i = np.iinfo(DT[t])
        d = np.clip((x >> 1) - (b.astype(np.int64) >> 1), i.min, i.max)
        return ((d * d) >> (14 if t == "q31" else 0)).sum(axis=1), zero
    v = x >> 8 if t == "q31" else x                       # var, std
    return v.sum(axis=1), (v * v).sum(axis=1)


def _finish_int(op, t, n, s0, s1):
    """The reference's epilogue on one item's sums (Python ints) -> the result word as a Python int."""
    bits = {"q31": 32, "q15": 16, "q7": 8}[t]
    if op == "mean":
        return _wrap(_tdiv(s0 if t == "q31" else _wrap(s0, 32), n), bits)
    if op == "power":
        return _wrap(s0, 32 if t == "q7" else 64)
    if op == "rms":
        if t == "q31":
            return int(cm.sqrt_q31(np.array([min((s0 // n) >> 31, 2 ** 31 - 1)]))[0])
        return int(sqrt_q15(np.array([_sat((s0 // n) >> 15, 16)]))[0])
    if op == "mse":
        if t == "q31":
            return _wrap((s0 // n) >> 15, 32)
        if t == "q15":
            return _sat(_wrap(s0 // n, 32) >> 13, 16)
        return _sat(_wrap(_wrap(s0, 32) // n, 16) >> 5, 8)
    if n <= 1:                                            # var, std
        return 0
    den = (n * (n - 1)) & 0xFFFFFFFF
    if t == "q31":
        d = _wrap((_wrap(_tdiv(s1, n - 1), 64) - _wrap(_tdiv(_wrap(s0 * s0, 64), den), 64)) >> 15, 32)
        return d if op == "var" else int(cm.sqrt_q31(np.array([d]))[0])
    s = _wrap(s0, 32)
    d = _wrap(_wrap(_tdiv(s1, n - 1), 32) - _wrap(_tdiv(s * s, den), 32), 32) >> 15
    return _wrap(d, 16) if op == "var" else int(sqrt_q15(np.array([_sat(d, 16)]))[0])


def in_contract(func, a, b=None):
    """No signed intermediate of the reference leaves its type (one item, exact integers)."""
    op, t = split(func)
    if t == "f32" or op not in SUM_OPS:
        return True
    a = [int(x) for x in np.asarray(a).reshape(-1)]
    b = [int(x) for x in np.asarray(b).reshape(-1)] if b is not None else None
    n = len(a)

    def prefixes_fit(terms, bits):
        s = 0
        for v in terms:
            s += v
            if not -(1 << (bits - 1)) <= s < (1 << (bits - 1)):
                return False
        return True

    if n == 0:
        return op in ("power", "var", "std")
    if op == "mean":
        return prefixes_fit(a, 64 if t == "q31" else 32)
    if op == "power":
        return prefixes_fit([(x * x) >> 14 for x in a] if t == "q31" else [x * x for x in a], 32 if t == "q7" else 64)
    if op == "rms":
        return t == "q31" or prefixes_fit([x * x for x in a], 64)
    if op == "mse":
        bits = {"q31": 32, "q15": 16, "q7": 8}[t]
        d = [_sat((x >> 1) - (y >> 1), bits) for x, y in zip(a, b)]
        return prefixes_fit([(v * v) >> 14 for v in d] if t == "q31" else [v * v for v in d], 32 if t == "q7" else 64)
    if n <= 1:
        return True
    den = (n * (n - 1)) & 0xFFFFFFFF
    if t == "q31":
        v = [x >> 8 for x in a]
        s = sum(v)
        if not (prefixes_fit(v, 64) and prefixes_fit([x * x for x in v], 64) and abs(s * s) < 2 ** 63):
            return False
        return abs(_tdiv(sum(x * x for x in v), n - 1) - _tdiv(s * s, den)) < 2 ** 63
    if not (prefixes_fit(a, 32) and prefixes_fit([x * x for x in a], 64)):
        return False
    s = sum(a)
    return abs(_wrap(_tdiv(sum(x * x for x in a), n - 1), 32) - _wrap(_tdiv(s * s, den), 32)) < 2 ** 31


def absmap(t, a):
    a = np.asarray(a)
    if t == "f32":
        with np.errstate(invalid="ignore"):
            return np.where(a > 0, a, -a).astype(np.float32)
    i = np.iinfo(DT[t])
    w = a.astype(np.int64)
    return np.where(w > 0, w, np.minimum(-w, i.max)).astype(DT[t])


def run(func, a, b=None):
    """The restated function on [..., n] operands -> {"value": [...]} and, for absmax / absmin, "index"."""
    if func == "cmplx_mag_fast_q15":
        return {"value": cmplx_mag_fast_q15(np.asarray(a))}
    op, t = split(func)
    a = np.asarray(a)
    lead = a.shape[:-1]
    flat = a.reshape(-1, a.shape[-1])
    fb = np.asarray(b).reshape(flat.shape) if b is not None else None
    rt = MDT[result_type(func)]
    if op in SUM_OPS:
        if t == "f32":
            v = _sum_f32(op, flat, fb)
        else:
            n = flat.shape[1]
            if n == 0 and op in ("mean", "rms", "mse"):
                raise ZeroDivisionError(func)
            s0, s1 = _sums_int(op, t, flat, fb)
            v = np.array([_finish_int(op, t, n, int(s0[i]), int(s1[i])) for i in range(flat.shape[0])], dtype=object)
            v = np.array([int(w) & 0xFFFFFFFFFFFFFFFF for w in v], dtype=np.uint64).view(np.int64)
        return {"value": np.asarray(v).astype(rt).reshape(lead)}
    if op in ("max_no_idx", "min_no_idx") and t == "f32":
        best = np.full(flat.shape[0], -FLT_MAX if op == "max_no_idx" else FLT_MAX, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            for k in range(flat.shape[1]):
                x = flat[:, k]
                best = np.where(best < x if op == "max_no_idx" else best > x, x, best)
        return {"value": best.reshape(lead)}
    src = absmap(t, flat) if op.startswith("abs") else flat
    v, i = cm.extreme("max" if "max" in op else "min", src)
    out = {"value": np.asarray(v, dtype=DT[t]).reshape(lead)}
    if has_index(func):
        out["index"] = np.asarray(i, dtype=np.uint32).reshape(lead)
    return out


# ---- the fixture's cases ------------------------------------------------------------------------------
# item lengths at which the kernels change path; from STORE_MAX on the fixture keeps no operands (they are
# regenerated by operands() and checked against a recorded CRC)
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 257, 1023, 1025, 4097, 33000)
STORE_MAX = 257
F32_CASES = ("zeros_8", "pzero_5", "subnormal_9", "overflow_9", "nanfirst_9", "nanmid_9", "nanlast_9", "inffirst_9",
             "infmid_9", "inflast_9", "neginf_6", "posinf_6", "const_9")
INT_CASES = ("allmin_255", "allmax_255", "const_9", "negmean_3", "negmean_7", "ext_67")


def case_names(func):
    if func == "cmplx_mag_fast_q15":
        return [f"rand_{n}" for n in (1, 3, 4, 5, 8, 67, 1025)] + ["allmin_5", "allmax_5", "ext_67"]
    op, t = split(func)
    names = [f"rand_{n}" for n in LENGTHS]
    names += list(F32_CASES if t == "f32" else INT_CASES)
    if op == "mse":
        names += ["opposite_17"]
    if op in ("var", "std") and t == "q15":
        names += ["wrap_65537"]
    if op.startswith("abs"):
        names += ["abstie_9", "abstie2_300"] + (["abssat_9"] if t != "f32" else [])
    return names


def case_n(case):
    return int(case.rsplit("_", 1)[1])


def stored(case):
    return case_n(case) <= STORE_MAX


def nan_rule(func):
    """f32 results are compared by the rule of tests/test_f32_classes.py: NaNs by position, other words by bits."""
    return result_type(func) == "f32"


def _rng(func, case):
    return np.random.default_rng(zlib.crc32(f"{func}/{case}".encode()))


def rand(t, shape, rng, amp_shift=0):
    """f32: uniform(-1, 1); fixed point: the full range >> amp_shift."""
    if t == "f32":
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    i = np.iinfo(DT[t])
    return rng.integers(i.min >> amp_shift, i.max >> amp_shift, shape, endpoint=True).astype(DT[t])


def amp_shift(func, n):
    """Random fixed-point items stay inside the reference's contract: q31 var / std from 1023 words on at amplitude
    2^-4 (sum * sum inside 64 bits), var / std_q15 at 65537 words at 2^-2 (the 32-bit sum)."""
    op, t = split(func) if func != "cmplx_mag_fast_q15" else ("", "q15")
    if op in ("var", "std") and t == "q31" and n >= 1023:
        return 4
    if op in ("var", "std") and t == "q15" and n >= 65537:
        return 2
    return 0


def operands(func, case):
    """{"a": ..., "b": ...} of one case, the same words on every call."""
    rng = _rng(func, case)
    kind, n = case.rsplit("_", 1)
    n = int(n)
    if func == "cmplx_mag_fast_q15":
        op, t, words = "mag_fast", "q15", 2 * n
    else:
        (op, t), words = split(func), n
    dt = DT[t]
    sh = amp_shift(func, n)
    a, b = rand(t, words, rng, sh), rand(t, words, rng, sh)
    if t != "f32":
        i = np.iinfo(dt)
        if kind == "allmin":
            a[:], b[:] = i.min, i.max
        elif kind == "allmax":
            a[:], b[:] = i.max, i.min
        elif kind == "const":
            a[:], b[:] = i.max // 26, i.max // 26
        elif kind == "negmean":
            a = np.array([-10, -3, 0] if n == 3 else [-1, -1, -1, -1, -1, 0, 0], dtype=dt)
            b = np.zeros(n, dtype=dt)
        elif kind == "ext":
            a, b = cm.extremes(t, words, rng), cm.extremes(t, words, rng)
        elif kind == "opposite":                            # a = -b at the extremes
            a = np.where(np.arange(n) % 2 == 0, i.min, i.max).astype(dt)
            b = np.where(np.arange(n) % 2 == 0, i.max, i.min).astype(dt)
        elif kind == "abssat":                              # |min| saturates to max: a tie with max, the first wins
            a = rand(t, n, rng, 2)
            if "max" in op:
                a[2], a[5] = i.min, i.max
            else:
                a[:] = i.max
                a[2], a[5] = i.min, i.max - 1
    else:
        if kind == "zeros":
            a, b = rng.choice(np.array([0.0, -0.0], dtype=np.float32), n), np.zeros(n, dtype=np.float32)
        elif kind == "pzero":
            a, b = np.zeros(n, dtype=np.float32), -np.zeros(n, dtype=np.float32)
        elif kind == "subnormal":
            k = rng.integers(-149, -130, n, endpoint=True)
            a = (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** k).astype(np.float32)
            b = (a * np.float32(0.5)).astype(np.float32)
        elif kind == "overflow":                            # finite words whose sum (and squares) overflow
            a = (rng.uniform(0.5, 1.0, n) * 3.0e38).astype(np.float32)
            b = -a
        elif kind in ("nanfirst", "nanmid", "nanlast", "inffirst", "infmid", "inflast"):
            pos = {"first": 0, "mid": n // 2, "last": n - 1}[kind[3:]]
            a[pos] = np.nan if kind.startswith("nan") else (np.inf if pos != n // 2 else -np.inf)
        elif kind == "neginf":
            a[:] = -np.inf
        elif kind == "posinf":
            a[:] = np.inf
        elif kind == "const":
            a[:], b[:] = np.float32(0.3), np.float32(0.3)
    if kind in ("abstie", "abstie2"):                       # |x| equal at two indices with opposite signs
        first, second = (2, 5) if n == 9 else (70, 263)
        if t == "f32":
            peak = np.float32(3.0 if "max" in op else 2.0 ** -20)
        else:
            peak = dt(np.iinfo(dt).max - 3 if "max" in op else 1)
            if "min" in op:
                a = np.where(np.abs(a.astype(np.int64)) < 2, dt(5), a).astype(dt)
            else:
                a = np.clip(a, -(int(peak) - 1), int(peak) - 1).astype(dt)
        a[first], a[second] = -peak, peak
    out = {"a": np.ascontiguousarray(a)}
    if func != "cmplx_mag_fast_q15" and op == "mse":
        out["b"] = np.ascontiguousarray(b)
    return out


def crc(g):
    c = 0
    for k in sorted(g):
        c = zlib.crc32(np.ascontiguousarray(g[k]).tobytes(), c)
    return c


def same_words(got, want, nan_positions=False):
    return cm.same_words(got, want, nan_positions)
