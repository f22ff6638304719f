"""numpy / Python-int restatement of the distance functions (the reference's scalar branches built with
-D__GNUC_PYTHON__ -DARM_MATH_LOOPUNROLL -ffp-contract=off) and the case list of tests/golden/distance.npz.

  f32      every sum is one chain sum = sum + term in element order from 0.0f, the term rounded to float32 before the
           add (numpy's float32 cumsum is that chain); divisions and square roots are IEEE; arm_sqrt_f32 gives +0.0
           for a negative or NaN argument.  braycurtis sum|a - b| / sum|a + b|; canberra sum |a - b| / (|a| + |b|)
           over the elements where a != 0 or b != 0; chebyshev starts from |a0 - b0| and replaces on d > max;
           cityblock sum|a - b|; euclidean sqrt(sum (a - b)^2); cosine 1 - dot / sqrt(pa * pb); correlation the same
           on x + (-mean), every sum then divided by (float)n (it also returns the shifted vectors, which the
           reference writes back); jensenshannon sqrt((sum a log(a / m) + sum b log(b / m)) / 2), m = (a + b) / 2, with
           the host's logf.
  boolean  TT, TF, FT are counts over the first n bits, whole words bit by bit and of a last partial word the top
           n % 32 bits; FF = n - TT - TF - FT; the epilogues in uint32 (wrapping) and float32 exactly as the C mixes
           them.
  DTW      the cost matrix cell by cell, MIN(x, y) = x < y ? x : y; the walk back of arm_dtw_path_f32 (None where the
           reference would never return); the two windows of arm_dtw_init_window_q7.
"""
import ctypes
import ctypes.util
import zlib

import numpy as np

import basic_math_ref as bm
import f32_classes as fc

F = np.float32
F32_MAX = F(3.4028234663852886e38)
MARK = bm.MARK["f32"]
LENGTHS = bm.LENGTHS
STORE_MAX = bm.STORE_MAX
F32_FUNCS = ("braycurtis", "canberra", "chebyshev", "cityblock", "correlation", "cosine", "euclidean", "jensenshannon")
BOOL_FUNCS = ("dice", "hamming", "jaccard", "kulsinski", "rogerstanimoto", "russellrao", "sokalmichener",
              "sokalsneath", "yule")
SAKOE_CHIBA, SLANTED_BAND = 1, 3

_libm = None


def logf(x):
    """The host libm's logf on every word of a float32 array."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    x = np.asarray(x, dtype=F)
    return np.array([_libm.logf(float(v)) for v in x.reshape(-1)], dtype=F).reshape(x.shape)


# ---- f32 -------------------------------------------------------------------------------------------------------
def chain(t):
    return np.cumsum(np.concatenate([np.zeros(1, F), np.asarray(t, dtype=F)]), dtype=F)[-1]


def sqrt0(v):
    return np.sqrt(F(v)) if v >= 0 else F(0)


def distance_f32(func, a, b):
    """-> the result word; correlation: (result, shifted a, shifted b)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    n = a.size
    with np.errstate(all="ignore"):
        if func == "braycurtis":
            return F(chain(np.abs(a - b)) / chain(np.abs(a + b)))
        if func == "canberra":
            keep = (a != 0) | (b != 0)
            return F(chain((np.abs(a - b) / (np.abs(a) + np.abs(b)))[keep]))
        if func == "chebyshev":
            d = np.abs(a - b)
            return d[0] if np.isnan(d[0]) else F(np.fmax.reduce(d))
        if func == "cityblock":
            return F(chain(np.abs(a - b)))
        if func == "euclidean":
            return F(sqrt0(chain((a - b) * (a - b))))
        if func == "cosine":
            return F(F(1) - chain(a * b) / sqrt0(chain(a * a) * chain(b * b)))
        if func == "correlation":
            nf = F(n)
            sa, sb = a + (-(chain(a) / nf)), b + (-(chain(b) / nf))
            pa, pb, dot = chain(sa * sa) / nf, chain(sb * sb) / nf, chain(sa * sb) / nf
            return F(F(1) - dot / sqrt0(pa * pb)), sa.astype(F), sb.astype(F)
        if func == "jensenshannon":
            m = (a + b) / F(2)
            left, right = chain(a * logf(a / m)), chain(b * logf(b / m))
            return F(sqrt0((left + right) / F(2)))
    raise ValueError(func)


def f32_case_names():
    names = [f"rand_{n}" for n in LENGTHS]
    names += [f"{c}_{n}" for c in fc.CLASSES for n in (65, 1025)]
    names += [f"{s}_67" for s in ("zeros00", "zerospm", "nanelem", "maxfirst", "maxlast", "maxrepeat", "nan0", "nanmid",
                                  "zeroden", "zeropower", "constant", "pair00", "azero", "jssubnormal")]
    return names


def f32_operands(func, case):
    """(a, b) of a case; the same operands for every function except that jensenshannon's random vectors are
    normalised positive ones."""
    kind, n = case.rsplit("_", 1)
    n = int(n)
    rng = np.random.default_rng(zlib.crc32(f"{'js' if func == 'jensenshannon' else 'f32'}/{case}".encode()))
    js = func == "jensenshannon"

    def rand():
        if js:
            v = rng.uniform(0.01, 1.0, n)
            return (v / v.sum()).astype(F)
        return rng.uniform(-1.0, 1.0, n).astype(F)

    if kind in fc.CLASSES:
        pos = [sorted(rng.choice(n, 3, replace=False).tolist()) for _ in range(2)]
        a = fc.f32_class_input(kind, (n,), rng, scale=3.0e38, positions=pos[0])
        b = fc.f32_class_input(kind, (n,), rng, scale=3.0e38, positions=pos[1])
        return a, b
    a, b = rand(), rand()
    if kind == "zeros00":
        a[[0, 5, n - 1]] = 0.0
        b[[0, 5, n - 1]] = 0.0
    elif kind == "zerospm":
        a[[0, 5, n - 1]] = 0.0
        b[[0, 5, n - 1]] = -0.0
        a[7], b[7] = -0.0, 0.0
    elif kind == "nanelem":
        a[3] = np.nan
        b[9] = np.nan
        a[11], b[11] = 0.0, np.nan
    elif kind in ("maxfirst", "maxlast", "maxrepeat"):
        idx = {"maxfirst": [0], "maxlast": [n - 1], "maxrepeat": [4, 20, n - 2]}[kind]
        a[idx], b[idx] = F(3.0), F(-2.0)
    elif kind == "nan0":
        a[0] = np.nan
    elif kind == "nanmid":
        b[n // 2] = np.nan
    elif kind == "zeroden":
        b = (-a).astype(F)
    elif kind == "zeropower":
        a[:] = 0.0
    elif kind == "constant":
        a[:] = F(0.375)
    elif kind == "pair00":
        a[6], b[6] = 0.0, 0.0
    elif kind == "azero":
        a[6] = 0.0
    elif kind == "jssubnormal":
        a[[2, 8]] = F(2.0 ** -140)
        b[[8, 12]] = F(2.0 ** -145)
    else:
        assert kind == "rand", case
    return a, b


# ---- boolean ---------------------------------------------------------------------------------------------------
BOOL_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1025, 4097, 33000)
BOOL_PATTERNS = ("rand", "zeros", "ones", "equal", "complement")
BOOL_WRAP = 200000                       # every second bit set: yule's 2 * (ctf * cft) wraps
BOOL_HUGE = (1 << 25) + 33               # counts above 2^24: the float conversions round


def bool_words(n):
    return (n + 31) // 32


def bool_case_names():
    names = [f"{p}_{n}_{t}" for n in BOOL_LENGTHS for p in BOOL_PATTERNS for t in ((0, 1) if n % 32 else (0,))]
    return names + [f"rand_{BOOL_WRAP}_0", f"dense_{BOOL_HUGE}_0", f"dense_{BOOL_HUGE}_1"]


def bool_case_n(case):
    return int(case.split("_")[1])


def bool_operands(case):
    """(a, b, n): packed uint32 words; the unused low bits of a last partial word are all 0 (tail 0) or all 1."""
    pat, n, tail = case.split("_")
    n, tail = int(n), int(tail)
    w = bool_words(n)
    rng = np.random.default_rng(zlib.crc32(f"bool/{pat}_{n}".encode()))        # both tails: the same counted bits
    a = rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
    if pat == "dense":
        a |= rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
        b |= rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
    elif pat == "zeros":
        a[:], b[:] = 0, 0
    elif pat == "ones":
        a[:], b[:] = 0xFFFFFFFF, 0xFFFFFFFF
    elif pat == "equal":
        b = a.copy()
    elif pat == "complement":
        b = ~a
    if n % 32:
        low = np.uint32((1 << (32 - n % 32)) - 1)
        for x in (a, b):
            x[-1] = (x[-1] | low) if tail else (x[-1] & ~low)
    return a, b, n


def _popcount(x):
    return int(np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).sum(dtype=np.int64))


def bool_counts(a, b, n):
    """(TT, TF, FT, FF) over the first n booleans."""
    w = bool_words(n)
    a, b = np.array(a[:w], dtype=np.uint32), np.array(b[:w], dtype=np.uint32)
    if n % 32:
        mask = np.uint32((0xFFFFFFFF << (32 - n % 32)) & 0xFFFFFFFF)
        a[-1] &= mask
        b[-1] &= mask
        nb = ~b
        nb[-1] &= mask
        na = ~a
        na[-1] &= mask
    else:
        na, nb = ~a, ~b
    tt, tf, ft = _popcount(a & b), _popcount(a & nb), _popcount(na & b)
    return tt, tf, ft, n - tt - tf - ft


def bool_finish(func, ctt, ctf, cft, cff, n):
    """The function's return expression: U wraps to uint32, f converts to float32 (round to nearest even)."""
    U = lambda x: x & 0xFFFFFFFF                                                # noqa: E731
    f = lambda x: F(float(x)) if x < (1 << 53) else F(x)                        # noqa: E731
    with np.errstate(all="ignore"):
        if func == "dice":
            return F(f(U(ctf + cft)) / (F(2) * f(ctt) + f(cft) + f(ctf)))
        if func == "hamming":
            return F(f(U(ctf + cft)) / f(n))
        if func == "jaccard":
            return F(f(U(ctf + cft)) / f(U(ctt + cft + ctf)))
        if func == "kulsinski":
            return F(f(U(ctf + cft - ctt + n)) / f(U(cft + ctf + n)))
        if func == "rogerstanimoto":
            r = U(2 * U(ctf + cft))
            return F(f(r) / f(U(r + ctt + cff)))
        if func == "russellrao":
            return F(f(U(n - ctt)) / f(n))
        if func == "sokalmichener":
            r, s = F(2) * f(U(ctf + cft)), f(U(cff + ctt))
            return F(r / (s + r))
        if func == "sokalsneath":
            r = F(2) * f(U(ctf + cft))
            return F(r / (r + f(ctt)))
        if func == "yule":
            r = U(2 * U(ctf * cft))
            return F(f(r) / (f(r) / F(2) + f(U(ctt * cff))))
    raise ValueError(func)


def boolean_distance(func, a, b, n):
    return bool_finish(func, *bool_counts(a, b, n), n)


def yule_wraps(a, b, n):
    tt, tf, ft, ff = bool_counts(a, b, n)
    return 2 * tf * ft >= 1 << 32 or tt * ff >= 1 << 32


# ---- DTW -------------------------------------------------------------------------------------------------------
DTW_SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (63, 7), (64, 7), (65, 7), (7, 65), (129, 130))
DTW_WINDOWS = ("none", "sakoe0", "sakoe1", "sakoe5", "slanted0", "slanted1", "slanted5")
DTW_SPECIAL = ("blockend", "gapcol0", "inf", "overflow", "ties", "tiessakoe1")


def dtw_case_names():
    names = [f"{w}_{q}x{t}" for (q, t) in DTW_SHAPES for w in DTW_WINDOWS]
    return names + [f"{s}_{q}x{t}" for s in DTW_SPECIAL for (q, t) in ((3, 5), (65, 7), (7, 65))]


def init_window(kind, size, q_len, t_len):
    """arm_dtw_init_window_q7 -> int8 [q_len, t_len], or None for an unknown type."""
    w = np.zeros((q_len, t_len), dtype=np.int8)
    if kind == SAKOE_CHIBA:
        for q in range(q_len):
            for t in range(t_len):
                w[q, t] = abs(q - t) <= size
    elif kind == SLANTED_BAND:
        for q in range(q_len):
            diag = F(F(F(1) * F(q)) * F(t_len)) / F(q_len)
            for t in range(t_len):
                w[q, t] = abs(F(F(t) - diag)) <= F(size)
    else:
        return None
    return w


def dtw_operands(case):
    """(D float32 [q, t], window int8 [q, t] or None): D is NaN everywhere outside the window."""
    kind, shape = case.split("_")
    q_len, t_len = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(zlib.crc32(f"dtw/{case}".encode()))
    d = rng.uniform(0.0, 1.0, (q_len, t_len)).astype(F)
    w = None
    if kind.startswith("sakoe"):
        w = init_window(SAKOE_CHIBA, int(kind[5:]), q_len, t_len)
    elif kind.startswith("slanted"):
        w = init_window(SLANTED_BAND, int(kind[7:]), q_len, t_len)
    elif kind == "blockend":
        w = np.ones((q_len, t_len), dtype=np.int8)
        w[-1, -1] = 0
    elif kind == "gapcol0":
        w = np.ones((q_len, t_len), dtype=np.int8)
        w[1, 0] = 0
        w[0, 2] = 2                                          # only a byte equal to 1 is inside
    elif kind == "inf":
        d[q_len // 2, t_len // 2] = np.inf
        d[0, 1] = np.inf
    elif kind == "overflow":
        w = np.ones((q_len, t_len), dtype=np.int8)
        w[1, 0] = 0
        d[:] = F(1.0e37) * d + F(1.0e37)                     # F32_MAX + D is +Inf below the gap; long sums overflow
    elif kind == "ties":
        d[:] = F(0.25)
    elif kind == "tiessakoe1":
        d[:] = F(0.25)
        w = init_window(SAKOE_CHIBA, 1, q_len, t_len)
    else:
        assert kind == "none", case
    if w is not None:
        d[w != 1] = np.nan
    return d, w


def _min(x, y):
    return x if x < y else y


def dtw_distance(d, w):
    """-> (status, result or None, cost matrix)."""
    q_len, t_len = d.shape
    win = (lambda q, t: True) if w is None else (lambda q, t: w[q, t] == 1)     # noqa: E731
    c = np.full((q_len, t_len), F32_MAX, dtype=F)
    with np.errstate(all="ignore"):
        c[0, 0] = d[0, 0]
        for q in range(1, q_len):
            if win(q, 0):
                c[q, 0] = c[q - 1, 0] + d[q, 0]
        for t in range(1, t_len):
            if win(0, t):
                c[0, t] = c[0, t - 1] + d[0, t]
        for q in range(1, q_len):
            for t in range(1, t_len):
                if win(q, t):
                    x = d[q, t]
                    c[q, t] = _min(c[q - 1, t - 1] + F(2) * x, _min(c[q, t - 1] + x, c[q - 1, t] + x))
        last = c[-1, -1]
        if last == F32_MAX:
            return -1, None, c
        return 0, F(last / F(q_len + t_len)), c


def dtw_path(c):
    """-> int16 [length, 2], or None where no neighbour is below F32_MAX (the reference loops for ever)."""
    q, t = c.shape[0] - 1, c.shape[1] - 1
    path = []
    while q > 0 or t > 0:
        p, cur = -1, F32_MAX
        if q > 0 and c[q - 1, t] < cur:
            cur, p = c[q - 1, t], 2
        if t > 0 and c[q, t - 1] < cur:
            cur, p = c[q, t - 1], 0
        if q > 0 and t > 0 and c[q - 1, t - 1] < cur:
            cur, p = c[q - 1, t - 1], 1
        if p < 0:
            return None
        path.append((q, t))
        if p <= 1:
            t -= 1
        if p >= 1:
            q -= 1
    path.append((0, 0))
    return np.array(path[::-1], dtype=np.int16)


# ---- the fixture -----------------------------------------------------------------------------------------------
def crc(*arrays):
    v = 0
    for x in arrays:
        if x is not None:
            v = zlib.crc32(np.ascontiguousarray(x).tobytes(), v)
    return v


def same_word(got, want):
    """One float32 result: NaNs by being NaN, every other word by its bits."""
    got, want = F(got), F(want)
    if np.isnan(got) or np.isnan(want):
        return bool(np.isnan(got) and np.isnan(want))
    return got.tobytes() == want.tobytes()
