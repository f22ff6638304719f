"""numpy / Python-int restatement of the support functions (the reference's scalar branches built with
-D__GNUC_PYTHON__ -DARM_MATH_LOOPUNROLL -ffp-contract=off, no ARM_MATH_ROUNDING, no ARM_MATH_DSP) and the case list of
tests/golden/support.npz.

  float_to_q   p = x * 2^31 / 2^15 / 2^7 as a float32 product (subnormals kept), truncated toward zero, clipped to
               the destination.  The reference's C cast is undefined for NaN and for |x| >= 2^32 (q31), 65536 (q15),
               2^24 (q7) (in_contract); there the product saturates by sign and NaN gives 0 (our rule, pinned only
               against this restatement).
  q_to_float   float32(x) / 2^31 / 2^15 / 2^7; the int -> float step rounds to nearest even (q31 only).
  q_to_q       << 16, << 24, << 8 widening, arithmetic >> 16, >> 24, >> 8 narrowing.
  copy, fill   the words, the value.
  sort         the IEEE total order of the words: key = bits ^ ((bits >> 31) & 0x7fffffff) as int32, ascending;
               descending is the reverse.  -0.0 before +0.0, negative NaNs first, positive NaNs last.
  weighted_average   acc1 = acc1 + in*w, acc2 = acc2 + w over the elements in order from 0.0f, then acc1 / acc2.
  barycenter   out = out + in[v] * w[v], accum = accum + w[v] over the vectors in order from 0.0f, then out / accum.
"""
import zlib

import numpy as np

import basic_math_ref as bm

TYPES = bm.TYPES
DT, MDT, MARK = bm.DT, bm.MDT, bm.MARK
NAME = {"f32": "float", "q31": "q31", "q15": "q15", "q7": "q7"}        # the type's name in arm_<a>_to_<b>
KIND = {v: k for k, v in NAME.items()}
CONVERSIONS = tuple(f"{NAME[s]}_to_{NAME[d]}" for s in TYPES for d in TYPES if s != d)
COPIES = tuple(f"copy_{t}" for t in TYPES)
FILLS = tuple(f"fill_{t}" for t in TYPES)
SORTS = ("sort_f32", "merge_sort_f32")
FUNCS = CONVERSIONS + COPIES + FILLS + SORTS + ("weighted_average_f32", "barycenter_f32")
ALGS = ("bitonic", "bubble", "heap", "insertion", "quick", "selection")   # arm_sort_alg 0 .. 5
SLOW_ALGS = (1, 3, 5)                                       # O(n^2): bubble, insertion, selection
SLOW_MAX = 4097                                             # the longest case the O(n^2) algorithms are given
BITONIC_MAX = 65535                                         # the reference's uint16_t loop counter wraps beyond
FLOAT_BOUND = {"q31": 2.0 ** 32, "q15": 65536.0, "q7": 2.0 ** 24}
SORT_WAVE_MAX, SORT_LDS_MAX = 256, 16384                    # kSortWaveMax, kSortLdsMax of csrc/kernels.hpp

LENGTHS = bm.LENGTHS
STORE_MAX = bm.STORE_MAX
BARY_SIZES = (1, 2, 3, 5, 64, 65, 257)
SORT_KINDS = ("rand", "sorted", "reversed", "equal", "dups", "inf", "subnormal", "mixedzero", "nan")
SORT_EDGES = (SORT_WAVE_MAX - 1, SORT_WAVE_MAX, SORT_WAVE_MAX + 1, 1023, 1024, 1025, 4097, SORT_LDS_MAX - 1,
              SORT_LDS_MAX, SORT_LDS_MAX + 1, 33000, 3 * SORT_LDS_MAX + 5)

marked, same_words, out_crc, case_n, stored = bm.marked, bm.same_words, bm.out_crc, bm.case_n, bm.stored


def types(func):
    """(source type, destination type) of a function; fill has no source (None)."""
    if func in CONVERSIONS:
        s, d = func.split("_to_")
        return KIND[s], KIND[d]
    t = func.rsplit("_", 1)[1]
    return (None if func in FILLS else t), t


def nan_rule(func):
    return types(func)[1] == "f32" and func not in SORTS + COPIES + FILLS


# ---- the restatement ----------------------------------------------------------------------------------------
def float_to_q(x, t):
    bits = {"q31": 32, "q15": 16, "q7": 8}[t]
    with np.errstate(all="ignore"):
        p = (np.asarray(x, dtype=np.float32) * np.float32(2.0 ** (bits - 1))).astype(np.float64)
    p = np.where(np.isnan(p), 0.0, p)
    p = np.trunc(np.clip(p, -2.0 ** 31, 2.0 ** 31 - 1))     # the 32-bit (q31: 64-bit, then clipped) cast
    return np.clip(p.astype(np.int64), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(DT[t])


def convert(s, d, x):
    x = np.asarray(x, dtype=DT[s])
    if s == d:
        return x.copy()
    if s == "f32":
        return float_to_q(x, d)
    bs = {"q31": 32, "q15": 16, "q7": 8}[s]
    if d == "f32":
        return x.astype(np.float32) / np.float32(2.0 ** (bs - 1))
    bd = {"q31": 32, "q15": 16, "q7": 8}[d]
    v = x.astype(np.int64)
    return (v << (bd - bs) if bd > bs else v >> (bs - bd)).astype(DT[d])


def sort_key(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def total_order_sort(x, ascending=True):
    """[..., n] float32 -> every row sorted by the IEEE total order of its words."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    k = np.sort(sort_key(x), axis=-1, kind="stable")
    out = (k ^ ((k >> 31) & 0x7FFFFFFF)).view(np.float32)
    return out if ascending else np.ascontiguousarray(out[..., ::-1])


def weighted_average(a, w):
    """[items, n] under [items, n] (or [n]) -> [items]."""
    a = np.asarray(a, dtype=np.float32)
    w = np.broadcast_to(np.asarray(w, dtype=np.float32), a.shape)
    acc1 = np.zeros(a.shape[0], dtype=np.float32)
    acc2 = np.zeros(a.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        p = a * w
        for k in range(a.shape[1]):
            acc1 = acc1 + p[:, k]
            acc2 = acc2 + w[:, k]
        return acc1 / acc2


def barycenter(a, w):
    """[items, nbVectors, vecDim] under [items, nbVectors] (or [nbVectors]) -> [items, vecDim]."""
    a = np.asarray(a, dtype=np.float32)
    w = np.broadcast_to(np.asarray(w, dtype=np.float32), a.shape[:2])
    out = np.zeros((a.shape[0], a.shape[2]), dtype=np.float32)
    accum = np.zeros(a.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        for v in range(a.shape[1]):
            out = out + a[:, v, :] * w[:, v, None]
            accum = accum + w[:, v]
        return out / accum[:, None]


def run(func, g, ascending=True):
    """The restated function on the operands of one case -> the output words (one item)."""
    s, d = types(func)
    if func in FILLS:
        return np.full(int(g["scalars"][1]), g["scalars"][0], dtype=DT[d])
    if func in SORTS:
        return total_order_sort(g["a"], ascending)
    if func == "weighted_average_f32":
        return weighted_average(g["a"][None, :], g["b"][None, :])
    if func == "barycenter_f32":
        nv, dim = g["scalars"]
        return barycenter(g["a"].reshape(1, nv, dim), g["b"][None, :])[0]
    return convert(s, d, g["a"])


def in_contract(func, g):
    """Whether the reference's C is defined on the operands: the float -> integer casts need |x| below the bound and
    no NaN."""
    s, d = types(func)
    if func in CONVERSIONS and s == "f32":
        a = np.asarray(g["a"], dtype=np.float64)
        return bool((~np.isnan(a)).all() and (np.abs(a[~np.isnan(a)]) < FLOAT_BOUND[d]).all())
    return True


def sort_exact(g):
    """Whether the reference's sorts give our words: no NaN and not both signs of zero in the input."""
    a = g["a"]
    z = a[a == 0]
    return not np.isnan(a).any() and not (z.size and np.signbit(z).any() and not np.signbit(z).all())


def reference_sorts(case):
    """The (alg, dir) pairs arm_sort_f32 of the reference is given on a case (the merge sort gets both dirs)."""
    n = case_n(case)
    if case.startswith("nan_"):
        return []
    algs = [a for a in range(6) if not (a in SLOW_ALGS and n > SLOW_MAX) and not (a == 0 and n > BITONIC_MAX)]
    return [(a, d) for a in algs for d in (0, 1)]


def may_be_unsorted(alg, dirv, n):
    """The two quirks of the reference's ARM_SORT_BITONIC: a copy when n is no power of two, no dir in its merges."""
    return alg == 0 and (dirv == 0 or n & (n - 1) != 0)


# ---- the fixture's cases ------------------------------------------------------------------------------
def case_names(func):
    s, d = types(func)
    if func in SORTS:
        names = [f"len_{n}" for n in range(1, 71)]
        names += [f"{k}_{n}" for k in SORT_KINDS for n in (5, 64, 257)]
        names += [f"rand_{n}" for n in SORT_EDGES] + ["dups_4097"]   # mixed zeros: stored cases only (no CRC pins them)
        return names
    if func == "barycenter_f32":
        return [f"v{nv}_{dim}" for nv in BARY_SIZES for dim in BARY_SIZES] + ["zerosum_5", "negw_65"]
    if func == "weighted_average_f32":
        return ["empty_0"] + [f"rand_{n}" for n in LENGTHS] + ["zerosum_16", "cancel_9", "nonfinite_9", "subnormal_9"]
    names = [f"rand_{n}" for n in LENGTHS]
    if func in FILLS:
        return names + ["zero_0", "min_17", "max_17"] + (["negzero_9", "nan_9"] if d == "f32" else [])
    names += ["ext_64"]
    if s == "f32" and func in CONVERSIONS:
        names += ["trunc_33", "subnormal_9", "edge_16"]
    return names


def out_of_contract_input():
    """Float words outside every float -> q bound: our saturation rule (never given to the reference)."""
    return np.array([np.inf, -np.inf, np.nan, -np.nan, 2.0 ** 40, -2.0 ** 40, 2.0 ** 32, -2.0 ** 32, 3.0e38, -3.0e38,
                     2.0 ** 31, 0.5, -0.5], dtype=np.float32)


def _rng(func, case):
    return np.random.default_rng(zlib.crc32(f"support/{func}/{case}".encode()))


def _ext(s, d, n, rng):
    """n source words at the extremes of the conversion s -> d."""
    if s != "f32":
        i = np.iinfo(DT[s])
        head = [i.min, i.max, i.min + 1, i.max - 1, 0, 1, -1, 2, -2, (i.max + 1) // 2, -((i.max + 1) // 2), 0x55, -0x56]
        if s == "q31":                                      # above 2^24: ties to even, the carry into 1.0f
            head += [0x01000001, 0x01000003, 0x01000002, 0x7FFFFFFF, 0x7FFFFF80, 0x7FFFFFBF, 0x7FFFFFC0, 0x7FFFFF40,
                     -0x01000001, -0x01000003, -0x7FFFFFFF, 0x00FFFFFF, 0x02000002, 0x02000006, 0x7FFFFF7F]
        if s != "q7":                                       # bits below the narrowing shifts, of both signs
            head += [0xFF, -0xFF, 0x100, -0x100, 0x7FFF, -0x7FFF, 0x80, -0x81]
        if s == "q31":
            head += [0xFFFF, -0xFFFF, 0x10000, -0x10000, 0xFFFFFF, -0xFFFFFF, 0x1000000, -0x1000000]
        v = bm.rand(s, n, rng)
        v[:len(head)] = np.array(head, dtype=np.int64).astype(DT[s])
        return v
    if d == "f32":                                          # copy_f32: words that must pass unchanged
        v = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        v.view(np.uint32)[:8] = [0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 1, 0x80000001]
        return v
    bits = {"q31": 31, "q15": 15, "q7": 7}[d]
    head = [1.0, -1.0, 0.0, -0.0] + [1.0 - 2.0 ** -k for k in (1, bits, bits + 1, 24)] + \
        [-(1.0 - 2.0 ** -k) for k in (1, bits, bits + 1, 24)] + \
        [0.7 / 2 ** bits, -0.7 / 2 ** bits, 1.7 / 2 ** bits, -1.7 / 2 ** bits, 0.999 / 2 ** bits, -0.999 / 2 ** bits,
         2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -127, 2.0, -2.0, 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23]
    big = np.float32(FLOAT_BOUND[d])
    head += [float(np.nextafter(big, np.float32(0))), -float(np.nextafter(big, np.float32(0))), float(big) / 2,
             -float(big) / 2, float(big) / 4, 1000.5, -1000.5]
    v = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    v[:len(head)] = np.array(head, dtype=np.float32)
    return v


def operands(func, case):
    """{"a", "b", "scalars"} of one case (whichever the function has), the same words on every call."""
    rng = _rng(func, case)
    s, d = types(func)
    kind, n = case.rsplit("_", 1)
    n = int(n)
    if func in FILLS:
        i = None if d == "f32" else np.iinfo(DT[d])
        value = {"zero": 0, "min": -bm.FLT_MAX if i is None else i.min, "max": bm.FLT_MAX if i is None else i.max,
                 "negzero": -0.0, "nan": np.nan}.get(kind)
        if value is None:
            value = bm.rand(d, 1, rng)[0]
        return {"scalars": (DT[d](value).item(), n)}
    if func in SORTS:
        a = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        if kind == "sorted":
            a = np.sort(a)
        elif kind == "reversed":
            a = np.sort(a)[::-1].copy()
        elif kind == "equal":
            a[:] = np.float32(0.375)
        elif kind == "dups":
            a = rng.choice(np.array([-2.5, -1.0, 0.0, 0.25, 0.25, 7.0], dtype=np.float32), n)
        elif kind == "inf":
            a[rng.integers(0, n, max(1, n // 4))] = np.inf
            a[rng.integers(0, n, max(1, n // 4))] = -np.inf
        elif kind == "subnormal":
            a = (a * np.float32(2.0 ** -126)).astype(np.float32)
            a[::3] = np.float32(2.0 ** -149) * rng.choice([-1.0, 1.0], a[::3].size).astype(np.float32)
        elif kind == "mixedzero":
            a[rng.integers(0, n, max(2, n // 3))] = 0.0
            a[rng.integers(0, n, max(2, n // 3))] = -0.0
            a[:2] = [0.0, -0.0]
        elif kind == "nan":
            bits = a.view(np.uint32)
            bits[rng.integers(0, n, max(1, n // 5))] = 0x7FC00000
            bits[rng.integers(0, n, max(1, n // 5))] = 0xFFC00001
            bits[:5] = [0x7F800001, 0xFF800000, 0x7F800000, 0xFFFFFFFF, 0x7FFFFFFF]
            a[rng.integers(5, max(6, n), 2) % n] = -0.0
        return {"a": np.ascontiguousarray(a)}
    if func == "weighted_average_f32":
        a, w = rng.uniform(-1.0, 1.0, n).astype(np.float32), rng.uniform(0.0, 1.0, n).astype(np.float32)
        if kind == "zerosum":
            w = np.where(np.arange(n) % 2 == 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)
        elif kind == "cancel":
            w = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        elif kind == "nonfinite":
            a[[0, n - 1]] = [np.inf, np.nan]
            w[n // 2] = np.inf
        elif kind == "subnormal":
            a = (a * np.float32(2.0 ** -130)).astype(np.float32)
            w = (w * np.float32(2.0 ** -20)).astype(np.float32)
        return {"a": a, "b": w}
    if func == "barycenter_f32":
        nv, dim = (int(kind[1:]), n) if kind.startswith("v") else (4 if kind == "zerosum" else 7, n)
        a, w = rng.uniform(-1.0, 1.0, nv * dim).astype(np.float32), rng.uniform(0.0, 1.0, nv).astype(np.float32)
        if kind == "zerosum":
            w = np.array([0.5, -0.5, 0.25, -0.25], dtype=np.float32)
        elif kind == "negw":
            w = rng.uniform(-1.0, 1.0, nv).astype(np.float32)
        return {"a": a, "b": w, "scalars": (nv, dim)}
    if kind == "ext":
        return {"a": _ext(s, d, n, rng)}
    if kind == "trunc":                                     # products with a fraction of both signs
        scale = np.float32(2.0 ** {"q31": 31, "q15": 15, "q7": 7}[d])
        k = rng.integers(-3, 4, n).astype(np.float32) + rng.uniform(-0.99, 0.99, n).astype(np.float32)
        return {"a": (k / scale).astype(np.float32)}
    if kind == "subnormal":
        k = rng.integers(-149, -127, n, endpoint=True)
        return {"a": (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** k).astype(np.float32)}
    if kind == "edge":                                      # the largest magnitudes inside the bound
        big = np.float32(FLOAT_BOUND[d])
        a = (rng.uniform(0.25, 0.999, n) * rng.choice([-1.0, 1.0], n) * float(big)).astype(np.float32)
        a[:2] = [np.nextafter(big, np.float32(0)), -np.nextafter(big, np.float32(0))]
        return {"a": a}
    if s == "f32":
        return {"a": rng.uniform(-1.25, 1.25, n).astype(np.float32)}      # a few words saturate
    return {"a": bm.rand(s, n, rng)}


def out_len(func, g):
    """Output words of a case."""
    if func in FILLS:
        return int(g["scalars"][1])
    if func == "weighted_average_f32":
        return 1
    return int(g["scalars"][1]) if func == "barycenter_f32" else g["a"].size


def is_stored(func, g):
    """Whether the fixture keeps the case's operands and output words (otherwise their CRCs only)."""
    return max([out_len(func, g)] + [g[k].size for k in ("a", "b") if k in g]) <= STORE_MAX


def crc(g):
    c = zlib.crc32(repr([float(v) for v in g.get("scalars", ())]).encode())
    for k in ("a", "b"):
        if k in g:
            c = zlib.crc32(np.ascontiguousarray(g[k]).tobytes(), c)
    return c
