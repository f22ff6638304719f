"""numpy restatement of arm_mat_{add,sub,scale}_{f32,q31,q15}, arm_mat_trans_{f32,q31,q15,q7},
arm_mat_cmplx_trans_{f32,q31,q15} and arm_mat_vec_mult_{f32,q31,q15,q7} (the reference's scalar branches built
with -D__GNUC_PYTHON__ -DARM_MATH_LOOPUNROLL -ffp-contract=off), and the case list of tests/golden/mat_basic.npz.

  add / sub   f32: one float32 operation per word.  q15: ssat16(a +- b).  q31: the sum clipped to int32.
  scale       f32: x * scale.  q15: ssat16(((int32)x * scaleFract) >> (15 - shift)), -16 <= shift <= 15.
              q31: in = (int32)(((int64)x * scaleFract) >> 32); out = in << (shift + 1) in wrapping 32-bit
              arithmetic; if in != (out >> (shift + 1)): out = 0x7FFFFFFF ^ (in >> 31).  -1 <= shift <= 30.
  trans       dst[c][r] = src[r][c]; the complex forms move (re, im) pairs and do not conjugate.
  vec_mult    f32: sum = 0.0f, then sum = sum + a[r][k] * v[k] for k ascending, product rounded first.
              q31: the exact sum mod 2^64, >> 31, truncated to int32.  q7: an int32 sum, ssat8(sum >> 7).
              q15: a 64-bit sum, ssat16(sum >> 15).  Rows of the 4-row groups (r < 4 (rows / 4)) add columns in
              pairs (0,1),(2,3),... whose two products are first added in wrapping int32 (__SMLALD), an odd last
              column alone; the 1-3 tail rows pair only inside whole groups of four columns and add the last
              cols & 3 columns alone.  Only four operands of -32768 make the int32 pair sum wrap.
  row offset  arm_mat_vec_mult_q15 and _q31 keep the row offset in a uint16_t: a 4-row group starting at row 4 g
              reads from (4 g cols) mod 65536 and its rows 1..3 follow at + cols each; tail row r reads from
              (r cols) mod 65536.  The f32 and q7 functions use a uint32_t.
"""
import numpy as np

SUCCESS, ARGUMENT_ERROR, SIZE_MISMATCH = 0, -1, -3
DT = {"f32": np.float32, "q31": np.int32, "q15": np.int16, "q7": np.int8}
# pre-fill of output buffers: 0x5A in every byte (f32: 1.5e16)
MARK = {"f32": np.array([0x5A5A5A5A], dtype=np.uint32).view(np.float32)[0], "q31": np.int32(0x5A5A5A5A),
        "q15": np.int16(0x5A5A), "q7": np.int8(0x5A)}
EW_TYPES = ("f32", "q31", "q15")
FUNCS = tuple(f"{op}_{t}" for op in ("add", "sub", "scale") for t in EW_TYPES) + \
    tuple(f"trans_{t}" for t in ("f32", "q31", "q15", "q7")) + tuple(f"cmplx_trans_{t}" for t in EW_TYPES) + \
    tuple(f"vec_mult_{t}" for t in ("f32", "q31", "q15", "q7"))
SHIFT_RANGE = {"q31": (-1, 30), "q15": (-16, 15)}


def split(func):
    op, t = func.rsplit("_", 1)
    return op, t


def marked(t, shape):
    return np.full(shape, MARK[t], dtype=DT[t])


def _clip(x, t):
    i = np.iinfo(DT[t])
    return np.clip(x, i.min, i.max).astype(DT[t])


def add(t, a, b, sign=1):
    if t == "f32":
        with np.errstate(all="ignore"):
            return a + b if sign > 0 else a - b
    return _clip(a.astype(np.int64) + sign * b.astype(np.int64), t)


def sub(t, a, b):
    return add(t, a, b, -1)


def scale(t, a, s, shift=0):
    if t == "f32":
        with np.errstate(all="ignore"):
            return a * np.float32(s)
    lo, hi = SHIFT_RANGE[t]
    assert lo <= shift <= hi
    if t == "q15":
        return _clip((a.astype(np.int32) * np.int32(s)) >> (15 - shift), t)
    k = shift + 1
    v = (a.astype(np.int64) * np.int64(s)) >> 32                               # int32 range
    out = ((v << k) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
    sat = np.int64(0x7FFFFFFF) ^ (v >> 31)
    return np.where(v != (out >> k), sat, out).astype(np.int32)


def trans(a):
    return np.ascontiguousarray(a.T)


def cmplx_trans(a):
    """a [rows, 2 cols] interleaved -> [cols, 2 rows]."""
    r, c2 = a.shape
    return np.ascontiguousarray(a.reshape(r, c2 // 2, 2).transpose(1, 0, 2)).reshape(c2 // 2, 2 * r)


def row_offsets(t, rows, cols):
    r = np.arange(rows, dtype=np.int64)
    if t in ("f32", "q7"):
        return r * cols
    grp = r < 4 * (rows // 4)
    return np.where(grp, (((r & ~3) * cols) & 0xFFFF) + (r & 3) * cols, (r * cols) & 0xFFFF)


def vec_mult(t, m, v):
    """m [rows, cols], v [cols] -> [rows]."""
    rows, cols = m.shape
    flat = m.reshape(-1)
    a = flat[row_offsets(t, rows, cols)[:, None] + np.arange(cols)[None, :]] if cols else m
    if t == "f32":
        s = np.zeros(rows, dtype=np.float32)
        with np.errstate(all="ignore"):
            for k in range(cols):
                s = s + a[:, k] * v[k]
        return s
    if t == "q31":
        with np.errstate(over="ignore"):
            s = (a.astype(np.int64) * v.astype(np.int64)[None, :]).sum(axis=1, dtype=np.int64)
        return (s >> 31).astype(np.int32)
    if t == "q7":
        s = (a.astype(np.int32) * v.astype(np.int32)[None, :]).sum(axis=1, dtype=np.int32)
        return _clip(s >> 7, t)
    p = a.astype(np.int32) * v.astype(np.int32)[None, :]
    out = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        end = cols & ~1 if r < 4 * (rows // 4) else cols & ~3
        with np.errstate(over="ignore"):
            pairs = p[r, 0:end:2] + p[r, 1:end:2]                               # wrapping int32
        out[r] = pairs.astype(np.int64).sum() + p[r, end:].astype(np.int64).sum()
    return _clip(out >> 15, t)


def run(func, g):
    """The restated function on a case's operands -> {"dst": ...} (with "status" unless vec_mult)."""
    op, t = split(func)
    if op in ("add", "sub"):
        return {"status": SUCCESS, "dst": add(t, g["a"], g["b"], 1 if op == "add" else -1)}
    if op == "scale":
        return {"status": SUCCESS, "dst": scale(t, g["a"], g["scale"][()], int(g["shift"]) if "shift" in g else 0)}
    if op == "trans":
        return {"status": SUCCESS, "dst": trans(g["a"])}
    if op == "cmplx_trans":
        return {"status": SUCCESS, "dst": cmplx_trans(g["a"])}
    return {"dst": vec_mult(t, g["m"], g["v"])}


# ---- the fixture's cases ------------------------------------------------------------------------------
EW_SHAPES = ((1, 1), (3, 5), (17, 31))
TRANS_SHAPES = ((1, 1), (3, 5), (9, 1), (33, 31))
VEC_SHAPES = ((1, 3), (3, 7), (4, 6), (5, 7), (9, 1), (8, 8), (13, 70))
BIG = (258, 256)                   # rows 256 / 257 lie past 65535 elements: the uint16_t offset wraps
VEC_AMP = {"q7": 40, "q15": 4000}       # random vec_mult operands: the sums stay off the clip (q7 BIG: 15)
MIN_SHAPES = ((4, 6), (5, 7), (3, 7), (1, 3))          # vec_mult_q15 with every operand -32768


def _shape(s):
    return "x".join(str(v) for v in s)


def case_names(func):
    op, t = split(func)
    if op in ("add", "sub"):
        names = [f"rand_{_shape(s)}" for s in EW_SHAPES]
        return names + (["sat_3x5"] if t != "f32" else ["nonfinite_3x5"])
    if op == "scale":
        if t == "f32":
            return [f"rand_{_shape(s)}" for s in EW_SHAPES] + ["nonfinite_3x5"]
        lo, hi = SHIFT_RANGE[t]
        return [f"rand_{_shape(s)}" for s in EW_SHAPES] + [f"shift{v}_3x5" for v in (lo, 0, hi)] + ["sat_3x5"]
    if op in ("trans", "cmplx_trans"):
        return [f"rand_{_shape(s)}" for s in TRANS_SHAPES]
    names = [f"rand_{_shape(s)}" for s in VEC_SHAPES] + [f"big_{_shape(BIG)}"]
    if t == "q15":
        names += [f"min_{_shape(s)}" for s in MIN_SHAPES] + ["pairwrap_7x7"]
    if t == "f32":
        names += ["nonfinite_5x7"]
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


def big_matrix(t, rng, amp=None):
    """BIG with rows that repeat with period 17 (the fixture compresses); rows 256 and 257 differ from rows 0
    and 1, so reading them from the wrapped offset shows."""
    base = rand(t, (17, BIG[1]), rng, amp)
    return np.ascontiguousarray(base[np.arange(BIG[0]) % 17])


def pairwrap_case():
    """7x7 q15: rows 0..3 are group rows, rows 4..6 tail rows, all equal.  Columns 4 and 5 hold -32768 against
    -32768 in the vector: a group row pairs them (2^30 + 2^30 wraps to -2^31), a tail row adds them alone."""
    m = np.zeros((7, 7), dtype=np.int16)
    m[:, 4:6] = -32768
    m[:, 0] = 100
    v = np.zeros(7, dtype=np.int16)
    v[4:6] = -32768
    v[0] = 50
    return m, v


def operands(func, case, rng):
    op, t = split(func)
    kind, size = case.rsplit("_", 1)
    shape = tuple(int(v) for v in size.split("x"))
    if op in ("add", "sub"):
        if kind == "sat":
            a, b = extremes(t, shape, rng), extremes(t, shape, rng)
            a.flat[:2] = np.iinfo(DT[t]).max, np.iinfo(DT[t]).min                # max + 1, min - 1 (sub: mirrored)
            b.flat[:2] = (1, -1) if op == "add" else (-1, 1)
            return {"a": a, "b": b}
        if kind == "nonfinite":
            a, b = rand(t, shape, rng), rand(t, shape, rng)
            a.flat[[1, 4, 7, 9]] = np.inf, -np.inf, np.nan, np.inf
            b.flat[[2, 4, 9]] = np.inf, -np.inf, np.inf if op == "sub" else -np.inf      # Inf - Inf at [9]
            return {"a": a, "b": b}
        return {"a": rand(t, shape, rng), "b": rand(t, shape, rng)}
    if op == "scale":
        if t == "f32":
            a = rand(t, shape, rng)
            if kind == "nonfinite":
                a.flat[[1, 4, 7, 9]] = np.inf, -np.inf, np.nan, 0.0
                return {"a": a, "scale": np.float32(np.inf)}                     # 0 * Inf at [9]
            return {"a": a, "scale": np.float32(rng.uniform(-2, 2))}
        g = {"a": extremes(t, shape, rng) if kind == "sat" else rand(t, shape, rng),
             "scale": DT[t](np.iinfo(DT[t]).max if kind == "sat" else rand(t, (), rng)),
             "shift": np.int32(int(kind[5:]) if kind.startswith("shift") else 1 if kind == "sat" else 0)}
        return g
    if op == "trans":
        return {"a": rand(t, shape, rng)}
    if op == "cmplx_trans":
        return {"a": rand(t, (shape[0], 2 * shape[1]), rng)}
    if kind == "min":
        return {"m": np.full(shape, -32768, dtype=np.int16), "v": np.full(shape[1], -32768, dtype=np.int16)}
    if kind == "pairwrap":
        m, v = pairwrap_case()
        return {"m": m, "v": v}
    if kind == "big":
        amp = 15 if t == "q7" else VEC_AMP.get(t)
        return {"m": big_matrix(t, rng, amp), "v": rand(t, shape[1], rng, amp)}
    if kind == "nonfinite":
        m, v = rand(t, shape, rng), rand(t, shape[1], rng)
        m[0, 2], m[1, 3], m[2, 0], m[3, 1], m[3, 5] = np.inf, -np.inf, np.nan, np.inf, -np.inf    # row 3: Inf - Inf
        v[1], v[5] = 0.5, 0.5
        return {"m": m, "v": v}
    amp = VEC_AMP.get(t)
    return {"m": rand(t, shape, rng, amp), "v": rand(t, shape[1], rng, amp)}


def same_words(got, want, nan_positions=False):
    """Bit equality; nan_positions: the f32 rule for non-finite inputs (tests/test_f32_classes.py): non-NaN
    words bit-equal, NaNs at the same positions."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not nan_positions or got.dtype != np.float32:
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all()) and got.view(np.uint32)[~gn].tobytes() == want.view(np.uint32)[~wn].tobytes()
