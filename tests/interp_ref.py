"""numpy restatement of the reference's interpolation functions (Source/InterpolationFunctions, scalar code built with
-ffp-contract=off) and the cases of tests/golden/interp.npz.

  linear_f32, bilinear_f32      one float32 operation per operation of the reference, in its order
  linear_q, bilinear_q          int64 arithmetic wrapped to the width of every assignment of the reference
  spline_init, spline_eval      the reference's loops with np.float32 scalars; spline_eval is the reference's own serial
                                walk over the queries (not the prefix maximum the kernel forms)
Outside the reference's defined behaviour the library defines a rule (include/arm_math.h) and this file restates it:
the casts (int32_t)((x - x1) / xSpacing), (int32_t)X and (int32_t)Y saturate by sign and give 0 for a NaN.  Each
operand function returns with its samples the mask of those whose result in the reference is defined; the fixtures
are compared on that mask only.

Every sample is independent of its neighbours, so the expected words of a prefix or a tiling of the samples are the
prefix or the tiling of the expected words.
"""
import zlib

import numpy as np

F = np.float32
MARK = F(1.5365222e+16)
SAMPLES = 520
KINDS = ("f32", "q31", "q15", "q7")
NP = {"f32": np.float32, "q31": np.int32, "q15": np.int16, "q7": np.int8}
LINEAR_SIZES = {"f32": (2, 3, 5, 4096, 16384, 16385), "q31": (2, 3, 4096), "q15": (2, 3, 4096), "q7": (2, 3, 4096)}
BILINEAR_SHAPES = ((2, 2), (3, 5), (5, 3), (64, 67))         # (numRows, numCols)
SPLINE_N = (2, 3, 4, 9, 65)
SPLINE_BLOCKS = (1, 20, 33, 257)
SPLINE_QUERIES = ("sorted", "knots", "unsorted", "nan")
X1, SPACING = F(-1.5), F(0.37)


def same_word(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _wrap(v, bits):
    half = 1 << (bits - 1)
    return ((np.asarray(v, dtype=np.int64) + half) & ((1 << bits) - 1)) - half


def cast_sat(p):
    """(int32_t)p as the library defines it: toward zero, saturating by sign, 0 for a NaN."""
    p = np.asarray(p, dtype=F)
    with np.errstate(all="ignore"):
        safe = np.where(np.isnan(p) | (np.abs(p) >= F(2.0 ** 31)), F(0), p)
        i = np.trunc(safe).astype(np.int64)
    i = np.where(p >= F(2.0 ** 31), 2 ** 31 - 1, np.where(p <= F(-2.0 ** 31), -2 ** 31, i))
    return i.astype(np.int64)


# ---- linear -------------------------------------------------------------------------------------------------------
def linear_f32(tab, x1, spacing, x):
    tab, x, x1, spacing = np.asarray(tab, dtype=F), np.asarray(x, dtype=F), F(x1), F(spacing)
    n = tab.size
    with np.errstate(all="ignore"):
        i = cast_sat((x - x1) / spacing)
        below = x < x1
        above = ~below & ((i & 0xffffffff) >= n - 1)
        ii = np.clip(i, 0, max(n - 2, 0))
        x0 = x1 + ii.astype(F) * spacing
        xn = x1 + (ii + 1).astype(F) * spacing
        y0, y1 = tab[ii], tab[np.minimum(ii + 1, n - 1)]
        y = y0 + (x - x0) * ((y1 - y0) / (xn - x0))
    return np.where(below, tab[0], np.where(above, tab[n - 1], y)).astype(F)


def linear_q(kind, tab, x):
    tab, x = np.asarray(tab).astype(np.int64), np.asarray(x, dtype=np.int32).astype(np.int64)
    n = tab.size
    last = _wrap(n - 1, 32)                                  # (int32_t)(nValues - 1)
    fract = x & 0xFFFFF
    if kind == "q7":
        index = (x >> 20) & 0xfff
        first, end = x < 0, (x >= 0) & (index >= n - 1)
    else:
        index = x >> 20
        end = index >= last
        first = ~end & (index < 0)
    ii = np.clip(index, 0, max(n - 2, 0))
    y0, y1 = tab[ii], tab[np.minimum(ii + 1, n - 1)]
    if kind == "q31":
        fr = fract << 11
        y = (y0 * (0x7FFFFFFF - fr)) >> 32
        y = _wrap(y + ((y1 * fr) >> 32), 32)
        y = _wrap(y << 1, 32)
    elif kind == "q15":
        y = _wrap((y0 * (0xFFFFF - fract) + y1 * fract) >> 20, 16)
    else:
        y = _wrap(_wrap(y0 * (0xFFFFF - fract) + y1 * fract, 32) >> 20, 8)
    return np.where(first, tab[0], np.where(end, tab[n - 1], y)).astype(NP[kind])


# ---- bilinear -----------------------------------------------------------------------------------------------------
def _corners(tab, xi, yi, inside):
    rows, cols = tab.shape
    flat = tab.reshape(-1)
    index = np.where(inside, xi + yi * cols, 0)
    return flat[index], flat[index + 1], flat[index + cols], flat[index + cols + 1]


def bilinear_f32(tab, X, Y):
    tab, X, Y = np.asarray(tab, dtype=F), np.asarray(X, dtype=F), np.asarray(Y, dtype=F)
    rows, cols = tab.shape
    xi, yi = cast_sat(X), cast_sat(Y)
    inside = ~((xi < 0) | (xi > cols - 2) | (yi < 0) | (yi > rows - 2))
    f00, f01, f10, f11 = _corners(tab, xi, yi, inside)
    with np.errstate(all="ignore"):
        b1, b2, b3, b4 = f00, f01 - f00, f10 - f00, f00 - f01 - f10 + f11
        xd, yd = X - xi.astype(F), Y - yi.astype(F)
        out = b1 + b2 * xd + b3 * yd + b4 * xd * yd
    return np.where(inside, out, F(0)).astype(F)


def bilinear_q(kind, tab, X, Y):
    tab = np.asarray(tab).astype(np.int64)
    X, Y = (np.asarray(v, dtype=np.int32).astype(np.int64) for v in (X, Y))
    rows, cols = tab.shape
    rI, cI = X >> 20, Y >> 20
    inside = ~((rI < 0) | (rI > cols - 2) | (cI < 0) | (cI > rows - 2))
    x1, x2, y1, y2 = _corners(tab, rI, cI, inside)
    xf, yf = X & 0xFFFFF, Y & 0xFFFFF
    if kind == "q31":
        xf, yf = xf << 11, yf << 11
        m = lambda a, b: (a * b) >> 32                        # noqa: E731
        acc = m(m(x1, 0x7FFFFFFF - xf), 0x7FFFFFFF - yf)
        acc = _wrap(acc + m(m(x2, 0x7FFFFFFF - yf), xf), 32)
        acc = _wrap(acc + m(m(y1, 0x7FFFFFFF - xf), yf), 32)
        acc = _wrap(acc + m(m(y2, xf), yf), 32)
        out = _wrap(acc << 2, 32)
    elif kind == "q15":
        s = lambda a, b: _wrap((a * b) >> 4, 32)              # noqa: E731
        acc = s(x1, 0xFFFFF - xf) * (0xFFFFF - yf)
        acc = acc + s(x2, 0xFFFFF - yf) * xf
        acc = acc + s(y1, 0xFFFFF - xf) * yf
        acc = acc + s(y2, xf) * yf
        out = _wrap(acc >> 36, 16)
    else:
        acc = (x1 * (0xFFFFF - xf)) * (0xFFFFF - yf)
        acc = acc + (x2 * (0xFFFFF - yf)) * xf
        acc = acc + (y1 * (0xFFFFF - xf)) * yf
        acc = acc + (y2 * yf) * xf
        out = _wrap(acc >> 40, 8)
    return np.where(inside, out, 0).astype(NP[kind])


# ---- spline -------------------------------------------------------------------------------------------------------
def spline_init(spline_type, x, y):
    """-> (coeffs [3 (n - 1)], temp [2 n - 1]) as arm_spline_init_f32 leaves them; n >= 2."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    n = x.size
    u, z = np.zeros(n - 1, F), np.zeros(n, F)
    b, c, d = np.zeros(n - 1, F), np.zeros(n - 1, F), np.zeros(n - 1, F)
    three, two, one = F(3), F(2), F(1)
    with np.errstate(all="ignore"):
        u[0] = F(0) if spline_type == 0 else F(-1)
        hm1 = x[1] - x[0]
        for i in range(1, n - 1):
            hi = x[i + 1] - x[i]
            Bi = three * (y[i + 1] - y[i]) / hi - three * (y[i] - y[i - 1]) / hm1
            li = two * (hi + hm1) - hm1 * u[i - 1]
            u[i] = hi / li
            z[i] = (Bi - hm1 * z[i - 1]) / li
            hm1 = hi
        if spline_type == 0:
            z[n - 1] = F(0)
        else:
            z[n - 1] = z[n - 2] / (one + u[n - 2])
        cp1 = z[n - 1]
        for i in range(n - 2, -1, -1):
            c[i] = z[i] - u[i] * cp1
            hi = x[i + 1] - x[i]
            b[i] = (y[i + 1] - y[i]) / hi - hi * (cp1 + two * c[i]) / three
            d[i] = (cp1 - c[i]) / (three * hi)
            cp1 = c[i]
    return np.concatenate([b, c, d]), np.concatenate([u, z])


def spline_intervals(x, xq):
    """The interval the reference's walk uses for each query."""
    n, i, out = len(x), 0, []
    for v in xq:
        while i < n - 1 and not (v <= x[i + 1]):
            i += 1
        out.append(min(i, n - 2))
    return np.array(out, dtype=np.int64)


def spline_eval(x, y, coeffs, xq):
    x, y, coeffs, xq = (np.asarray(a, dtype=F) for a in (x, y, coeffs, xq))
    n = x.size
    b, c, d = coeffs[:n - 1], coeffs[n - 1:2 * (n - 1)], coeffs[2 * (n - 1):]
    iv = spline_intervals(x, xq)
    with np.errstate(all="ignore"):
        t = xq - x[iv]
        return (y[iv] + b[iv] * t + c[iv] * t * t + d[iv] * t * t * t).astype(F)


# ---- the cases ----------------------------------------------------------------------------------------------------
def linear_case_names():
    return [f"{k}_{n}" for k in KINDS for n in LINEAR_SIZES[k]]


def linear_case(name):
    """-> (kind, table, samples [SAMPLES], defined mask)."""
    kind, n = name.split("_")[0], int(name.split("_")[1])
    rng = _rng("linear/" + name)
    if kind == "f32":
        tab = rng.normal(0.0, 1.0, n).astype(F)
        k = np.array(sorted({0, 1, 2, n - 3, n - 2, n - 1, n} & set(range(n + 1))), dtype=np.int64)
        knots = X1 + k.astype(F) * SPACING
        end = X1 + F(n - 1) * SPACING
        special = np.concatenate([
            knots, np.nextafter(knots, F(np.inf)), np.nextafter(knots, F(-np.inf)),
            np.array([X1 - F(1), end + F(0.5) * SPACING, end + F(2) * SPACING, X1 + F(1e6) * SPACING,
                      end - F(0.5) * SPACING, end - F(0.01) * SPACING, -np.inf, -1e30, np.nan, np.inf, 1e30, 3e9],
                     dtype=F)]).astype(F)
        rest = rng.uniform(float(X1 - SPACING), float(end + SPACING), SAMPLES - special.size).astype(F)
        x = np.concatenate([special, rest])
        with np.errstate(all="ignore"):
            q = (x - X1) / SPACING
        defined = ~(np.isnan(q) | (q >= F(2.0 ** 31))) | (x < X1)
        return kind, tab, x, defined
    info = np.iinfo(NP[kind])
    tab = rng.integers(info.min, info.max, n, endpoint=True).astype(NP[kind])
    idx = np.array([0, 1, n - 2, n - 1, n, n + 1, 2047, -1, -2, -2048], dtype=np.int64)
    fr = np.array([0, 1, 0x80000, 0xFFFFE, 0xFFFFF], dtype=np.int64)
    special = ((idx[:, None] << 20) | fr[None, :]).reshape(-1)
    special = np.concatenate([special, [-1, -2 ** 31, 2 ** 31 - 1, 0xFFF00000 - 2 ** 32, 0xFFFFFFFF - 2 ** 32]])
    m = SAMPLES - special.size
    rest = (rng.integers(-2, n + 1, m, endpoint=True) << 20) | rng.integers(0, 1 << 20, m)
    x = _wrap(np.concatenate([special, rest]), 32).astype(np.int32)
    return kind, tab, x, np.ones(SAMPLES, dtype=bool)


def bilinear_case_names():
    return [f"{k}_{r}x{c}" for k in KINDS for r, c in BILINEAR_SHAPES]


def bilinear_case(name):
    """-> (kind, table [rows, cols], X [SAMPLES], Y [SAMPLES], defined mask)."""
    kind, shape = name.split("_")
    rows, cols = (int(v) for v in shape.split("x"))
    rng = _rng("bilinear/" + name)
    if kind == "f32":
        tab = rng.normal(0.0, 1.0, (rows, cols)).astype(F)
        sx = np.array([0, 0.25, cols - 2, cols - 1.001, cols - 1, cols, -0.5, -1, -1.5, np.nan, np.inf, -np.inf, 3e9],
                      dtype=F)
        sy = np.array([0, 0.75, rows - 2, rows - 1.001, rows - 1, rows, -0.5, -1, -1.5, np.nan, np.inf, -np.inf, -3e9],
                      dtype=F)
        gx, gy = np.meshgrid(sx, sy)
        m = SAMPLES - gx.size
        X = np.concatenate([gx.reshape(-1), rng.uniform(-1.0, cols, m)]).astype(F)
        Y = np.concatenate([gy.reshape(-1), rng.uniform(-1.0, rows, m)]).astype(F)
        bad = lambda v: np.isnan(v) | (np.abs(v) >= F(2.0 ** 31))       # noqa: E731
        return kind, tab, X, Y, ~(bad(X) | bad(Y))
    info = np.iinfo(NP[kind])
    tab = rng.integers(info.min, info.max, (rows, cols), endpoint=True).astype(NP[kind])

    def axis(n, salt):
        idx = np.array([0, n - 2, n - 1, -1, 2047], dtype=np.int64)
        fr = np.array([0, 0xFFFFF], dtype=np.int64)
        return ((idx[:, None] << 20) | fr[None, :]).reshape(-1)
    gx, gy = np.meshgrid(axis(cols, 0), axis(rows, 1))
    m = SAMPLES - gx.size
    X = np.concatenate([gx.reshape(-1), (rng.integers(0, cols - 1, m, endpoint=True) << 20) | rng.integers(0, 1 << 20, m)])
    Y = np.concatenate([gy.reshape(-1), (rng.integers(0, rows - 1, m, endpoint=True) << 20) | rng.integers(0, 1 << 20, m)])
    return kind, tab, _wrap(X, 32).astype(np.int32), _wrap(Y, 32).astype(np.int32), np.ones(SAMPLES, dtype=bool)


def spline_knots(n, item=0):
    """-> (x [n] increasing, y [n]) of item `item` of the n-knot cases."""
    rng = _rng(f"spline/{n}/{item}")
    x = np.cumsum(rng.uniform(0.1, 1.0, n)).astype(F)
    return x, rng.normal(0.0, 1.0, n).astype(F)


def spline_queries(kind, x, block, item=0):
    """blockSize queries over [x[0] - 1, x[n - 1] + 1]: below the first knot, above the last, and between."""
    rng = _rng(f"queries/{kind}/{x.size}/{block}/{item}")
    q = np.sort(rng.uniform(float(x[0]) - 1.0, float(x[-1]) + 1.0, block)).astype(F)
    if kind == "knots":
        q[::2] = x[rng.integers(0, x.size, q[::2].size)]
        q = np.sort(q)
    elif kind == "unsorted":
        rng.shuffle(q)
    elif kind == "nan":
        q[block // 2] = np.nan
    return q


def spline_case_names():
    return [f"{n}_{t}_{k}_{b}" for n in SPLINE_N for t in (0, 1) for k in SPLINE_QUERIES for b in SPLINE_BLOCKS]


def spline_case(name):
    """-> (type, x, y, xq)."""
    n, t, kind, block = name.split("_")
    x, y = spline_knots(int(n))
    return int(t), x, y, spline_queries(kind, x, int(block))
