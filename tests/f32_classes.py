"""float32 value classes for the bit-exact f32 tests (helper, not a test file): inputs made of
subnormals, signed zeros, words near overflow, infinities and NaNs, and a word-for-word comparison
that tells +0.0 from -0.0 and a subnormal from zero.

    x = f32_class_input(cls, shape, seed, scale=None, positions=None)
    assert_same_words(got, want)
    classes_of(y) -> {"subnormal", "pzero", "nzero", "inf", "nan", "normal"} shares
"""
import numpy as np

CLASSES = ("subnormal", "negzero", "signzero", "mixed", "overflow", "nonfinite")
TINY = np.finfo(np.float32).tiny           # 2^-126, the smallest normal


def _size(shape):
    return int(np.prod(shape, dtype=np.int64))


def f32_class_input(cls, shape, seed, scale=None, positions=None):
    """A float32 array of `shape` of one value class ("uniform" is the ordinary stream); seed is an
    integer or a numpy Generator to draw from:

    subnormal  uniform(0.5, 1) * +-1 * 2^k, k integer in [-149, -130]: every word a nonzero subnormal
    negzero    every word -0.0
    signzero   a random choice of +0.0 / -0.0
    mixed      exponents 2^-20 .. 2^20, 10 % +0.0, 10 % -0.0
    overflow   finite, uniform(0.5, 1) * +-1 * scale (the caller's scale: sums overflow, words do not)
    nonfinite  uniform(-1, 1) with +Inf, -Inf and NaN at the caller's three distinct flat positions
    uniform    uniform(-1, 1)
    """
    rng = np.random.default_rng(seed)
    n = _size(shape)
    if cls == "uniform":
        v = rng.uniform(-1.0, 1.0, n)
    elif cls == "subnormal":
        k = rng.integers(-149, -130, n, endpoint=True)
        v = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** k
    elif cls == "negzero":
        v = np.full(n, -0.0)
    elif cls == "signzero":
        v = rng.choice([0.0, -0.0], n)
    elif cls == "mixed":
        v = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-20, 21, n)
        z = rng.uniform(0, 1, n)
        v[z < 0.1] = 0.0
        v[(z >= 0.1) & (z < 0.2)] = -0.0
    elif cls == "overflow":
        assert scale is not None and np.isfinite(np.float32(scale)), "overflow: the caller chooses a finite scale"
        v = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * float(scale)
    elif cls == "nonfinite":
        assert positions is not None and len(set(positions)) == 3, "nonfinite: three distinct positions"
        v = rng.uniform(-1.0, 1.0, n)
        v[list(positions)] = [np.inf, -np.inf, np.nan]
    else:
        raise ValueError(cls)
    with np.errstate(over="raise"):
        out = v.astype(np.float32).reshape(shape)
    if cls == "subnormal":      # 2^-149 * [0.5, 1) rounds to 0 or 2^-149: keep every word nonzero
        flat = out.reshape(-1)
        flat[flat == 0] = np.float32(2.0 ** -149)
    return out


def _words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_words(got, want, what=""):
    """Equal NaN masks, and every word that is not a NaN equal as uint32: +0.0 / -0.0, +-Inf and
    subnormals are compared by their bits.

    NaNs are compared by position only.  A NaN that an operation generates (Inf - Inf, 0 * Inf) is
    0xFFC00000 on the host's SSE unit and 0x7FC00000 on gfx9, and when two NaNs meet in one operation
    the two machines also differ in which operand's payload survives, so the bits of a NaN say
    nothing about the arithmetic that led to it; where it stands does.

    The failure message gives the first five differing indices with both words in hex."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g, w = _words(got).reshape(-1), _words(want).reshape(-1)
    gn, wn = np.isnan(got).reshape(-1), np.isnan(want).reshape(-1)
    bad = (gn != wn) | (~gn & ~wn & (g != w))
    if bad.any():
        idx = np.flatnonzero(bad)
        first = ", ".join(f"[{i}] got 0x{g[i]:08X} want 0x{w[i]:08X}" for i in idx[:5])
        raise AssertionError(f"{what}: {idx.size} of {g.size} words differ: {first}")


def classes_of(y):
    """Shares of the words of y that are nonzero subnormals, +0.0, -0.0, +-Inf, NaN, finite normals."""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    a = np.abs(y)
    neg = np.signbit(y)
    n = max(y.size, 1)
    return {"subnormal": float(np.count_nonzero((a > 0) & (a < TINY))) / n,
            "pzero": float(np.count_nonzero((y == 0) & ~neg)) / n,
            "nzero": float(np.count_nonzero((y == 0) & neg)) / n,
            "inf": float(np.count_nonzero(np.isinf(y))) / n,
            "nan": float(np.count_nonzero(np.isnan(y))) / n,
            "normal": float(np.count_nonzero(np.isfinite(y) & (a >= TINY))) / n}
